// Slot property probe (utils/property_predictor.py:99-189 of the reference): per image, the cost of giving object o to slot s, the exact
// minimum-cost assignment of the N objects to N distinct slots, and from the matching the loss, d loss / d out and the metrics.
//   probe_match    one wave per image, WPB waves per workgroup, every buffer of an image in the wave's own slice of LDS:
//     1. out [K, O] and y [N, T] are staged; per slot and categorical property lp = log_softmax(softmax(out[s, a:b])) (the reference
//        hands F.softmax's result to CrossEntropyLoss, so the soft-max is taken twice)
//     2. C[o, s] = sum over the properties, in schema order, of -lp[s, a + int(y[o, t])]  or  mean((out[s, a:a+2] - y[o, t:t+2])^2)
//     3. dynamic programme over slot bit-masks: best[mask] = min over s in mask of best[mask \ s] + C[popcount(mask) - 1, s], level by
//        level (level c holds the masks of c slots, object c - 1 is placed last), the argmin kept in choice[mask]; 2^K floats and
//        2^K bytes.  Ties go to the lowest slot index (strict <, s ascending), the end state to the lowest mask; the backtrack reads
//        choice[], it compares no floats again.
//     4. per image: loss, correct-class counts, the reference's R^2 and distance sums -> part[b, :]; d loss / d out through both
//        soft-maxes (zero rows for unmatched slots), scaled by dloss
//   probe_reduce   metrics[j] = scale_j * sum_b part[b, j]: one wave per column, lane-strided partial sums in image order, then a
//                  butterfly.  No atomics: a result depends on (B, K, N) alone and two runs agree bit for bit.
//   probe_leaky_fwd / _bwd   LeakyReLU of the mlp3 head in place; the backward reads the stored activation, whose sign is its input's
//                  (zero takes the slope, as torch does)
// A target class outside its property's range poisons that cost with NaN (the reference raises there); every index that addresses
// memory is clamped first.  Loop bounds are K, N, O, P from the arguments, validated by probe_match_launch before the launch.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

struct LdsLay { int so, sl, sy, sc, best, col, choice, bytes; };

__host__ __device__ inline LdsLay probe_lds(int K, int N, int O, int T) {
    LdsLay l;
    int f = 0;
    l.so = f; f += K * O;                 // staged outputs
    l.sl = f; f += K * O;                 // log-probabilities, later the gradient
    l.sy = f; f += N * T;
    l.sc = f; f += N * K;
    l.best = f; f += 1 << K;
    l.col = f; f += N;
    l.choice = f * 4;                     // bytes from here
    l.bytes = (l.choice + (1 << K) + 15) & ~15;
    return l;
}

// lp[0:w] = softmax(z[0:w]); returns the log-sum-exp of lp, so log_softmax(softmax(z)) = lp - return value
__device__ inline float double_softmax(const float* z, int w, float* lp) {
    float m = z[0];
    for (int i = 1; i < w; ++i) m = fmaxf(m, z[i]);
    float S = 0.f;
    for (int i = 0; i < w; ++i) S += expf(z[i] - m);
    float mp = 0.f;
    for (int i = 0; i < w; ++i) { lp[i] = expf(z[i] - m) / S; mp = fmaxf(mp, lp[i]); }
    float S2 = 0.f;
    for (int i = 0; i < w; ++i) S2 += expf(lp[i] - mp);
    return mp + logf(S2);
}

__global__ __launch_bounds__(256) void probe_match_kernel(const float* __restrict__ out, int ld_row, long long ld_img, const float* __restrict__ y,
                                                          const float* __restrict__ dloss, float* __restrict__ cost, int* __restrict__ col,
                                                          float* __restrict__ part, float* __restrict__ dout, int B, int K, int N, int T, int O,
                                                          ProbeSchema sc) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LdsLay L = probe_lds(K, N, O, T);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const long long b = (long long)blockIdx.x * wpb + wave;
    const bool live = b < B;                                       // idle waves of the last workgroup still meet every barrier
    unsigned char* base = smem + (size_t)wave * L.bytes;
    float* f = reinterpret_cast<float*>(base);
    float *so = f + L.so, *sl = f + L.sl, *sy = f + L.sy, *sC = f + L.sc, *best = f + L.best;
    int* scol = reinterpret_cast<int*>(f + L.col);
    unsigned char* choice = base + L.choice;
    const int P = sc.P, nmask = 1 << K;

    if (live) {
        for (int i = lane; i < K * O; i += 64) so[i] = out[b * ld_img + (long long)(i / O) * ld_row + i % O];
        for (int i = lane; i < N * T; i += 64) sy[i] = y[b * N * T + i];
    }
    __syncthreads();
    // 1. log_softmax(softmax(.)) of every (slot, categorical property)
    if (live)
        for (int it = lane; it < K * P; it += 64) {
            const int s = it / P, p = it % P;
            if (sc.kind[p]) continue;
            const int a = sc.a[p], w = sc.b[p] - a;
            float* lp = sl + s * O + a;
            const float lse = double_softmax(so + s * O + a, w, lp);
            for (int i = 0; i < w; ++i) lp[i] -= lse;
        }
    __syncthreads();
    // 2. cost matrix
    if (live)
        for (int it = lane; it < N * K; it += 64) {
            const int o = it / K, s = it % K;
            float c = 0.f;
            for (int p = 0; p < P; ++p) {
                const int a = sc.a[p], t = sc.t[p];
                if (sc.kind[p]) {
                    const float dx = so[s * O + a] - sy[o * T + t], dy = so[s * O + a + 1] - sy[o * T + t + 1];
                    c += (dx * dx + dy * dy) * 0.5f;
                } else {
                    const float yv = sy[o * T + t];
                    const int w = sc.b[p] - a;
                    const bool ok = yv >= 0.f && yv < (float)w;
                    const int cls = ok ? (int)yv : 0;
                    c += ok ? -sl[s * O + a + cls] : NAN;
                }
            }
            sC[it] = c;
            if (cost) cost[b * N * K + it] = c;
        }
    if (live && lane == 0) best[0] = 0.f;
    __syncthreads();
    // 3. assignment: level c places object c - 1 on one slot of every mask of c slots
    for (int c = 1; c <= N; ++c) {
        if (live)
            for (int mask = lane; mask < nmask; mask += 64) {
                if (__popc(mask) != c) continue;
                float v = INFINITY;
                int bs = __ffs(mask) - 1;
                for (int s = 0; s < K; ++s) {
                    if (!((mask >> s) & 1)) continue;
                    const float cand = best[mask ^ (1 << s)] + sC[(c - 1) * K + s];
                    if (cand < v) { v = cand; bs = s; }
                }
                best[mask] = v;
                choice[mask] = (unsigned char)bs;
            }
        __syncthreads();
    }
    if (live) {
        float v = INFINITY;
        int bm = nmask;                                            // nmask: none seen yet
        for (int mask = lane; mask < nmask; mask += 64)
            if (__popc(mask) == N && (bm == nmask || best[mask] < v)) { v = best[mask]; bm = mask; }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off, 64);
            const int om = __shfl_xor(bm, off, 64);
            if (om != nmask && (bm == nmask || ov < v || (ov == v && om < bm))) { v = ov; bm = om; }
        }
        bm = __shfl(bm, 0, 64);
        if (bm == nmask) bm = (1 << N) - 1;                        // unreachable (N <= K): stays a valid mask
        if (lane == 0) {
            int mask = bm;
            for (int o = N - 1; o >= 0; --o) {
                int s = choice[mask];
                if (!((mask >> s) & 1)) s = __ffs(mask) - 1;       // cannot happen: choice[] is written for every mask of a level
                scol[o] = s;
                mask ^= 1 << s;
            }
        }
    }
    __syncthreads();
    // 4. matched loss, metrics, gradient.  sl becomes the gradient of this image
    if (live) {
        for (int i = lane; i < K * O; i += 64) sl[i] = 0.f;
        if (col)
            for (int o = lane; o < N; o += 64) col[b * N + o] = scol[o];
    }
    __syncthreads();
    if (live) {
        const float g = dloss ? dloss[0] : 1.f;
        for (int it = lane; it < N * P; it += 64) {
            const int o = it / P, p = it % P, s = scol[o], a = sc.a[p], t = sc.t[p];
            float* gr = sl + s * O + a;
            const float* z = so + s * O + a;
            if (sc.kind[p]) {
                gr[0] = g * (z[0] - sy[o * T + t]);
                gr[1] = g * (z[1] - sy[o * T + t + 1]);
            } else {
                // loss = -log_softmax(q)[cls], q = softmax(z): d loss / d q = r - onehot (r = softmax(q)); d z_i = q_i (dq_i - sum_j dq_j q_j)
                const int w = sc.b[p] - a;
                const float yv = sy[o * T + t];
                const int cls = (yv >= 0.f && yv < (float)w) ? (int)yv : 0;
                const float lse = double_softmax(z, w, gr);         // gr = q
                float dot = 0.f;
                for (int i = 0; i < w; ++i) dot += (expf(gr[i] - lse) - (i == cls ? 1.f : 0.f)) * gr[i];
                for (int i = 0; i < w; ++i) gr[i] = g * gr[i] * (expf(gr[i] - lse) - (i == cls ? 1.f : 0.f) - dot);
            }
        }
        if (lane == 0) {                                           // part[b] = loss, one entry per property, the distance sum
            float* pb = part + b * (P + 2);
            float loss = 0.f;
            for (int o = 0; o < N; ++o) loss += sC[o * K + scol[o]];
            pb[0] = loss;
            pb[P + 1] = 0.f;
            for (int p = 0; p < P; ++p) {
                const int a = sc.a[p], t = sc.t[p];
                float m = 0.f;
                if (sc.kind[p]) {
                    float dist = 0.f;
                    for (int o = 0; o < N; ++o) {
                        const float dx = so[scol[o] * O + a] - sy[o * T + t], dy = so[scol[o] * O + a + 1] - sy[o * T + t + 1];
                        dist += sqrtf(dx * dx + dy * dy);
                    }
                    pb[P + 1] = dist;
                    for (int c = 0; c < 2; ++c) {                  // the reference's ratio ||out - mean(y)||^2 / ||y - mean(y)||^2 per coordinate
                        float mean = 0.f, sst = 0.f, sse = 0.f;
                        for (int o = 0; o < N; ++o) mean += sy[o * T + t + c];
                        mean /= (float)N;
                        for (int o = 0; o < N; ++o) {
                            const float dt = sy[o * T + t + c] - mean, de = so[scol[o] * O + a + c] - mean;
                            sst += dt * dt;
                            sse += de * de;
                        }
                        m += sse / sst;
                    }
                } else {
                    const int w = sc.b[p] - a;
                    for (int o = 0; o < N; ++o) {
                        const float* z = so + scol[o] * O + a;
                        int am = 0;
                        for (int i = 1; i < w; ++i)
                            if (z[i] > z[am]) am = i;
                        m += ((float)am == sy[o * T + t]) ? 1.f : 0.f;
                    }
                }
                pb[1 + p] = m;
            }
        }
    }
    __syncthreads();
    if (live && dout)
        for (int i = lane; i < K * O; i += 64) dout[b * ld_img + (long long)(i / O) * ld_row + i % O] = sl[i];
}

__global__ __launch_bounds__(64) void probe_reduce_kernel(const float* __restrict__ part, float* __restrict__ metrics, int B, int N, ProbeSchema sc) {
    const int j = blockIdx.x, ncol = sc.P + 2;
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += 64) s += part[(long long)b * ncol + j];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        float scale = 1.f;                                          // the loss is a sum over images and objects
        if (j == sc.P + 1 || (j >= 1 && j <= sc.P && !sc.kind[j - 1])) scale = 1.f / ((float)B * (float)N);
        else if (j >= 1 && j <= sc.P) scale = 1.f / (2.f * (float)B);
        metrics[j] = s * scale;
    }
}

__global__ __launch_bounds__(256) void probe_leaky_fwd_kernel(float* __restrict__ x, long long n, float slope) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { const float v = x[t]; x[t] = v > 0.f ? v : v * slope; }
}
__global__ __launch_bounds__(256) void probe_leaky_bwd_kernel(float* __restrict__ dx, const float* __restrict__ h, long long n, float slope) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dx[t] = h[t] > 0.f ? dx[t] : dx[t] * slope;
}

}  // namespace

int probe_schema_check(const ProbeSchema& sc, int T, int O) {
    OCRL_REQUIRE(sc.P >= 1 && sc.P <= PROBE_MAX_PROPS, "probe: 1 <= properties <= %d (got %d)", PROBE_MAX_PROPS, sc.P);
    int nxy = 0;
    for (int p = 0; p < sc.P; ++p) {
        const int w = sc.b[p] - sc.a[p], tw = sc.kind[p] ? 2 : 1;
        OCRL_REQUIRE(sc.kind[p] == 0 || sc.kind[p] == 1, "probe: property %d has kind %d (0 = categorical, 1 = xy)", p, sc.kind[p]);
        OCRL_REQUIRE(sc.a[p] >= 0 && w >= 1 && sc.b[p] <= O, "probe: property %d reads outputs [%d, %d) of %d", p, sc.a[p], sc.b[p], O);
        OCRL_REQUIRE(sc.t[p] >= 0 && sc.t[p] + tw <= T, "probe: property %d reads targets [%d, %d) of %d", p, sc.t[p], sc.t[p] + tw, T);
        OCRL_REQUIRE(!sc.kind[p] || w == 2, "probe: the xy property needs 2 outputs (dims: 2), got %d", w);
        OCRL_REQUIRE(p == 0 || sc.a[p] >= sc.b[p - 1], "probe: the output ranges must ascend without overlap (property %d starts at %d)", p, sc.a[p]);
        nxy += sc.kind[p];
    }
    OCRL_REQUIRE(nxy <= 1, "probe: at most one xy property (got %d)", nxy);
    return 0;
}

int probe_match_check(int B, int K, int N, int T, int O) {
    OCRL_REQUIRE(B >= 1 && N >= 1 && T >= 1 && O >= 1, "probe: batch, objects, state width and output width >= 1 (got %d, %d, %d, %d)", B, N, T, O);
    OCRL_REQUIRE(K >= 1 && K <= PROBE_MAX_SLOTS, "probe: %d slots; the assignment is built for 1 .. %d slots", K, PROBE_MAX_SLOTS);
    OCRL_REQUIRE(N <= K, "probe: %d objects cannot be matched to %d slots", N, K);
    OCRL_REQUIRE(O <= PROBE_MAX_WIDTH && T <= PROBE_MAX_WIDTH, "probe: output / state width above %d (got %d, %d)", PROBE_MAX_WIDTH, O, T);
    OCRL_REQUIRE(probe_lds(K, N, O, T).bytes <= 64 * 1024, "probe: %d slots of %d outputs do not fit the LDS of one wave", K, O);
    return 0;
}

int probe_match_launch(const float* out, int ld_row, long long ld_img, const float* y, const float* dloss, float* cost, int* col, float* part,
                       float* metrics, float* dout, int B, int K, int N, int T, int O, const ProbeSchema& sc, hipStream_t st) {
    RC(probe_match_check(B, K, N, T, O));
    RC(probe_schema_check(sc, T, O));
    OCRL_REQUIRE(ld_row >= O && ld_img >= (long long)(K - 1) * ld_row + O, "probe: strides %d / %lld do not hold [%d, %d]", ld_row, ld_img, K, O);
    const int per = probe_lds(K, N, O, T).bytes;
    int wpb = 64 * 1024 / per;
    if (wpb > 4) wpb = 4;
    hipLaunchKernelGGL(probe_match_kernel, dim3(cdiv(B, wpb)), dim3(64 * wpb), (size_t)per * wpb, st, out, ld_row, ld_img, y, dloss, cost, col, part,
                       dout, B, K, N, T, O, sc);
    OCRL_CHECK_LAUNCH("probe_match");
    hipLaunchKernelGGL(probe_reduce_kernel, dim3(sc.P + 2), dim3(64), 0, st, part, metrics, B, N, sc);
    OCRL_CHECK_LAUNCH("probe_reduce");
    return 0;
}

int probe_leaky_fwd_launch(float* x, long long n, float slope, hipStream_t st) {
    hipLaunchKernelGGL(probe_leaky_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, n, slope);
    OCRL_CHECK_LAUNCH("probe_leaky_fwd");
    return 0;
}
int probe_leaky_bwd_launch(float* dx, const float* h, long long n, float slope, hipStream_t st) {
    hipLaunchKernelGGL(probe_leaky_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dx, h, n, slope);
    OCRL_CHECK_LAUNCH("probe_leaky_bwd");
    return 0;
}
