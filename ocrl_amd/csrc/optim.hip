// Global inf-norm gradient clip + Adam on flat fp32 buffers (reference: ocrs/base.py:65-72,
// torch.nn.utils.clip_grad_norm_(…, "inf") and torch.optim.Adam defaults), the TF-style RMSprop update A2C takes after the same clip, and
// the L2 clip + either update over several flat buffers under one joint norm (multi_*, at the end).
#include "common.h"
#include "kernels.h"

// The inf-norm is reduced on the bit patterns of |g|: for non-negative floats the unsigned integer order is the float order, +inf
// lies above every finite value and every NaN pattern above +inf, so the maximum is exact, independent of the order of the fold, and
// a NaN anywhere in the buffer reaches the norm (fmaxf would drop it, and with it the sign of a diverged run in the log), as in
// torch.nn.utils.clip_grad_norm_.
__device__ inline unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }
__device__ inline unsigned wave_max_bits(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// part[blk] = max |g| over the block's grid-stride range
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ g, long long n4, float* __restrict__ part) {
    __shared__ unsigned red[4];
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        m = max(m, max(max(abs_bits(v.x), abs_bits(v.y)), max(abs_bits(v.z), abs_bits(v.w))));
    }
    m = wave_max_bits(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = __uint_as_float(max(max(red[0], red[1]), max(red[2], red[3])));
}
__global__ void absmax_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    unsigned m = 0u;
    for (int i = threadIdx.x; i < n; i += 64) m = max(m, abs_bits(part[i]));
    m = wave_max_bits(m);
    if (threadIdx.x == 0) out[0] = __uint_as_float(m);
}

// g *= min(1, clip/(norm+1e-6)) (clip <= 0: no clipping); then the Adam update, all in one pass.  The min keeps a NaN quotient
// (torch.clamp(max=1) does; fminf would return 1), so a NaN norm reaches every weight.  omb1 / omb2 are 1 - beta and bc1 /
// bc2_sqrt the bias corrections, all computed in double from the decimal betas and rounded once: 1.f - 0.999f is 1.3e-5 away from
// 0.001 (the rounding of 0.999f, small against 1, is 2^-14 of the difference), and 1 - 0.999f^t carries the same error at small t.
__device__ __forceinline__ float clip_coef(const float* __restrict__ norm, float clip, float gscale) {
    float coef = gscale;
    if (clip > 0.f) {
        const float c = clip / (norm[0] * gscale + 1e-6f);
        coef *= c > 1.0f ? 1.0f : c;
    }
    return coef;
}
// one element of the update; step = lr / bc1
__device__ __forceinline__ void adam_upd(float gg, float& mm, float& vq, float& pp, float coef, float step, float omb1, float b2, float omb2,
                                         float eps, float bc2_sqrt) {
    gg *= coef;
    mm = mm + (gg - mm) * omb1;                        // exp_avg.lerp_(grad, 1 - beta1)
    vq = vq * b2 + omb2 * gg * gg;
    const float denom = sqrtf(vq) / bc2_sqrt + eps;
    pp -= step * (mm / denom);
}
__global__ __launch_bounds__(256) void clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, long long n4, const float* __restrict__ norm, float clip,
                                                       float lr, float omb1, float b2, float omb2, float eps, float bc1, float bc2_sqrt, float gscale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float coef = clip_coef(norm, clip, gscale);
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i], pv = reinterpret_cast<float4*>(p)[i];
    const float step = lr / bc1;
    auto upd = [&](float gg, float& mm, float& vq, float& pp) { adam_upd(gg, mm, vq, pp, coef, step, omb1, b2, omb2, eps, bc2_sqrt); };
    upd(gv.x, mv.x, vv.x, pv.x); upd(gv.y, mv.y, vv.y, pv.y); upd(gv.z, mv.z, vv.z, pv.z); upd(gv.w, mv.w, vv.w, pv.w);
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(p)[i] = pv;
}
// the same update on the n < 4 elements a buffer's length leaves past its last group of four (ocrl_flat_clip_adam_l2)
__global__ __launch_bounds__(64) void clip_adam_tail_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int n, const float* __restrict__ norm, float clip, float lr,
                                                           float omb1, float b2, float omb2, float eps, float bc1, float bc2_sqrt, float gscale) {
    const int i = threadIdx.x;
    if (i >= n) return;
    float mm = m[i], vq = v[i], pp = p[i];
    adam_upd(g[i], mm, vq, pp, clip_coef(norm, clip, gscale), lr / bc1, omb1, b2, omb2, eps, bc2_sqrt);
    m[i] = mm; v[i] = vq; p[i] = pp;
}

// One element of the TF-style RMSprop update (stable-baselines3's RMSpropTFLike: momentum 0, not centred, no weight decay): the epsilon
// sits inside the square root, and the caller starts sq at ones.  oma = 1 - alpha, taken in double from the decimal alpha.
__device__ __forceinline__ void rmsprop_upd(float gg, float& sq, float& pp, float coef, float lr, float alpha, float oma, float eps) {
    gg *= coef;
    sq = alpha * sq + oma * gg * gg;
    pp -= lr * (gg / sqrtf(sq + eps));
}
__global__ __launch_bounds__(256) void clip_rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, long long n4,
                                                          const float* __restrict__ norm, float clip, float lr, float alpha, float oma, float eps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float coef = clip_coef(norm, clip, 1.f);
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 sv = reinterpret_cast<float4*>(sq)[i], pv = reinterpret_cast<float4*>(p)[i];
    rmsprop_upd(gv.x, sv.x, pv.x, coef, lr, alpha, oma, eps); rmsprop_upd(gv.y, sv.y, pv.y, coef, lr, alpha, oma, eps);
    rmsprop_upd(gv.z, sv.z, pv.z, coef, lr, alpha, oma, eps); rmsprop_upd(gv.w, sv.w, pv.w, coef, lr, alpha, oma, eps);
    reinterpret_cast<float4*>(sq)[i] = sv;
    reinterpret_cast<float4*>(p)[i] = pv;
}
// the same update on the n < 4 elements a buffer's length leaves past its last group of four
__global__ __launch_bounds__(64) void clip_rmsprop_tail_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, int n,
                                                              const float* __restrict__ norm, float clip, float lr, float alpha, float oma, float eps) {
    const int i = threadIdx.x;
    if (i >= n) return;
    float s = sq[i], pp = p[i];
    rmsprop_upd(g[i], s, pp, clip_coef(norm, clip, 1.f), lr, alpha, oma, eps);
    sq[i] = s; p[i] = pp;
}

int absmax_launch(const float* g, long long n, float* out, float* ws, size_t ws_floats, hipStream_t st) {
    OCRL_REQUIRE(n % 4 == 0 && ws_floats >= 1024, "absmax: n %% 4 != 0 or workspace too small");
    int nblk = cdiv(n / 4, 256);
    if (nblk > 1024) nblk = 1024;
    hipLaunchKernelGGL(absmax_kernel, dim3(nblk), dim3(256), 0, st, g, n / 4, ws);
    OCRL_CHECK_LAUNCH("absmax");
    hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(64), 0, st, ws, nblk, out);
    OCRL_CHECK_LAUNCH("absmax_final");
    return 0;
}
int clip_adam_launch(float* p, const float* g, float* m, float* v, long long n, const float* norm, float clip, float lr, double b1,
                     double b2, double eps, int step, float gscale, hipStream_t st) {
    OCRL_REQUIRE(n % 4 == 0 && step >= 1, "clip_adam: n %% 4 != 0 or step < 1");
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);      // from the decimal betas, as torch.optim.Adam does
    hipLaunchKernelGGL(clip_adam_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, p, g, m, v, n / 4, norm, clip, lr,
                       (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, (float)bc1, (float)sqrt(bc2), gscale);
    OCRL_CHECK_LAUNCH("clip_adam");
    return 0;
}
int clip_adam_tail_launch(float* p, const float* g, float* m, float* v, int n, const float* norm, float clip, float lr, double b1, double b2,
                          double eps, int step, float gscale, hipStream_t st) {
    OCRL_REQUIRE(n >= 1 && n < 4 && step >= 1, "clip_adam_tail: 1 <= n <= 3 and step >= 1");
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
    hipLaunchKernelGGL(clip_adam_tail_kernel, dim3(1), dim3(64), 0, st, p, g, m, v, n, norm, clip, lr, (float)(1.0 - b1), (float)b2,
                       (float)(1.0 - b2), (float)eps, (float)bc1, (float)sqrt(bc2), gscale);
    OCRL_CHECK_LAUNCH("clip_adam_tail");
    return 0;
}
int clip_rmsprop_launch(float* p, const float* g, float* sq, long long n, const float* norm, float clip, float lr, double alpha, double eps,
                        hipStream_t st) {
    OCRL_REQUIRE(n >= 4 && n % 4 == 0, "clip_rmsprop: n %% 4 != 0 or n < 4");
    hipLaunchKernelGGL(clip_rmsprop_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, p, g, sq, n / 4, norm, clip, lr, (float)alpha,
                       (float)(1.0 - alpha), (float)eps);
    OCRL_CHECK_LAUNCH("clip_rmsprop");
    return 0;
}
int clip_rmsprop_tail_launch(float* p, const float* g, float* sq, int n, const float* norm, float clip, float lr, double alpha, double eps,
                             hipStream_t st) {
    OCRL_REQUIRE(n >= 1 && n < 4, "clip_rmsprop_tail: 1 <= n <= 3");
    hipLaunchKernelGGL(clip_rmsprop_tail_kernel, dim3(1), dim3(64), 0, st, p, g, sq, n, norm, clip, lr, (float)alpha, (float)(1.0 - alpha), (float)eps);
    OCRL_CHECK_LAUNCH("clip_rmsprop_tail");
    return 0;
}

// ---- the same clip + update over up to FLAT_MAX_SEG flat buffers at once (ocrl_flat_clip_*_l2_multi): the norm is that of all the
// gradients together.  The segment table is a kernel argument, passed by value: nothing is uploaded.  Segment s owns the blocks
// [blk0[s], blk0[s + 1]) of the partial-sum launch and of the update launch alike; a block finds s from blockIdx alone, so s is uniform
// across it, and walks its segment's groups of four floats grid-stride.  The n % 4 floats a segment's length leaves past its last
// group of four are taken element by element inside the same launches.
static_assert(FLAT_MAX_SEG == 8, "seg_of compares against seven boundaries");
__device__ __forceinline__ int seg_of(const FlatSegs& t) {
    const int b = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int i = 1; i < FLAT_MAX_SEG; ++i) s += (i < t.nseg && b >= t.blk0[i]) ? 1 : 0;
    return s;
}
// part[blk] = the block's share of its segment's sum of squares
__global__ __launch_bounds__(256) void multi_sumsq_kernel(const FlatSegs t, float* __restrict__ part) {
    __shared__ float red[4];
    const int s = seg_of(t), lb = blockIdx.x - t.blk0[s], nb = t.blk0[s + 1] - t.blk0[s];
    const float* __restrict__ g = t.g[s];
    const long long n = t.n[s], n4 = n >> 2;
    float a = 0.f;
    for (long long i = (long long)lb * 256 + threadIdx.x; i < n4; i += (long long)nb * 256) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        a += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    if (lb == nb - 1 && (long long)threadIdx.x < n - 4 * n4) { const float x = g[4 * n4 + threadIdx.x]; a += x * x; }
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// norm[0] = sqrt of the sum of the partials, which lie in segment order, then block order: thread j adds part[j], part[j + 256], ... in
// that order, then the fixed tree of the block.  One block of 256 threads.
__global__ __launch_bounds__(256) void multi_norm_kernel(const float* __restrict__ part, int n, float* __restrict__ norm) {
    __shared__ float red[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) a += part[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) norm[0] = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
}
// ADAM: s0 = m, s1 = v and (c0 .. c5) = (lr / bc1, 1 - beta1, beta2, 1 - beta2, eps, sqrt(bc2)); else s0 = sq and (c0 .. c3) = (lr, alpha,
// 1 - alpha, eps)
template <bool ADAM>
__global__ __launch_bounds__(256) void multi_update_kernel(const FlatSegs t, const float* __restrict__ norm, float clip, float c0, float c1,
                                                          float c2, float c3, float c4, float c5) {
    const int s = seg_of(t), lb = blockIdx.x - t.blk0[s], nb = t.blk0[s + 1] - t.blk0[s];
    float* __restrict__ p = t.p[s];
    const float* __restrict__ g = t.g[s];
    float* __restrict__ s0 = t.s0[s];
    float* __restrict__ s1 = t.s1[s];
    const long long n = t.n[s], n4 = n >> 2;
    const float coef = clip_coef(norm, clip, 1.f);
    auto upd = [&](float gg, float& a, float& b, float& pp) {
        if (ADAM) adam_upd(gg, a, b, pp, coef, c0, c1, c2, c3, c4, c5);
        else rmsprop_upd(gg, a, pp, coef, c0, c1, c2, c3);
    };
    for (long long i = (long long)lb * 256 + threadIdx.x; i < n4; i += (long long)nb * 256) {
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 av = reinterpret_cast<float4*>(s0)[i], pv = reinterpret_cast<float4*>(p)[i], bv = av;
        if (ADAM) bv = reinterpret_cast<float4*>(s1)[i];
        upd(gv.x, av.x, bv.x, pv.x); upd(gv.y, av.y, bv.y, pv.y); upd(gv.z, av.z, bv.z, pv.z); upd(gv.w, av.w, bv.w, pv.w);
        reinterpret_cast<float4*>(s0)[i] = av;
        if (ADAM) reinterpret_cast<float4*>(s1)[i] = bv;
        reinterpret_cast<float4*>(p)[i] = pv;
    }
    if (lb == nb - 1 && (long long)threadIdx.x < n - 4 * n4) {
        const long long i = 4 * n4 + threadIdx.x;
        float a = s0[i], b = ADAM ? s1[i] : 0.f, pp = p[i];
        upd(g[i], a, b, pp);
        s0[i] = a;
        if (ADAM) s1[i] = b;
        p[i] = pp;
    }
}

// blk0: each segment gets one block per 256 groups of four floats, at least one and at most FLAT_SEG_BLOCKS
static void flat_segs_blocks(FlatSegs& t) {
    t.blk0[0] = 0;
    for (int s = 0; s < FLAT_MAX_SEG; ++s) {
        int nb = 0;
        if (s < t.nseg) {
            const long long want = (t.n[s] / 4 + 255) / 256;
            nb = want < 1 ? 1 : want > FLAT_SEG_BLOCKS ? FLAT_SEG_BLOCKS : (int)want;
        }
        t.blk0[s + 1] = t.blk0[s] + nb;
    }
}
static int multi_norm_launch(const FlatSegs& t, float* norm, float* ws, size_t ws_floats, hipStream_t st) {
    const int nblk = t.blk0[t.nseg];
    OCRL_REQUIRE(t.nseg >= 1 && t.nseg <= FLAT_MAX_SEG && nblk >= 1 && ws && ws_floats >= (size_t)nblk, "flat multi: bad segment table or scratch");
    hipLaunchKernelGGL(multi_sumsq_kernel, dim3(nblk), dim3(256), 0, st, t, ws);
    OCRL_CHECK_LAUNCH("multi_sumsq");
    hipLaunchKernelGGL(multi_norm_kernel, dim3(1), dim3(256), 0, st, ws, nblk, norm);
    OCRL_CHECK_LAUNCH("multi_norm");
    return 0;
}
int multi_clip_adam_launch(FlatSegs t, float* norm, float clip, float lr, double b1, double b2, double eps, int step, float* ws, size_t ws_floats,
                           hipStream_t st) {
    OCRL_REQUIRE(step >= 1, "multi_clip_adam: step < 1");
    flat_segs_blocks(t);
    RC(multi_norm_launch(t, norm, ws, ws_floats, st));
    const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);      // as clip_adam_launch takes them
    hipLaunchKernelGGL(multi_update_kernel<true>, dim3(t.blk0[t.nseg]), dim3(256), 0, st, t, norm, clip, lr / (float)bc1, (float)(1.0 - b1),
                       (float)b2, (float)(1.0 - b2), (float)eps, (float)sqrt(bc2));
    OCRL_CHECK_LAUNCH("multi_clip_adam");
    return 0;
}
int multi_clip_rmsprop_launch(FlatSegs t, float* norm, float clip, float lr, double alpha, double eps, float* ws, size_t ws_floats, hipStream_t st) {
    flat_segs_blocks(t);
    RC(multi_norm_launch(t, norm, ws, ws_floats, st));
    hipLaunchKernelGGL(multi_update_kernel<false>, dim3(t.blk0[t.nseg]), dim3(256), 0, st, t, norm, clip, lr, (float)alpha, (float)(1.0 - alpha),
                       (float)eps, 0.f, 0.f);
    OCRL_CHECK_LAUNCH("multi_clip_rmsprop");
    return 0;
}
