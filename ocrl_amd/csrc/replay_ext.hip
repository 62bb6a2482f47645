// DQN's replay extensions on the device (include/ocrl_hip_replay.h): n-step returns read from the ring and the proportional priority
// store.  The TD step with double Q-learning, per-row discounts and importance weights is dqn.hip's dqn_td with its options compiled in.
//   replay_sample_nstep  one thread per row: a slot whose n-step window is stored and an environment, from the counter RNG
//   replay_gather_nstep  workgroup (b, chunk) as replay_gather; every thread walks the window's dones (uniform reads), so that the
//                        workgroup knows which slot holds the observation after the return
//   per_*                the priority store: uint32 leaves under levels of exact uint64 sums with fan-out 64.  A wave owns a node: lane i
//                        reads child i, the wave adds (rebuild) or scans (the sampler's descent).  Integer sums: no order to fix.
// No atomics.  A workgroup that rebuilds several levels in turn puts a barrier between them: the nodes of a level are written and read
// by waves of that one workgroup.
#include "replay_ext.h"

namespace {

__device__ __forceinline__ long long below(uint32_t w, long long m) { return (long long)(((unsigned long long)w * (unsigned long long)m) >> 32); }

__global__ __launch_bounds__(256) void replay_sample_nstep_kernel(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full,
                                                                  int n, long long* __restrict__ idx) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    const uint2 w = rng_bits4_keyed(rng_key(seed, SITE_REPLAY_SAMPLE, (uint32_t)update), (uint32_t)r);
    const long long t = full ? (pos + 1 + below(w.x, N - n)) % N : below(w.x, pos - n + 1);
    idx[r] = t * E + below(w.y, E);
}

// Workgroup (b, c) as dqn.hip's replay_gather_kernel.  The walk reads at most n rewards and dones of one environment, the same for every
// thread of the workgroup; its products and sums are single fp32 roundings in the written order.
template <typename V>
__global__ __launch_bounds__(256) void replay_gather_nstep_kernel(ReplayGatherNstepArgs a) {
    const ReplayGatherArgs& g = a.g;
    const int b = blockIdx.x;
    const long long total = (long long)g.N * g.E;
    long long id = g.idx[b];
    id = id < 0 ? 0 : id >= total ? total - 1 : id;
    const long long t = id / g.E, e = id - t * g.E;
    float R = 0.f, disc = 1.f;
    unsigned char stop = 0;
    long long tn = t;                                       // ends as (t + m) % N
    {
        // each product and sum is one fp32 rounding: hipcc would fuse R + disc * r otherwise (its __fmul_rn / __fadd_rn are plain
        // operators and do not stop that)
#pragma clang fp contract(off)
        for (int k = 0; k < a.n; ++k) {
            const long long idk = tn * g.E + e;
            const float term = disc * g.rewards[idk];
            R = R + term;
            disc = disc * a.gamma;
            tn = tn + 1 == g.N ? 0 : tn + 1;
            stop = g.dones[idk];
            if (stop) break;
        }
    }
    const V* src = reinterpret_cast<const V*>(g.obs + id * g.S);
    const V* nxt = reinterpret_cast<const V*>(g.obs + (tn * g.E + e) * g.S);
    V* d0 = reinterpret_cast<V*>(g.obs_out + (long long)b * g.S);
    V* d1 = reinterpret_cast<V*>(g.next_out + (long long)b * g.S);
    const long long nv = g.S / (long long)sizeof(V);
    for (long long v = (long long)blockIdx.y * 256 + threadIdx.x; v < nv; v += (long long)gridDim.y * 256) {
        d0[v] = src[v];
        d1[v] = nxt[v];
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        g.actions_out[b] = g.actions[id];
        g.rewards_out[b] = R;
        g.dones_out[b] = stop;
        a.discounts_out[b] = disc;
    }
}

// ---- the priority store
constexpr int PER_WAVES = 16;                               // waves of the single-workgroup kernels (1024 threads)

// child i of level l's nodes: a leaf (l == 0) or a sum; 0 past the level's end
__device__ __forceinline__ unsigned long long per_child(const PerTree& T, int l, long long i) {
    if (i >= T.n[l]) return 0ull;
    return l == 0 ? (unsigned long long)T.leaves[i] : T.lvl[l - 1][i];
}

// all 64 lanes of a wave: node j of level l >= 1 = the sum of its children
__device__ __forceinline__ void per_rebuild(const PerTree& T, int l, long long j) {
    const int lane = threadIdx.x & 63;
    unsigned long long v = per_child(T, l - 1, j * PER_FAN + lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) T.lvl[l - 1][j] = v;
}

__device__ __forceinline__ uint32_t per_quant(float ad, float alpha, float eps) {
#pragma clang fp contract(off)
    float v = fabsf(ad) + eps;
    if (alpha == 0.f) v = 1.f;
    else if (alpha != 1.f) v = powf(v, alpha);
    const float scaled = v * 65536.f;
    const float x = scaled + 0.5f;
    if (!(x < 16777216.f)) return PER_Q_MAX;                // large, infinite or NaN
    if (!(x >= 1.f)) return 1u;
    return (uint32_t)floorf(x);
}

__global__ __launch_bounds__(256) void per_init_kernel(PerTree T) {
    uint32_t* w = T.leaves;                                 // the buffer's first word
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T.words; i += (long long)gridDim.x * 256) w[i] = i == T.n[0] ? PER_Q_ONE : 0u;
}

// wave (blockIdx.x * 4 + wave) owns level-1 node j0 + that: writes its leaves inside [first, last] and sums all 64
__global__ __launch_bounds__(256) void per_set_leaves_kernel(PerTree T, long long first, long long last, int mode, long long j0, long long j1) {
    const int lane = threadIdx.x & 63;
    const long long j = j0 + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j > j1) return;                                     // the whole wave
    const long long i = j * PER_FAN + lane;
    unsigned long long v = 0ull;
    if (i < T.n[0]) {
        if (i >= first && i <= last) {
            const uint32_t q = mode ? *T.maxq : 0u;
            T.leaves[i] = q;
            v = q;
        } else {
            v = T.leaves[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) T.lvl[0][j] = v;
}

// one workgroup: levels from .. L above the nodes lo .. hi of level from - 1, a level at a time
__global__ __launch_bounds__(1024) void per_up_range_kernel(PerTree T, int from, long long lo, long long hi) {
    const int wave = threadIdx.x >> 6;
    for (int l = from; l <= T.L; ++l) {
        lo /= PER_FAN; hi /= PER_FAN;
        for (long long j = lo + wave; j <= hi; j += PER_WAVES) per_rebuild(T, l, j);
        __syncthreads();
    }
}

// one workgroup: the leaves of the batch and maxq, then the levels above them.  A level with no more nodes than the batch has rows is
// rebuilt whole (the top node once, not once per row).
__global__ __launch_bounds__(1024) void per_update_kernel(PerTree T, const long long* __restrict__ idx, const float* __restrict__ abs_td, int B, float alpha,
                                                          float eps) {
    __shared__ uint32_t red[1024];
    const int tid = threadIdx.x, wave = tid >> 6;
    uint32_t mx = 0u;
    for (int b = tid; b < B; b += 1024) {
        const uint32_t q = per_quant(abs_td[b], alpha, eps);
        mx = q > mx ? q : mx;
        long long id = idx[b];
        id = id < 0 ? 0 : id >= T.n[0] ? T.n[0] - 1 : id;
        if (T.leaves[id] != 0u) T.leaves[id] = q;
    }
    red[tid] = mx;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
        __syncthreads();
    }
    if (tid == 0 && red[0] > *T.maxq) *T.maxq = red[0];
    for (int l = 1; l <= T.L; ++l) {
        if (T.n[l] <= B) {
            for (long long j = wave; j < T.n[l]; j += PER_WAVES) per_rebuild(T, l, j);
        } else {
            for (int b = wave; b < B; b += PER_WAVES) {
                long long id = idx[b];
                id = id < 0 ? 0 : id >= T.n[0] ? T.n[0] - 1 : id;
                per_rebuild(T, l, id >> (6 * l));
            }
        }
        __syncthreads();
    }
}

// wave (blockIdx.x * 4 + wave) owns row r: from the total down, lane i holds child i's inclusive prefix; the first lane whose prefix
// exceeds the target is the child the target falls into.  weights[r] takes the leaf's q as a float (exact) for per_weights_kernel.
__global__ __launch_bounds__(256) void per_sample_kernel(PerTree T, unsigned long long seed, unsigned long long update, int B,
                                                         const unsigned long long* __restrict__ targets, long long* __restrict__ idx,
                                                         float* __restrict__ weights) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;                                     // the whole wave
    const unsigned long long total = T.lvl[T.L - 1][0];
    if (total == 0ull) {
        if (lane == 0) { idx[r] = -1; weights[r] = 0.f; }
        return;
    }
    unsigned long long target;
    if (targets) {
        target = targets[r] < total ? targets[r] : total - 1;
    } else {
        const uint2 w = rng_bits4_keyed(rng_key(seed, SITE_PER_SAMPLE, (uint32_t)update), (uint32_t)r);
        target = __umul64hi(((unsigned long long)w.x << 32) | (unsigned long long)w.y, total);
    }
    long long j = 0;
    for (int l = T.L - 1; l >= 0; --l) {                    // the children's level
        const unsigned long long v = per_child(T, l, j * PER_FAN + lane);
        unsigned long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const unsigned long long mask = __ballot(incl > target);
        const int sel = mask ? __ffsll((long long)mask) - 1 : 63;      // mask is never empty while the sums are those of the leaves
        target -= __shfl(incl - v, sel, 64);
        j = j * PER_FAN + sel;
        j = j < T.n[l] ? j : T.n[l] - 1;
    }
    if (lane == 0) {
        idx[r] = j;
        weights[r] = (float)T.leaves[j];
    }
}

// one workgroup: q_min of the batch, then weights[r] = (q_min / q_r)^beta in place
__global__ __launch_bounds__(256) void per_weights_kernel(float* __restrict__ weights, int B, float beta) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float mn = 3.0e38f;
    for (int b = tid; b < B; b += 256) {
        const float q = weights[b];
        if (q > 0.f && q < mn) mn = q;
    }
    red[tid] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fminf(red[tid], red[tid + o]);
        __syncthreads();
    }
    mn = red[0];
    for (int b = tid; b < B; b += 256) {
        const float q = weights[b];
        float w = 0.f;
        if (q > 0.f) {
            const float ratio = __fdiv_rn(mn, q);
            w = beta == 0.f ? 1.f : beta == 1.f ? ratio : powf(ratio, beta);
        }
        weights[b] = w;
    }
}

}  // namespace

int replay_sample_nstep_launch(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, int n, long long* idx,
                               hipStream_t st) {
    hipLaunchKernelGGL(replay_sample_nstep_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, seed, update, B, N, E, pos, full, n, idx);
    OCRL_CHECK_LAUNCH("replay_sample_nstep");
    return 0;
}
int replay_gather_nstep_launch(const ReplayGatherNstepArgs& a, hipStream_t st) {
    const bool wide = a.g.S % 16 == 0;
    const long long nv = a.g.S / (wide ? 16 : 4);
    const int chunks = nv > 256 * 64 ? 64 : cdiv(nv, 256);
    if (wide)
        hipLaunchKernelGGL(replay_gather_nstep_kernel<uint4>, dim3(a.g.B, chunks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(replay_gather_nstep_kernel<uint32_t>, dim3(a.g.B, chunks), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("replay_gather_nstep");
    return 0;
}
int per_init_launch(const PerTree& t, hipStream_t st) {
    const int blocks = t.words > 256LL * 4096 ? 4096 : cdiv(t.words, 256);
    hipLaunchKernelGGL(per_init_kernel, dim3(blocks), dim3(256), 0, st, t);
    OCRL_CHECK_LAUNCH("per_init");
    return 0;
}
int per_set_range_launch(const PerTree& t, long long first, long long count, int mode, hipStream_t st) {
    const long long last = first + count - 1, j0 = first / PER_FAN, j1 = last / PER_FAN;
    hipLaunchKernelGGL(per_set_leaves_kernel, dim3(cdiv(j1 - j0 + 1, 4)), dim3(256), 0, st, t, first, last, mode, j0, j1);
    OCRL_CHECK_LAUNCH("per_set_leaves");
    if (t.L >= 2) {
        hipLaunchKernelGGL(per_up_range_kernel, dim3(1), dim3(1024), 0, st, t, 2, j0, j1);
        OCRL_CHECK_LAUNCH("per_up_range");
    }
    return 0;
}
int per_update_launch(const PerTree& t, const long long* idx, const float* abs_td, int B, float alpha, float eps, hipStream_t st) {
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(1024), 0, st, t, idx, abs_td, B, alpha, eps);
    OCRL_CHECK_LAUNCH("per_update");
    return 0;
}
int per_sample_launch(const PerTree& t, unsigned long long seed, unsigned long long update, int B, float beta, const unsigned long long* targets,
                      long long* idx, float* weights, hipStream_t st) {
    hipLaunchKernelGGL(per_sample_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, t, seed, update, B, targets, idx, weights);
    OCRL_CHECK_LAUNCH("per_sample");
    hipLaunchKernelGGL(per_weights_kernel, dim3(1), dim3(256), 0, st, weights, B, beta);
    OCRL_CHECK_LAUNCH("per_weights");
    return 0;
}
