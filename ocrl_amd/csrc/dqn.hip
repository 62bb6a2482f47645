// DQN on the device (include/ocrl_hip_dqn.h): the collection step, the fused TD step and the replay ring's sampling and batch read.
// The Q head is a chain of small Linear layers and runs on the actor-critic head's tile code (acnet_tile.h): a workgroup owns 16 batch
// rows, the chain's activations stay in LDS and the Q values of the tile end in `lg`.
//   dqn_act           the forward with the choice in the same launch: lane r of a tile chooses for row r (eps_greedy of qhead_tile.h)
//   dqn_td            forward, TD target, Huber loss, dQ and the backward per row tile in one kernel; Q and the layer cotangents never
//                     leave LDS.  Partial dw go to the workgroup's slab, the three scalar sums to its row of scal_slab.  Two
//                     instantiations: the plain step, and the one with the optional inputs of ocrl_hip_replay.h (double Q-learning,
//                     per-row discounts, importance weights, |delta| out): the same tiles, the same order of every sum
//   head_scalars      loss, mean Q[a], mean y from the slabs' partial sums, in slab order (dw is folded by acnet_reduce); C51's and the
//                     classifier's three scalars too
//   replay_gather     obs, next_obs, actions, rewards, dones of B transitions: workgroup (b, chunk) copies a stretch of both observations
//   replay_sample     one thread per row: a valid slot and an environment from the counter RNG
// Order of every sum: acnet.hip's for the layers and the slabs; a tile's scalar terms are added in row order, the tiles of a slab in tile
// order, the slabs in slab order.  No atomics.
#include "qhead_tile.h"

namespace {

// Forward of a tile, then lane r < rows chooses for row r from the Q values in LDS (A <= 64: the scan is serial in a).
__global__ __launch_bounds__(256) void dqn_act_kernel(AcnetArgs p, DqnActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    fwd_tile(p, row0, rows, buf, lg, nullptr);          // ends on a barrier: lg is complete (no value head: vl is not touched)
    const int r = threadIdx.x;
    if (r < rows) eps_greedy(lg + r * LA, p.A, row0 + r, s);
}

__global__ __launch_bounds__(256) void dqn_act_uniforms_kernel(unsigned long long seed, unsigned long long row_offset, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 w = rng_bits4(seed, SITE_DQN_ACT, row_offset + (unsigned long long)i);
    out[2 * i] = unit24(w.x >> 8);
    out[2 * i + 1] = unit24(w.y >> 8);
}

// The TD step of one tile after its forward: thread r < 16 owns row r.  Replaces the Q values in lg by dL/dQ (L = the mean loss) and adds
// the row's three terms (Huber loss, Q[a], y) to the slab's partial sums.  EXT compiles the target's optional inputs in (ocrl_hip_replay.h);
// where one is not given the operations are the plain step's own, in its order.
template <bool EXT>
__device__ void td_rows(const AcnetArgs& p, const DqnTdArgs& s, long long row0, int rows, bool first, float* lg, float (*rs)[3]) {
    const int r = threadIdx.x;
    if (r < TR) {
        float t[3] = {0.f, 0.f, 0.f};
        float* z = lg + r * LA;
        const int A = p.A;
        float g = 0.f;
        int act = 0;
        if (r < rows) {
            const long long row = row0 + r;
            long long a = s.actions[row];
            act = (int)(a < 0 ? 0 : a >= A ? A - 1 : a);
            const float q = z[act];
            float y = s.rewards[row];
            if (!s.dones[row]) {                        // a select: next_q of a finished row is not read
                const float* nq = s.next_q + row * A;
                float m = nq[0];
                if (EXT && s.next_q_online) {           // the target's value where the online network has its (lowest) maximum
                    const float* on = s.next_q_online + row * A;
                    float mo = on[0];
                    int best = 0;
                    for (int k = 1; k < A; ++k)
                        if (on[k] > mo) { mo = on[k]; best = k; }
                    m = nq[best];
                } else {
                    for (int k = 1; k < A; ++k) m = nq[k] > m ? nq[k] : m;
                }
                const float disc = EXT && s.discounts ? s.discounts[row] : s.gamma;
                y += disc * m;
            }
            const float delta = q - y, ad = fabsf(delta);
            float l = ad < 1.f ? 0.5f * delta * delta : ad - 0.5f;
            float c = fminf(fmaxf(delta, -1.f), 1.f);
            if (EXT && s.weights) {
                const float w = s.weights[row];
                l = w * l;
                c = w * c;
            }
            t[0] = l; t[1] = q; t[2] = y;
            g = c / (float)p.B;
            if (EXT && s.abs_td) s.abs_td[row] = ad;
        }
        for (int k = 0; k < A; ++k) z[k] = 0.f;
        z[act] = g;
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[r][j] = t[j];
    }
    __syncthreads();
    tile_scalars<3>(rs, first, p.scal_slab);
}

template <bool EXT>
__global__ __launch_bounds__(256) void dqn_td_kernel(AcnetArgs p, DqnTdArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float rs[TR][3];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        fwd_tile(p, row0, rows, buf, lg, nullptr);
        td_rows<EXT>(p, s, row0, rows, first, lg, rs);
        bwd_tile(p, row0, rows, first, buf, lg, nullptr);
        __syncthreads();
    }
}

// out[j] = the slabs' partial sums of scalar j in slab order, over B; `count2` leaves scalar 2 a count (the classifier's valid rows)
__global__ __launch_bounds__(64) void head_scalars_kernel(const float* __restrict__ scal_slab, int S, int B, int count2, float* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= 3) return;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += scal_slab[k * 8 + j];
    out[j] = count2 && j == 2 ? s : s / (float)B;
}

// Workgroup (b, c): transition b, units c * 256 + t, + 256 gridDim.y, ... of its two observations; V is the access (16 or 4 bytes).
template <typename V>
__global__ __launch_bounds__(256) void replay_gather_kernel(ReplayGatherArgs g) {
    const int b = blockIdx.x;
    const long long total = (long long)g.N * g.E;
    long long id = g.idx[b];
    id = id < 0 ? 0 : id >= total ? total - 1 : id;
    const long long t = id / g.E, e = id - t * g.E, tn = t + 1 == g.N ? 0 : t + 1;
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
        g.rewards_out[b] = g.rewards[id];
        g.dones_out[b] = g.dones[id];
    }
}

__device__ __forceinline__ long long below(uint32_t w, long long m) { return (long long)(((unsigned long long)w * (unsigned long long)m) >> 32); }

__global__ __launch_bounds__(256) void replay_sample_kernel(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full,
                                                            long long* __restrict__ idx) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    const uint2 w = rng_bits4_keyed(rng_key(seed, SITE_REPLAY_SAMPLE, (uint32_t)update), (uint32_t)r);
    const long long t = full ? (pos + 1 + below(w.x, N - 1)) % N : below(w.x, pos);
    idx[r] = t * E + below(w.y, E);
}

}  // namespace

int dqn_act_launch(const AcnetArgs& a, const DqnActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(dqn_act_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, s);
    OCRL_CHECK_LAUNCH("dqn_act");
    return 0;
}
int dqn_act_uniforms_launch(unsigned long long seed, unsigned long long row_offset, long long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(dqn_act_uniforms_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, seed, row_offset, n, out);
    OCRL_CHECK_LAUNCH("dqn_act_uniforms");
    return 0;
}
int dqn_td_launch(const AcnetArgs& a, const DqnTdArgs& s, bool ext, hipStream_t st) {
    if (ext)
        hipLaunchKernelGGL(dqn_td_kernel<true>, dim3(a.S), dim3(256), 0, st, a, s);
    else
        hipLaunchKernelGGL(dqn_td_kernel<false>, dim3(a.S), dim3(256), 0, st, a, s);
    OCRL_CHECK_LAUNCH(ext ? "dqn_td_ext" : "dqn_td");
    return 0;
}
int head_scalars_launch(const float* scal_slab, int S, int B, bool count2, float* out, hipStream_t st) {
    hipLaunchKernelGGL(head_scalars_kernel, dim3(1), dim3(64), 0, st, scal_slab, S, B, count2 ? 1 : 0, out);
    OCRL_CHECK_LAUNCH("head_scalars");
    return 0;
}
int replay_gather_launch(const ReplayGatherArgs& g, hipStream_t st) {
    const bool wide = g.S % 16 == 0;
    const long long nv = g.S / (wide ? 16 : 4);
    const int chunks = nv > 256 * 64 ? 64 : cdiv(nv, 256);
    if (wide)
        hipLaunchKernelGGL(replay_gather_kernel<uint4>, dim3(g.B, chunks), dim3(256), 0, st, g);
    else
        hipLaunchKernelGGL(replay_gather_kernel<uint32_t>, dim3(g.B, chunks), dim3(256), 0, st, g);
    OCRL_CHECK_LAUNCH("replay_gather");
    return 0;
}
int replay_sample_launch(unsigned long long seed, unsigned long long update, int B, int N, int E, int pos, int full, long long* idx, hipStream_t st) {
    hipLaunchKernelGGL(replay_sample_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, seed, update, B, N, E, pos, full, idx);
    OCRL_CHECK_LAUNCH("replay_sample");
    return 0;
}
