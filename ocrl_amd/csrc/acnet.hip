// Actor-critic head and PPO minibatch step (sb3s/custom_acnets.py:8-96 plus the action / value heads and the loss that
// stable-baselines3's ActorCriticPolicy and PPO.train put on it; include/ocrl_hip.h ocrl_acnet_*, ocrl_gae).
// Chains of small Linear layers: shared trunk -> policy trunk -> logits, shared trunk -> value trunk -> values.  One workgroup
// (4 waves) owns a tile of 16 batch rows and walks the whole chain with the tile's activations in LDS; every product runs on
// v_mfma_f32_16x16x4_f32 (exact fp32), weights are streamed from global memory straight into the B operand (the first layer's
// [width, F] never has to fit LDS), and the features are read from global memory as the A operand.
//   acnet_fwd        one launch: features -> latents, logits, values; with `saved` set, each trunk layer's output also goes to
//                    the workspace (what dW needs)
//   acnet_bwd        cotangents of latents / logits / values -> per-slab partial dW, db and dfeatures
//   acnet_ppo        forward, log-softmax, log-prob gather, entropy, ratio, clipping, the loss sums and their gradient, and the
//                    backward, per row tile in one kernel; logits, probabilities and layer cotangents never leave LDS
//   acnet_a2c        the same for A2C's loss (no ratio, no clipping): -adv log_prob, the squared value error and the entropy
//   acnet_act        the forward with the rollout's tail in the same launch: log-softmax, the action (drawn from one 24-bit uniform
//                    per row, or the argmax) and its log-probability; one lane owns a row's tail (include/ocrl_hip.h ocrl_acnet_act)
//   acnet_reduce     dw = sum of the slabs in slab order; the six PPO (four A2C) scalars from their partial sums
//   acnet_adv_stats  mean and 1 / (std + 1e-8) (unbiased std) of the advantages, one workgroup, fixed order
//   gae              generalised advantage estimation, one thread per environment walking T backwards
// Order of every sum: a layer output is acc0 + acc1 + bias with acc0 / acc1 the MFMA chains over the even / odd 16-wide k chunks in
// ascending k; workgroup s accumulates its tiles s, s + S, ... into slab s in that order; slabs are summed in slab order.  Nothing
// depends on timing (no atomics), and a row's forward result does not depend on which tile or position it sits in.
// The tile steps themselves (lin_fwd_tile, fwd_tile, lin_bwd_tile, bwd_tile) are acnet_tile.h, which dqn.hip shares.
#include "acnet_tile.h"

namespace {

__global__ __launch_bounds__(256) void acnet_fwd_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    fwd_tile(p, row0, rows, buf, lg, vl);
}

// the uniform of global row `idx` of a sampling stream: the top 24 bits of one counter draw, in [0, 1)
__host__ __device__ inline float act_uniform(unsigned long long seed, unsigned long long idx) {
    const uint32_t key = rng_key(seed, SITE_ACNET_ACT, (uint32_t)(idx >> 32));
    return (float)(rng_bits1_keyed(key, (uint32_t)idx) >> 8) * (1.f / 16777216.f);
}

// Forward of a tile, then lane r < rows finishes row r from the logits and the value in LDS (A <= 64: the tail is serial in a).
__global__ __launch_bounds__(256) void acnet_act_kernel(AcnetArgs p, AcnetActArgs s) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    const long long row0 = (long long)blockIdx.x * TR;
    const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
    fwd_tile(p, row0, rows, buf, lg, vl);               // ends on a barrier: lg and vl are complete
    const int r = threadIdx.x;
    if (r >= rows) return;
    const long long row = row0 + r;
    const float* z = lg + r * LA;
    const int A = p.A;
    float m = z[0];
    int best = 0;
    for (int a = 1; a < A; ++a)
        if (z[a] > m) { m = z[a]; best = a; }           // strict: the lowest index of the maximum
    float se = 0.f;
    for (int a = 0; a < A; ++a) se += expf(z[a] - m);
    const float lse = m + logf(se);
    int act = best;
    if (!s.deterministic) {
        const float u = s.uniforms ? s.uniforms[row] : act_uniform(s.seed, s.row_offset + (unsigned long long)row);
        float c = 0.f;
        act = 0;
        for (int a = 0; a + 1 < A; ++a) {
            c += expf(z[a] - lse);
            act += c <= u ? 1 : 0;
        }
    }
    s.actions[row] = act;
    s.log_prob[row] = z[act] - lse;
}

__global__ __launch_bounds__(256) void acnet_act_uniforms_kernel(unsigned long long seed, unsigned long long row_offset, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = act_uniform(seed, row_offset + (unsigned long long)i);
}

__global__ __launch_bounds__(256) void acnet_bwd_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        if (p.A > 0) {
            for (int e = threadIdx.x; e < TR * p.A; e += blockDim.x) {
                const int r = e / p.A, a = e - r * p.A;
                lg[r * LA + a] = (p.dlogits && r < rows) ? p.dlogits[(row0 + r) * p.A + a] : 0.f;
            }
            if (threadIdx.x < TR) vl[threadIdx.x] = (p.dvalues && (int)threadIdx.x < rows) ? p.dvalues[row0 + threadIdx.x] : 0.f;
        }
        __syncthreads();
        bwd_tile(p, row0, rows, tile == (int)blockIdx.x, buf, lg, vl);
        __syncthreads();
    }
}

// The PPO minibatch step of one tile after its forward: thread r < 16 owns row r.  Replaces the logits in lg by dL/dlogits and the values
// in vl by dL/dvalues (L = the mean loss: every row carries 1 / B), and adds the row's six terms to the slab's partial sums.
__device__ void ppo_rows(const AcnetArgs& p, long long row0, int rows, bool first, float* lg, float* vl, float (*rs)[6]) {
    const int r = threadIdx.x;
    if (r < TR) {
        float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float* z = lg + r * LA;
        if (r < rows) {
            const long long row = row0 + r;
            const int A = p.A;
            float m = z[0];
            for (int a = 1; a < A; ++a) m = fmaxf(m, z[a]);
            float se = 0.f;
            for (int a = 0; a < A; ++a) se += expf(z[a] - m);
            const float lse = m + logf(se);
            float H = 0.f;
            for (int a = 0; a < A; ++a) { const float lq = z[a] - lse; H -= expf(lq) * lq; }
            long long act = p.actions[row];
            act = act < 0 ? 0 : act >= A ? A - 1 : act;
            const float logp = z[act] - lse, old = p.old_logp[row];
            float adv = p.adv[row];
            if (p.norm) adv = (adv - p.stats[0]) * p.stats[1];
            const float lr = logp - old, ratio = expf(lr), lo = 1.f - p.clip, hi = 1.f + p.clip;
            const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, lo), hi);
            const bool inside = ratio >= lo && ratio <= hi;
            // d min(s1, s2) / d logp: s1 alone carries a gradient once the clamp is active; a tie shares it evenly (torch.min)
            const float dmin = inside ? s1 : s1 < s2 ? s1 : s1 == s2 ? 0.5f * s1 : 0.f;
            const float v = vl[r], dv = v - p.ret[row], invB = 1.f / (float)p.B;
            t[0] = -fminf(s1, s2); t[1] = dv * dv; t[2] = -H; t[3] = (ratio - 1.f) - lr; t[4] = fabsf(ratio - 1.f) > p.clip ? 1.f : 0.f;
            for (int a = 0; a < A; ++a) {
                const float lq = z[a] - lse, q = expf(lq);
                const float dlogp = (a == act ? 1.f : 0.f) - q;
                z[a] = invB * (-dmin * dlogp + p.ent_coef * q * (lq + H));
            }
            vl[r] = invB * p.vf_coef * 2.f * dv;
        } else {
            for (int a = 0; a < p.A; ++a) z[a] = 0.f;
            vl[r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) rs[r][j] = t[j];
    }
    __syncthreads();
    tile_scalars<5>(rs, first, p.scal_slab);
}

__global__ __launch_bounds__(256) void acnet_ppo_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    __shared__ float rs[TR][6];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        fwd_tile(p, row0, rows, buf, lg, vl);
        ppo_rows(p, row0, rows, first, lg, vl, rs);
        bwd_tile(p, row0, rows, first, buf, lg, vl);
        __syncthreads();
    }
}

// The A2C step of one tile after its forward, in the shape of ppo_rows: lse, q_a and H are computed by the same operations.  Replaces
// the logits in lg by dL/dlogits and the values in vl by dL/dvalues and adds the row's three terms (-adv log_prob, (v - ret)^2, -H) to the
// slab's partial sums.
__device__ void a2c_rows(const AcnetArgs& p, long long row0, int rows, bool first, float* lg, float* vl, float (*rs)[3]) {
    const int r = threadIdx.x;
    if (r < TR) {
        float t[3] = {0.f, 0.f, 0.f};
        float* z = lg + r * LA;
        if (r < rows) {
            const long long row = row0 + r;
            const int A = p.A;
            float m = z[0];
            for (int a = 1; a < A; ++a) m = fmaxf(m, z[a]);
            float se = 0.f;
            for (int a = 0; a < A; ++a) se += expf(z[a] - m);
            const float lse = m + logf(se);
            float H = 0.f;
            for (int a = 0; a < A; ++a) { const float lq = z[a] - lse; H -= expf(lq) * lq; }
            long long act = p.actions[row];
            act = act < 0 ? 0 : act >= A ? A - 1 : act;
            const float logp = z[act] - lse;
            float adv = p.adv[row];
            if (p.norm) adv = (adv - p.stats[0]) * p.stats[1];
            const float v = vl[r], dv = v - p.ret[row], invB = 1.f / (float)p.B;
            t[0] = -(adv * logp); t[1] = dv * dv; t[2] = -H;
            for (int a = 0; a < A; ++a) {
                const float lq = z[a] - lse, q = expf(lq);
                const float dlogp = (a == act ? 1.f : 0.f) - q;
                z[a] = invB * (-adv * dlogp + p.ent_coef * q * (lq + H));
            }
            vl[r] = invB * p.vf_coef * 2.f * dv;
        } else {
            for (int a = 0; a < p.A; ++a) z[a] = 0.f;
            vl[r] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) rs[r][j] = t[j];
    }
    __syncthreads();
    tile_scalars<3>(rs, first, p.scal_slab);
}

__global__ __launch_bounds__(256) void acnet_a2c_kernel(AcnetArgs p) {
    __shared__ __attribute__((aligned(16))) float buf[3 * TR * LD];
    __shared__ __attribute__((aligned(16))) float lg[TR * LA];
    __shared__ float vl[TR];
    __shared__ float rs[TR][3];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += p.S) {
        const long long row0 = (long long)tile * TR;
        const int rows = p.B - row0 < TR ? (int)(p.B - row0) : TR;
        const bool first = tile == (int)blockIdx.x;
        fwd_tile(p, row0, rows, buf, lg, vl);
        a2c_rows(p, row0, rows, first, lg, vl, rs);
        bwd_tile(p, row0, rows, first, buf, lg, vl);
        __syncthreads();
    }
}

// scalars: the first three partial sums are policy, value and entropy terms for both losses; PPO carries two more (nsum = 5: approx_kl
// and the clip fraction, outputs 4 and 5), A2C none (nsum = 3: four outputs)
__global__ __launch_bounds__(256) void acnet_reduce_kernel(AcnetReduceArgs r) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < r.total) {
        float s = 0.f;
        for (int k = 0; k < r.S; ++k) s += r.slab[k * r.stride + e];
        int q = 0;
        while (q + 1 < r.np && e >= r.off[q + 1]) ++q;
        r.dst[q][e - r.off[q]] = s;
    }
    if (r.scal_slab && blockIdx.x == 0 && threadIdx.x == 0) {
        float t[5];
        for (int j = 0; j < r.nsum; ++j) {
            float s = 0.f;
            for (int k = 0; k < r.S; ++k) s += r.scal_slab[k * 8 + j];
            t[j] = s / (float)r.B;
        }
        r.scal_out[0] = t[0] + r.ent_coef * t[2] + r.vf_coef * t[1];
        r.scal_out[1] = t[0]; r.scal_out[2] = t[1]; r.scal_out[3] = t[2];
        for (int j = 3; j < r.nsum; ++j) r.scal_out[j + 1] = t[j];
    }
}

// fixed-order block sum: thread t adds elements t, t + 256, ...; the 256 partials are folded in a tree
__device__ float block_sum256(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    block_tree_sum<256>(sh);
    const float s = sh[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(256) void acnet_adv_stats_kernel(const float* __restrict__ adv, int B, float* __restrict__ stats) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int e = threadIdx.x; e < B; e += 256) s += adv[e];
    const float mean = block_sum256(s, sh) / (float)B;
    float q = 0.f;
    for (int e = threadIdx.x; e < B; e += 256) { const float d = adv[e] - mean; q += d * d; }
    const float var = block_sum256(q, sh) / (float)(B - 1);
    if (threadIdx.x == 0) { stats[0] = mean; stats[1] = 1.f / (sqrtf(var) + 1e-8f); }
}

__global__ __launch_bounds__(64) void gae_kernel(const float* __restrict__ rw, const float* __restrict__ val, const float* __restrict__ st,
                                                 const float* __restrict__ lastv, const float* __restrict__ dones, float* __restrict__ adv,
                                                 float* __restrict__ ret, int T, int E, float gamma, float lam) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    float a = 0.f, nv = lastv[e], nt = 1.f - dones[e];
    for (int t = T - 1; t >= 0; --t) {
        const long long q = (long long)t * E + e;
        const float v = val[q];
        const float delta = rw[q] + gamma * nv * nt - v;
        a = delta + gamma * lam * nt * a;
        adv[q] = a;
        ret[q] = a + v;
        nv = v;
        nt = 1.f - st[q];
    }
}

}  // namespace

int acnet_fwd_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_fwd_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_fwd");
    return 0;
}
int acnet_act_launch(const AcnetArgs& a, const AcnetActArgs& s, hipStream_t st) {
    hipLaunchKernelGGL(acnet_act_kernel, dim3(cdiv(a.B, TR)), dim3(256), 0, st, a, s);
    OCRL_CHECK_LAUNCH("acnet_act");
    return 0;
}
int acnet_act_uniforms_launch(unsigned long long seed, unsigned long long row_offset, long long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(acnet_act_uniforms_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, seed, row_offset, n, out);
    OCRL_CHECK_LAUNCH("acnet_act_uniforms");
    return 0;
}
int acnet_bwd_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_bwd_kernel, dim3(a.S), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_bwd");
    return 0;
}
int acnet_ppo_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_ppo_kernel, dim3(a.S), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_ppo");
    return 0;
}
int acnet_a2c_launch(const AcnetArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(acnet_a2c_kernel, dim3(a.S), dim3(256), 0, st, a);
    OCRL_CHECK_LAUNCH("acnet_a2c");
    return 0;
}
int acnet_reduce_launch(const AcnetReduceArgs& r, hipStream_t st) {
    hipLaunchKernelGGL(acnet_reduce_kernel, dim3(cdiv(r.total > 0 ? r.total : 1, 256)), dim3(256), 0, st, r);
    OCRL_CHECK_LAUNCH("acnet_reduce");
    return 0;
}
int acnet_adv_stats_launch(const float* adv, int B, float* stats, hipStream_t st) {
    hipLaunchKernelGGL(acnet_adv_stats_kernel, dim3(1), dim3(256), 0, st, adv, B, stats);
    OCRL_CHECK_LAUNCH("acnet_adv_stats");
    return 0;
}
int acnet_gae_launch(const float* rewards, const float* values, const float* starts, const float* last_values, const float* dones, float* adv, float* ret,
                     int T, int E, float gamma, float lam, hipStream_t st) {
    hipLaunchKernelGGL(gae_kernel, dim3(cdiv(E, 64)), dim3(64), 0, st, rewards, values, starts, last_values, dones, adv, ret, T, E, gamma, lam);
    OCRL_CHECK_LAUNCH("ocrl_gae");
    return 0;
}
