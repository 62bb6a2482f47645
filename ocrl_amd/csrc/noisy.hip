// DQN's noisy linear layers (include/ocrl_hip_noisy.h states the arithmetic; noisy.h the arguments): the draw of the factorised noise, the
// perturbed weights and the gradient of the noise scales.  Elementwise and memory-bound: a thread takes one group of four consecutive
// floats of a tensor (one 16-byte load per operand, one 16-byte store; the tensors' bases are 16-byte aligned, their rows are not, so the
// group is cut from the flat tensor and (o, i) follow from one division per thread), the ragged last group of a tensor goes float by float.
// Built with -ffp-contract=off like sprite_env.hip; the products and sums below are spelled with the round-to-nearest intrinsics besides,
// which are never fused.
#include "noisy.h"

namespace {
constexpr int NB = 256;            // threads of a workgroup

__global__ __launch_bounds__(NB) void noisy_factors_kernel(NoisyFactorArgs a) {
    const int e = blockIdx.x * NB + threadIdx.x;
    if (e >= a.lay.total) return;
    int l = 0, s = 0, i = e, n = a.in[0];
#pragma unroll
    for (int k = 0; k < NOISY_MAX_LAYERS; ++k) {               // the block of `factors` e lies in: static indices into the arguments
        if (k < a.n_layers && e >= a.lay.fin[k]) {
            l = k;
            s = e >= a.lay.fout[k];
            i = e - (s ? a.lay.fout[k] : a.lay.fin[k]);
            n = s ? a.out[k] : a.in[k];
        }
    }
    float f = 0.f;                                             // the padding of a block
    if (i < n) {
        float g;
        if (a.eps) {
            g = a.eps[e];
        } else {
            const uint64_t ctr = ((a.draw & 0xffffffffull) << 32) | ((uint64_t)l << 28) | ((uint64_t)s << 27) | (uint64_t)i;
            const uint2 b = rng_bits4(a.seed, SITE_NOISY, ctr);
            g = sqrtf(-2.0f * __logf(u01_24(b.x))) * __cosf(6.2831853f * u01_24(b.y));       // slot_eps's Gaussian (elementwise.hip)
        }
        f = copysignf(sqrtf(fabsf(g)), g);
    }
    a.factors[e] = f;
}

template <bool GRAD>
__device__ __forceinline__ float noisy_value(float a, float s, float p) {
    return GRAD ? __fmul_rn(a, p) : __fadd_rn(a, __fmul_rn(s, p));
}

// GRAD == false: dst = a + s * p (a = mu, s = sigma); GRAD == true: dst = a * p (a = dw_eff).  p = f_out[o] * f_in[i], f_out[o] for a bias.
template <bool GRAD>
__global__ __launch_bounds__(NB) void noisy_apply_kernel(NoisyArgs a) {
    const long long blk = blockIdx.x;
    NoisyLayer L = a.lay[0];
    bool bias = false;
    long long b0 = 0;
#pragma unroll
    for (int k = 0; k < NOISY_MAX_LAYERS; ++k) {               // the tensor of this workgroup: uniform, static indices into the arguments
        if (k < a.n_layers && blk >= a.first[2 * k]) {
            L = a.lay[k];
            bias = blk >= a.first[2 * k + 1];
            b0 = bias ? a.first[2 * k + 1] : a.first[2 * k];
        }
    }
    const long long numel = bias ? (long long)L.out : (long long)L.out * L.in;
    const long long e0 = ((blk - b0) * NB + threadIdx.x) * 4;
    if (e0 >= numel) return;
    const float* __restrict__ A = bias ? L.a_b : L.a_w;
    const float* __restrict__ S = bias ? L.s_b : L.s_w;
    float* __restrict__ D = bias ? L.dst_b : L.dst_w;
    const float* __restrict__ fin = a.factors + L.fin;
    const float* __restrict__ fout = a.factors + L.fout;
    const int cnt = numel - e0 < 4 ? (int)(numel - e0) : 4;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) p[j] = fout[e0 + j];
    } else {
        long long o;
        int i;
        if (numel <= (1ll << 32)) {                            // e0 < 2^32: one 32-bit division
            o = (unsigned)e0 / (unsigned)L.in;
            i = (int)((unsigned)e0 % (unsigned)L.in);
        } else {
            o = e0 / L.in;
            i = (int)(e0 % L.in);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) p[j] = __fmul_rn(fout[o], fin[i]);
            if (++i == L.in) { i = 0; ++o; }
        }
    }
    if (cnt == 4) {
        const float4 va = *reinterpret_cast<const float4*>(A + e0);
        float4 vs = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!GRAD) vs = *reinterpret_cast<const float4*>(S + e0);
        float4 r;
        r.x = noisy_value<GRAD>(va.x, vs.x, p[0]);
        r.y = noisy_value<GRAD>(va.y, vs.y, p[1]);
        r.z = noisy_value<GRAD>(va.z, vs.z, p[2]);
        r.w = noisy_value<GRAD>(va.w, vs.w, p[3]);
        *reinterpret_cast<float4*>(D + e0) = r;
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < cnt) D[e0 + j] = noisy_value<GRAD>(A[e0 + j], GRAD ? 0.f : S[e0 + j], p[j]);
    }
}
}  // namespace

NoisyFactorLayout noisy_factor_layout(const ocrl_noisy_desc* d) {
    NoisyFactorLayout y{};
    int off = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        y.fin[l] = off; off += (d->in[l] + 3) & ~3;
        y.fout[l] = off; off += (d->out[l] + 3) & ~3;
    }
    y.total = off;
    return y;
}

int noisy_factors_launch(const NoisyFactorArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(noisy_factors_kernel, dim3(cdiv(a.lay.total, NB)), dim3(NB), 0, st, a);
    OCRL_CHECK_LAUNCH("noisy_factors");
    return 0;
}

int noisy_apply_launch(NoisyArgs& a, bool grad, hipStream_t st) {
    long long blocks = 0;
    for (int l = 0; l < a.n_layers; ++l) {
        a.first[2 * l] = blocks;
        blocks += cdiv(((long long)a.lay[l].out * a.lay[l].in + 3) / 4, NB);
        a.first[2 * l + 1] = blocks;
        blocks += cdiv((a.lay[l].out + 3) / 4, NB);
    }
    a.first[2 * a.n_layers] = blocks;
    OCRL_REQUIRE(blocks < (1ll << 31), "noisy: %lld workgroups leave the range of one launch", blocks);
    if (grad) hipLaunchKernelGGL(noisy_apply_kernel<true>, dim3((unsigned)blocks), dim3(NB), 0, st, a);
    else hipLaunchKernelGGL(noisy_apply_kernel<false>, dim3((unsigned)blocks), dim3(NB), 0, st, a);
    OCRL_CHECK_LAUNCH(grad ? "noisy_grad" : "noisy_perturb");
    return 0;
}
