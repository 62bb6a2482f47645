// Global inf-norm gradient clip + Adam on flat fp32 buffers (reference: ocrs/base.py:65-72,
// torch.nn.utils.clip_grad_norm_(…, "inf") and torch.optim.Adam defaults), and the TF-style RMSprop update A2C takes after the same clip.
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
