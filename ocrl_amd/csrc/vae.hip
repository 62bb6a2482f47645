// VAE representation module (ocrs/vaes/vae_module.py, include/ocrl_hip.h ocrl_vae_*): the kernels that are not convolutions or GEMMs.
// The convolutions are the implicit GEMMs of naturecnn.hip (2 x 2 stride 2 in the encoder, 3 x 3 pad 1 on the decoder's small maps),
// conv.hip (3 x 3 pad 1 at 32 x 32 and above) and the library's GEMM (every 1 x 1 convolution and the three Linears).
//
// The maps run NHWC, while _mu / _var read the encoder map flattened in NCHW order and _in_dec's output is reshaped NCHW.  So the
// Linears' weights are permuted when they are packed for a call, never the activations:
//   vae_permute     [R, C HW] <-> [R, HW C] on the columns (_mu, _var) or [C HW, R] <-> [HW C, R] on the rows (_in_dec and its bias)
//   vae_pad_rows    [rows, K] -> [rows_pad, K] with zero rows (the 64 -> C output convolution as a 4-wide GEMM)
//   vae_kl_fwd      latent = eps exp(0.5 logvar) + mu; per-image KL partial -0.5 sum_j (1 + lv - mu^2 - exp(lv)), one workgroup per
//                   image, summed in a fixed tree order; optionally mu copied out as the representation
//   vae_loss        kld = (1/B) sum_b partial[b] in image order; loss = mse + kld_weight kld; metrics = (loss, mse, kld)
//   vae_kl_bwd      (g = d loss, 0 when absent) d mu = d latent + g w mu / B (+ d rep);  d logvar = d latent 0.5 eps exp(0.5 lv) + g w 0.5 (exp(lv) - 1) / B
//   vae_scale       y = x * g (g: the loss cotangent on the device)
//   vae_recon_nchw  [B, H, W, 4] -> [B, C, H, W]
// No atomics: every result is reproducible bit for bit.
#include "common.h"
#include "kernels.h"

namespace {

// one index of the [.., C HW] (NCHW flatten) side for index j of the [.., HW C] (NHWC) side
__device__ __forceinline__ long long chw_of_hwc(long long j, int C, int HW) {
    const long long p = j / C, c = j - p * C;
    return c * HW + p;
}

__global__ __launch_bounds__(256) void vae_permute_kernel(const float* __restrict__ src, float* __restrict__ dst, long long R, long long F,
                                                          int C, int HW, int rows, int pack) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * F) return;
    // t walks the packed (NHWC) side; rows: F = C HW rows of R columns, else R rows of F = C HW columns
    long long r, j;
    if (rows) { j = t / R; r = t - j * R; }
    else { r = t / F; j = t - r * F; }
    const long long u = chw_of_hwc(j, C, HW);
    const long long hwc = rows ? j * R + r : r * F + j;
    const long long chw = rows ? u * R + r : r * F + u;
    if (pack) dst[hwc] = src[chw];
    else dst[chw] = src[hwc];
}

__global__ __launch_bounds__(256) void vae_pad_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int rows_pad, int K) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows_pad * K) return;
    const int r = t / K;
    dst[t] = r < rows ? src[t] : 0.f;
}

__global__ __launch_bounds__(256) void vae_kl_fwd_kernel(const float* __restrict__ ml, const float* __restrict__ eps, float* __restrict__ latent,
                                                         float* __restrict__ part, float* __restrict__ rep, int L) {
    __shared__ float red[256];
    const int b = blockIdx.x;
    const float* mu = ml + (long long)b * 2 * L;
    const float* lv = mu + L;
    float s = 0.f;
    for (int j = threadIdx.x; j < L; j += 256) {                      // fixed per-thread order
        const float m = mu[j], v = lv[j];
        const float e = expf(v);
        latent[(long long)b * L + j] = eps[(long long)b * L + j] * expf(0.5f * v) + m;
        s += 1.f + v - m * m - e;
        if (rep) rep[(long long)b * L + j] = m;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    block_tree_sum<256>(red);
    if (threadIdx.x == 0) part[b] = -0.5f * red[0];
}

__global__ __launch_bounds__(64) void vae_loss_kernel(const float* __restrict__ part, float* __restrict__ metrics, int B, float kld_weight) {
    if (threadIdx.x != 0) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[b];
    const float kld = s / (float)B;
    const float mse = metrics[1];                                     // written by mse_launch
    metrics[0] = mse + kld_weight * kld;
    metrics[2] = kld;
}

__global__ __launch_bounds__(256) void vae_kl_bwd_kernel(const float* __restrict__ ml, const float* __restrict__ eps, const float* __restrict__ dlat,
                                                         const float* __restrict__ drep, const float* __restrict__ dloss, float* __restrict__ dml,
                                                         int B, int L, float kld_weight) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * L) return;
    const long long b = t / L, j = t - b * L;
    const float m = ml[b * 2 * L + j], v = ml[b * 2 * L + L + j];
    const float g = dloss ? dloss[0] : 0.f;                            // no loss cotangent: no KL term
    const float gk = g * kld_weight / (float)B;
    const float dl = dlat ? dlat[t] : 0.f;
    float dm = dl + gk * m;
    if (drep) dm += drep[t];
    const float dv = dl * 0.5f * eps[t] * expf(0.5f * v) + gk * 0.5f * (expf(v) - 1.f);
    dml[b * 2 * L + j] = dm;
    dml[b * 2 * L + L + j] = dv;
}

__global__ __launch_bounds__(256) void vae_scale_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ g, long long n) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] = g ? x[t] * g[0] : x[t];
}

__global__ __launch_bounds__(256) void vae_recon_nchw_kernel(const float* __restrict__ r4, float* __restrict__ out, int B, int C, int HW) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * C * HW) return;
    const long long b = t / ((long long)C * HW);
    const long long rem = t - b * C * HW;
    const int c = (int)(rem / HW), p = (int)(rem - (long long)c * HW);
    out[t] = r4[(b * HW + p) * 4 + c];
}

}  // namespace

int vae_permute_launch(const float* src, float* dst, long long R, int C, int HW, int rows, int pack, hipStream_t st) {
    const long long n = R * C * HW;
    hipLaunchKernelGGL(vae_permute_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, src, dst, R, (long long)C * HW, C, HW, rows, pack);
    OCRL_CHECK_LAUNCH("vae_permute");
    return 0;
}

int vae_pad_rows_launch(const float* src, float* dst, int rows, int rows_pad, int K, hipStream_t st) {
    OCRL_REQUIRE(rows <= rows_pad, "vae_pad_rows: %d rows do not fit %d", rows, rows_pad);
    hipLaunchKernelGGL(vae_pad_rows_kernel, dim3(cdiv((long long)rows_pad * K, 256)), dim3(256), 0, st, src, dst, rows, rows_pad, K);
    OCRL_CHECK_LAUNCH("vae_pad_rows");
    return 0;
}

int vae_kl_fwd_launch(const float* ml, const float* eps, float* latent, float* part, float* rep, int B, int L, hipStream_t st) {
    hipLaunchKernelGGL(vae_kl_fwd_kernel, dim3(B), dim3(256), 0, st, ml, eps, latent, part, rep, L);
    OCRL_CHECK_LAUNCH("vae_kl_fwd");
    return 0;
}

int vae_loss_launch(const float* part, float* metrics, int B, float kld_weight, hipStream_t st) {
    hipLaunchKernelGGL(vae_loss_kernel, dim3(1), dim3(64), 0, st, part, metrics, B, kld_weight);
    OCRL_CHECK_LAUNCH("vae_loss");
    return 0;
}

int vae_kl_bwd_launch(const float* ml, const float* eps, const float* dlat, const float* drep, const float* dloss, float* dml, int B, int L,
                      float kld_weight, hipStream_t st) {
    hipLaunchKernelGGL(vae_kl_bwd_kernel, dim3(cdiv((long long)B * L, 256)), dim3(256), 0, st, ml, eps, dlat, drep, dloss, dml, B, L, kld_weight);
    OCRL_CHECK_LAUNCH("vae_kl_bwd");
    return 0;
}

int vae_scale_launch(const float* x, float* y, const float* g, long long n, hipStream_t st) {
    hipLaunchKernelGGL(vae_scale_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, y, g, n);
    OCRL_CHECK_LAUNCH("vae_scale");
    return 0;
}

int vae_recon_nchw_launch(const float* r4, float* out, int B, int C, int HW, hipStream_t st) {
    hipLaunchKernelGGL(vae_recon_nchw_kernel, dim3(cdiv((long long)B * C * HW, 256)), dim3(256), 0, st, r4, out, B, C, HW);
    OCRL_CHECK_LAUNCH("vae_recon_nchw");
    return 0;
}
