// The pre-training scenes (the RandomObjs episode of ocrl_amd/utils/data.py:random_sprite_scenes restated) made on the device: scene i of
// a seed is a function of (seed, i) alone.  One launch per batch.  A workgroup takes a row band of one scene: its first thread redraws
// the scene's objects (a serial rejection chain of a few dozen draws) into LDS, then every thread takes four consecutive pixels of a
// row, finds which objects cover each of them once, and writes every requested output from that: the fp32 planes with 16-byte stores,
// the bytes as three words.  No atomics; every loop is bounded.  Compiled with -ffp-contract=off: each position is the written sequence
// of fp32 roundings, so a numpy fp32 restatement (tests/scenes_ref.py) follows it bit for bit, and the pixels are those of
// ocrl_sprite_render (the same predicates, sprite_shapes.h).
#include "scenes.h"
#include "sprite_shapes.h"

#pragma clang fp contract(off)

namespace {

// 24 random bits of draw j of scene i: counter (i << 16) | j of the site's stream
__host__ __device__ inline uint32_t scene_bits24(unsigned long long seed, uint64_t i, uint32_t j) {
    const uint64_t c = (i << SCENES_DRAW_BITS) | (uint64_t)j;
    return rng_bits1_keyed(rng_key(seed, SITE_SCENES, (uint32_t)(c >> 32)), (uint32_t)c) >> 8;
}
__host__ __device__ inline uint64_t scene_index(long long index) { return (uint64_t)index & ((1ull << SCENES_INDEX_BITS) - 1ull); }

struct SceneStream {
    unsigned long long seed;
    uint64_t i;
    uint32_t j;
    __device__ uint32_t bits() { return scene_bits24(seed, i, j++); }
    __device__ int below(int m) { return (int)((bits() * (uint32_t)m) >> 24); }            // uniform in [0, m), m <= 256
    __device__ float u01() { return (float)bits() * (1.f / 16777216.f); }                  // k / 2^24 in [0, 1)
};

__constant__ float SCENE_SCALES[2] = {0.15f, 0.22f};

// the K objects of scene i, in draw order: scale, position (at most 64 candidates), shape, colour
__device__ void draw_scene(unsigned long long seed, uint64_t i, int K, int* col, int* shp, int* scl, float* px, float* py) {
    SceneStream s{seed, i, 0u};
    for (int k = 0; k < K; ++k) {
        const int z = s.below(2);
        const float r = SCENE_SCALES[z] * 0.5f;
        const float a = r + 0.08f, b = (1.0f - r) - 0.08f;
        const float w = b - a;
        float x = 0.f, y = 0.f;
        bool ok = false;
        for (int c = 0; c < SCENES_CANDIDATES && !ok; ++c) {
            const float ux = w * s.u01();
            x = a + ux;
            const float uy = w * s.u01();
            y = a + uy;
            ok = !(dist2d(0.5f, 0.5f, x, y) < 0.15f);
            for (int j = 0; j < k; ++j)
                if (dist2d(px[j], py[j], x, y) < 0.15f) ok = false;
        }
        px[k] = x; py[k] = y; scl[k] = z;                      // rejected 64 times: the last candidate stands
        shp[k] = s.below(4);
        col[k] = s.below(4);
    }
}

__global__ __launch_bounds__(256) void scenes_batch_kernel(int H, int K, int band_rows, int bands, unsigned long long seed,
                                                           const long long* __restrict__ indices, ScenesOut o) {
    __shared__ float s_cx[SCENES_MAX_OBJS], s_cy[SCENES_MAX_OBJS];
    __shared__ int s_col[SCENES_MAX_OBJS], s_shape[SCENES_MAX_OBJS], s_scl[SCENES_MAX_OBJS];
    const int b = blockIdx.x / bands, band = blockIdx.x % bands;
    if (threadIdx.x == 0) draw_scene(seed, scene_index(indices[b]), K, s_col, s_shape, s_scl, s_cx, s_cy);
    __syncthreads();
    if (o.objs && band == 0 && threadIdx.x < K) {
        const int k = threadIdx.x;
        float* q = o.objs + ((size_t)b * K + k) * 5;
        q[0] = (float)s_col[k]; q[1] = (float)s_shape[k]; q[2] = (float)s_scl[k]; q[3] = s_cx[k]; q[4] = s_cy[k];
    }
    if (!o.obs && !o.obs_u8 && !o.masks) return;
    const int W = H, W4 = W / 4;
    const int y0 = band * band_rows, y1 = y0 + band_rows < H ? y0 + band_rows : H;
    const int groups = (y1 - y0) * W4;
    const float fH = (float)H;
    const size_t plane = (size_t)H * W;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int y = y0 + g / W4, x4 = (g % W4) * 4;
        const float py = ((float)y + 0.5f) / fH;
        float dxp[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) dxp[p] = ((float)(x4 + p) + 0.5f) / fH;
        int top[4] = {-1, -1, -1, -1};                        // the last object covering the pixel: painter's order
        for (int k = 0; k < K; ++k) {
            const float dy = py - s_cy[k], r = SCENE_SCALES[s_scl[k]] * 0.5f;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (sprite_covers(s_shape[k], dxp[p] - s_cx[k], dy, r)) top[p] = k;
        }
        const size_t at = (size_t)y * W + x4;
        if (o.obs || o.obs_u8) {
            uint32_t px[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) px[p] = top[p] >= 0 ? SPRITE_RGB[s_col[top[p]]] : 0u;
            if (o.obs) {
#pragma unroll
                for (int c = 0; c < 3; ++c)                    // the arithmetic of ocrl_obs_u8_to_f32 on the byte
                    *reinterpret_cast<float4*>(o.obs + ((size_t)b * 3 + c) * plane + at) =
                        make_float4((float)((px[0] >> (8 * c)) & 0xFFu) / 255.0f, (float)((px[1] >> (8 * c)) & 0xFFu) / 255.0f,
                                    (float)((px[2] >> (8 * c)) & 0xFFu) / 255.0f, (float)((px[3] >> (8 * c)) & 0xFFu) / 255.0f);
            }
            if (o.obs_u8) {                                    // 12 bytes r g b r g b ... as three words
                uint32_t* dst = reinterpret_cast<uint32_t*>(o.obs_u8 + ((size_t)b * plane + at) * 3);
                dst[0] = (px[0] & 0xFFFFFFu) | ((px[1] & 0xFFu) << 24);
                dst[1] = ((px[1] >> 8) & 0xFFFFu) | ((px[2] & 0xFFFFu) << 16);
                dst[2] = ((px[2] >> 16) & 0xFFu) | ((px[3] & 0xFFFFFFu) << 8);
            }
        }
        if (o.masks) {
            float* m = o.masks + (size_t)b * (K + 1) * plane + at;
            for (int k = 0; k <= K; ++k) {                     // plane K, the background: no object, top == -1
                const int want = k < K ? k : -1;
                *reinterpret_cast<float4*>(m + (size_t)k * plane) = make_float4(top[0] == want ? 1.f : 0.f, top[1] == want ? 1.f : 0.f,
                                                                                top[2] == want ? 1.f : 0.f, top[3] == want ? 1.f : 0.f);
            }
        }
    }
}

__global__ __launch_bounds__(256) void scenes_uniforms_kernel(unsigned long long seed, long long index, int first, int n, float* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    out[t] = (float)scene_bits24(seed, scene_index(index), (uint32_t)(first + t)) * (1.f / 16777216.f);
}

}  // namespace

int scenes_batch_launch(int H, int K, unsigned long long seed, const long long* indices, int B, const ScenesOut& o, hipStream_t st) {
    const int band_rows = scenes_band_rows(H), bands = cdiv(H, band_rows);
    hipLaunchKernelGGL(scenes_batch_kernel, dim3((unsigned)((long long)B * bands)), dim3(256), 0, st, H, K, band_rows, bands, seed, indices, o);
    OCRL_CHECK_LAUNCH("scenes_batch");
    return 0;
}
int scenes_uniforms_launch(unsigned long long seed, long long index, int first, int n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(scenes_uniforms_kernel, GRID1D(n), 0, st, seed, index, first, n, out);
    OCRL_CHECK_LAUNCH("scenes_uniforms");
    return 0;
}
