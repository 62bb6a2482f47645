// The Target and Odd-One-Out sprite tasks (envs/synthetic_envs/{base,target,oddoneout}.py restated) as a vectorised environment: state,
// transition, reward, auto-reset and rendering on the device; the tasks differ in how an episode's objects are made, nothing else.  reset / step: one thread per environment (an episode's draws are a serial rejection chain).  render: the
// only part with bytes to move; a workgroup takes a row band of one environment, keeps the sprite table in LDS and writes 4 pixels of a
// channel plane per 32-bit store.  No atomics; every loop is bounded.  Compiled with -ffp-contract=off: each position is the written
// sequence of fp32 roundings, so a numpy fp32 restatement (tests/sprite_env_ref.py) follows it bit for bit.
#include "sprite_episode.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(64) void sprite_env_reset_kernel(ocrl_sprite_env_desc d, float* __restrict__ rows, int* __restrict__ aux, unsigned long long seed,
                                                              const unsigned char* __restrict__ mask, long long episode) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= d.E) return;
    if (mask && !mask[e]) return;
    int* a = aux + (size_t)e * SPRITE_AUX;
    const uint32_t k = episode >= 0 ? (uint32_t)episode : (uint32_t)a[3] + 1u;
    new_episode(d, rows + (size_t)e * (d.hi + 1) * 5, a, seed, (uint32_t)e, k);
}

__global__ __launch_bounds__(64) void sprite_env_step_kernel(ocrl_sprite_env_desc d, float* __restrict__ rows, int* __restrict__ aux, unsigned long long seed,
                                                             const long long* __restrict__ actions, SpriteStepOut o) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= d.E) return;
    const int R = d.hi + 1;
    float* q = rows + (size_t)e * R * 5;
    int* a = aux + (size_t)e * SPRITE_AUX;
    int n = a[0], target = a[1];
    n = n < 1 ? 1 : (n > d.hi ? d.hi : n);                                   // a hand-set state cannot index outside the rows
    target = target < 0 ? 0 : (target >= n ? n - 1 : target);
    const SpriteMove m = sprite_move(d, q, n, target, a[2], actions[e]);      // the transition: sprite_episode.h
    q[n * 5 + 3] = m.x; q[n * 5 + 4] = m.y;
    const int steps = a[2] + 1;
    const bool done = m.done, success = m.success;
    const float reward = m.reward;
    double* ret = reinterpret_cast<double*>(a + 6);
    const double total = *ret + (double)reward;
    const int len = a[4] + 1;
    o.rewards[e] = reward;
    o.dones[e] = done ? 1 : 0;
    o.success[e] = success ? 1 : 0;
    o.ep_return[e] = done ? total : 0.0;
    o.ep_length[e] = done ? len : 0;
    if (done) new_episode(d, q, a, seed, (uint32_t)e, (uint32_t)a[3] + 1u);
    else { a[2] = steps; a[4] = len; *ret = total; }
}

__global__ __launch_bounds__(256) void sprite_env_uniforms_kernel(unsigned long long seed, long long env0, int n_envs, long long episode, int first, int n,
                                                                  float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_envs * n) return;
    const uint32_t e = (uint32_t)(env0 + i / n), j = (uint32_t)(first + i % n);
    out[i] = (float)env_bits24(seed, e, (uint32_t)episode, j) * (1.f / 16777216.f);
}

// ---------------------------------------------------------------------------------------------------------------- state observations
// render(mode="state") of the reference (base.py:365-394), one thread per row: the scale becomes its index in the global SCALES list
// [0.15, 0.22] (-1: neither; an all-zero row, the padding after the agent, stays zero), a colour of -1 gives (-1, -1, -1, 0, 0)
__global__ __launch_bounds__(256) void sprite_state_obs_kernel(const float* __restrict__ rows, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* r = rows + i * 5;
    const float c = r[0], s = r[1], z = r[2], x = r[3], y = r[4];
    float* o = out + i * 5;
    if (c == -1.f) {
        o[0] = -1.f; o[1] = -1.f; o[2] = -1.f; o[3] = 0.f; o[4] = 0.f;
        return;
    }
    const bool empty = c == 0.f && s == 0.f && z == 0.f && x == 0.f && y == 0.f;
    o[0] = c; o[1] = s; o[2] = (z == 0.15f || empty) ? 0.f : (z == 0.22f ? 1.f : -1.f); o[3] = x; o[4] = y;
}

// ---------------------------------------------------------------------------------------------------------------- the renderer
// (the shape predicates and the colour table: sprite_shapes.h)
// mode 0: [E, 3, H, W]; 1: [E, H, W, 3]; 2: masks [E, R + 1, H, W, 1] (row j alone and unoccluded; the background last)
__global__ __launch_bounds__(256) void sprite_render_kernel(const float* __restrict__ rows, int R, int H, int band_rows, int bands, int mode,
                                                            unsigned char* __restrict__ out) {
    __shared__ float s_cx[SPRITE_MAX_ROWS], s_cy[SPRITE_MAX_ROWS], s_r[SPRITE_MAX_ROWS];
    __shared__ int s_shape[SPRITE_MAX_ROWS];                                 // -1: not drawn
    __shared__ uint32_t s_rgb[SPRITE_MAX_ROWS];
    const int e = blockIdx.x / bands, band = blockIdx.x % bands;
    if (threadIdx.x < SPRITE_MAX_ROWS) {
        const int j = threadIdx.x;
        int shape = -1;
        uint32_t rgb = 0;
        float cx = 0.f, cy = 0.f, r = 0.f;
        if (j < R) {
            const float* q = rows + ((size_t)e * R + j) * 5;
            const float c = q[0], h = q[1], z = q[2];
            if (sprite_row_drawn(c, h, z)) {                                 // colour -1, an id that is not drawn or an empty row: not drawn
                shape = (int)h; rgb = SPRITE_RGB[(int)c]; r = z * 0.5f; cx = q[3]; cy = q[4];
            }
        }
        s_shape[j] = shape; s_rgb[j] = rgb; s_cx[j] = cx; s_cy[j] = cy; s_r[j] = r;
    }
    __syncthreads();
    const int W = H, W4 = W / 4;
    const int y0 = band * band_rows, y1 = y0 + band_rows < H ? y0 + band_rows : H;
    const int groups = (y1 - y0) * W4;
    const float fH = (float)H;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int y = y0 + g / W4, x4 = (g % W4) * 4;
        const float py = ((float)y + 0.5f) / fH;
        if (mode == 2) {
            uint32_t any = 0;
            for (int j = 0; j < R; ++j) {
                uint32_t m = 0;
                const float dy = py - s_cy[j];
                if (s_shape[j] >= 0 && sprite_in_reach(dy, s_r[j])) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float dx = ((float)(x4 + p) + 0.5f) / fH - s_cx[j];
                        if (sprite_covers(s_shape[j], dx, dy, s_r[j])) m |= 1u << (8 * p);
                    }
                }
                any |= m;
                *reinterpret_cast<uint32_t*>(out + (((size_t)e * (R + 1) + j) * H + y) * W + x4) = m;
            }
            *reinterpret_cast<uint32_t*>(out + (((size_t)e * (R + 1) + R) * H + y) * W + x4) = any ^ 0x01010101u;
            continue;
        }
        uint32_t px[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < R; ++j) {                                        // painter's order: a later row overwrites
            const float dy = py - s_cy[j];
            if (s_shape[j] < 0 || !sprite_in_reach(dy, s_r[j])) continue;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float dx = ((float)(x4 + p) + 0.5f) / fH - s_cx[j];
                if (sprite_covers(s_shape[j], dx, dy, s_r[j])) px[p] = s_rgb[j];
            }
        }
        if (mode == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t w = ((px[0] >> (8 * c)) & 0xFFu) | (((px[1] >> (8 * c)) & 0xFFu) << 8) | (((px[2] >> (8 * c)) & 0xFFu) << 16) |
                                   (((px[3] >> (8 * c)) & 0xFFu) << 24);
                *reinterpret_cast<uint32_t*>(out + (((size_t)e * 3 + c) * H + y) * W + x4) = w;
            }
        } else {                                                             // 12 bytes r g b r g b ... as three words
            uint32_t* dst = reinterpret_cast<uint32_t*>(out + (((size_t)e * H + y) * W + x4) * 3);
            dst[0] = (px[0] & 0xFFFFFFu) | ((px[1] & 0xFFu) << 24);
            dst[1] = ((px[1] >> 8) & 0xFFFFu) | ((px[2] & 0xFFFFu) << 16);
            dst[2] = ((px[2] >> 16) & 0xFFu) | ((px[3] & 0xFFFFFFu) << 8);
        }
    }
}

}  // namespace

int sprite_env_reset_launch(const ocrl_sprite_env_desc& d, float* rows, int* aux, unsigned long long seed, const unsigned char* mask, long long episode,
                            hipStream_t st) {
    hipLaunchKernelGGL(sprite_env_reset_kernel, dim3(cdiv(d.E, 64)), dim3(64), 0, st, d, rows, aux, seed, mask, episode);
    OCRL_CHECK_LAUNCH("sprite_env_reset");
    return 0;
}
int sprite_env_step_launch(const ocrl_sprite_env_desc& d, float* rows, int* aux, unsigned long long seed, const long long* actions, const SpriteStepOut& o,
                           hipStream_t st) {
    hipLaunchKernelGGL(sprite_env_step_kernel, dim3(cdiv(d.E, 64)), dim3(64), 0, st, d, rows, aux, seed, actions, o);
    OCRL_CHECK_LAUNCH("sprite_env_step");
    return 0;
}
int sprite_render_launch(const float* rows, int E, int R, int H, int mode, unsigned char* out, hipStream_t st) {
    int band_rows = 1024 / H;                                                // about 256 groups of four pixels, one per thread, to a workgroup
    band_rows = band_rows < 1 ? 1 : (band_rows > H ? H : band_rows);
    const int bands = cdiv(H, band_rows);
    hipLaunchKernelGGL(sprite_render_kernel, dim3((unsigned)((long long)E * bands)), dim3(256), 0, st, rows, R, H, band_rows, bands, mode, out);
    OCRL_CHECK_LAUNCH("sprite_render");
    return 0;
}
int sprite_env_uniforms_launch(unsigned long long seed, long long env0, int n_envs, long long episode, int first, int n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sprite_env_uniforms_kernel, dim3(cdiv((long long)n_envs * n, 256)), dim3(256), 0, st, seed, env0, n_envs, episode, first, n, out);
    OCRL_CHECK_LAUNCH("sprite_env_uniforms");
    return 0;
}
int sprite_state_obs_launch(const float* rows, long long n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sprite_state_obs_kernel, GRID1D(n), 0, st, rows, n, out);
    OCRL_CHECK_LAUNCH("sprite_state_obs");
    return 0;
}
