// The first frames of the sprite tasks' episodes as a pre-training dataset (the reference collects its target-* and odd-one-out-*
// datasets with only_initial: True), made on the device: scene (e << 24) | k of a seed is what environment e of that seed shows when its
// episode k begins, because both run new_episode (sprite_episode.h).  One launch per batch, shaped like scenes_batch_kernel.  A workgroup
// takes a row band of one scene (several in a large batch): its first thread makes the episode into LDS, then every thread takes four consecutive pixels of a row,
// finds which rows cover each of them once, and writes every requested output from that: the fp32 planes with 16-byte stores, the bytes
// as three words.  No atomics; every loop is bounded.  Compiled with -ffp-contract=off, as sprite_env.hip is: the same episode, bit for
// bit, and the pixels are those of ocrl_sprite_render (the same predicates, sprite_shapes.h).
// The rollout form (include/ocrl_hip_rollout.h; only_initial: False) is the same scene t steps later: after the episode the first thread
// walks it under a uniform random policy with the environment's own transition (sprite_move, sprite_episode.h), then the same bands render.
#include "scenes.h"
#include "sprite_episode.h"

#pragma clang fp contract(off)

namespace {

// Every workgroup repeats its scene's episode, a serial chain of some tens of microseconds, so a launch is as long as its rounds of
// resident workgroups are many: 256 compute units hold 4 of these workgroups each.  A batch that would need more than that many
// workgroups at one band each gives a workgroup several bands of its scene instead, down to one workgroup per scene.
#define TASK_SCENES_WORKGROUPS 1024

// what the rollout form adds to a scene (include/ocrl_hip_rollout.h); the first-frame kernel never reads it
struct TaskWalk {
    const int* steps;               // [B] or null: then the step is drawn in [0, max_step]
    int max_step;
    int* steps_taken;               // [B] or null
};

// One scene: the workgroup's first thread makes the episode into LDS and, with WALK, walks it there under the uniform random policy;
// then the band loop renders that state.  The walk is the environment's own transition (sprite_move) on the episode's own stream: at
// most min(t, max_steps) iterations of a few fp32 operations and n distances each, after the episode's much longer chain.
template <bool WALK>
__device__ __forceinline__ void task_scene(const ocrl_sprite_env_desc& d, int band_rows, int bands, int per_scene, unsigned long long seed,
                                           const long long* __restrict__ indices, const TaskScenesOut& o, const TaskWalk& w) {
    __shared__ float s_rows[SPRITE_MAX_ROWS * 5];
    __shared__ __align__(8) int s_aux[SPRITE_AUX];
    __shared__ float s_cx[SPRITE_MAX_ROWS], s_cy[SPRITE_MAX_ROWS], s_r[SPRITE_MAX_ROWS];
    __shared__ int s_shape[SPRITE_MAX_ROWS];                                 // -1: not drawn
    __shared__ uint32_t s_rgb[SPRITE_MAX_ROWS];
    const int R = d.hi + 1, H = d.H;
    const int b = blockIdx.x / per_scene, first = blockIdx.x % per_scene;       // this workgroup's bands: first, first + per_scene, ..
    if (threadIdx.x == 0) {
        const uint64_t i = (uint64_t)indices[b] & ((1ull << TASK_SCENES_INDEX_BITS) - 1ull);
        const uint32_t e = (uint32_t)(i >> 24), k = (uint32_t)(i & 0xFFFFFFu);
        new_episode(d, s_rows, s_aux, seed, e, k);
        if constexpr (WALK) {
            int t = w.steps ? w.steps[b] : (int)((env_bits24(seed, e, k, SPRITE_WALK_DRAW0 - 1u) * (uint32_t)(w.max_step + 1)) >> 24);
            const int most = d.max_steps < SPRITE_WALK_MAX_STEPS ? d.max_steps : SPRITE_WALK_MAX_STEPS;
            t = t < 0 ? 0 : (t > most ? most : t);
            const int n = s_aux[0], target = s_aux[1];
            int taken = 0;
            for (; taken < t; ++taken) {                                     // step `taken` of the walk; its step_count is `taken`
                const long long act = (long long)((env_bits24(seed, e, k, SPRITE_WALK_DRAW0 + (uint32_t)taken) * 4u) >> 24);
                const SpriteMove m = sprite_move(d, s_rows, n, target, taken, act);
                if (m.done) break;                                           // a step that ends the episode is not committed: no terminal frame
                s_rows[n * 5 + 3] = m.x; s_rows[n * 5 + 4] = m.y;
            }
            if (w.steps_taken && first == 0) w.steps_taken[b] = taken;
        }
    }
    __syncthreads();
    if (threadIdx.x < R) {                                                   // the sprite table of sprite_render_kernel; the state observation
        const int j = threadIdx.x;
        const float* q = s_rows + j * 5;
        const float c = q[0], h = q[1], z = q[2], x = q[3], y = q[4];
        int shape = -1;
        uint32_t rgb = 0;
        float cx = 0.f, cy = 0.f, r = 0.f;
        if (sprite_row_drawn(c, h, z)) {                                      // an empty row (the padding after the agent): not drawn
            shape = (int)h; rgb = SPRITE_RGB[(int)c]; r = z * 0.5f; cx = x; cy = y;
        }
        s_shape[j] = shape; s_rgb[j] = rgb; s_cx[j] = cx; s_cy[j] = cy; s_r[j] = r;
        if (o.objs && first == 0) {                                           // sprite_state_obs_kernel's row: the scale as its index in [0.15, 0.22]
            float* dst = o.objs + ((size_t)b * R + j) * 5;
            if (c == -1.f) {
                dst[0] = -1.f; dst[1] = -1.f; dst[2] = -1.f; dst[3] = 0.f; dst[4] = 0.f;
            } else {
                const bool empty = c == 0.f && h == 0.f && z == 0.f && x == 0.f && y == 0.f;
                dst[0] = c; dst[1] = h; dst[2] = (z == 0.15f || empty) ? 0.f : (z == 0.22f ? 1.f : -1.f); dst[3] = x; dst[4] = y;
            }
        }
    }
    if (o.labels && first == 0 && threadIdx.x == 0) o.labels[b] = (long long)s_aux[1];
    if (!o.obs && !o.obs_u8 && !o.masks) return;
    __syncthreads();
    const int W = H, W4 = W / 4;
    const float fH = (float)H;
    const size_t plane = (size_t)H * W;
    for (int band = first; band < bands; band += per_scene) {
        const int y0 = band * band_rows, y1 = y0 + band_rows < H ? y0 + band_rows : H;
        const int groups = (y1 - y0) * W4;
        for (int g = threadIdx.x; g < groups; g += 256) {
            const int y = y0 + g / W4, x4 = (g % W4) * 4;
            const float py = ((float)y + 0.5f) / fH;
            float pxc[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) pxc[p] = ((float)(x4 + p) + 0.5f) / fH;
            const size_t at = (size_t)y * W + x4;
            float* m = o.masks ? o.masks + (size_t)b * (R + 1) * plane + at : nullptr;
            uint32_t px[4] = {0u, 0u, 0u, 0u};
            bool any[4] = {false, false, false, false};
            for (int j = 0; j < R; ++j) {                                        // painter's order: a later row overwrites
                bool cov[4] = {false, false, false, false};
                const float dy = py - s_cy[j];
                if (s_shape[j] >= 0 && sprite_in_reach(dy, s_r[j])) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        cov[p] = sprite_covers(s_shape[j], pxc[p] - s_cx[j], dy, s_r[j]);
                        if (cov[p]) { px[p] = s_rgb[j]; any[p] = true; }
                    }
                }
                if (m)                                                           // plane j: row j alone and unoccluded
                    *reinterpret_cast<float4*>(m + (size_t)j * plane) = make_float4(cov[0] ? 1.f : 0.f, cov[1] ? 1.f : 0.f, cov[2] ? 1.f : 0.f, cov[3] ? 1.f : 0.f);
            }
            if (m)                                                               // the last plane: no row covers the pixel
                *reinterpret_cast<float4*>(m + (size_t)R * plane) = make_float4(any[0] ? 0.f : 1.f, any[1] ? 0.f : 1.f, any[2] ? 0.f : 1.f, any[3] ? 0.f : 1.f);
            if (o.obs) {
#pragma unroll
                for (int c = 0; c < 3; ++c)                                      // the arithmetic of ocrl_obs_u8_to_f32 on the byte
                    *reinterpret_cast<float4*>(o.obs + ((size_t)b * 3 + c) * plane + at) =
                        make_float4((float)((px[0] >> (8 * c)) & 0xFFu) / 255.0f, (float)((px[1] >> (8 * c)) & 0xFFu) / 255.0f,
                                    (float)((px[2] >> (8 * c)) & 0xFFu) / 255.0f, (float)((px[3] >> (8 * c)) & 0xFFu) / 255.0f);
            }
            if (o.obs_u8) {                                                      // 12 bytes r g b r g b ... as three words
                uint32_t* dst = reinterpret_cast<uint32_t*>(o.obs_u8 + ((size_t)b * plane + at) * 3);
                dst[0] = (px[0] & 0xFFFFFFu) | ((px[1] & 0xFFu) << 24);
                dst[1] = ((px[1] >> 8) & 0xFFFFu) | ((px[2] & 0xFFFFu) << 16);
                dst[2] = ((px[2] >> 16) & 0xFFu) | ((px[3] & 0xFFFFFFu) << 8);
            }
        }
    }
}


__global__ __launch_bounds__(256) void task_scenes_batch_kernel(ocrl_sprite_env_desc d, int band_rows, int bands, int per_scene, unsigned long long seed,
                                                                const long long* __restrict__ indices, TaskScenesOut o) {
    task_scene<false>(d, band_rows, bands, per_scene, seed, indices, o, TaskWalk{nullptr, 0, nullptr});
}

__global__ __launch_bounds__(256) void task_scenes_rollout_kernel(ocrl_sprite_env_desc d, int band_rows, int bands, int per_scene, unsigned long long seed,
                                                                  const long long* __restrict__ indices, TaskScenesOut o, TaskWalk w) {
    task_scene<true>(d, band_rows, bands, per_scene, seed, indices, o, w);
}

}  // namespace

namespace {
// workgroups to a scene; each takes every per_scene-th band
int task_scenes_per_scene(int B, int bands, const TaskScenesOut& o) {
    int per_scene = TASK_SCENES_WORKGROUPS / B;
    per_scene = per_scene < 1 ? 1 : (per_scene > bands ? bands : per_scene);
    return (o.obs || o.obs_u8 || o.masks) ? per_scene : 1;                                 // rows and labels alone: one workgroup per scene
}
}  // namespace

int task_scenes_batch_launch(const ocrl_sprite_env_desc& d, unsigned long long seed, const long long* indices, int B, const TaskScenesOut& o, hipStream_t st) {
    const int band_rows = scenes_band_rows(d.H), bands = cdiv(d.H, band_rows);
    const int per_scene = task_scenes_per_scene(B, bands, o);
    hipLaunchKernelGGL(task_scenes_batch_kernel, dim3((unsigned)((long long)B * per_scene)), dim3(256), 0, st, d, band_rows, bands, per_scene, seed, indices, o);
    OCRL_CHECK_LAUNCH("task_scenes_batch");
    return 0;
}
int task_scenes_rollout_launch(const ocrl_sprite_env_desc& d, unsigned long long seed, const long long* indices, const int* steps, int max_step, int B,
                               const TaskScenesOut& o, int* steps_taken, hipStream_t st) {
    const int band_rows = scenes_band_rows(d.H), bands = cdiv(d.H, band_rows);
    const int per_scene = task_scenes_per_scene(B, bands, o);
    hipLaunchKernelGGL(task_scenes_rollout_kernel, dim3((unsigned)((long long)B * per_scene)), dim3(256), 0, st, d, band_rows, bands, per_scene, seed, indices, o,
                       TaskWalk{steps, max_step, steps_taken});
    OCRL_CHECK_LAUNCH("task_scenes_rollout");
    return 0;
}
