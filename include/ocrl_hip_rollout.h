/* C ABI of the task datasets' later frames in libocrl_hip.so (gfx950): a sprite task's episode after a random walk, made on the device.
 * A third header beside ocrl_hip.h and ocrl_hip_dqn.h, self-contained and in the same dialect (ocrl_amd/_abi.py reads each on its own and
 * follows no #include, so the descriptor crosses as `const void*`); the error convention is ocrl_hip.h's: the entry returns 0 on
 * success, the message of a failure is ocrl_last_error().
 *
 * ocrl_task_scenes_rollout_batch is ocrl_task_scenes_batch (ocrl_hip.h: "task scenes") with a step count: scene (i, t) of a seed is what
 * the environment of that seed shows t steps into the episode of index i under a uniform random policy.  It is a function of
 * (desc, seed, i, t) alone: the same whichever batch it is in, at whichever position, and whichever outputs are asked for.  Stateless:
 * the caller owns every buffer (obs and masks 16-byte aligned, obs_u8 4-byte aligned); everything is enqueued on `stream` (a hipStream_t)
 * with no host synchronisation, no atomics and no unbounded loop.  One launch per call.
 *
 * desc: a pointer to an ocrl_sprite_env_desc (ocrl_hip.h), validated exactly as by ocrl_task_scenes_batch; E is not used but must be
 *   valid; frames are H x H.  indices: device int64 [B], B >= 1, read as ocrl_task_scenes_batch reads them: masked to the low 44 bits,
 *   environment e = i >> 24, episode k = i & 0xFFFFFF.
 * The episode is that of ocrl_sprite_env_reset for (seed, e, k), unchanged ("The draws" of ocrl_hip.h).
 * The actions.  Step s = 0, 1, .. takes action a_s = (bits24 * 4) >> 24 of draw j = 2^19 + s of the same episode's stream (site 500,
 *   counter (e << 44) | (k << 20) | j).  An episode's own draws stop below 72 002 and j has 20 bits, so these collide with nothing;
 *   ocrl_sprite_env_uniforms(first = 2^19) returns them.
 * The transition is ocrl_sprite_env_step's, the same fp32 sequence (one function in the library): the move by step_size, the clip to
 *   [r_agent, 1 - r_agent], step_count + 1 >= max_steps, the first object in index order closer than agent_scale.  A step that would end
 *   the episode is not committed: the state after s steps stands and the walk stops there.  Otherwise it is committed, until s == t.
 *   So with L the step that ends the episode (counting from 1), the scene is the state after min(t, L - 1) steps: exactly the frames an
 *   environment can show during that episode (it starts the next episode inside the ending step and never shows a terminal frame).
 * t, one of two ways:
 *   steps != NULL: device int32 [B]; each value is clamped to [0, min(max_steps, 2^19)] inside the kernel.  max_step is not read.
 *   steps == NULL: 0 <= max_step <= 255, and t = (bits24 * (max_step + 1)) >> 24 of draw j = 2^19 - 1 of the episode's stream, then
 *     clamped likewise: one frame per episode at a uniformly drawn step.
 *   The walk takes at most min(t, max_steps) iterations.
 * Outputs, each may be NULL: obs, obs_u8, masks, objs and labels exactly as ocrl_task_scenes_batch defines them, of the walked state
 *   (only the agent's x, y in objs differ from the first frame; labels do not change); steps_taken [B] int32 = min(t, L - 1).
 *   With t = 0 every output equals ocrl_task_scenes_batch's bit for bit.
 * Rejected, non-zero with a message, before any launch: steps == NULL with max_step outside [0, 255]; a null or invalid descriptor;
 *   B < 1; null indices; all six outputs null; misaligned outputs; a batch beyond the grid limit. */
#ifndef OCRL_HIP_ROLLOUT_H
#define OCRL_HIP_ROLLOUT_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int ocrl_task_scenes_rollout_batch(const void* desc /* const ocrl_sprite_env_desc* */, unsigned long long seed,
                                   const long long* indices /* device int64 [B] */, const int* steps /* device int32 [B] or NULL = draw */,
                                   int max_step, int B, float* obs /* [B,3,H,W] or NULL */, unsigned char* obs_u8 /* [B,H,W,3] or NULL */,
                                   float* masks /* [B,hi+2,H,W] or NULL */, float* objs /* [B,hi+1,5] or NULL */,
                                   long long* labels /* [B] or NULL */, int* steps_taken /* [B] or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
