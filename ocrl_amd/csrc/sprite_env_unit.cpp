// C ABI of the sprite environments (include/ocrl_hip.h: ocrl_sprite_*, ocrl_task_scenes_batch; include/ocrl_hip_rollout.h): the Target and Odd-One-Out tasks of
// envs/synthetic_envs/{base,target,oddoneout}.py as a vectorised environment.  Stateless: the caller owns the state buffer (ocrl_sprite_env_state_floats floats) and every output.
#include "../../include/ocrl_hip_rollout.h"
#include "scenes.h"
#include "sprite_env.h"
#include "sprite_shapes.h"

namespace {
int check_env(const ocrl_sprite_env_desc* d, const char* who) {
    OCRL_REQUIRE(d, "%s: null descriptor", who);
    OCRL_REQUIRE(d->task >= 0 && d->task <= 1, "%s: task 0 (Target) or 1 (Odd-One-Out) (got %d)", who, d->task);
    OCRL_REQUIRE(d->E >= 1 && d->E < (1 << 20), "%s: 1 <= environments < 2^20 (got %d)", who, d->E);
    OCRL_REQUIRE(d->H >= 8 && d->H <= 512 && d->H % 4 == 0, "%s: obs_size must be a multiple of 4 in [8, 512] (got %d)", who, d->H);
    OCRL_REQUIRE(d->lo >= 1 && d->lo <= d->hi && d->hi <= OCRL_SPRITE_MAX_OBJECTS, "%s: num_objects_range [lo, hi] needs 1 <= lo <= hi <= %d (got [%d, %d])",
                 who, OCRL_SPRITE_MAX_OBJECTS, d->lo, d->hi);
    OCRL_REQUIRE(d->mode >= 0 && d->mode <= 2, "%s: mode 0 (easy), 1 (normal) or 2 (hard) (got %d)", who, d->mode);
    OCRL_REQUIRE(d->mode != 0 || (d->lo >= 2 && d->hi <= 4), "%s: easy mode has boxes for 2, 3 or 4 objects (got [%d, %d])", who, d->lo, d->hi);
    OCRL_REQUIRE(d->mode != 1 || (d->lo == 4 && d->hi == 4), "%s: normal mode has boxes for exactly 4 objects (got [%d, %d])", who, d->lo, d->hi);
    OCRL_REQUIRE(d->rew_type >= 0 && d->rew_type <= 2, "%s: rew_type 0 (sparse), 1 (normal) or 2 (dense) (got %d)", who, d->rew_type);
    OCRL_REQUIRE(d->max_steps >= 1, "%s: max_steps >= 1 (got %d)", who, d->max_steps);
    OCRL_REQUIRE(d->n_colors >= 1 && d->n_colors <= 8 && d->n_shapes >= 1 && d->n_shapes <= 8 && d->n_scales >= 1 && d->n_scales <= 8,
                 "%s: 1 to 8 COLORS, SHAPES and SCALES each (got %d, %d, %d)", who, d->n_colors, d->n_shapes, d->n_scales);
    const bool targeted = d->task != 1;                          // the Odd-One-Out task ignores target_*
    for (int i = 0; i < d->n_colors + 2; ++i) {
        if (i == d->n_colors && !targeted) continue;
        const int c = i < d->n_colors ? d->colors[i] : (i == d->n_colors ? d->target_color : d->agent_color);
        OCRL_REQUIRE(c >= 0 && c < 7, "%s: colour id %d is not one of the 7 colours", who, c);
    }
    for (int i = 0; i < d->n_shapes + 2; ++i) {
        if (i == d->n_shapes && !targeted) continue;
        const int s = i < d->n_shapes ? d->shapes[i] : (i == d->n_shapes ? d->target_shape : d->agent_shape);
        OCRL_REQUIRE(sprite_shape_drawn(s), "%s: shape id %d is not drawn (0 square, 1 triangle, 2 star_4, 3 circle, 7 star_5, 9 spoke_4)", who, s);
    }
    for (int i = 0; i < d->n_scales + 2; ++i) {
        if (i == d->n_scales && !targeted) continue;
        const float z = i < d->n_scales ? d->scales[i] : (i == d->n_scales ? d->target_scale : d->agent_scale);
        OCRL_REQUIRE(z > 0.f && z < 1.f, "%s: scales lie in (0, 1) (got %g)", who, (double)z);
    }
    OCRL_REQUIRE(d->agent_x >= 0.f && d->agent_x <= 1.f && d->agent_y >= 0.f && d->agent_y <= 1.f, "%s: agent_pos lies in [0, 1]^2", who);
    OCRL_REQUIRE(d->step_size > 0.f && d->dist_agent >= 0.f && d->dist_objs >= 0.f && d->dist_wall >= 0.f,
                 "%s: moving_step_size > 0 and the three distances >= 0", who);
    OCRL_REQUIRE(d->unseen_mode >= 0 && d->unseen_mode <= 2, "%s: unseen_mode 0 (none), 1 (train) or 2 (test) (got %d)", who, d->unseen_mode);
    if (d->task == 0) {
        OCRL_REQUIRE(d->obj_comp == 0 && d->unseen_mode == 0, "%s: obj_comp and unseen_mode belong to task 1 (Odd-One-Out) (got %d, %d with task 0)", who,
                     d->obj_comp, d->unseen_mode);
        return 0;
    }
    OCRL_REQUIRE(d->lo >= 3, "%s: Odd-One-Out needs num_objects_range lo >= 3, two others must share a value (got %d)", who, d->lo);
    OCRL_REQUIRE(d->n_colors > 1 || d->n_shapes > 1 || d->n_scales > 1,
                 "%s: Odd-One-Out needs more than one entry in COLORS, SHAPES or SCALES to pick the odd value from", who);
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < i; ++j)
            OCRL_REQUIRE(!(i < d->n_colors && d->colors[i] == d->colors[j]) && !(i < d->n_shapes && d->shapes[i] == d->shapes[j]) &&
                             !(i < d->n_scales && d->scales[i] == d->scales[j]),
                         "%s: Odd-One-Out needs distinct entries in COLORS, SHAPES and SCALES (entries %d and %d are equal)", who, j, i);
    if (d->unseen_mode != 0) {
        OCRL_REQUIRE(d->n_shapes == 1 && d->n_scales == 1, "%s: an unseen_mode needs one entry each in SHAPES and SCALES, the odd kind must be the colour (got %d, %d)",
                     who, d->n_shapes, d->n_scales);
        OCRL_REQUIRE(d->n_colors >= 3, "%s: an unseen_mode needs 3 or more COLORS (got %d)", who, d->n_colors);
        int found = 0;
        for (int i = 0; i < d->n_colors; ++i) found |= (d->colors[i] == d->unseen_colors[0] ? 1 : 0) | (d->colors[i] == d->unseen_colors[1] ? 2 : 0);
        OCRL_REQUIRE(d->unseen_colors[0] != d->unseen_colors[1] && found == 3, "%s: unseen_colors must be two different entries of COLORS (got %d, %d)", who,
                     d->unseen_colors[0], d->unseen_colors[1]);
    }
    return 0;
}

// what both task-scene entry points require of their arguments before a launch; `others`: an output besides the three pixel ones is asked for
int check_task_scenes(const ocrl_sprite_env_desc* d, const char* who, const long long* indices, int B, const float* obs, const unsigned char* obs_u8,
                      const float* masks, bool others, const char* outputs) {
    RC(check_env(d, who));
    OCRL_REQUIRE(B >= 1, "%s: batch >= 1 (got %d)", who, B);
    OCRL_REQUIRE(indices, "%s: null indices", who);
    OCRL_REQUIRE(obs || obs_u8 || masks || others, "%s: no output requested (%s are all null)", who, outputs);
    OCRL_REQUIRE(((uintptr_t)obs | (uintptr_t)masks) % 16 == 0 && (uintptr_t)obs_u8 % 4 == 0, "%s: obs and masks must be 16-byte aligned, obs_u8 4-byte aligned", who);
    OCRL_REQUIRE((long long)B * cdiv(d->H, scenes_band_rows(d->H)) < (1LL << 31), "%s: %d scenes of %d rows exceed one launch", who, B, d->H);
    return 0;
}
}  // namespace

extern "C" {

size_t ocrl_sprite_env_desc_size(void) { return sizeof(ocrl_sprite_env_desc); }

size_t ocrl_sprite_env_state_floats(const ocrl_sprite_env_desc* d) {
    if (check_env(d, "ocrl_sprite_env_state_floats")) return 0;
    return sprite_layout(d).total;
}

int ocrl_sprite_env_reset(const ocrl_sprite_env_desc* d, float* state, unsigned long long seed, const unsigned char* mask, long long episode, void* stream) {
    RC(check_env(d, "ocrl_sprite_env_reset"));
    OCRL_REQUIRE(state, "ocrl_sprite_env_reset: null state");
    OCRL_REQUIRE(episode >= -1 && episode < (1LL << 24), "ocrl_sprite_env_reset: episode is -1 (the next one) or in [0, 2^24) (got %lld)", episode);
    const SpriteLay y = sprite_layout(d);
    return sprite_env_reset_launch(*d, state, reinterpret_cast<int*>(state + y.aux), seed, mask, episode, static_cast<hipStream_t>(stream));
}

int ocrl_sprite_env_step(const ocrl_sprite_env_desc* d, float* state, unsigned long long seed, const long long* actions, float* rewards,
                         unsigned char* dones, unsigned char* success, double* ep_return, int* ep_length, void* stream) {
    RC(check_env(d, "ocrl_sprite_env_step"));
    OCRL_REQUIRE(state && actions && rewards && dones && success && ep_return && ep_length, "ocrl_sprite_env_step: null argument");
    const SpriteLay y = sprite_layout(d);
    const SpriteStepOut o{rewards, dones, success, ep_return, ep_length};
    return sprite_env_step_launch(*d, state, reinterpret_cast<int*>(state + y.aux), seed, actions, o, static_cast<hipStream_t>(stream));
}

int ocrl_sprite_render(const float* rows, int E, int R, int H, int mode, unsigned char* out, void* stream) {
    OCRL_REQUIRE(rows && out, "ocrl_sprite_render: null argument");
    OCRL_REQUIRE(E >= 1 && R >= 1 && R <= SPRITE_MAX_ROWS, "ocrl_sprite_render: environments >= 1 and 1 <= rows <= %d (got %d, %d)", SPRITE_MAX_ROWS, E, R);
    OCRL_REQUIRE(H >= 8 && H <= 512 && H % 4 == 0, "ocrl_sprite_render: obs_size must be a multiple of 4 in [8, 512] (got %d)", H);
    OCRL_REQUIRE(mode >= 0 && mode <= 2, "ocrl_sprite_render: mode 0 ([E,3,H,W]), 1 ([E,H,W,3]) or 2 (masks) (got %d)", mode);
    const int band_rows = 1024 / H < 1 ? 1 : 1024 / H;
    OCRL_REQUIRE((long long)E * cdiv(H, band_rows) < (1LL << 31), "ocrl_sprite_render: %d environments of %d rows exceed one launch", E, H);
    return sprite_render_launch(rows, E, R, H, mode, out, static_cast<hipStream_t>(stream));
}

int ocrl_sprite_state_obs(const float* rows, int E, int R, float* out, void* stream) {
    OCRL_REQUIRE(rows && out, "ocrl_sprite_state_obs: null argument");
    OCRL_REQUIRE(E >= 1 && R >= 1 && R <= SPRITE_MAX_ROWS, "ocrl_sprite_state_obs: environments >= 1 and 1 <= rows <= %d (got %d, %d)", SPRITE_MAX_ROWS, E, R);
    return sprite_state_obs_launch(rows, (long long)E * R, out, static_cast<hipStream_t>(stream));
}

int ocrl_task_scenes_batch(const ocrl_sprite_env_desc* d, unsigned long long seed, const long long* indices, int B, float* obs, unsigned char* obs_u8,
                           float* masks, float* objs, long long* labels, void* stream) {
    RC(check_task_scenes(d, "ocrl_task_scenes_batch", indices, B, obs, obs_u8, masks, objs || labels, "obs, obs_u8, masks, objs and labels"));
    return task_scenes_batch_launch(*d, seed, indices, B, TaskScenesOut{obs, obs_u8, masks, objs, labels}, static_cast<hipStream_t>(stream));
}

int ocrl_task_scenes_rollout_batch(const void* desc, unsigned long long seed, const long long* indices, const int* steps, int max_step, int B, float* obs,
                                   unsigned char* obs_u8, float* masks, float* objs, long long* labels, int* steps_taken, void* stream) {
    const ocrl_sprite_env_desc* d = static_cast<const ocrl_sprite_env_desc*>(desc);
    OCRL_REQUIRE(steps || (max_step >= 0 && max_step <= 255),
                 "ocrl_task_scenes_rollout_batch: max_step lies in [0, 255] when steps is null, the step is drawn in [0, max_step] (got %d)", max_step);
    RC(check_task_scenes(d, "ocrl_task_scenes_rollout_batch", indices, B, obs, obs_u8, masks, objs || labels || steps_taken,
                         "obs, obs_u8, masks, objs, labels and steps_taken"));
    return task_scenes_rollout_launch(*d, seed, indices, steps, max_step, B, TaskScenesOut{obs, obs_u8, masks, objs, labels}, steps_taken,
                                      static_cast<hipStream_t>(stream));
}

int ocrl_sprite_env_uniforms(unsigned long long seed, long long env0, int n_envs, long long episode, int first, int n, float* out, void* stream) {
    OCRL_REQUIRE(out && n >= 1 && n_envs >= 1, "ocrl_sprite_env_uniforms: null output, n < 1 or n_envs < 1");
    OCRL_REQUIRE(env0 >= 0 && env0 + n_envs <= (1 << 20) && episode >= 0 && episode < (1LL << 24) && first >= 0 && (long long)first + n <= SPRITE_MAX_DRAWS,
                 "ocrl_sprite_env_uniforms: environments < 2^20, episode < 2^24, draws < 2^20");
    return sprite_env_uniforms_launch(seed, env0, n_envs, episode, first, n, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
