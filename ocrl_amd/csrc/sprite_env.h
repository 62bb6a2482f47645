// Kernel arguments and launchers of the sprite environments (sprite_env.hip; C entry points in sprite_env_unit.cpp).
#pragma once
#include "../../include/ocrl_hip.h"
#include "common.h"

#define SITE_SPRITE_ENV 500u        // rng site of an episode's draws (acnet.h has 400, pool_unit.cpp 300 .. 399)
#define SPRITE_MAX_ROWS (OCRL_SPRITE_MAX_OBJECTS + 1)
#define SPRITE_AUX 8                // int32 words per environment after the rows: n, target, step_count, episode, ep_length, unique kind, ep_return (double)
#define SPRITE_TRIPLE_TRIES 64      // redraws of a non-target's (colour, shape, scale) before the last one stands
#define SPRITE_CANDIDATES 256       // position candidates per object
#define SPRITE_RESTARTS 8           // whole-placement restarts before a dead-ended object keeps its last candidate
#define SPRITE_MAX_DRAWS (1 << 20)  // draw indices of one episode: 2 + 15 * 64 * 3 + 9 * 15 * 256 * 2 = 72 002 are ever used (Odd-One-Out: fewer)

// where the pieces of a state buffer lie (floats from its start)
struct SpriteLay {
    int R;                          // rows per environment: hi + 1
    size_t aux, total;
};
inline SpriteLay sprite_layout(const ocrl_sprite_env_desc* d) {
    SpriteLay y;
    WsTake take;
    y.R = d->hi + 1;
    take((size_t)d->E * y.R * 5);
    y.aux = take((size_t)d->E * SPRITE_AUX);
    y.total = take.end;
    return y;
}

struct SpriteStepOut {
    float* rewards;                 // [E]
    unsigned char *dones, *success; // [E]
    double* ep_return;              // [E] the finished episode's return (0 where none finished)
    int* ep_length;                 // [E]
};

#define TASK_SCENES_INDEX_BITS 44   // a task scene's index is taken modulo 2^44: environment (20 bits) << 24 | episode (24 bits)

struct TaskScenesOut {              // task_scenes.hip; any of them may be null
    float* obs;                     // [B, 3, H, W]
    unsigned char* obs_u8;          // [B, H, W, 3]
    float* masks;                   // [B, hi + 2, H, W]
    float* objs;                    // [B, hi + 1, 5]
    long long* labels;              // [B]
};

int task_scenes_batch_launch(const ocrl_sprite_env_desc& d, unsigned long long seed, const long long* indices, int B, const TaskScenesOut& o, hipStream_t st);
// the same scenes after a random walk: steps [B] or null (then drawn in [0, max_step]), steps_taken [B] or null
int task_scenes_rollout_launch(const ocrl_sprite_env_desc& d, unsigned long long seed, const long long* indices, const int* steps, int max_step, int B,
                               const TaskScenesOut& o, int* steps_taken, hipStream_t st);
int sprite_env_reset_launch(const ocrl_sprite_env_desc& d, float* rows, int* aux, unsigned long long seed, const unsigned char* mask, long long episode,
                            hipStream_t st);
int sprite_env_step_launch(const ocrl_sprite_env_desc& d, float* rows, int* aux, unsigned long long seed, const long long* actions, const SpriteStepOut& o,
                           hipStream_t st);
int sprite_render_launch(const float* rows, int E, int R, int H, int mode, unsigned char* out, hipStream_t st);
int sprite_env_uniforms_launch(unsigned long long seed, long long env0, int n_envs, long long episode, int first, int n, float* out, hipStream_t st);
int sprite_state_obs_launch(const float* rows, long long n, float* out, hipStream_t st);
