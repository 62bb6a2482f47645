// Kernel arguments and launchers of the pre-training scenes (scenes.hip; C entry points in scenes_unit.cpp).
#pragma once
#include "../../include/ocrl_hip.h"
#include "common.h"

#define SITE_SCENES 510u            // rng site of a scene's draws (sprite_env.h has 500)
#define SCENES_CANDIDATES 64        // position candidates per object; the last one stands
#define SCENES_MAX_OBJS OCRL_SPRITE_MAX_OBJECTS
#define SCENES_INDEX_BITS 40        // a scene index is taken modulo 2^40 ...
#define SCENES_DRAW_BITS 16         // ... and leaves 16 bits of the counter to the draw: 15 * (1 + 2 * 64 + 2) = 1965 are ever used

struct ScenesOut {                  // any of them may be null
    float* obs;                     // [B, 3, H, W]
    unsigned char* obs_u8;          // [B, H, W, 3]
    float* masks;                   // [B, K + 1, H, W]
    float* objs;                    // [B, K, 5]
};

// rows of a frame that one workgroup paints: about 256 groups of four pixels, one per thread (the rule of sprite_render_launch)
inline int scenes_band_rows(int H) {
    const int r = 1024 / H;
    return r < 1 ? 1 : (r > H ? H : r);
}

int scenes_batch_launch(int H, int K, unsigned long long seed, const long long* indices, int B, const ScenesOut& o, hipStream_t st);
int scenes_uniforms_launch(unsigned long long seed, long long index, int first, int n, float* out, hipStream_t st);
