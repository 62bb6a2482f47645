// How an episode of the sprite tasks is made (the Target and Odd-One-Out episodes, include/ocrl_hip.h: "The draws"), for every kernel
// that starts one: the environments' reset and step (sprite_env.hip) and the task datasets' frames (task_scenes.hip).  An episode
// is a function of (seed, e, k) alone, so both see the same one; how a step moves it is written once too (sprite_move).  Every file that includes this is compiled with -ffp-contract=off:
// each position is the written sequence of fp32 roundings (tests/sprite_env_ref.py and tests/oddoneout_ref.py follow it bit for bit).
#pragma once
#include "sprite_env.h"
#include "sprite_shapes.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------- the draws
// 24 random bits of draw j of episode k of environment e: counter (e << 44) | ((k mod 2^24) << 20) | j of the site's stream
__host__ __device__ inline uint32_t env_bits24(unsigned long long seed, uint32_t e, uint32_t k, uint32_t j) {
    const uint64_t c = ((uint64_t)e << 44) | ((uint64_t)(k & 0xFFFFFFu) << 20) | (uint64_t)j;
    return rng_bits1_keyed(rng_key(seed, SITE_SPRITE_ENV, (uint32_t)(c >> 32)), (uint32_t)c) >> 8;
}

struct Stream {
    unsigned long long seed;
    uint32_t e, k, j;
    __device__ uint32_t bits() { return env_bits24(seed, e, k, j++); }
    __device__ int below(int m) { return (int)((bits() * (uint32_t)m) >> 24); }            // uniform in [0, m), m <= 256
    __device__ float u01() { return (float)bits() * (1.f / 16777216.f); }                  // k / 2^24 in [0, 1)
};

// [x_min, x_max, y_min, y_max] of object i (base.py:158-219)
__device__ inline void obj_box(int mode, int n, int i, float* b) {
    if (mode == 2) { b[0] = 0.f; b[1] = 1.f; b[2] = 0.f; b[3] = 1.f; return; }
    const bool left = i < 2, low = i == 1 || i == 2;
    if (mode == 1) {
        b[0] = left ? 0.f : 0.5f; b[1] = left ? 0.5f : 1.f;
        b[2] = low ? 0.f : 0.5f;  b[3] = low ? 0.5f : 1.f;
        return;
    }
    if (n == 4) {
        b[0] = left ? 0.2f : 0.7f; b[1] = left ? 0.3f : 0.8f;
        b[2] = low ? 0.2f : 0.7f;  b[3] = low ? 0.3f : 0.8f;
    } else {
        b[0] = left ? 0.15f : 0.65f; b[1] = left ? 0.35f : 0.85f;
        b[2] = low ? 0.15f : 0.65f;  b[3] = low ? 0.35f : 0.85f;
    }
}

__device__ inline float draw_pos(Stream& s, int mode, float lo, float hi, float r, float wall) {
    if (lo == hi) return lo;                                   // a degenerate interval takes no draw
    float a = lo, b = hi;
    if (mode != 0) { a = (lo + r) + wall; b = (hi - r) - wall; }
    const float w = b - a;
    const float p = w * s.u01();
    return a + p;
}

// the Target episode's objects: the target index, then every other object's triple, redrawn while it equals the target's -> target
__device__ int target_objects(const ocrl_sprite_env_desc& d, Stream& s, int n, float* col, float* shp, float* scl) {
    const int target = s.below(n);
    for (int i = 0; i < n; ++i) {
        int c = d.target_color, h = d.target_shape;
        float z = d.target_scale;
        if (i != target) {
            for (int t = 0; t < SPRITE_TRIPLE_TRIES; ++t) {
                c = d.colors[s.below(d.n_colors)];
                h = d.shapes[s.below(d.n_shapes)];
                z = d.scales[s.below(d.n_scales)];
                if (!(c == d.target_color && h == d.target_shape && z == d.target_scale)) break;
            }
        }
        col[i] = (float)c; shp[i] = (float)h; scl[i] = z;
    }
    return target;
}

// rule 6 of the Odd-One-Out episode: the objects of `todo` (a bit each) take values of A in groups of at least two
__device__ inline void ooo_fill(Stream& s, uint32_t todo, const float* A, int nA, float* out) {
    int z = __popc(todo);
    while (z > 0) {                                            // every round fills at least two objects, or the last one
        const float v = A[s.below(nA)];
        int g = 2 + s.below(z - 1);
        g = g > z ? z : g;                                     // z == 1 cannot begin a round (lo >= 3); it must not index outside either
        for (; g > 0; --g, --z) {
            uint32_t m = todo;
            for (int r = s.below(z); r > 0; --r) m &= m - 1;   // the r-th object still unfilled, in index order
            const int i = __ffs(m) - 1;
            out[i] = v;
            todo &= ~(1u << i);
        }
        if (z == 1) { out[__ffs(todo) - 1] = v; todo = 0u; z = 0; }
    }
}

// the Odd-One-Out episode's objects (oddoneout.py:19-126 as the header's rules 2 to 6) -> target; prop = colour, shape, scale rows
__device__ int ooo_objects(const ocrl_sprite_env_desc& d, Stream& s, int n, int& kind, float (*prop)[SPRITE_MAX_ROWS]) {
    float list[3][8];
    const int cnt[3] = {d.n_colors, d.n_shapes, d.n_scales};
    for (int i = 0; i < 8; ++i) { list[0][i] = (float)d.colors[i]; list[1][i] = (float)d.shapes[i]; list[2][i] = d.scales[i]; }
    const int target = d.unseen_mode ? 0 : s.below(n);
    int kinds[3] = {0, 0, 0}, nk = 0;
    for (int K = 0; K < 3; ++K)
        if (cnt[K] > 1) kinds[nk++] = K;
    const int T = kinds[s.below(nk)];
    const float u = d.unseen_mode == 2 ? (float)d.unseen_colors[s.below(2)] : list[T][s.below(cnt[T])];
    prop[T][target] = u;
    if (d.obj_comp)
        for (int K = 0; K < 3; ++K) {
            if (K == T) continue;
            const float v = list[K][s.below(cnt[K])];
            for (int i = 0; i < n; ++i) prop[K][i] = v;
        }
    const uint32_t all = (1u << n) - 1u;
    const float c0 = (float)d.unseen_colors[0], c1 = (float)d.unseen_colors[1];
    const bool paired = d.unseen_mode != 0 && T == 0 && (u == c0 || u == c1);
    const float other = u == c0 ? c1 : c0;
    for (int K = 0; K < 3; ++K) {
        if (K != T) {
            if (!d.obj_comp) ooo_fill(s, all, list[K], cnt[K], prop[K]);
            continue;
        }
        float A[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int nA = 0;
        for (int i = 0; i < cnt[K]; ++i) {
            const float v = list[K][i];
            bool ok = v != u;
            if (paired) ok = ok && (d.unseen_mode == 1 ? v != other : v == other);
            if (ok) A[nA++] = v;
        }
        ooo_fill(s, all & ~(1u << target), A, nA, prop[K]);
    }
    kind = T;
    return target;
}

// a new episode of environment e into its rows (R x 5) and aux words
__device__ void new_episode(const ocrl_sprite_env_desc& d, float* __restrict__ q, int* __restrict__ aux, unsigned long long seed, uint32_t e, uint32_t k) {
    const int R = d.hi + 1;
    Stream s{seed, e, k, 0u};
    const int n = d.lo + s.below(d.hi - d.lo + 1);
    float prop[3][SPRITE_MAX_ROWS], px[SPRITE_MAX_ROWS], py[SPRITE_MAX_ROWS];
    float *col = prop[0], *shp = prop[1], *scl = prop[2];
    int kind = 0;
    const int target = d.task == 1 ? ooo_objects(d, s, n, kind, prop) : target_objects(d, s, n, col, shp, scl);
    for (int i = 0; i < n; ++i) { px[i] = 0.f; py[i] = 0.f; }
    const float ax = d.mode == 2 ? d.agent_x : 0.5f, ay = d.mode == 2 ? d.agent_y : 0.5f;
    const float ra = d.agent_scale * 0.5f;
    for (int attempt = 0; attempt <= SPRITE_RESTARTS; ++attempt) {
        bool dead = false;
        for (int i = 0; i < n && !dead; ++i) {
            float b[4];
            obj_box(d.mode, n, i, b);
            const float r = scl[i] * 0.5f;
            bool ok = false;
            float x = 0.f, y = 0.f;
            for (int c = 0; c < SPRITE_CANDIDATES && !ok; ++c) {
                x = draw_pos(s, d.mode, b[0], b[1], r, d.dist_wall);
                y = draw_pos(s, d.mode, b[2], b[3], r, d.dist_wall);
                ok = true;
                for (int j = 0; j < i; ++j) {
                    const float thr = d.occlusion ? 0.15f : (r + scl[j] * 0.5f) + d.dist_objs;
                    if (dist2d(px[j], py[j], x, y) < thr) ok = false;
                }
                const float thr = d.occlusion ? 0.15f : (r + ra) + d.dist_agent;
                if (dist2d(ax, ay, x, y) < thr) ok = false;
            }
            px[i] = x; py[i] = y;
            if (!ok && attempt < SPRITE_RESTARTS) dead = true;  // restart the whole placement on fresh draws; on the last attempt the candidate stands
        }
        if (!dead) break;
    }
    for (int i = 0; i < R; ++i) {
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (i < n) { v[0] = col[i]; v[1] = shp[i]; v[2] = scl[i]; v[3] = px[i]; v[4] = py[i]; }
        else if (i == n) { v[0] = (float)d.agent_color; v[1] = (float)d.agent_shape; v[2] = d.agent_scale; v[3] = ax; v[4] = ay; }
        for (int c = 0; c < 5; ++c) q[i * 5 + c] = v[c];
    }
    aux[0] = n; aux[1] = target; aux[2] = 0; aux[3] = (int)k; aux[4] = 0; aux[5] = kind;
    *reinterpret_cast<double*>(aux + 6) = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- the transition
// One step of the environment (include/ocrl_hip.h: _step) from the rows q of an episode with n objects, `step_count` steps in: where the
// agent stands afterwards, what the step pays and whether it ends the episode.  Nothing is written: the environment's step
// (sprite_env.hip) commits the position or starts the next episode, the task datasets' walk (task_scenes.hip) commits it only while the
// episode goes on.  Both call this, so a walked frame is a frame the environment shows.
struct SpriteMove {
    float x, y, reward;
    bool done, success;
};
__device__ inline SpriteMove sprite_move(const ocrl_sprite_env_desc& d, const float* q, int n, int target, int step_count, long long act) {
    float x = q[n * 5 + 3], y = q[n * 5 + 4];
    const float tx = q[target * 5 + 3], ty = q[target * 5 + 4];
    const float before = dist2d(tx, ty, x, y);
    if (act == 0) y = y + d.step_size;
    else if (act == 1) x = x - d.step_size;
    else if (act == 2) y = y - d.step_size;
    else if (act == 3) x = x + d.step_size;                                  // anything else leaves the agent where it is
    const float ra = d.agent_scale * 0.5f, top = 1.0f - ra;
    x = fminf(fmaxf(x, ra), top);
    y = fminf(fmaxf(y, ra), top);
    bool done = step_count + 1 >= d.max_steps, success = false;
    float reward = 0.f;
    if (d.rew_type == 2) reward = dist2d(tx, ty, x, y) < before ? 0.01f : -0.01f;
    for (int i = 0; i < n; ++i) {
        if (dist2d(q[i * 5 + 3], q[i * 5 + 4], x, y) < d.agent_scale) {
            if (i == target) { reward = 1.0f; success = true; }
            else reward = d.rew_type == 1 ? 0.1f : 0.f;
            done = true;
            break;
        }
    }
    return SpriteMove{x, y, reward, done, success};
}

// the walk of a task dataset's later frames (include/ocrl_hip_rollout.h): the uniform random policy's action s is draw 2^19 + s of the
// episode's own stream and the drawn step count draw 2^19 - 1; an episode's own draws stop below 72 002 (sprite_env.h: SPRITE_MAX_DRAWS)
#define SPRITE_WALK_DRAW0 (1u << 19)
#define SPRITE_WALK_MAX_STEPS (1 << 19)     // draws 2^19 .. 2^20 - 1: what the 20 bits of j leave

}  // namespace
