// What the sprite environments (sprite_env.hip, task_scenes.hip) and the pre-training scenes (scenes.hip) draw alike: the distance of two
// centres, the shape predicates, which rows are painted and the colour table.  All three files are compiled with -ffp-contract=off: every
// expression here is the written sequence of fp32 roundings, which the numpy restatements (tests/sprite_env_ref.py, tests/scenes_ref.py,
// tests/ood_shapes_ref.py) follow bit for bit.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

__device__ inline float dist2d(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    const float xx = dx * dx, yy = dy * dy;
    return sqrtf(xx + yy);
}

// The shape ids are the names' indices in the reference's SHAPES list; six of them are drawn: 0 square, 1 triangle, 2 star_4, 3 circle,
// 7 star_5, 9 spoke_4.  The one place that says so: the library's validation (sprite_env_unit.cpp) and the painted rows below read it.
#define SPRITE_DRAWN_SHAPES 0x28Fu          // bit id set: drawn
__host__ __device__ inline bool sprite_shape_drawn(int id) { return id >= 0 && id < 10 && ((SPRITE_DRAWN_SHAPES >> id) & 1u) != 0u; }

// Which rows (colour id, shape id, scale, ..) the renderers paint: a colour in 0..6, a drawn shape id (the value truncated, as the
// tables are indexed) and a scale > 0.  Colour -1, every other shape id and an empty row (the padding after the agent) are not painted.
__device__ inline bool sprite_row_drawn(float c, float h, float z) {
    return c >= 0.f && c < 7.f && h >= 0.f && h < 10.f && sprite_shape_drawn((int)h) && z > 0.f;
}

// One tip of star_5 whose axis points along (s, -c) (s, c: sine and cosine of the tip's angle from straight up; up is -y): a runs along
// the axis, b is the distance from it.  The tip's triangle: its apex at a = tip, its two sides through the neighbouring notches
// (a, b) = (an, +-bn), cut off at a = 0.  run = tip - an.
__device__ inline bool star5_tip(float dx, float ny, float s, float c, float tip, float run, float bn) {
    const float a = dx * s + ny * c;
    const float b = fabsf(dx * c - ny * s);
    return a >= 0.f && b * run <= bn * (tip - a);
}

// star_5: the ten-vertex star polygon with tips at radius 1.25 r, 72 degrees apart from straight up, and notches at 0.63 r halfway
// between them, as the union of the five tips' triangles.  A triangle's base at a = 0 has the half width 1.25 r * bn / run = 0.6252 r
// and ends 18 degrees off the neighbouring tips' axes, where the polygon reaches 0.797 r: what a triangle adds to its tip's kite
// (centre, notch, tip, notch) lies inside the neighbours' kites, so the union is the polygon itself.  The triangles overlap, so there
// is no seam between tips for a rounding to open (wedges |b| <= a tan 36 would leave one, straight down from the centre among others).
// sin and cos of 72 and 144 degrees and 0.63 * (cos, sin) of 36 degrees are fp32 constants: no sinf, cosf or atan2f at run time.
__device__ inline bool star5_covers(float dx, float dy, float r) {
    const float ny = -dy, tip = 1.25f * r, an = 0.5096807f * r, bn = 0.3703047f * r;
    const float run = tip - an;
    const bool t0 = star5_tip(dx, ny, 0.f, 1.f, tip, run, bn);
    const bool t1 = star5_tip(dx, ny, 0.95105654f, 0.309017f, tip, run, bn);
    const bool t2 = star5_tip(dx, ny, 0.58778524f, -0.809017f, tip, run, bn);
    const bool t3 = star5_tip(dx, ny, -0.58778524f, -0.809017f, tip, run, bn);
    const bool t4 = star5_tip(dx, ny, -0.95105654f, 0.309017f, tip, run, bn);
    return t0 | t1 | t2 | t3 | t4;
}

// spoke_4: an upright Greek cross, two bars of half width 0.4 r and half length 1.25 r
__device__ inline bool spoke4_covers(float ax, float ay, float r) {
    const float w = 0.4f * r, l = 1.25f * r;
    return (ax <= w && ay <= l) || (ay <= w && ax <= l);
}

// the predicates of ocrl_amd/utils/data.py:_mask in fp32; (dx, dy) = pixel centre - sprite centre, r = scale / 2
__device__ inline bool sprite_covers(int shape, float dx, float dy, float r) {
    const float ax = fabsf(dx), ay = fabsf(dy);
    if (shape == 0) return ax <= r && ay <= r;
    if (shape == 1) {
        const float t = (dy + r) / (2.f * r);
        return t >= 0.f && t <= 1.f && ax <= r * t;
    }
    if (shape == 2) return sqrtf(ax) + sqrtf(ay) <= sqrtf(r) * 1.25f;
    if (shape == 7) return star5_covers(dx, dy, r);
    if (shape == 9) return spoke4_covers(ax, ay, r);
    const float xx = dx * dx, yy = dy * dy;
    return xx + yy <= r * r;
}

// A bound for every predicate above: none covers a pixel whose |dx| or |dy| exceeds 1.6 r (star_4 reaches 1.5625 r along the axes, give
// or take the rounding of its roots; star_5 and spoke_4 1.25 r; the others r).  The renderers test a pixel row's dy against it before
// any predicate runs; where it fails every predicate is false, so the frames are the same bits with or without the test.
__device__ inline bool sprite_in_reach(float d, float r) { return fabsf(d) <= 1.6f * r; }

static __constant__ uint32_t SPRITE_RGB[7] = {0xFF0000u, 0x00FF00u, 0x00FFFFu, 0x0000FFu, 0xFFFF00u, 0xCBC0FFu, 0x2A2AA5u};       // byte 0 = red
