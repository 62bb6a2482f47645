// The row arithmetic of the 16-lane LayerNorm (eps 1e-5, biased variance): 16 lanes own a row of F = 64 * NV floats, lane c4 holding
// the NV float4 at columns (k * 16 + c4) * 4, k = 0 .. NV-1.  layernorm16_fwd_kernel / layernorm16_bwd_kernel (elementwise.hip) and the
// fused slot-attention input chain (sa_input.hip) all call these functions, which is what makes their results equal bit for bit.
//
// The build contracts a * b + c to an FMA, so the shape of every expression below (parentheses, the order of `* rs * g + b`) is part of
// the result; where a shape leaves the compiler two ways to contract, the one to take is written out (layernorm16_row_fwd).
// __forceinline__: sa_input's kernels sit at their register budget and cannot afford a call.
#pragma once
#include "common.h"

// A lane's partial sum over its float4 starts from its first term when there is one float4 and from +0 when there are more; the two
// differ when every term is -0 (the sign then travels through x - mu), and each width keeps what it has always computed.  -0 is the
// identity of the addition for every float, so seeding with it leaves the first term as it is.
template <int NV>
constexpr float LN16_SEED = NV == 1 ? -0.f : 0.f;

// The forward of a row in two steps: layernorm16_row_fwd leaves mu and rs (equal in the group's 16 lanes) and turns this lane's NV
// float4 of the row, v, into dd = x - mu; layernorm16_affine is y = dd * rs * g + b of one float4.  The kernels call the second step
// where they store y (under their guard that the row exists), and sa_input's backward calls it alone to rebuild LN(e4).
template <int NV>
__device__ __forceinline__ void layernorm16_row_fwd(float4* v, float& mu, float& rs) {
    static_assert(NV == 1 || NV == 3, "the contraction rule below is that of the 64- and 192-wide kernels");
    constexpr float inv_f = 1.0f / (64 * NV);
    float s = LN16_SEED<NV>;
#pragma unroll
    for (int k = 0; k < NV; ++k) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    mu = group16_sum(s) * inv_f;
    float q = LN16_SEED<NV>;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const float4 d = make_float4(v[k].x - mu, v[k].y - mu, v[k].z - mu, v[k].w - mu);
        // a*a + b*b can contract to fma(a, a, b*b), to fma(b, b, a*a) or not at all, and the compiler's choice depends on the code
        // around the expression, so the one to take is written out.  It is the one the 64- and 192-wide kernels have always computed
        // and serves those two widths only: the first product fused for a lane's first two float4, both products rounded for the
        // third.  A new width chooses its own rule here (the static_assert above).
        if (k < 2) q += fmaf(d.x, d.x, d.y * d.y) + fmaf(d.z, d.z, d.w * d.w);
        else {
#pragma clang fp contract(off)
            q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
        v[k] = d;
    }
    rs = rsqrtf(group16_sum(q) * inv_f + 1e-5f);
}
__device__ __forceinline__ float4 layernorm16_affine(float4 dd, float rs, float4 g, float4 b) {
    return make_float4(dd.x * rs * g.x + b.x, dd.y * rs * g.y + b.y, dd.z * rs * g.z + b.z, dd.w * rs * g.w + b.w);
}

// The backward of a row, dx = rs * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)), in two steps, because its callers store dx under a guard
// (the row exists) and every lane of the group has to reach the shuffles: layernorm16_row_bwd adds the row's terms into this lane's
// dgamma / dbeta accumulators dg / db and returns what dx needs; layernorm16_row_dx, called under the guard, is dx of float4 k.
template <int NV>
struct Ln16Bwd {
    float4 xh[NV], d4[NV];     // xhat and dy * gamma
    float s1, s2;              // mean(dy*g), mean(dy*g*xhat)
};
template <int NV>
__device__ __forceinline__ Ln16Bwd<NV> layernorm16_row_bwd(const float4* x, const float4* dy, float mu, float rs, const float4* g, float4* dg, float4* db) {
    constexpr float inv_f = 1.0f / (64 * NV);
    Ln16Bwd<NV> r;
    float s1 = LN16_SEED<NV>, s2 = LN16_SEED<NV>;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        r.xh[k] = make_float4((x[k].x - mu) * rs, (x[k].y - mu) * rs, (x[k].z - mu) * rs, (x[k].w - mu) * rs);
        const float4 yy = dy[k], xh = r.xh[k];
        dg[k].x += yy.x * xh.x; dg[k].y += yy.y * xh.y; dg[k].z += yy.z * xh.z; dg[k].w += yy.w * xh.w;
        db[k].x += yy.x; db[k].y += yy.y; db[k].z += yy.z; db[k].w += yy.w;
        const float4 d4 = r.d4[k] = make_float4(yy.x * g[k].x, yy.y * g[k].y, yy.z * g[k].z, yy.w * g[k].w);
        s1 += (d4.x + d4.y) + (d4.z + d4.w);
        {   // as ambiguous as the squares of the forward; here all four products have always been rounded, at both widths
#pragma clang fp contract(off)
            s2 += (d4.x * xh.x + d4.y * xh.y) + (d4.z * xh.z + d4.w * xh.w);
        }
    }
    r.s1 = group16_sum(s1) * inv_f;
    r.s2 = group16_sum(s2) * inv_f;
    return r;
}
template <int NV>
__device__ __forceinline__ float4 layernorm16_row_dx(const Ln16Bwd<NV>& r, float rs, int k) {
    const float4 d4 = r.d4[k], xh = r.xh[k];
    return make_float4(rs * (d4.x - r.s1 - xh.x * r.s2), rs * (d4.y - r.s1 - xh.y * r.s2), rs * (d4.z - r.s1 - xh.z * r.s2), rs * (d4.w - r.s1 - xh.w * r.s2));
}
