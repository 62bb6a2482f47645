// Shared helpers for the ocrl_hip kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// one v_mfma_f32_16x16x4_f32 step: c += a (16 x 4, one float per lane) * b (4 x 16), c a lane's four accumulator rows
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ---- error convention: every C-ABI entry returns 0 on success; message via ocrl_last_error()
void ocrl_set_error(const char* fmt, ...);

#define OCRL_REQUIRE(cond, ...)                         \
    do {                                                \
        if (!(cond)) {                                  \
            ocrl_set_error(__VA_ARGS__);                \
            return 1;                                   \
        }                                               \
    } while (0)

// propagates a non-zero status of an internal call (the message is already set)
#define RC(x)                  \
    do {                       \
        int rc__ = (x);        \
        if (rc__) return rc__; \
    } while (0)

#define OCRL_CHECK_LAUNCH(name)                                              \
    do {                                                                     \
        hipError_t e__ = hipGetLastError();                                  \
        if (e__ != hipSuccess) {                                             \
            ocrl_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

#define OCRL_HIP(call)                                                       \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) {                                             \
            ocrl_set_error("%s failed: %s", #call, hipGetErrorString(e__));  \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// carves a workspace into 256-byte aligned blocks: take(n) returns the float offset of the next n floats; `end` is the total
struct WsTake {
    size_t end = 0;
    size_t operator()(size_t n) { const size_t r = end; end += (n + 63) & ~(size_t)63; return r; }
};

// ---- counter-based RNG: stateless, so forward and backward regenerate the same dropout decisions without storing masks.
// 64 bits per call from two passes of a 32-bit avalanche mixer (two multiplies and three xor-shifts each; the "lowbias32" constants,
// bias 0.17 %) over the element counter xor a per-(seed, site) key, with the key added once more inside the mixer (rng_mix32k).  Round 1 used Philox-2x32-7 (14 quarter-rate integer multiplies per
// call); this form needs 4 (measured: +0.4 % images/s — the Gumbel kernel turned out to be bound by its logs and exp, not the draws).
// tests/test_gpu_determinism.py::test_device_rng_quality checks rates, serial and cross-site / cross-seed correlations.
__host__ __device__ inline uint32_t rng_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// 64 random bits for the group of four consecutive elements idx4 = element_index / 4 at `site`.
// key: uniform over a launch (scalar work); the high counter bits enter here so that >2^32 groups do not repeat
__host__ __device__ inline uint32_t rng_key(uint64_t seed, uint32_t site, uint32_t idx4_hi) {
    return rng_mix32((uint32_t)seed ^ (site * 0x9E3779B9u)) ^ rng_mix32((uint32_t)(seed >> 32) + 0x85EBCA6Bu * (idx4_hi + 1u));
}
// The key enters twice: xor-ed into the counter and, through a second word derived from it, ADDED between the mixer's two multiplies.
// With the xor alone every (seed, site) stream was the same fixed permutation of the counter, translated: stream A at group i equalled
// stream B at group i ^ (kA ^ kB), so two steps or sites could share a whole noise field as a block permutation.  The addition after the
// first multiply does not commute with the xor-translate (tests/test_gpu_determinism.py::test_device_rng_streams_are_not_translates).
__host__ __device__ inline uint32_t rng_mix32k(uint32_t x, uint32_t k2) {
    x ^= x >> 16; x *= 0x7FEB352Du;
    x += k2;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint2 rng_bits4_keyed(uint32_t key, uint32_t idx4_lo) {
    const uint32_t c = idx4_lo ^ key;
    const uint32_t k2 = key * 0x9E3779B9u + 0x7F4A7C15u;      // uniform over a launch: scalar work
    return make_uint2(rng_mix32k(c, k2), rng_mix32k(c ^ 0x68E31DA4u, k2) + key);
}
// the first word alone (callers that need one uniform per counter)
__host__ __device__ inline uint32_t rng_bits1_keyed(uint32_t key, uint32_t idx_lo) {
    return rng_mix32k(idx_lo ^ key, key * 0x9E3779B9u + 0x7F4A7C15u);
}
__host__ __device__ inline uint2 rng_bits4(uint64_t seed, uint32_t site, uint64_t idx4) {
    return rng_bits4_keyed(rng_key(seed, site, (uint32_t)(idx4 >> 32)), (uint32_t)idx4);
}

// keep decision for element e (0..3) of a group: 16-bit uniform >= thresh, thresh = round(p * 65536)
__host__ __device__ inline bool rng_keep(uint2 bits, int e, uint32_t thresh) {
    const uint32_t w = (e & 2) ? bits.y : bits.x;
    const uint32_t u = (e & 1) ? (w >> 16) : (w & 0xFFFFu);
    return u >= thresh;
}
__host__ __device__ inline uint32_t drop_thresh(float p) { return (uint32_t)(p * 65536.0f + 0.5f); }

// two 24-bit uniforms in (0,1) from a 64-bit draw
__host__ __device__ inline float u01_24(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// dropout site ids (shared by forward, backward and the mask dump used by the parity tests)
enum : uint32_t {
    SITE_ZPOS = 1,
    SITE_BLK_BASE = 16,   // + 8 * block + {0: self.attn, 1: self.out, 2: cross.attn, 3: cross.out, 4: ffn}
    SITE_GUMBEL_Z = 200,
    SITE_GUMBEL_ZH = 201,
    SITE_SLOT_NOISE = 202,
};

// Dropout index contract of the causal self-attention probabilities (site SITE_BLK_BASE + 8 * block + 0; csrc/attention.hip):
// the keep decision of (image b, head, query q, key) is element
//     i = ((b * h + head) * T + q) * T4 + key,     T4 = attn_drop_ld(T) = T rounded up to a multiple of 4,
// i.e. group i >> 2, slot i & 3 = key & 3 of the site's stream.  Every row starts on a group boundary, so the four kernels (which
// draw one group per four consecutive keys) and the mask dump agree for every T; the dump of the site is [B, h, T, T4], of which
// [..., :T] is the mask.  For T % 4 == 0 this is the dense index ((b * h + head) * T + q) * T + key.
__host__ __device__ inline int attn_drop_ld(int T) { return (T + 3) & ~3; }

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ inline float elu_(float v) { return v > 0.f ? v : expf(v) - 1.f; }
// coordinate i of S evenly spaced points over [-1, 1] (IODINE's coordinate channels)
__device__ inline float io_lin(int i, int S) { return S > 1 ? -1.f + 2.f * (float)i / (float)(S - 1) : -1.f; }

// ---- reductions whose order is part of the result.  The library is tested to the bit (two-run determinism, fused == unfused, fixture
// replays), so each order is written once, here; wave_sum / wave_max above run their xor-shuffle stages 32 -> 1.
//
// Sum over an aligned group of 16 lanes: xor-shuffle stages 1, 2, 4, 8.  Not wave_sum cut short: that runs the stages downwards, which
// is another association of the same sum.
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Arg-max over a wave, stages 32 -> 1: the other lane's pair is taken when its value is greater, or equal with a smaller index -- the
// first index wins ties, like torch.argmax on the CPU.  Every lane ends with the wave's pair.
__device__ __forceinline__ void wave_argmax(float& best, int& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
}
// Fixed halving tree over red[0 .. N) in LDS, N = the workgroup's size, filled and synchronised by the caller: level o = N/2, N/4, .. 1
// does red[t] (op)= red[t + o] for t < o, with a barrier after every level.  The result is red[0], valid for every thread on return; a
// caller that goes on to overwrite `red` puts its own barrier after reading it.
template <int N>
__device__ __forceinline__ void block_tree_sum(float* red) {
    const int t = threadIdx.x;
    for (int o = N / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
}
template <int N>
__device__ __forceinline__ void block_tree_max(float* red) {
    const int t = threadIdx.x;
    for (int o = N / 2; o > 0; o >>= 1) {
        if (t < o) red[t] = fmaxf(red[t], red[t + o]);
        __syncthreads();
    }
}

// ---- host side (the launchers)
// every pointer 16-byte aligned (float4 access); a null pointer, an optional tensor left out, counts as aligned (uintptr_t: <stdint.h> above)
template <typename... P>
static inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// one thread per element, 256 to a workgroup
#define GRID1D(n) dim3(cdiv((n), 256)), dim3(256)
