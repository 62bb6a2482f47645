// C ABI of the pre-training scenes (include/ocrl_hip.h: ocrl_scenes_*).  Stateless: the caller owns every buffer.
#include "scenes.h"

extern "C" {

int ocrl_scenes_batch(const ocrl_scenes_desc* d, unsigned long long seed, const long long* indices, int B, float* obs, unsigned char* obs_u8,
                      float* masks, float* objs, void* stream) {
    OCRL_REQUIRE(d, "ocrl_scenes_batch: null descriptor");
    OCRL_REQUIRE(d->H >= 8 && d->H <= 512 && d->H % 4 == 0, "ocrl_scenes_batch: obs_size must be a multiple of 4 in [8, 512] (got %d)", d->H);
    OCRL_REQUIRE(d->K >= 1 && d->K <= SCENES_MAX_OBJS, "ocrl_scenes_batch: 1 <= objects <= %d (got %d)", SCENES_MAX_OBJS, d->K);
    OCRL_REQUIRE(B >= 1, "ocrl_scenes_batch: batch >= 1 (got %d)", B);
    OCRL_REQUIRE(indices, "ocrl_scenes_batch: null indices");
    OCRL_REQUIRE(obs || obs_u8 || masks || objs, "ocrl_scenes_batch: no output requested (obs, obs_u8, masks and objs are all null)");
    OCRL_REQUIRE(((uintptr_t)obs | (uintptr_t)masks) % 16 == 0 && (uintptr_t)obs_u8 % 4 == 0,
                 "ocrl_scenes_batch: obs and masks must be 16-byte aligned, obs_u8 4-byte aligned");
    OCRL_REQUIRE((long long)B * cdiv(d->H, scenes_band_rows(d->H)) < (1LL << 31), "ocrl_scenes_batch: %d scenes of %d rows exceed one launch", B, d->H);
    return scenes_batch_launch(d->H, d->K, seed, indices, B, ScenesOut{obs, obs_u8, masks, objs}, static_cast<hipStream_t>(stream));
}

int ocrl_scenes_uniforms(unsigned long long seed, long long index, int first, int n, float* out, void* stream) {
    OCRL_REQUIRE(out && n >= 1, "ocrl_scenes_uniforms: null output or n < 1");
    OCRL_REQUIRE(first >= 0 && (long long)first + n <= (1LL << SCENES_DRAW_BITS), "ocrl_scenes_uniforms: draws < 2^%d (got first %d, n %d)", SCENES_DRAW_BITS,
                 first, n);
    return scenes_uniforms_launch(seed, index, first, n, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
