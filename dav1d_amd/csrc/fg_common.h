// What the film grain kernels share (fg.hip: templates and the application into a picture; surface_grain.hip: the application fused into the
// surface export): the template geometry, the generator step, the parameters the kernels take and the template lookup.
#pragma once
#include "common.h"
#include "capi.h"
#include <string.h>

namespace {

enum { GW = 82, GH = 73, SGW = 44, SGH = 38 };

__device__ __forceinline__ unsigned lfsr_step(const unsigned r) {
    const unsigned bit = ((r >> 0) ^ (r >> 1) ^ (r >> 3) ^ (r >> 12)) & 1;
    return (r >> 1) | (bit << 15);
}
__device__ __forceinline__ int round2(const int x, const int shift) { return (x + ((1 << shift) >> 1)) >> shift; }

struct FgParams {                 // the scalar part of Dav1dFilmGrainData the kernels need
    unsigned seed;
    int num_y_points, chroma_scaling_from_luma, num_uv_points[2];
    int scaling_shift, ar_coeff_lag, ar_coeff_shift, grain_scale_shift;
    int uv_mult[2], uv_luma_mult[2], uv_offset[2];
    int overlap_flag, clip_to_restricted_range;
    int8_t ar_coeffs_y[24];
    int8_t ar_coeffs_uv[2][28];
};

// sample_lut, src/filmgrain_tmpl.c:156-167
__device__ __forceinline__ int sample_lut(const int16_t *lut, const int randval, const int subx, const int suby,
                                          const int bx, const int by, const int x, const int y)
{
    const int offx = 3 + (2 >> subx) * (3 + (randval >> 4));
    const int offy = 3 + (2 >> suby) * (3 + (randval & 0xF));
    return lut[(offy + y + (32 >> suby) * by) * GW + offx + x + (32 >> subx) * bx];
}

inline FgParams make_params(const Dav1dHipFilmGrainData *d) {
    FgParams p;
    memset(&p, 0, sizeof(p));
    p.seed = d->seed; p.num_y_points = d->num_y_points; p.chroma_scaling_from_luma = d->chroma_scaling_from_luma;
    p.scaling_shift = d->scaling_shift; p.ar_coeff_lag = d->ar_coeff_lag; p.ar_coeff_shift = (int) d->ar_coeff_shift;
    p.grain_scale_shift = d->grain_scale_shift; p.overlap_flag = d->overlap_flag; p.clip_to_restricted_range = d->clip_to_restricted_range;
    for (int i = 0; i < 2; i++) {
        p.num_uv_points[i] = d->num_uv_points[i];
        p.uv_mult[i] = d->uv_mult[i]; p.uv_luma_mult[i] = d->uv_luma_mult[i]; p.uv_offset[i] = d->uv_offset[i];
        memcpy(p.ar_coeffs_uv[i], d->ar_coeffs_uv[i], 28);
    }
    memcpy(p.ar_coeffs_y, d->ar_coeffs_y, 24);
    return p;
}

} // namespace
