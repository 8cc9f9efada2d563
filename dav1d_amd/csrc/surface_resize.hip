// Tensor-ready RGB at any size: dav1d_hip_surface_export_rgb_resized, dav1d_hip_surface_rgb_resized_rows_needed and
// dav1d_hip_surface_export_rgb_resized_batch (include/dav1d_hip.h).  They write what dav1d_hip_surface_export_rgb writes from the
// picture Q whose planes are R of the crop windows: per plane and per axis, the area scaler S where the axis goes down or keeps its length, linear
// interpolation with half-sample centres where it goes up.  One pass over the source, one launch; Q never reaches memory.
//
// The kernel is surface_rgb_scale.hip's — scale_rgbx_cell of surface_common.h, its cells, its ring, its output — instantiated with RESIZE: an axis
// whose bit of ScalePlane::up is set takes the bounds of its LDS window (scale_span) and its taps (resize_weights) from R.
//   window  (o s) / d - 1 <= i0(o) <= (o s) / d for s < d, so n consecutive outputs of an axis that goes up hold their taps in at most n + 2 samples from
//           max((o0 s) / d - 1, 0) on (scale_span; a sample at either end may go unused, it lies inside the crop window).  The largest cell, 128 across
//           and 8 down (the cell of every ratio up to 2:1, so of every axis that goes up), reads at most 130 columns and 10 rows, from an alignment
//           offset of up to 7: 18 units and 17 rows of the SC_MAXU = 33 and SC_MAXR = 40 that LDS holds.  No growth.
//   taps    one or two per output, 12-bit weights that sum to 4096, both positive: the two taps of the definition are merged where the clamp to the
//           window puts them on one sample (the first and last outputs) and a tap of weight 0 is dropped, so nothing outside the crop window of the
//           plane is read.  The passes down and across, their roundings and the 24-bit multiplies are S's.
//   mixing  the flags are the plane's: an item may go up across and down down, luma may go up where chroma keeps its length (h = 3 to 4 at 4:2:0).
// The batch is surface_batch.hip's (surface_batch.h): the same table, search, staging ring and two launches for mixed picture states.
#include "surface_batch.h"

namespace {

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256, sizeof(pixel) == 1 ? 5 : 4) void surface_resize_rgbx_kernel(const ScaleRgbxArgs a, const Out out)
{
    __shared__ ScaleLds<pixel> L;
    scale_rgbx_cell<pixel, TILED, Out, true>(L, a, (int) blockIdx.x, out);
}

// ---- the host side

template <typename pixel, bool TILED, typename Out>
int launch_rgbx_resized(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                        const ScaleGeom &g, const Dav1dHipRgbParams &p, const int row0, const int row1, const Out &out)
{
    unsigned n_groups;
    const ScaleRgbxArgs a = make_scale_rgbx_args<pixel, TILED, typename Out::T>(dst, src, planes, g, p, row0, row1, &n_groups);
    hipLaunchKernelGGL((surface_resize_rgbx_kernel<pixel, TILED, Out>), dim3(n_groups), dim3(256), 0, c->stream, a, out);
    return hip_rc(hipGetLastError());
}

// what dav1d_hip_surface_export_rgb_scaled refuses, in its order, less the size rule; then the filter
int resized_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, const Dav1dHipRgbParams &p,
                       const int filter, const int row0, const int row1, SurfaceCall *const call, ScaleGeom *const g)
{
    if (const int rc = rgbx_scaled_args_check(dst, src, crop, p, row0, row1, call, g, true)) return rc;
    return filter == DAV1D_HIP_RESIZE_BILINEAR ? 0 : -ENOTSUP;
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_resized(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                    const Dav1dHipRgbParams *params, int filter, int drow0, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    ScaleGeom g;
    if (!c) return -EINVAL;
    if (const int rc = resized_args_check(dst, src, crop, p, filter, drow0, drow1, &call, &g)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    const int row0 = call.row0, row1 = call.row1;
    if (row1 <= row0) return 0;
    void *const *const planes = call.planes;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        typedef decltype(px) pixel;
        return with_rgb_out<pixel>(dst->sample, p, src->bpc, [&](const auto &out) {
            return launch_rgbx_resized<pixel, decltype(state)::value>(c, dst, src, planes, g, p, row0, row1, out);
        });
    }));
}

extern "C" int dav1d_hip_surface_rgb_resized_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                         const Dav1dHipRgbParams *params, int filter, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    ScaleGeom g;
    return sized_rows_needed(resized_args_check(dst, src, crop, p, filter, 0, drow1, &call, &g), call, g, p.chroma_pos != 0, src);
}

extern "C" int dav1d_hip_surface_export_rgb_resized_batch(Dav1dHipContext *c, int n, const Dav1dHipSurface *dst, const Dav1dHipPicture *const *src,
                                                          const Dav1dHipSurfaceRect *crop, const Dav1dHipRgbParams *params, int filter, int *bad_item)
{
    return export_batch_call<true>(c, n, dst, src, crop, params, filter == DAV1D_HIP_RESIZE_BILINEAR ? 0 : -ENOTSUP, bad_item);
}
