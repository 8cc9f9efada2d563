// Tensor-ready RGB at another size: dav1d_hip_surface_export_rgb_scaled (include/dav1d_hip.h) writes what dav1d_hip_surface_export_rgb
// writes from the picture Q whose planes are the scaled planes of dav1d_hip_surface_export_scaled.  One pass over the source where it lives, one launch;
// the scaled planes never reach memory.
//
// The frame is surface_scale.hip's RGB kernel: a workgroup of four waves owns a cell of Q's chroma planes, scales U and V into LDS, then scales the luma
// above the cell piece by piece and converts.  Two things differ.
//   ring    at chroma_pos != 0 a luma sample takes up to 2 x 2 samples of Q's chroma: its own, the column to the right, and the row below (chroma_pos
//           1: above or below).  The workgroup scales the cell and that part of a ring around it — one column on the right, one row below, at
//           chroma_pos 1 one above — clamped to Q's chroma plane: the cl() of the definition, not a read outside the crop.  scale_cell holds at most
//           SC_OW x SC_OR outputs and a window of SC_MAXU units x SC_MAXR rows, which any SC_OW / 64 / 32 x SC_OR / 4 consecutive outputs of their
//           ratio class fit; so the OWNED cell shrinks where an axis has a ring and cell + ring keeps the window, LDS and occupancy of today:
//           ow - 4 = 124 / 60 / 28 across (a multiple of 4: the luma above a cell then starts at a multiple of 8 samples, a lane's 8-sample unit stays
//           whole and its 16-byte stores aligned) and oh - 2 = 6 / 2 (chroma_pos 1) or oh - 1 = 7 / 3 (chroma_pos 2) down.  Without a ring
//           (chroma_pos 0, 4:4:4, 4:0:0; 4:2:2 down) the cell is the scaler's.
//   output  surface_rgb.hip's: U and V are scaled into one array of words (u | v << 16: scale_cell's HALF 1, 2), the vertical taps (sum 4) and the horizontal
//           taps (sum 2) run on both halves at once, one rounding (s + 4) >> 3; the colour terms are v_mad_i32_i24; planes leave through store_run,
//           packed runs of 24 / 32 samples through store_packed.
//
// The kernel's body is scale_rgbx_cell of surface_common.h, and the host side that checks a call and fills ScaleRgbxArgs is there too: surface_batch.hip
// runs the same body from a table of such calls.
#include "surface_call.h"

namespace {

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_scale_rgbx_kernel(const ScaleRgbxArgs a, const Out out)
{
    __shared__ ScaleLds<pixel> L;
    scale_rgbx_cell<pixel, TILED, Out>(L, a, (int) blockIdx.x, out);
}

// ---- the host side

template <typename pixel, bool TILED, typename Out>
int launch_rgbx_scaled(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                       const ScaleGeom &g, const Dav1dHipRgbParams &p, const int row0, const int row1, const Out &out)
{
    unsigned n_groups;
    const ScaleRgbxArgs a = make_scale_rgbx_args<pixel, TILED, typename Out::T>(dst, src, planes, g, p, row0, row1, &n_groups);
    hipLaunchKernelGGL((surface_scale_rgbx_kernel<pixel, TILED, Out>), dim3(n_groups), dim3(256), 0, c->stream, a, out);
    return hip_rc(hipGetLastError());
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_scaled(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                   const Dav1dHipRgbParams *params, int drow0, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    ScaleGeom g;
    if (!c) return -EINVAL;
    if (const int rc = rgbx_scaled_args_check(dst, src, crop, p, drow0, drow1, &call, &g)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    const int row0 = call.row0, row1 = call.row1;
    if (row1 <= row0) return 0;
    void *const *const planes = call.planes;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        typedef decltype(px) pixel;
        return with_rgb_out<pixel>(dst->sample, p, src->bpc, [&](const auto &out) {
            return launch_rgbx_scaled<pixel, decltype(state)::value>(c, dst, src, planes, g, p, row0, row1, out);
        });
    }));
}

extern "C" int dav1d_hip_surface_rgb_scaled_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                        const Dav1dHipRgbParams *params, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    ScaleGeom g;
    return sized_rows_needed(rgbx_scaled_args_check(dst, src, crop, p, 0, drow1, &call, &g), call, g, p.chroma_pos != 0, src);
}
