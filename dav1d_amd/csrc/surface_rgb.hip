// Tensor-ready RGB (dav1d_hip_surface_export_rgb, include/dav1d_hip.h): the RGB export of surface.hip with chroma upsampled at its
// site, packed RGB / RGBA rows next to the planes, binary16 next to float32, and a per-channel normalisation.  Like its siblings one
// bandwidth-bound integer pass without LDS; `src` is read where it lives, raster planes or tiled twin.
//
// The unit is the export's: a lane holds 8 adjacent chroma pairs and serves the (8 << SSH) x (1 << SSV) luma samples above them, a wave a 64 x 8
// cell of the chroma plane (lane = row * 8 + unit), every load a whole line.  What the bilinear taps need beyond a lane's own 8 pairs — one
// pair to the right, the row above, the row below — comes from the neighbouring lanes of the wave (lane + 1, lane - 8, lane + 8: cross-lane
// shuffles of registers, no LDS staging and no scratch), and at the cell's right column, its top row and its bottom row (or the first / last
// chroma row of a band) from one more load: the row above / below as a load8, the column to the right as the one sample that is needed.  A wave
// requests every line it touches once.  Built this way rather than by staging cell + halo in LDS because the pairs are in registers already when
// they are needed and the exchange is a handful of ds_bpermute per wave: an LDS image would add a write, a wait and a read of everything for
// the same loads.
//
// The arithmetic runs on U and V at once: a pair is u | v << 16, the tap sums stay below 8 * 4095 + 4 < 2^16, so one 32-bit add or shift serves
// both halves.  The vertical taps (sum 4) are applied first, without rounding: P[i][m] for luma row i of the lane and chroma column m = 0 .. 8
// (8: the neighbour to the right); the horizontal taps (sum 2) and the single rounding (+ 4) >> 3 follow per luma sample.  Columns right of the
// plane repeat its last one (the clamp of the definition), rows above / below it repeat the first / last.
#include "surface_call.h"

namespace {

// today's sample: one channel at a time, out(v, c)
template <typename Out> struct PerChannel {
    typedef typename Out::T T;
    Out out; T alpha;
    __device__ __forceinline__ void operator()(const int r, const int g, const int b, T &R, T &G, T &B) const { R = out(r, 0); G = out(g, 1); B = out(b, 2); }
};

template <typename pixel, bool TILED, int SSH, int SSV, typename Out>
__global__ __launch_bounds__(64) void surface_rgbx_kernel(const RgbxArgs ax, const Out out)
{
    const PerChannel<Out> fn = { out, out.alpha };
    rgbx_cell<pixel, TILED, SSH, SSV>(ax, (int) blockIdx.x, fn);
}

template <typename pixel, bool TILED, typename Out>
int launch_rgbx(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                const Dav1dHipRgbParams &p, const int row0, const int row1, const Out &out)
{
    typedef typename Out::T T;
    unsigned n_cells;
    const RgbxArgs ax = make_rgbx_args<pixel, TILED, T>(dst, src, planes, p, row0, row1, &n_cells);
    const SurfaceGeom g = surface_geom(src, row0, row1);
    const dim3 grid(n_cells);
    hipStream_t st = c->stream;
    if (g.ss_ver) hipLaunchKernelGGL((surface_rgbx_kernel<pixel, TILED, 1, 1, Out>), grid, dim3(64), 0, st, ax, out);
    else if (g.ss_hor) hipLaunchKernelGGL((surface_rgbx_kernel<pixel, TILED, 1, 0, Out>), grid, dim3(64), 0, st, ax, out);
    else hipLaunchKernelGGL((surface_rgbx_kernel<pixel, TILED, 0, 0, Out>), grid, dim3(64), 0, st, ax, out);
    return hip_rc(hipGetLastError());
}

// what the call refuses beyond the export's own rules
int rgbx_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipRgbParams &p, const int row0, const int row1,
                    SurfaceCall *const call)
{
    if (const int rc = surface_args_check(dst, src, row0, row1, call, false, true)) return rc;
    if (const int rc = rgb_params_check(dst, p)) return rc;
    return 0;
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipRgbParams *params,
                                            int row0, int row1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    if (!c) return -EINVAL;
    if (const int rc = rgbx_args_check(dst, src, p, row0, row1, &call)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    row0 = call.row0; row1 = call.row1;
    void *const *const planes = call.planes;
    if (row1 <= row0) return 0;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        typedef decltype(px) pixel;
        return with_rgb_out<pixel>(dst->sample, p, src->bpc, [&](const auto &out) {
            return launch_rgbx<pixel, decltype(state)::value>(c, dst, src, planes, p, row0, row1, out);
        });
    }));
}

extern "C" int dav1d_hip_surface_rgb_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipRgbParams *params, int row1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    if (const int rc = rgbx_args_check(dst, src, p, 0, row1, &call)) return rc;
    const int h = src->p[0].h, r1 = call.row1;
    if (r1 <= 0) return 0;
    const int need = r1 + (src->layout == DAV1D_HIP_LAYOUT_I420 && p.chroma_pos ? 2 : 0);
    return need > h ? h : need;
}
