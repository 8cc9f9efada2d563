// Output on the device at another size: dav1d_hip_surface_export_scaled (include/dav1d_hip.h) writes what dav1d_hip_surface_export writes from the
// picture whose planes are a crop of the source's planes, each scaled down by the area scaler S of DESIGN.md 10.2 (12-bit weights, separable, the
// vertical pass first).  One pass over the source where it lives (raster planes or the tiled twin, which is not un-tiled), one launch.
//
// A workgroup of four waves owns a CELL of a destination plane: ow x oh output samples, ow = 128 / 64 / 32 for a horizontal ratio up to 2 / 4 / 8
// and oh = 8 / 4 for a vertical ratio up to 4 / 8.  So the source window of a cell is at most 257 x 33 samples and never less than 128 x 8: a
// 128-byte line of the source (a row piece of a raster plane, an 8x8 tile — two at 8 bits — of the twin) meets at most two cells per axis, and the
// sample two neighbouring cells share is the only re-read.  The window is loaded with the export's loads (lane = row * 8 + unit: a wave takes
// eight whole tiles or eight 128-byte row pieces per instruction, surface_common.h) into LDS; then
//     weights   the 12-bit weights of the cell's columns and rows, once per cell, by the threads that would otherwise wait for the loads
//     vertical  t[j][x] = (sum wy * raw + 8) >> 4 for the cell's rows j and every column x of the window        (20 bits, LDS)
//     across    out[j][o] = (sum wx * t + 2^19) >> 20, v_mad_u32_u24: both factors below 2^24, the sum below 2^32  (LDS)
//     store     a lane leaves 8 adjacent samples through the export's functors and store_run
// Semi-planar chroma and RGB run the scaler two or three times in the workgroup (U, V, then Y cell by cell above them) and combine from LDS.
#include "surface_call.h"

namespace {

// ---- planar and semi-planar: every destination plane is a part, a workgroup a cell of one
struct ScalePart {
    ScalePlane a, b;        // (b: V of an interleaved part)
    void *d;
    long long dstride;      // bytes
    int y0, y1;             // rows of the destination plane
    int n_cx, n_cells;
    int interleave, dwide;
};
struct ScaleCopyArgs { ScalePart part[3]; };

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_scale_copy_kernel(const ScaleCopyArgs a, const Out out)
{
    typedef typename Out::T T;
    __shared__ ScaleLds<pixel> L;
    int g = (int) blockIdx.x, k = 0;
    if (g >= a.part[0].n_cells) {
        g -= a.part[0].n_cells; k = 1;
        if (g >= a.part[1].n_cells) { g -= a.part[1].n_cells; k = 2; }
    }
    const ScalePart &p = a.part[k];
    const int cy = g / p.n_cx, cx = g - cy * p.n_cx;
    const int ox0 = cx * p.a.ow, oyb = (p.y0 / p.a.oh + cy) * p.a.oh;
    const int nox = dv::imin(p.a.ow, p.a.dw - ox0), j0 = dv::imax(oyb, p.y0), j1 = dv::imin(oyb + p.a.oh, p.y1);
    scale_cell<pixel, TILED>(L, p.a, ox0, nox, oyb, j0, j1, L.out[0]);
    if (p.interleave) scale_cell<pixel, TILED>(L, p.b, ox0, nox, oyb, j0, j1, L.out[1]);
    const int nun = (nox + 7) >> 3;
    for (int it = (int) threadIdx.x; it < (j1 - j0) * nun; it += 256) {
        const int j = it / nun, u = it - j * nun, y = j0 + j, x = ox0 + u * 8, n = nox - u * 8;
        const uint16_t *const s0 = &L.out[0][(y - oyb) * SC_OW + u * 8], *const s1 = &L.out[1][(y - oyb) * SC_OW + u * 8];
        T *const row = (T *) ((uint8_t *) p.d + (size_t) y * p.dstride);
        if (p.interleave) {
            T t[16];
#pragma unroll
            for (int i = 0; i < 8; i++) { t[2 * i] = out(s0[i]); t[2 * i + 1] = out(s1[i]); }
            store_run<T, 16>(row + 2 * x, t, 2 * n, p.dwide);
        } else {
            T t[8];
#pragma unroll
            for (int i = 0; i < 8; i++) t[i] = out(s0[i]);
            store_run<T, 8>(row + x, t, n, p.dwide);
        }
    }
}

// ---- RGB planes: a workgroup owns a cell of the scaled chroma planes (of the luma plane at 4:0:0) and the luma above it, which it scales cell
// by cell; the colour of a sample is the export's (rgb_chroma_terms, rgb_of) from the scaled Y, U, V in LDS
struct ScaleRgbArgs {
    ScalePlane pl[3];
    RgbArgs c;              // d, dstride, dwide and the colour part
    int ssh, ssv;
    int row0, row1;         // destination luma rows
    int crow0, crow1;       // ... and chroma rows
    int n_cx;
};

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_scale_rgb_kernel(const ScaleRgbArgs a, const Out out)
{
    typedef typename Out::T T;
    __shared__ ScaleLds<pixel> L;
    const ScalePlane &pc = a.pl[a.c.mono ? 0 : 1], &py = a.pl[0];
    const int g = (int) blockIdx.x, cy = g / a.n_cx, cx = g - cy * a.n_cx;
    const int cx0 = cx * pc.ow, cyb = (a.crow0 / pc.oh + cy) * pc.oh;
    const int ncx = dv::imin(pc.ow, pc.dw - cx0), cj0 = dv::imax(cyb, a.crow0), cj1 = dv::imin(cyb + pc.oh, a.crow1);
    if (!a.c.mono) {
        scale_cell<pixel, TILED>(L, a.pl[1], cx0, ncx, cyb, cj0, cj1, L.out[1]);
        scale_cell<pixel, TILED>(L, a.pl[2], cx0, ncx, cyb, cj0, cj1, L.out[2]);
    }
    // the luma of the cell
    const int lx0 = cx0 << a.ssh, lx1 = dv::imin((cx0 + ncx) << a.ssh, py.dw);
    const int ly0 = dv::imax(cj0 << a.ssv, a.row0), ly1 = dv::imin(cj1 << a.ssv, a.row1);
    for (int lyb = cyb << a.ssv; lyb < ly1; lyb += py.oh) {
        const int j0 = dv::imax(lyb, ly0), j1 = dv::imin(lyb + py.oh, ly1);
        if (j1 <= j0) continue;
        for (int lx = lx0; lx < lx1; lx += py.ow) {
            const int nox = dv::imin(py.ow, lx1 - lx);
            scale_cell<pixel, TILED>(L, py, lx, nox, lyb, j0, j1, L.out[0]);
            const int nun = (nox + 7) >> 3;
            for (int it = (int) threadIdx.x; it < (j1 - j0) * nun; it += 256) {
                const int j = it / nun, u = it - j * nun, y = j0 + j, x = lx + u * 8, n = nox - u * 8;
                const uint16_t *const sy = &L.out[0][(y - lyb) * SC_OW + u * 8];
                const int crow = ((y >> a.ssv) - cyb) * SC_OW - cx0;
                T R[8], G[8], B[8];
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int ci = crow + ((x + e) >> a.ssh);
                    int tr, tg, tb;
                    rgb_chroma_terms(a.c, a.c.mono ? 0 : (int) L.out[1][ci] - a.c.mid, a.c.mono ? 0 : (int) L.out[2][ci] - a.c.mid, tr, tg, tb);
                    rgb_of(a.c, out, (int) sy[e], tr, tg, tb, R[e], G[e], B[e]);
                }
                const size_t off = (size_t) x * sizeof(T);
                store_run<T, 8>((T *) ((uint8_t *) a.c.d[0] + (size_t) y * a.c.dstride[0] + off), R, n, a.c.dwide);
                store_run<T, 8>((T *) ((uint8_t *) a.c.d[1] + (size_t) y * a.c.dstride[1] + off), G, n, a.c.dwide);
                store_run<T, 8>((T *) ((uint8_t *) a.c.d[2] + (size_t) y * a.c.dstride[2] + off), B, n, a.c.dwide);
            }
        }
    }
}

template <typename pixel, bool TILED, typename Out>
int launch_scaled(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                  const ScaleGeom &g, const int row0, const int row1, const Out &out)
{
    typedef typename Out::T T;
    const int dch = (g.dh + g.ss_ver) >> g.ss_ver;
    const int crow0 = row0 >> g.ss_ver, crow1 = row1 >= g.dh ? dch : row1 >> g.ss_ver;
    if (dst->format == DAV1D_HIP_SURFACE_RGB_PLANAR) {
        ScaleRgbArgs a = ScaleRgbArgs();
        for (int pl = 0; pl < (g.mono ? 1 : 3); pl++) a.pl[pl] = make_scale_plane<pixel, TILED>(src, planes, g, pl);
        const int store_align = 8 * (int) sizeof(T) > 16 ? 16 : 8 * (int) sizeof(T);
        a.c.dwide = 1;
        for (int pl = 0; pl < 3; pl++) {
            a.c.d[pl] = dst->data[pl]; a.c.dstride[pl] = dst->stride[pl];
            a.c.dwide &= aligned_to(dst->data[pl], dst->stride[pl], store_align);
        }
        rgb_set_matrix(a.c, dst, src->bpc, g.mono);
        a.ssh = g.ss_hor; a.ssv = g.ss_ver; a.row0 = row0; a.row1 = row1;
        a.crow0 = g.mono ? row0 : crow0; a.crow1 = g.mono ? row1 : crow1;
        const ScalePlane &pc = a.pl[g.mono ? 0 : 1];
        a.n_cx = (pc.dw + pc.ow - 1) / pc.ow;
        const int n_cy = (a.crow1 + pc.oh - 1) / pc.oh - a.crow0 / pc.oh;
        hipLaunchKernelGGL((surface_scale_rgb_kernel<pixel, TILED, Out>), dim3((unsigned) a.n_cx * (unsigned) n_cy), dim3(256), 0, c->stream, a, out);
        return hip_rc(hipGetLastError());
    }
    ScaleCopyArgs a = ScaleCopyArgs();
    const bool semi = dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR;
    const int n_parts = g.mono ? 1 : semi ? 2 : 3;
    unsigned n_cells = 0;
    for (int k = 0; k < n_parts; k++) {
        ScalePart &p = a.part[k];
        p.interleave = semi && k == 1;
        p.a = make_scale_plane<pixel, TILED>(src, planes, g, k);
        if (p.interleave) p.b = make_scale_plane<pixel, TILED>(src, planes, g, 2);
        p.d = dst->data[k]; p.dstride = dst->stride[k];
        p.y0 = k ? crow0 : row0; p.y1 = k ? crow1 : row1;
        p.n_cx = (p.a.dw + p.a.ow - 1) / p.a.ow;
        p.n_cells = p.n_cx * ((p.y1 + p.a.oh - 1) / p.a.oh - p.y0 / p.a.oh);
        const int run = (p.interleave ? 16 : 8) * (int) sizeof(T);
        p.dwide = aligned_to(p.d, p.dstride, run > 16 ? 16 : run);
        n_cells += (unsigned) p.n_cells;
    }
    hipLaunchKernelGGL((surface_scale_copy_kernel<pixel, TILED, Out>), dim3(n_cells), dim3(256), 0, c->stream, a, out);
    return hip_rc(hipGetLastError());
}

} // namespace

extern "C" int dav1d_hip_surface_export_scaled(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                               int drow0, int drow1)
{
    SurfaceCall call;
    if (const int rc = surface_call_check(c, dst, src, drow0, drow1, &call, true)) return rc;
    ScaleGeom g;
    if (const int rc = scale_geom_check(dst, src, crop, &g)) return rc;
    const int row0 = call.row0, row1 = call.row1;
    if (row1 <= row0) return 0;
    void *const *const planes = call.planes;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        typedef decltype(px) pixel;
        return with_out<pixel>(dst->sample, src->bpc, [&](const auto &out) {
            return launch_scaled<pixel, decltype(state)::value>(c, dst, src, planes, g, row0, row1, out);
        });
    }));
}

extern "C" int dav1d_hip_surface_scaled_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop, int drow1)
{
    SurfaceCall call;
    if (const int rc = surface_args_check(dst, src, 0, drow1, &call, true)) return rc;
    ScaleGeom g;
    return sized_rows_needed(scale_geom_check(dst, src, crop, &g), call, g, false, src);
}
