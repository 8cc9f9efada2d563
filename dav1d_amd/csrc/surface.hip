// Output on the device: a decoded picture leaves the library as a surface the caller owns (dav1d_hip_surface_export, include/dav1d_hip.h).
// One bandwidth-bound pass: integer, no LDS, nothing that waits on another workgroup.  It reads the picture where it lives — raster planes, or the
// 8x8-tiled twin (Dav1dHipPicture.twin) without un-tiling it first — and writes the visible samples in the caller's layout.
//
// The unit of work is 8 horizontally adjacent samples: one 16-byte row of an 8x8 tile of the twin at 10 / 12 bits, one 16-byte piece of a raster
// row.  A wave is laid out as 8 rows x 8 units (lane = row * 8 + unit), i.e. a 64 x 8 cell of a plane: a load of the wave takes eight WHOLE
// tiles of the twin (eight 128-byte lines, each lane its 16 bytes) or eight 128-byte pieces of raster rows, a store leaves eight pieces of
// 128 consecutive bytes of destination rows (256 where a lane leaves 32: interleaved chroma, float samples).  Both sides are whole memory lines when
// the destination rows start on one; no line is requested twice.
#include "surface_call.h"

namespace {

constexpr int COPY_ROWS = 8;       // cells (of 8 rows) under one another per wave: 8 KB in flight per wave at 16 bits, like the retile passes (mcx.hip)

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(64) void surface_copy_kernel(const CopyArgs a, const Out out)
{
    int g = (int) dv::xcd_chunk_id(blockIdx.x, gridDim.x);        // neighbouring cells on one XCD (speed only)
    SurfPart p = a.part[0];
    if (g >= p.n_waves) {
        g -= p.n_waves; p = a.part[1];
        if (g >= p.n_waves) { g -= p.n_waves; p = a.part[2]; }
    }
    const int cyg = g / p.n_cx, cx = g - cyg * p.n_cx;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const int x = cx * 64 + c * 8, n = p.w - x;
    if (n <= 0) return;
    const int ybase = ((p.y0 >> 3) + cyg * COPY_ROWS) * 8 + r;
    if (p.interleave) {          // two source planes: half the cells at a time, the same bytes in flight
        copy_cells<pixel, TILED, Out, true, COPY_ROWS / 2>(p, out, x, n, ybase);
        copy_cells<pixel, TILED, Out, true, COPY_ROWS / 2>(p, out, x, n, ybase + COPY_ROWS * 4);
    } else
        copy_cells<pixel, TILED, Out, false, COPY_ROWS>(p, out, x, n, ybase);
}

// A lane holds 8 chroma pairs and serves the (8 << SSH) x (1 << SSV) luma samples above them (chroma replicated): chroma is read once.
template <typename pixel, bool TILED, int SSH, int SSV, typename Out>
__global__ __launch_bounds__(64) void surface_rgb_kernel(const RgbArgs a, const Out out)
{
    typedef typename Out::T T;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const int g = (int) blockIdx.x;
    const int cyg = g / a.n_cx, cx = g - cyg * a.n_cx;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const int xc = cx * 64 + c * 8, yc = ((a.crow0 >> 3) + cyg) * 8 + r;
    if (xc >= a.cw || yc < a.crow0 || yc >= a.crow1) return;
    piece_t u, v, yy[1 << SSV][1 << SSH];
    if (!a.mono) {
        u = load8<pixel, TILED>(a.s[1], a.sstride[1], xc, yc, a.cw - xc, a.swide[1]);
        v = load8<pixel, TILED>(a.s[2], a.sstride[1], xc, yc, a.cw - xc, a.swide[1]);
    }
#pragma unroll
    for (int i = 0; i < 1 << SSV; i++)
#pragma unroll
        for (int j = 0; j < 1 << SSH; j++) {
            const int x = (xc << SSH) + j * 8, y = (yc << SSV) + i;
            if (x < a.w && y < a.row1) yy[i][j] = load8<pixel, TILED>(a.s[0], a.sstride[0], x, y, a.w - x, a.swide[0]);
        }
#pragma unroll
    for (int j = 0; j < 1 << SSH; j++) {
        const int x = (xc << SSH) + j * 8;
        if (x >= a.w) continue;
        // the chroma terms of the 8 samples of this unit (the same for the rows of the lane)
        int tr[8], tg[8], tb[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int ce = (j * 8 + e) >> SSH;
            const int cb = a.mono ? 0 : sample_of<pixel>(u, ce) - a.mid, cr = a.mono ? 0 : sample_of<pixel>(v, ce) - a.mid;
            tr[e] = a.identity ? cr + a.mid : a.crv * cr + 8192;
            tg[e] = a.identity ? 0 : 8192 - a.cgu * cb - a.cgv * cr;
            tb[e] = a.identity ? cb + a.mid : a.cbu * cb + 8192;
        }
#pragma unroll
        for (int i = 0; i < 1 << SSV; i++) {
            const int y = (yc << SSV) + i;
            if (y >= a.row1) continue;
            T R[8], G[8], B[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int Y = sample_of<pixel>(yy[i][j], e);
                if (a.identity) { R[e] = out(tr[e]); G[e] = out(Y); B[e] = out(tb[e]); continue; }
                const int l = a.cy * (Y - a.yoff);
                R[e] = out(dv::iclip((l + tr[e]) >> 14, 0, a.max));
                G[e] = out(dv::iclip((l + tg[e]) >> 14, 0, a.max));
                B[e] = out(dv::iclip((l + tb[e]) >> 14, 0, a.max));
            }
            const size_t off = (size_t) x * sizeof(T);
            store_run<T, 8>((T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0] + off), R, a.w - x, a.dwide);
            store_run<T, 8>((T *) ((uint8_t *) a.d[1] + (size_t) y * a.dstride[1] + off), G, a.w - x, a.dwide);
            store_run<T, 8>((T *) ((uint8_t *) a.d[2] + (size_t) y * a.dstride[2] + off), B, a.w - x, a.dwide);
        }
    }
}

template <typename pixel, bool TILED, typename Out>
int launch_rgb(const RgbArgs &a, const Out &out, const int ss_hor, const int ss_ver, const dim3 grid, hipStream_t st)
{
    if (ss_ver) hipLaunchKernelGGL((surface_rgb_kernel<pixel, TILED, 1, 1, Out>), grid, dim3(64), 0, st, a, out);
    else if (ss_hor) hipLaunchKernelGGL((surface_rgb_kernel<pixel, TILED, 1, 0, Out>), grid, dim3(64), 0, st, a, out);
    else hipLaunchKernelGGL((surface_rgb_kernel<pixel, TILED, 0, 0, Out>), grid, dim3(64), 0, st, a, out);
    return 0;
}

template <typename pixel, bool TILED, typename Out>
int launch_surface(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                   const int row0, const int row1, const Out &out)
{
    typedef typename Out::T T;
    if (dst->format == DAV1D_HIP_SURFACE_RGB_PLANAR) {
        unsigned n_cells;
        const RgbArgs a = make_rgb_args<pixel, TILED, T>(dst, src, planes, row0, row1, &n_cells);
        const SurfaceGeom g = surface_geom(src, row0, row1);
        launch_rgb<pixel, TILED, Out>(a, out, g.ss_hor, g.ss_ver, dim3(n_cells), c->stream);
        return hip_rc(hipGetLastError());
    }
    unsigned n_waves;
    const CopyArgs a = make_copy_args<pixel, TILED, T>(dst, src, planes, row0, row1, COPY_ROWS, 1, &n_waves);
    hipLaunchKernelGGL((surface_copy_kernel<pixel, TILED, Out>), dim3(n_waves), dim3(64), 0, c->stream, a, out);
    return hip_rc(hipGetLastError());
}

} // namespace

extern "C" int dav1d_hip_surface_export(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, int row0, int row1)
{
    SurfaceCall call;
    if (const int rc = surface_call_check(c, dst, src, row0, row1, &call)) return rc;
    row0 = call.row0; row1 = call.row1;
    const bool tiled = call.tiled;
    void *const *const planes = call.planes;
    if (row1 <= row0) return 0;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, tiled, [&](auto px, auto state) {
        typedef decltype(px) pixel;
        return with_out<pixel>(dst->sample, src->bpc, [&](const auto &out) {
            return launch_surface<pixel, decltype(state)::value>(c, dst, src, planes, row0, row1, out);
        });
    }));
}
