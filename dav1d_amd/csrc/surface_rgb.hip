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
#include "surface_common.h"

namespace {

struct RgbxArgs {
    RgbArgs r;
    int ch;                 // rows of the chroma plane
    int pos;                // chroma_pos
    int hf, vf;             // taps across / down other than replication
    int packed;             // samples a pixel in data[0] (3, 4), 0: planes
};

// one sample of a plane (the same line request as the load8 around it)
template <typename pixel, bool TILED>
__device__ __forceinline__ uint32_t load1(const void *const base, const int stride, const int x, const int y)
{
    const pixel *const p = (const pixel *) base;
    if (TILED) return p[(size_t) (y >> 3) * 8 * stride + (size_t) (x >> 3) * 64 + (y & 7) * 8 + (x & 7)];
    return p[(size_t) y * stride + x];
}

template <typename pixel> __device__ __forceinline__ uint32_t pair_of(const Piece<8 * sizeof(pixel)> &u, const Piece<8 * sizeof(pixel)> &v, const int m) {
    return (uint32_t) sample_of<pixel>(u, m) | (uint32_t) sample_of<pixel>(v, m) << 16;
}
template <typename piece_t> __device__ __forceinline__ piece_t piece_from_lane(const piece_t &p, const int lane) {
    piece_t o;
#pragma unroll
    for (int k = 0; k < (int) (sizeof(piece_t) / 4); k++) o.a[k] = (uint32_t) __shfl((int) p.a[k], lane);
    return o;
}
// the vertical taps of luma rows 2k (top) and 2k + 1 (bottom) on pairs of the rows above, at and below chroma row k, weights summing to 4
__device__ __forceinline__ void taps_down(const int pos, const uint32_t up, const uint32_t own, const uint32_t dn, uint32_t &top, uint32_t &bot)
{
    if (pos == 1) { top = up + 3 * own; bot = 3 * own + dn; }
    else { top = 4 * own; bot = 2 * (own + dn); }
}

template <typename pixel, bool TILED, int SSH, int SSV, typename Out>
__global__ __launch_bounds__(64) void surface_rgbx_kernel(const RgbxArgs ax, const Out out)
{
    typedef typename Out::T T;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const RgbArgs &a = ax.r;
    const int g = (int) blockIdx.x;
    const int cyg = g / a.n_cx, cx = g - cyg * a.n_cx;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const int xc = cx * 64 + c * 8, yc = ((a.crow0 >> 3) + cyg) * 8 + r;
    // (no lane leaves before the exchanges below: every lane of the wave takes part in them)
    const bool active = xc < a.cw && yc >= a.crow0 && yc < a.crow1;
    const int nloc = a.cw - xc;                      // chroma columns from this lane's first to the plane's end
    const bool vf = SSV && ax.vf, hf = SSH && ax.hf;
    piece_t u = piece_t(), v = piece_t(), yy[1 << SSV][1 << SSH];
    if (active && !a.mono) {
        u = load8<pixel, TILED>(a.s[1], a.sstride[1], xc, yc, nloc, a.swide[1]);
        v = load8<pixel, TILED>(a.s[2], a.sstride[1], xc, yc, nloc, a.swide[1]);
    }
    // the rows above and below: the lanes above and below in the cell, a load at the cell's (the band's) first and last row, the row itself at the plane's
    const bool edge_up = r == 0 || yc == a.crow0, edge_dn = r == 7 || yc == a.crow1 - 1;
    piece_t uu = u, vu = v, ud = u, vd = v;
    if (vf) {
        uu = piece_from_lane(u, lane - 8); vu = piece_from_lane(v, lane - 8);
        ud = piece_from_lane(u, lane + 8); vd = piece_from_lane(v, lane + 8);
        if (active && edge_up) {
            if (yc == 0) { uu = u; vu = v; }
            else {
                uu = load8<pixel, TILED>(a.s[1], a.sstride[1], xc, yc - 1, nloc, a.swide[1]);
                vu = load8<pixel, TILED>(a.s[2], a.sstride[1], xc, yc - 1, nloc, a.swide[1]);
            }
        }
        if (active && edge_dn) {
            if (yc == ax.ch - 1) { ud = u; vd = v; }
            else {
                ud = load8<pixel, TILED>(a.s[1], a.sstride[1], xc, yc + 1, nloc, a.swide[1]);
                vd = load8<pixel, TILED>(a.s[2], a.sstride[1], xc, yc + 1, nloc, a.swide[1]);
            }
        }
    }
    // the pair right of the lane's eight, rows above and below it likewise: the next lane's first, or (last lane of the cell's row) a load
    const bool halo = active && hf && c == 7 && nloc > 8;
    uint32_t h_own = 0, h_up = 0, h_dn = 0;
    if (halo) h_own = load1<pixel, TILED>(a.s[1], a.sstride[1], xc + 8, yc) | load1<pixel, TILED>(a.s[2], a.sstride[1], xc + 8, yc) << 16;
    if (hf && vf) {
        h_up = (uint32_t) __shfl((int) h_own, lane - 8);
        h_dn = (uint32_t) __shfl((int) h_own, lane + 8);
        if (halo && edge_up) h_up = yc == 0 ? h_own : load1<pixel, TILED>(a.s[1], a.sstride[1], xc + 8, yc - 1) | load1<pixel, TILED>(a.s[2], a.sstride[1], xc + 8, yc - 1) << 16;
        if (halo && edge_dn) h_dn = yc == ax.ch - 1 ? h_own : load1<pixel, TILED>(a.s[1], a.sstride[1], xc + 8, yc + 1) | load1<pixel, TILED>(a.s[2], a.sstride[1], xc + 8, yc + 1) << 16;
    }
    if (active) {
#pragma unroll
        for (int i = 0; i < 1 << SSV; i++)
#pragma unroll
            for (int j = 0; j < 1 << SSH; j++) {
                const int x = (xc << SSH) + j * 8, y = (yc << SSV) + i;
                if (x < a.w && y < a.row1) yy[i][j] = load8<pixel, TILED>(a.s[0], a.sstride[0], x, y, a.w - x, a.swide[0]);
            }
    }
    // P[i][m]: the vertical taps (sum 4) of luma row i on chroma column m of the lane, U and V in the halves of a word; m = 8 is the neighbour
    uint32_t P[1 << SSV][9];
    const uint32_t grey = (uint32_t) a.mid * 0x10001u;
#pragma unroll
    for (int m = 0; m < 8; m++) {
        const uint32_t own = a.mono ? grey : pair_of<pixel>(u, v, m);
        if (vf) taps_down(ax.pos, pair_of<pixel>(uu, vu, m), own, pair_of<pixel>(ud, vd, m), P[0][m], P[SSV][m]);
        else P[0][m] = P[SSV][m] = 4 * own;
    }
    if (hf) {
        uint32_t hp[2];
        if (vf) taps_down(ax.pos, h_up, h_own, h_dn, hp[0], hp[1]);
        else hp[0] = hp[1] = 4 * h_own;
#pragma unroll
        for (int i = 0; i < 1 << SSV; i++) {
            const uint32_t next = (uint32_t) __shfl((int) P[i][0], lane + 1);
            P[i][8] = c == 7 ? hp[i] : next;
#pragma unroll
            for (int m = 1; m < 9; m++) P[i][m] = m < nloc ? P[i][m] : P[i][m - 1];       // right of the plane: its last column
        }
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < 1 << SSH; j++) {
        const int x = (xc << SSH) + j * 8;
        if (x >= a.w) continue;
        int tr[8], tg[8], tb[8];
#pragma unroll
        for (int i = 0; i < 1 << SSV; i++) {
            const int y = (yc << SSV) + i;
            if (y >= a.row1) continue;
            if (i == 0 || vf) {      // the chroma terms of the 8 samples of this unit (without taps down: the same for both rows of the lane)
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int k = SSH ? j * 4 + (e >> 1) : e;
                    uint32_t s = 2 * P[i][k];
                    if (SSH && (e & 1) && hf) s = P[i][k] + P[i][k + 1];
                    s = ((s + 0x00040004u) >> 3) & 0x1fff1fffu;
                    const int cb = (int) (s & 0xffff) - a.mid, cr = (int) (s >> 16) - a.mid;
                    if (a.identity) { tr[e] = cr + a.mid; tg[e] = 0; tb[e] = cb + a.mid; }
                    else {
                        tr[e] = dv::mad_i24(a.crv, cr, 8192);
                        tg[e] = dv::mad_i24(-a.cgv, cr, dv::mad_i24(-a.cgu, cb, 8192));
                        tb[e] = dv::mad_i24(a.cbu, cb, 8192);
                    }
                }
            }
            T R[8], G[8], B[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int Y = sample_of<pixel>(yy[i][j], e);
                if (a.identity) { R[e] = out(tr[e], 0); G[e] = out(Y, 1); B[e] = out(tb[e], 2); continue; }
                const int l = dv::mul_i24(a.cy, Y - a.yoff);
                R[e] = out(dv::iclip((l + tr[e]) >> 14, 0, a.max), 0);
                G[e] = out(dv::iclip((l + tg[e]) >> 14, 0, a.max), 1);
                B[e] = out(dv::iclip((l + tb[e]) >> 14, 0, a.max), 2);
            }
            const int n = a.w - x;
            if (ax.packed == 3) {
                T t[24];
#pragma unroll
                for (int e = 0; e < 8; e++) { t[3 * e] = R[e]; t[3 * e + 1] = G[e]; t[3 * e + 2] = B[e]; }
                store_packed<T, 24>((T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0]) + (size_t) x * 3, t, 3 * n, a.dwide);
            } else if (ax.packed == 4) {
                T t[32];
#pragma unroll
                for (int e = 0; e < 8; e++) { t[4 * e] = R[e]; t[4 * e + 1] = G[e]; t[4 * e + 2] = B[e]; t[4 * e + 3] = out.alpha; }
                store_packed<T, 32>((T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0]) + (size_t) x * 4, t, 4 * n, a.dwide);
            } else {
                const size_t off = (size_t) x * sizeof(T);
                store_run<T, 8>((T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0] + off), R, n, a.dwide);
                store_run<T, 8>((T *) ((uint8_t *) a.d[1] + (size_t) y * a.dstride[1] + off), G, n, a.dwide);
                store_run<T, 8>((T *) ((uint8_t *) a.d[2] + (size_t) y * a.dstride[2] + off), B, n, a.dwide);
            }
        }
    }
}

template <typename pixel, bool TILED, typename Out>
int launch_rgbx(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                const Dav1dHipRgbParams &p, const int row0, const int row1, const Out &out)
{
    typedef typename Out::T T;
    unsigned n_cells;
    RgbxArgs ax = RgbxArgs();
    ax.r = make_rgb_args<pixel, TILED, T>(dst, src, planes, row0, row1, &n_cells);
    const SurfaceGeom g = surface_geom(src, row0, row1);
    ax.ch = g.ch; ax.pos = p.chroma_pos;
    ax.hf = g.ss_hor && p.chroma_pos; ax.vf = g.ss_ver && p.chroma_pos;
    ax.packed = dst->format == DAV1D_HIP_SURFACE_RGB_PACKED ? 3 : dst->format == DAV1D_HIP_SURFACE_RGBA_PACKED ? 4 : 0;
    if (ax.packed) {          // one plane; a lane's run starts at a multiple of its size, so the chunk's alignment of base and stride decides
        const int run = 8 * ax.packed * (int) sizeof(T);
        ax.r.dwide = aligned_to(dst->data[0], dst->stride[0], run % 16 ? 8 : 16);
        ax.r.d[1] = ax.r.d[2] = nullptr;
    }
    const dim3 grid(n_cells);
    hipStream_t st = c->stream;
    if (g.ss_ver) hipLaunchKernelGGL((surface_rgbx_kernel<pixel, TILED, 1, 1, Out>), grid, dim3(64), 0, st, ax, out);
    else if (g.ss_hor) hipLaunchKernelGGL((surface_rgbx_kernel<pixel, TILED, 1, 0, Out>), grid, dim3(64), 0, st, ax, out);
    else hipLaunchKernelGGL((surface_rgbx_kernel<pixel, TILED, 0, 0, Out>), grid, dim3(64), 0, st, ax, out);
    return hip_rc(hipGetLastError());
}

template <typename pixel, bool TILED>
int launch_rgbx_sample(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                       const Dav1dHipRgbParams &p, const int row0, const int row1)
{
    const int max = (1 << src->bpc) - 1;
    if (dst->sample == DAV1D_HIP_SAMPLE_F32) {
        RgbF32 o; set_float(o, p, src->bpc); o.alpha = 1.0f;
        return launch_rgbx<pixel, TILED, RgbF32>(c, dst, src, planes, p, row0, row1, o);
    }
    if (dst->sample == DAV1D_HIP_SAMPLE_F16) {
        RgbF16 o; set_float(o, p, src->bpc); o.alpha = 0x3c00;
        return launch_rgbx<pixel, TILED, RgbF16>(c, dst, src, planes, p, row0, row1, o);
    }
    if constexpr (sizeof(pixel) == 2) {
        if (dst->sample == DAV1D_HIP_SAMPLE_MSB16) {
            RgbInt<OutMsb16> o; o.b.shift = 16 - src->bpc; o.alpha = (uint16_t) (max << o.b.shift);
            return launch_rgbx<pixel, TILED, RgbInt<OutMsb16>>(c, dst, src, planes, p, row0, row1, o);
        }
    }
    RgbInt<OutNative<pixel>> o; o.alpha = (pixel) max;
    return launch_rgbx<pixel, TILED, RgbInt<OutNative<pixel>>>(c, dst, src, planes, p, row0, row1, o);
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
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    SurfaceCall call;
    if (!c) return -EINVAL;
    if (const int rc = rgbx_args_check(dst, src, p, row0, row1, &call)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    row0 = call.row0; row1 = call.row1;
    void *const *const planes = call.planes;
    if (row1 <= row0) return 0;
    (void) hipEventRecord(c->ev_t0, c->stream);
    int rc;
    if (src->bpc == 8) rc = call.tiled ? launch_rgbx_sample<uint8_t, true>(c, dst, src, planes, p, row0, row1) : launch_rgbx_sample<uint8_t, false>(c, dst, src, planes, p, row0, row1);
    else rc = call.tiled ? launch_rgbx_sample<uint16_t, true>(c, dst, src, planes, p, row0, row1) : launch_rgbx_sample<uint16_t, false>(c, dst, src, planes, p, row0, row1);
    (void) hipEventRecord(c->ev_t1, c->stream);
    c->last_ms_pending = !rc;
    return rc;
}

extern "C" int dav1d_hip_surface_rgb_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipRgbParams *params, int row1)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    SurfaceCall call;
    if (const int rc = rgbx_args_check(dst, src, p, 0, row1, &call)) return rc;
    const int h = src->p[0].h, r1 = call.row1;
    if (r1 <= 0) return 0;
    const int need = r1 + (src->layout == DAV1D_HIP_LAYOUT_I420 && p.chroma_pos ? 2 : 0);
    return need > h ? h : need;
}
