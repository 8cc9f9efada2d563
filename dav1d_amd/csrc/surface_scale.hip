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
#include "surface_common.h"

namespace {

constexpr int SC_OW = 128, SC_OR = 8, SC_TAPS = 9;      // the largest cell; taps per axis
constexpr int SC_MAXU = 33;                             // units of 8 samples across a window: 257 samples from an offset of up to 7
constexpr int SC_PITCH = SC_MAXU * 8 + 8;               // samples per LDS row
constexpr int SC_MAXR = 40;                             // rows of a window: 33 from an offset of up to 7

struct ScalePlane {
    const void *s;
    int sstride, swide, pw;     // pixels per row; one vector load per unit; visible samples per row of the plane (the narrow loads end there)
    int x0, y0, sw, sh;         // the window of the plane that is scaled
    int dw, dh;                 // ... to this size
    int ow, oh;                 // the cell
};

template <typename pixel> struct ScaleLds {
    alignas(16) pixel raw[SC_MAXR * SC_PITCH];
    uint32_t t[SC_OR * SC_PITCH];
    uint16_t wx[SC_TAPS][SC_OW], wy[SC_TAPS][SC_OR];
    uint16_t ix[SC_OW], iy[SC_OR];      // the first tap: column / row of the LDS window
    uint8_t nx[SC_OW], ny[SC_OR];       // taps
    alignas(16) uint16_t out[3][SC_OR * SC_OW];
};

// taps and weights of output `o` of an axis (s source samples to d); *first = i0
__device__ __forceinline__ int scale_weights(const int o, const int s, const int d, int *const first, uint16_t *const w, const int wstride)
{
    const uint64_t a = (uint64_t) o * (unsigned) s, b = a + (unsigned) s;
    const int i0 = (int) (a / (unsigned) d), i1 = (int) ((b + (unsigned) d - 1) / (unsigned) d) - 1;
    const int n = i1 - i0 + 1;
    uint64_t edge = (uint64_t) (i0 + 1) * (unsigned) d;
    unsigned prev = 0;
    for (int k = 0; k < SC_TAPS; k++, edge += (unsigned) d) {
        if (k >= n) break;
        const unsigned cov = (unsigned) ((edge < b ? edge : b) - a);           // <= s
        const unsigned q = (cov * 4096u + ((unsigned) s >> 1)) / (unsigned) s;
        w[k * wstride] = (uint16_t) (q - prev);
        prev = q;
    }
    *first = i0;
    return n;
}

// Outputs [ox0, ox0 + nox) x [j0, j1) of plane p into out[(j - oyb) * SC_OW + (o - ox0)].  Every argument is uniform in the workgroup; all of
// its threads call.  nox <= SC_OW, oyb <= j0, j1 - oyb <= SC_OR.
template <typename pixel, bool TILED>
__device__ __forceinline__ void scale_cell(ScaleLds<pixel> &L, const ScalePlane &p, const int ox0, const int nox, const int oyb, const int j0, const int j1,
                                           uint16_t *const out)
{
    typedef Piece<8 * sizeof(pixel)> piece_t;
    if (j1 <= j0 || nox <= 0) return;
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ax0 = p.x0 + (int) ((uint64_t) ox0 * (unsigned) p.sw / (unsigned) p.dw);
    const int ax1 = p.x0 + (int) (((uint64_t) (ox0 + nox) * (unsigned) p.sw + (unsigned) p.dw - 1) / (unsigned) p.dw);
    const int ay0 = p.y0 + (int) ((uint64_t) j0 * (unsigned) p.sh / (unsigned) p.dh);
    const int ay1 = p.y0 + (int) (((uint64_t) j1 * (unsigned) p.sh + (unsigned) p.dh - 1) / (unsigned) p.dh);
    const int ux0 = ax0 & ~7, ry0 = ay0 & ~7;
    const int ncols = ax1 - ux0, nrows = ay1 - ry0;
    const int nU = (ncols + 7) >> 3, nUg = (nU + 7) >> 3, nRg = (nrows + 7) >> 3;
    if (nU > SC_MAXU || nrows > SC_MAXR) return;          // (not with the cells the host chooses)
    // ---- the window: a wave takes 8 rows x 8 units at a time, four loads in flight
    const int n_items = nUg * nRg, r = lane >> 3, c = lane & 7;
    for (int base = wave; base < n_items; base += 16) {
        piece_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int it = base + 4 * k, rg = it / nUg, ug = it - rg * nUg;
            const int unit = ug * 8 + c, y = ry0 + rg * 8 + r, x = ux0 + unit * 8;
            if (it < n_items && unit < nU && y >= ay0 && y < ay1) v[k] = load8<pixel, TILED>(p.s, p.sstride, x, y, p.pw - x, p.swide);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int it = base + 4 * k, rg = it / nUg, ug = it - rg * nUg;
            const int unit = ug * 8 + c, y = ry0 + rg * 8 + r;
            if (it < n_items && unit < nU && y >= ay0 && y < ay1) *reinterpret_cast<piece_t *>(&L.raw[(y - ry0) * SC_PITCH + unit * 8]) = v[k];
        }
    }
    // ---- the weights
    if (tid < nox) {
        int i0;
        L.nx[tid] = (uint8_t) scale_weights(ox0 + tid, p.sw, p.dw, &i0, &L.wx[0][tid], SC_OW);
        L.ix[tid] = (uint16_t) (p.x0 + i0 - ux0);
    } else if (tid >= SC_OW && tid < SC_OW + (j1 - j0)) {
        const int jr = j0 - oyb + tid - SC_OW;
        int i0;
        L.ny[jr] = (uint8_t) scale_weights(oyb + jr, p.sh, p.dh, &i0, &L.wy[0][jr], SC_OR);
        L.iy[jr] = (uint16_t) (p.y0 + i0 - ry0);
    }
    __syncthreads();
    // ---- down: every column of the window, for the rows of the cell
    const int nj = j1 - j0;
    for (int it = tid; it < nj * ncols; it += 256) {
        const int j = it / ncols, col = it - j * ncols, jr = j + j0 - oyb;
        const pixel *const src = &L.raw[L.iy[jr] * SC_PITCH + col];
        const int n = L.ny[jr];
        unsigned sum = 8;
#pragma unroll
        for (int k = 0; k < SC_TAPS; k++)
            if (k < n) sum = dv::mad_u24(L.wy[k][jr], src[k * SC_PITCH], sum);
        L.t[j * SC_PITCH + col] = sum >> 4;
    }
    __syncthreads();
    // ---- across
    for (int it = tid; it < nj * nox; it += 256) {
        const int j = it / nox, o = it - j * nox;
        const uint32_t *const src = &L.t[j * SC_PITCH + L.ix[o]];
        const int n = L.nx[o];
        unsigned sum = 1u << 19;
#pragma unroll
        for (int k = 0; k < SC_TAPS; k++)
            if (k < n) sum = dv::mad_u24(L.wx[k][o], src[k], sum);
        out[(j + j0 - oyb) * SC_OW + o] = (uint16_t) (sum >> 20);
    }
    __syncthreads();
}

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

// ---- the host side

struct ScaleGeom {
    int x0, y0, w, h;       // the crop
    int dw, dh;
    int mono, ss_hor, ss_ver;
};

// the crop and the ratio: what dav1d_hip_surface_export_scaled refuses beyond what the plain export does
inline int scale_geom_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, ScaleGeom *const g)
{
    const int W = src->p[0].w, H = src->p[0].h;
    g->mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    g->ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420; g->ss_hor = !g->mono && src->layout != DAV1D_HIP_LAYOUT_I444;
    g->x0 = crop ? crop->x0 : 0; g->y0 = crop ? crop->y0 : 0; g->w = crop ? crop->w : W; g->h = crop ? crop->h : H;
    g->dw = dst->w; g->dh = dst->h;
    if (g->w <= 0 || g->h <= 0 || g->x0 < 0 || g->y0 < 0 || g->x0 > W - g->w || g->y0 > H - g->h) return -EINVAL;
    if ((g->ss_hor && (g->x0 & 1)) || (g->ss_ver && (g->y0 & 1))) return -EINVAL;
    if (g->dw > g->w || g->dh > g->h || g->w > 8LL * g->dw || g->h > 8LL * g->dh) return -ENOTSUP;
    return 0;
}

template <typename pixel, bool TILED>
ScalePlane make_scale_plane(const Dav1dHipPicture *const src, void *const *const planes, const ScaleGeom &g, const int pl)
{
    const int ssh = pl ? g.ss_hor : 0, ssv = pl ? g.ss_ver : 0;
    ScalePlane p = ScalePlane();
    p.s = planes[pl];
    p.sstride = (int) (src->p[pl].stride / (ptrdiff_t) sizeof(pixel));
    p.swide = TILED || aligned_to(planes[pl], src->p[pl].stride, 8 * (int) sizeof(pixel));
    p.pw = src->p[pl].w;
    p.x0 = g.x0 >> ssh; p.y0 = g.y0 >> ssv; p.sw = (g.w + ssh) >> ssh; p.sh = (g.h + ssv) >> ssv;
    p.dw = (g.dw + ssh) >> ssh; p.dh = (g.dh + ssv) >> ssv;
    p.ow = p.sw <= 2LL * p.dw ? 128 : p.sw <= 4LL * p.dw ? 64 : 32;
    p.oh = p.sh <= 4LL * p.dh ? 8 : 4;
    return p;
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

template <typename pixel, bool TILED>
int launch_scaled_sample(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                         const ScaleGeom &g, const int row0, const int row1)
{
    if (dst->sample == DAV1D_HIP_SAMPLE_F32) {
        OutF32 o; o.scale = (float) (1.0 / (double) ((1 << src->bpc) - 1));
        return launch_scaled<pixel, TILED, OutF32>(c, dst, src, planes, g, row0, row1, o);
    }
    if constexpr (sizeof(pixel) == 2) {
        if (dst->sample == DAV1D_HIP_SAMPLE_MSB16) {
            OutMsb16 o; o.shift = 16 - src->bpc;
            return launch_scaled<pixel, TILED, OutMsb16>(c, dst, src, planes, g, row0, row1, o);
        }
    }
    return launch_scaled<pixel, TILED, OutNative<pixel>>(c, dst, src, planes, g, row0, row1, OutNative<pixel>());
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
    (void) hipEventRecord(c->ev_t0, c->stream);
    int rc;
    if (src->bpc == 8) rc = call.tiled ? launch_scaled_sample<uint8_t, true>(c, dst, src, planes, g, row0, row1) : launch_scaled_sample<uint8_t, false>(c, dst, src, planes, g, row0, row1);
    else rc = call.tiled ? launch_scaled_sample<uint16_t, true>(c, dst, src, planes, g, row0, row1) : launch_scaled_sample<uint16_t, false>(c, dst, src, planes, g, row0, row1);
    (void) hipEventRecord(c->ev_t1, c->stream);
    c->last_ms_pending = !rc;
    return rc;
}

extern "C" int dav1d_hip_surface_scaled_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop, int drow1)
{
    SurfaceCall call;
    if (const int rc = surface_args_check(dst, src, 0, drow1, &call, true)) return rc;
    ScaleGeom g;
    if (const int rc = scale_geom_check(dst, src, crop, &g)) return rc;
    const int r1 = call.row1;
    if (r1 <= 0) return 0;
    long long need = g.y0 + ((long long) r1 * g.h + g.dh - 1) / g.dh;
    if (!g.mono) {
        const int sh = (g.h + g.ss_ver) >> g.ss_ver, dch = (g.dh + g.ss_ver) >> g.ss_ver, cr1 = r1 >= g.dh ? dch : r1 >> g.ss_ver;
        const long long cneed = ((long long) (g.y0 >> g.ss_ver) + ((long long) cr1 * sh + dch - 1) / dch) << g.ss_ver;
        if (cneed > need) need = cneed;
    }
    return (int) (need > src->p[0].h ? src->p[0].h : need);
}
