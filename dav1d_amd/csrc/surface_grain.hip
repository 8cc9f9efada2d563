// Output on the device with film grain: dav1d_hip_surface_export_grain (include/dav1d_hip.h) writes what dav1d_hip_surface_export writes from the
// picture dav1d_hip_fg_apply_prepared produces, in one pass over the source: no grained picture in between, no un-tile of a source that lives in its
// twin.  Grain is defined on the output only, so the pass that writes the output is where it belongs.
//
// The unit and the wave are the export's (surface_common.h, surface.hip): a lane owns 8 adjacent samples, a wave a 64 x 8 cell.  8 divides 32, so a
// unit lies in ONE grain block (at 4:2:0 / 4:2:2 a chroma unit in one 16-wide chroma block, over 16 luma samples of one luma block): the block's
// random offset, and with it the row of the template, is the same for the 8 samples.  The arithmetic per sample is fg_apply_kernel's (fg.hip), in
// its order: template sample, the 2-sample overlap blends across and up, round2(scaling[val] * grain, shift), clip.  Chroma takes its scaling
// index from the UNGRAINED luma of row y << ss_ver (pairs averaged when subsampled across, the column clamped to w - 1: the sample right of w is
// not defined in a twin and is never used).
//
// Workgroups are four waves: they share the scaling tables in LDS (random lookups, 1 << bpc bytes each).  The templates stay in memory: a unit
// reads 16 consecutive bytes of one template row, 36 KB of templates serve the whole launch from the caches, and 36 KB of LDS per workgroup
// would cost more to fill than the workgroup's own pixels.  Which planes get grain is uniform per launch (kernel arguments, not template
// parameters): a part of a planar surface that gets none runs the plain copy body.
#include "surface_call.h"
#include "fg_common.h"

namespace {

struct GrainArgs {
    const int16_t *luts;        // [3][GH + 1][GW]
    const uint8_t *scaling;     // [3][scaling_size]
    const uint8_t *offs;        // [block row][nbx]
    int nbx;
    int scaling_size, scaling_shift, overlap, csfl;
    int w;                      // luma samples per row (the clamp of the chroma's luma column)
    int sx, sy;                 // chroma subsampling
    int bitdepth_max, grain_min, grain_max;
    int lo, hi[2];              // clip: luma / chroma upper end
    int uv_mult[2], uv_luma_mult[2], uv_offset[2];      // (uv_offset already shifted to the bit depth)
    int on[3];                  // the plane gets grain
};

constexpr int GRAIN_ROWS = 4;      // cells under one another per wave (planar / semi-planar): one 32-row luma block row per wave when aligned

__device__ __forceinline__ int blend5(const int a, const int wa, const int b, const int wb, const GrainArgs &k) {
    return dv::iclip(round2(a * wa + b * wb, 5), k.grain_min, k.grain_max);
}

// the grain of the 8 samples at (x, y) of a plane subsampled by (sx, sy), x a multiple of 8: fg_apply_kernel's per-sample lookups and blends
__device__ __forceinline__ void grain8(int (&g)[8], const GrainArgs &k, const int16_t *const lut, const int sx, const int sy, const int x, const int y)
{
    const int bw = 32 >> sx, bh = 32 >> sy;
    const int bxi = x >> (5 - sx), row = y >> (5 - sy), xin = x & (bw - 1), yin = y & (bh - 1);
    const uint8_t *const orow = k.offs + (size_t) row * k.nbx;
    const int mx = 2 >> sx, my = 2 >> sy;
    const int oc = orow[bxi];
    const int16_t *const pc = lut + (3 + my * (3 + (oc & 15)) + yin) * GW + 3 + mx * (3 + (oc >> 4)) + xin;
#pragma unroll
    for (int e = 0; e < 8; e++) g[e] = pc[e];
    const bool left = k.overlap && bxi && !xin, up = k.overlap && row && yin < my;
    if (left) {         // the first 2 >> sx samples of a block: blended with the block on the left, continued
        const int ol = orow[bxi - 1];
        const int16_t *const pl = lut + (3 + my * (3 + (ol & 15)) + yin) * GW + 3 + mx * (3 + (ol >> 4)) + bw;
#pragma unroll
        for (int e = 0; e < 2; e++)
            if (e < mx) g[e] = blend5(pl[e], sx ? 23 : e ? 17 : 27, g[e], sx ? 22 : e ? 27 : 17, k);
    }
    if (up) {           // the first 2 >> sy rows: blended with the block above, continued (itself blended with ITS left neighbour first)
        const int ou = orow[bxi - k.nbx];
        const int16_t *const pu = lut + (3 + my * (3 + (ou & 15)) + yin + bh) * GW + 3 + mx * (3 + (ou >> 4)) + xin;
        int t[8];
#pragma unroll
        for (int e = 0; e < 8; e++) t[e] = pu[e];
        if (left) {
            const int olu = orow[bxi - 1 - k.nbx];
            const int16_t *const plu = lut + (3 + my * (3 + (olu & 15)) + yin + bh) * GW + 3 + mx * (3 + (olu >> 4)) + bw;
#pragma unroll
            for (int e = 0; e < 2; e++)
                if (e < mx) t[e] = blend5(plu[e], sx ? 23 : e ? 17 : 27, t[e], sx ? 22 : e ? 27 : 17, k);
        }
        const int wa = sy ? 23 : yin ? 17 : 27, wb = sy ? 22 : yin ? 27 : 17;
#pragma unroll
        for (int e = 0; e < 8; e++) g[e] = blend5(t[e], wa, g[e], wb, k);
    }
}

// luma: 8 samples of `v` with their grain (sc: the luma scaling table in LDS).  The mask keeps a lookup inside the table for what lies right of
// the picture in a twin (never stored); it changes no sample of the picture.
template <typename pixel>
__device__ __forceinline__ void grain_luma8(int (&res)[8], const Piece<8 * sizeof(pixel)> &v, const GrainArgs &k, const uint8_t *const sc, const int x, const int y)
{
    int g[8];
    grain8(g, k, k.luts, 0, 0, x, y);
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int s = sample_of<pixel>(v, e);
        res[e] = dv::iclip(s + round2(sc[s & k.bitdepth_max] * g[e], k.scaling_shift), k.lo, k.hi[0]);
    }
}

// the scaling index source of 8 chroma samples at xc: the luma under them, la at (xc << sx), lb 8 further (sx only; not loaded where it starts
// right of the picture: then every use of it is clamped away or belongs to no sample)
template <typename pixel>
__device__ __forceinline__ void luma_under8(int (&lum)[8], const Piece<8 * sizeof(pixel)> &la, const Piece<8 * sizeof(pixel)> &lb, const GrainArgs &k, const int sx, const int xc)
{
    if (!sx) {
#pragma unroll
        for (int e = 0; e < 8; e++) lum[e] = sample_of<pixel>(la, e);
        return;
    }
    const int lx = xc << 1;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int a = e < 4 ? sample_of<pixel>(la, 2 * e) : sample_of<pixel>(lb, 2 * e - 8);
        const int b = e < 4 ? sample_of<pixel>(la, 2 * e + 1) : sample_of<pixel>(lb, 2 * e - 7);
        lum[e] = (a + (lx + 2 * e + 1 < k.w ? b : a) + 1) >> 1;
    }
}

// chroma plane 1 + uv: 8 samples of `v` at (xc, yc) with their grain; lum from luma_under8; sc: the plane's scaling table in LDS
template <typename pixel>
__device__ __forceinline__ void grain_chroma8(int (&res)[8], const Piece<8 * sizeof(pixel)> &v, const int (&lum)[8], const GrainArgs &k, const uint8_t *const sc,
                                              const int uv, const int sx, const int sy, const int xc, const int yc)
{
    int g[8];
    grain8(g, k, k.luts + (1 + uv) * (GH + 1) * GW, sx, sy, xc, yc);
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int s = sample_of<pixel>(v, e);
        int val = lum[e];
        if (!k.csfl) val = dv::iclip(((lum[e] * k.uv_luma_mult[uv] + s * k.uv_mult[uv]) >> 6) + k.uv_offset[uv], 0, k.bitdepth_max);
        res[e] = dv::iclip(s + round2(sc[val & k.bitdepth_max] * g[e], k.scaling_shift), k.lo, k.hi[1]);
    }
}

template <typename pixel>
__device__ __forceinline__ void plain8(int (&res)[8], const Piece<8 * sizeof(pixel)> &v) {
#pragma unroll
    for (int e = 0; e < 8; e++) res[e] = sample_of<pixel>(v, e);
}

// table `t` of the handle into LDS by the whole workgroup (16-byte pieces: the tables are 16-byte aligned, their size a multiple of 256)
__device__ __forceinline__ void stage_table(uint8_t *const dst, const GrainArgs &k, const int t)
{
    const uint8_t *const src = k.scaling + (size_t) t * k.scaling_size;
    for (int i = (int) threadIdx.x * 16; i < k.scaling_size; i += 256 * 16) *reinterpret_cast<Piece<16> *>(dst + i) = *reinterpret_cast<const Piece<16> *>(src + i);
}

// ---- planar and semi-planar.  ROWS cells under one another, loads first (the part's own pieces and, for chroma, the luma under them)
template <typename pixel, bool TILED, typename Out, bool INTERLEAVE, int ROWS>
__device__ __forceinline__ void grain_cells(const SurfPart &p, const Out &out, const GrainArgs &k, const uint8_t *const sc0, const uint8_t *const sc1,
                                            const int pl, const void *const luma, const int lstride, const int lwide, const int x, const int n, const int ybase)
{
    typedef typename Out::T T;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const int sx = pl ? k.sx : 0, sy = pl ? k.sy : 0;
    const bool on0 = k.on[pl], on1 = INTERLEAVE && k.on[2];
    const bool need_luma = pl && (on0 || on1);
    const int lx = x << sx;
    piece_t u[ROWS], v[INTERLEAVE ? ROWS : 1], la[ROWS], lb[ROWS];
#pragma unroll
    for (int q = 0; q < ROWS; q++) {
        const int y = ybase + q * 8;
        if (y < p.y0 || y >= p.y1) continue;
        u[q] = load8<pixel, TILED>(p.s0, p.sstride, x, y, n, p.swide);
        if (INTERLEAVE) v[q] = load8<pixel, TILED>(p.s1, p.sstride, x, y, n, p.swide);
        la[q] = piece_t(); lb[q] = piece_t();
        if (need_luma) {
            la[q] = load8<pixel, TILED>(luma, lstride, lx, y << sy, k.w - lx, lwide);
            if (sx && lx + 8 < k.w) lb[q] = load8<pixel, TILED>(luma, lstride, lx + 8, y << sy, k.w - lx - 8, lwide);
        }
    }
#pragma unroll
    for (int q = 0; q < ROWS; q++) {
        const int y = ybase + q * 8;
        if (y < p.y0 || y >= p.y1) continue;
        int r0[8], r1[8], lum[8];
        if (need_luma) luma_under8<pixel>(lum, la[q], lb[q], k, sx, x);
        if (!pl) { if (on0) grain_luma8<pixel>(r0, u[q], k, sc0, x, y); else plain8<pixel>(r0, u[q]); }
        else if (on0) grain_chroma8<pixel>(r0, u[q], lum, k, sc0, pl - 1, sx, sy, x, y);
        else plain8<pixel>(r0, u[q]);
        T *const row = (T *) ((uint8_t *) p.d + (size_t) y * p.dstride);
        if (INTERLEAVE) {
            if (on1) grain_chroma8<pixel>(r1, v[q], lum, k, sc1, 1, sx, sy, x, y); else plain8<pixel>(r1, v[q]);
            T t[16];
#pragma unroll
            for (int i = 0; i < 8; i++) { t[2 * i] = out(r0[i]); t[2 * i + 1] = out(r1[i]); }
            store_run<T, 16>(row + 2 * x, t, 2 * n, p.dwide);
        } else {
            T t[8];
#pragma unroll
            for (int i = 0; i < 8; i++) t[i] = out(r0[i]);
            store_run<T, 8>(row + x, t, n, p.dwide);
        }
    }
}

// the waves of a workgroup belong to one part (make_copy_args rounds a part's waves up to four)
template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_grain_copy_kernel(const CopyArgs a, const Out out, const GrainArgs k, const void *const luma, const int lstride, const int lwide)
{
    __shared__ __attribute__((aligned(16))) uint8_t sc_s[2][4096];
    int g = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    int pl = 0;
    SurfPart p = a.part[0];
    if (g >= p.n_waves) {
        g -= p.n_waves; p = a.part[1]; pl = 1;
        if (g >= p.n_waves) { g -= p.n_waves; p = a.part[2]; pl = 2; }
    }
    const bool any = k.on[pl] || (p.interleave && k.on[2]);
    if (any) {          // (uniform in the workgroup)
        if (k.on[pl]) stage_table(sc_s[0], k, pl && !k.csfl ? pl : 0);
        if (p.interleave && k.on[2]) stage_table(sc_s[1], k, k.csfl ? 0 : 2);
        __syncthreads();
    }
    const int cyg = g / p.n_cx, cx = g - cyg * p.n_cx;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const int x = cx * 64 + c * 8, n = p.w - x;
    if (n <= 0) return;
    const int ybase = ((p.y0 >> 3) + cyg * GRAIN_ROWS) * 8 + r;
    if (!any) {         // a plane without grain: the plain copy body
        if (p.interleave) {
            copy_cells<pixel, TILED, Out, true, GRAIN_ROWS / 2>(p, out, x, n, ybase);
            copy_cells<pixel, TILED, Out, true, GRAIN_ROWS / 2>(p, out, x, n, ybase + GRAIN_ROWS * 4);
        } else
            copy_cells<pixel, TILED, Out, false, GRAIN_ROWS>(p, out, x, n, ybase);
    } else if (p.interleave) {
        grain_cells<pixel, TILED, Out, true, GRAIN_ROWS / 2>(p, out, k, sc_s[0], sc_s[1], pl, luma, lstride, lwide, x, n, ybase);
        grain_cells<pixel, TILED, Out, true, GRAIN_ROWS / 2>(p, out, k, sc_s[0], sc_s[1], pl, luma, lstride, lwide, x, n, ybase + GRAIN_ROWS * 4);
    } else
        grain_cells<pixel, TILED, Out, false, GRAIN_ROWS>(p, out, k, sc_s[0], sc_s[1], pl, luma, lstride, lwide, x, n, ybase);
}

// ---- RGB planes: surface_rgb_kernel's lane (8 chroma pairs and the (8 << SSH) x (1 << SSV) luma samples above them).  The luma of row
// yc << SSV is in registers anyway: chroma grain costs no load of its own.
template <typename pixel, bool TILED, int SSH, int SSV, typename Out>
__global__ __launch_bounds__(256) void surface_grain_rgb_kernel(const RgbArgs a, const Out out, const GrainArgs k, const int n_cells)
{
    typedef typename Out::T T;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    __shared__ __attribute__((aligned(16))) uint8_t sc_s[3][4096];
    if (k.on[0] || k.csfl) stage_table(sc_s[0], k, 0);
    if (!k.csfl) {
        if (k.on[1]) stage_table(sc_s[1], k, 1);
        if (k.on[2]) stage_table(sc_s[2], k, 2);
    }
    __syncthreads();
    const int g = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);
    if (g >= n_cells) return;
    const int cyg = g / a.n_cx, cx = g - cyg * a.n_cx;
    const int lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const int xc = cx * 64 + c * 8, yc = ((a.crow0 >> 3) + cyg) * 8 + r;
    if (xc >= a.cw || yc < a.crow0 || yc >= a.crow1) return;
    piece_t u = piece_t(), v = piece_t(), yy[1 << SSV][1 << SSH];
    if (!a.mono) {
        u = load8<pixel, TILED>(a.s[1], a.sstride[1], xc, yc, a.cw - xc, a.swide[1]);
        v = load8<pixel, TILED>(a.s[2], a.sstride[1], xc, yc, a.cw - xc, a.swide[1]);
    }
#pragma unroll
    for (int i = 0; i < 1 << SSV; i++)
#pragma unroll
        for (int j = 0; j < 1 << SSH; j++) {
            const int x = (xc << SSH) + j * 8, y = (yc << SSV) + i;
            yy[i][j] = piece_t();
            if (x < a.w && y < a.row1) yy[i][j] = load8<pixel, TILED>(a.s[0], a.sstride[0], x, y, a.w - x, a.swide[0]);
        }
    // chroma first: from the ungrained luma of row yc << SSV (yy[0][*]: that row is always inside the band)
    int cu[8], cv[8];
    if (!a.mono) {
        int lum[8];
        if (k.on[1] || k.on[2]) luma_under8<pixel>(lum, yy[0][0], yy[0][(1 << SSH) - 1], k, SSH, xc);
        if (k.on[1]) grain_chroma8<pixel>(cu, u, lum, k, sc_s[k.csfl ? 0 : 1], 0, SSH, SSV, xc, yc); else plain8<pixel>(cu, u);
        if (k.on[2]) grain_chroma8<pixel>(cv, v, lum, k, sc_s[k.csfl ? 0 : 2], 1, SSH, SSV, xc, yc); else plain8<pixel>(cv, v);
    }
#pragma unroll
    for (int j = 0; j < 1 << SSH; j++) {
        const int x = (xc << SSH) + j * 8;
        if (x >= a.w) continue;
        int tr[8], tg[8], tb[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int ce = (j * 8 + e) >> SSH;
            rgb_chroma_terms(a, a.mono ? 0 : cu[ce] - a.mid, a.mono ? 0 : cv[ce] - a.mid, tr[e], tg[e], tb[e]);
        }
#pragma unroll
        for (int i = 0; i < 1 << SSV; i++) {
            const int y = (yc << SSV) + i;
            if (y >= a.row1) continue;
            int Y[8];
            if (k.on[0]) grain_luma8<pixel>(Y, yy[i][j], k, sc_s[0], x, y); else plain8<pixel>(Y, yy[i][j]);
            T R[8], G[8], B[8];
#pragma unroll
            for (int e = 0; e < 8; e++) rgb_of(a, out, Y[e], tr[e], tg[e], tb[e], R[e], G[e], B[e]);
            const size_t off = (size_t) x * sizeof(T);
            store_run<T, 8>((T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0] + off), R, a.w - x, a.dwide);
            store_run<T, 8>((T *) ((uint8_t *) a.d[1] + (size_t) y * a.dstride[1] + off), G, a.w - x, a.dwide);
            store_run<T, 8>((T *) ((uint8_t *) a.d[2] + (size_t) y * a.dstride[2] + off), B, a.w - x, a.dwide);
        }
    }
}

template <typename pixel, bool TILED, typename Out>
int launch_grain(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                 const int row0, const int row1, const Out &out, const GrainArgs &k)
{
    typedef typename Out::T T;
    if (dst->format == DAV1D_HIP_SURFACE_RGB_PLANAR) {
        unsigned n_cells;
        const RgbArgs a = make_rgb_args<pixel, TILED, T>(dst, src, planes, row0, row1, &n_cells);
        const dim3 grid((n_cells + 3) / 4);
        if (k.sy) hipLaunchKernelGGL((surface_grain_rgb_kernel<pixel, TILED, 1, 1, Out>), grid, dim3(256), 0, c->stream, a, out, k, (int) n_cells);
        else if (k.sx) hipLaunchKernelGGL((surface_grain_rgb_kernel<pixel, TILED, 1, 0, Out>), grid, dim3(256), 0, c->stream, a, out, k, (int) n_cells);
        else hipLaunchKernelGGL((surface_grain_rgb_kernel<pixel, TILED, 0, 0, Out>), grid, dim3(256), 0, c->stream, a, out, k, (int) n_cells);
        return hip_rc(hipGetLastError());
    }
    unsigned n_waves;
    const CopyArgs a = make_copy_args<pixel, TILED, T>(dst, src, planes, row0, row1, GRAIN_ROWS, 4, &n_waves);
    const int lstride = (int) (src->p[0].stride / (ptrdiff_t) sizeof(pixel));
    const int lwide = TILED || aligned_to(planes[0], src->p[0].stride, 8 * (int) sizeof(pixel));
    hipLaunchKernelGGL((surface_grain_copy_kernel<pixel, TILED, Out>), dim3(n_waves / 4), dim3(256), 0, c->stream, a, out, k, (const void *) planes[0], lstride, lwide);
    return hip_rc(hipGetLastError());
}

// the handle's offsets table of this geometry: a new one (the caller fills it on the context's stream) the first time, kept until the handle goes
const uint8_t *offsets_of(Dav1dHipContext *const c, const Dav1dHipGrain *const g, const int nbx, const int nby, int *const rc)
{
    *rc = 0;
    for (const Dav1dHipGrain::Offsets &o : g->offs)
        if (o.nbx == nbx && o.nby == nby) return o.dev;
    Dav1dHipGrain::Offsets o = { nullptr, nbx, nby };
    if ((*rc = hip_rc(hipMalloc((void **) &o.dev, (size_t) nbx * nby + 16)))) return nullptr;
    g->offs.push_back(o);
    return o.dev;
}

} // namespace

extern "C" int dav1d_hip_surface_export_grain(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipGrain *grain,
                                              int is_id, int row0, int row1)
{
    SurfaceCall call;
    if (const int rc = surface_call_check(c, dst, src, row0, row1, &call)) return rc;
    if (!grain || grain->bpc != src->bpc || grain->layout != src->layout) return -EINVAL;
    const Dav1dHipFilmGrainData *const d = &grain->data;
    const SurfaceGeom geo = surface_geom(src, call.row0, call.row1);
    GrainArgs k;
    memset(&k, 0, sizeof(k));
    k.on[0] = d->num_y_points != 0;
    for (int i = 0; i < 2; i++) k.on[1 + i] = !geo.mono && (d->num_uv_points[i] || d->chroma_scaling_from_luma);
    if (!k.on[0] && !k.on[1] && !k.on[2]) return dav1d_hip_surface_export(c, dst, src, row0, row1);        // no plane of this picture gets grain
    if (call.row1 <= call.row0) return 0;
    const int nbx = (geo.w + 31) / 32, nby = (geo.h + 31) / 32;
    const size_t n_tables = grain->offs.size();
    int rc;
    const uint8_t *const offs = offsets_of(c, grain, nbx, nby, &rc);
    if (rc) return rc;
    const int bd8 = src->bpc - 8;
    k.luts = (const int16_t *) grain->dev; k.scaling = grain->dev + grain->lut_bytes; k.offs = offs; k.nbx = nbx;
    k.scaling_size = (int) grain->scaling_size; k.scaling_shift = d->scaling_shift; k.overlap = d->overlap_flag; k.csfl = d->chroma_scaling_from_luma;
    k.w = geo.w; k.sx = geo.ss_hor; k.sy = geo.ss_ver;
    k.bitdepth_max = (1 << src->bpc) - 1; k.grain_min = -(128 << bd8); k.grain_max = (128 << bd8) - 1;
    k.lo = 0; k.hi[0] = k.hi[1] = k.bitdepth_max;
    if (d->clip_to_restricted_range) { k.lo = 16 << bd8; k.hi[0] = 235 << bd8; k.hi[1] = (is_id ? 235 : 240) << bd8; }
    for (int i = 0; i < 2; i++) { k.uv_mult[i] = d->uv_mult[i]; k.uv_luma_mult[i] = d->uv_luma_mult[i]; k.uv_offset[i] = d->uv_offset[i] * (1 << bd8); }
    rc = hip_rc(hipStreamWaitEvent(c->stream, grain->ready, 0));
    if (rc) return rc;
    const CallTimer t(c);          // (behind the wait, in front of the offsets)
    if (grain->offs.size() != n_tables) {
        rc = dav1d_hip_launch_fg_offsets(const_cast<uint8_t *>(offs), d->seed, nby, nbx, c->stream);
        if (rc) { grain->offs.pop_back(); (void) hipFree(const_cast<uint8_t *>(offs)); }        // (nothing was enqueued that reads it)
    }
    void *const *const planes = call.planes;
    if (!rc) rc = with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        typedef decltype(px) pixel;
        return with_out<pixel>(dst->sample, src->bpc, [&](const auto &out) {
            return launch_grain<pixel, decltype(state)::value>(c, dst, src, planes, call.row0, call.row1, out, k);
        });
    });
    return t.done(rc);
}
