// Output on the device: a decoded picture leaves the library as a surface the caller owns (dav1d_hip_surface_export, include/dav1d_hip.h).
// One bandwidth-bound pass: integer, no LDS, nothing that waits on another workgroup.  It reads the picture where it lives — raster planes, or the
// 8x8-tiled twin (Dav1dHipPicture.twin) without un-tiling it first — and writes the visible samples in the caller's layout.
//
// The unit of work is 8 horizontally adjacent samples: one 16-byte row of an 8x8 tile of the twin at 10 / 12 bits, one 16-byte piece of a raster
// row.  A wave is laid out as 8 rows x 8 units (lane = row * 8 + unit), i.e. a 64 x 8 cell of a plane: a load of the wave takes eight WHOLE
// tiles of the twin (eight 128-byte lines, each lane its 16 bytes) or eight 128-byte pieces of raster rows, a store leaves eight pieces of
// 128 consecutive bytes of destination rows (256 where a lane leaves 32: interleaved chroma, float samples).  Both sides are whole memory lines when
// the destination rows start on one; no line is requested twice.
#include "capi.h"
#include <string.h>

namespace {

template <int BYTES> struct alignas(BYTES) Piece { uint32_t a[BYTES / 4]; };

// 8 samples of a plane at (x, y), x a multiple of 8.  `wide`: base and stride allow one vector load (always so in the twin); else the n valid samples one by one.
template <typename pixel, bool TILED>
__device__ __forceinline__ Piece<8 * sizeof(pixel)> load8(const void *const base, const int stride, const int x, const int y, const int n, const bool wide)
{
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const pixel *const p = (const pixel *) base;
    if (TILED)        // tile (x >> 3, y >> 3) at ty * 8 * stride + tx * 64, row r of it 8 pixels further
        return *reinterpret_cast<const piece_t *>(p + (size_t) (y >> 3) * 8 * stride + (size_t) (x >> 3) * 64 + (y & 7) * 8);
    const pixel *const row = p + (size_t) y * stride + x;
    if (wide) return *reinterpret_cast<const piece_t *>(row);
    pixel t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = i < n ? row[i] : (pixel) 0;
    piece_t v;
    __builtin_memcpy(&v, t, sizeof(v));
    return v;
}
template <typename pixel> __device__ __forceinline__ int sample_of(const Piece<8 * sizeof(pixel)> &v, const int i) {
    return sizeof(pixel) == 2 ? (int) ((v.a[i >> 1] >> ((i & 1) * 16)) & 0xffff) : (int) ((v.a[i >> 2] >> ((i & 3) * 8)) & 0xff);
}

// N output samples to consecutive addresses: vector stores of up to 16 bytes where the destination allows and the run is whole, else the first n one by one
template <typename T, int N>
__device__ __forceinline__ void store_run(T *const dst, const T (&t)[N], const int n, const bool wide)
{
    constexpr int BYTES = N * (int) sizeof(T), CH = BYTES >= 16 ? 16 : BYTES;
    if (wide && n >= N) {
#pragma unroll
        for (int i = 0; i < BYTES / CH; i++) {
            Piece<CH> pc;
            __builtin_memcpy(&pc, (const char *) t + i * CH, CH);
            reinterpret_cast<Piece<CH> *>(dst)[i] = pc;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) if (i < n) dst[i] = t[i];
    }
}

// ---- the output sample, as a small functor (the kernels are templates over it)
template <typename pixel> struct OutNative { typedef pixel T; __device__ __forceinline__ T operator()(const int v) const { return (T) v; } };
struct OutMsb16 { typedef uint16_t T; int shift; __device__ __forceinline__ T operator()(const int v) const { return (T) (v << shift); } };
struct OutF32 { typedef float T; float scale; __device__ __forceinline__ T operator()(const int v) const { return (float) v * scale; } };

// ---- planar and semi-planar surfaces: every destination plane is a `part`, the waves of a launch are dealt over the parts
struct SurfPart {
    const void *s0, *s1;    // source plane (s1: the second one of an interleaved part, V)
    void *d;
    long long dstride;      // bytes
    int sstride;            // pixels
    int w;                  // visible samples per source row
    int y0, y1;             // rows of the source plane
    int n_cx;               // 64-sample cells across
    int n_waves;
    int interleave, swide, dwide, pad;
};
struct CopyArgs { SurfPart part[3]; };

constexpr int COPY_ROWS = 8;       // cells (of 8 rows) under one another per wave: 8 KB in flight per wave at 16 bits, like the retile passes (mcx.hip)

// ROWS cells (of 8 rows) under one another, loads first: ROWS (x 2 when interleaving) pieces in flight per lane
template <typename pixel, bool TILED, typename Out, bool INTERLEAVE, int ROWS>
__device__ __forceinline__ void copy_cells(const SurfPart &p, const Out &out, const int x, const int n, const int ybase)
{
    typedef typename Out::T T;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    piece_t u[ROWS], v[INTERLEAVE ? ROWS : 1];
#pragma unroll
    for (int k = 0; k < ROWS; k++) {
        const int y = ybase + k * 8;
        if (y < p.y0 || y >= p.y1) continue;
        u[k] = load8<pixel, TILED>(p.s0, p.sstride, x, y, n, p.swide);
        if (INTERLEAVE) v[k] = load8<pixel, TILED>(p.s1, p.sstride, x, y, n, p.swide);
    }
#pragma unroll
    for (int k = 0; k < ROWS; k++) {
        const int y = ybase + k * 8;
        if (y < p.y0 || y >= p.y1) continue;
        T *const row = (T *) ((uint8_t *) p.d + (size_t) y * p.dstride);
        if (INTERLEAVE) {
            T t[16];
#pragma unroll
            for (int i = 0; i < 8; i++) { t[2 * i] = out(sample_of<pixel>(u[k], i)); t[2 * i + 1] = out(sample_of<pixel>(v[k], i)); }
            store_run<T, 16>(row + 2 * x, t, 2 * n, p.dwide);
        } else {
            T t[8];
#pragma unroll
            for (int i = 0; i < 8; i++) t[i] = out(sample_of<pixel>(u[k], i));
            store_run<T, 8>(row + x, t, n, p.dwide);
        }
    }
}

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

// ---- RGB planes.  Integers q(x) = floor(x * 16384 + 0.5) evaluated in double, per matrix (Kr, Kb; Kg = 1 - Kr - Kb), range and depth d
// (max = (1 << d) - 1; limited: sy = max / (219 << (d - 8)), sc = max / (224 << (d - 8)); full: sy = sc = 1):
//     CY = q(sy), CRV = q(2 (1 - Kr) sc), CBU = q(2 (1 - Kb) sc), CGU = q(2 (1 - Kb) Kb / Kg sc), CGV = q(2 (1 - Kr) Kr / Kg sc)
// and, with y = Y - (16 << (d - 8)) (limited) or Y (full), cb = U - (1 << (d - 1)), cr = V - (1 << (d - 1)):
//     R = clip((CY y + CRV cr + 8192) >> 14), G = clip((CY y - CGU cb - CGV cr + 8192) >> 14), B = clip((CY y + CBU cb + 8192) >> 14)
// in int32 (below 2^28 in magnitude at 12 bits), arithmetic shift, clip to [0, max].
//                                           [matrix: BT.709, BT.601, BT.2020 NCL][full range][8, 10, 12 bits][CY, CRV, CBU, CGU, CGV]
const int rgb_coef[3][2][3][5] = {
    { { { 19077, 29372, 34610, 3494, 8731 }, { 19133, 29459, 34711, 3504, 8757 }, { 19147, 29480, 34737, 3507, 8763 } },        // BT.709 (Kr 0.2126, Kb 0.0722) limited
      { { 16384, 25802, 30402, 3069, 7670 }, { 16384, 25802, 30402, 3069, 7670 }, { 16384, 25802, 30402, 3069, 7670 } } },      //        full
    { { { 19077, 26149, 33050, 6419, 13320 }, { 19133, 26226, 33148, 6438, 13359 }, { 19147, 26245, 33172, 6442, 13369 } },     // BT.601 (Kr 0.299, Kb 0.114) limited
      { { 16384, 22970, 29032, 5638, 11700 }, { 16384, 22970, 29032, 5638, 11700 }, { 16384, 22970, 29032, 5638, 11700 } } },   //        full
    { { { 19077, 27503, 35091, 3069, 10657 }, { 19133, 27584, 35194, 3078, 10688 }, { 19147, 27605, 35220, 3080, 10696 } },     // BT.2020 NCL (Kr 0.2627, Kb 0.0593) limited
      { { 16384, 24160, 30825, 2696, 9361 }, { 16384, 24160, 30825, 2696, 9361 }, { 16384, 24160, 30825, 2696, 9361 } } },      //        full
};

struct RgbArgs {
    const void *s[3];
    void *d[3];             // R, G, B
    long long dstride[3];   // bytes
    int sstride[2];         // pixels: luma, chroma
    int swide[2];
    int dwide;
    int w, cw;              // visible samples per luma / chroma row
    int row1;               // luma rows end here (they start at crow0 << SSV: row0 is even)
    int crow0, crow1;       // chroma rows (the luma rows themselves at 4:4:4 and 4:0:0)
    int n_cx;               // cells of 64 chroma samples across
    int cy, crv, cbu, cgu, cgv, yoff, mid, max;
    int identity, mono;
};

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

inline bool aligned_to(const void *const p, const long long stride, const int a) { return !((uintptr_t) p % a) && !(stride % a); }

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
    const int w = src->p[0].w, h = src->p[0].h;
    const int mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    const int ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420, ss_hor = !mono && src->layout != DAV1D_HIP_LAYOUT_I444;
    const int cw = mono ? w : src->p[1].w, ch = mono ? h : src->p[1].h;
    const int crow0 = row0 >> ss_ver, crow1 = row1 >= h ? ch : row1 >> ss_ver;
    const int load_align = 8 * (int) sizeof(pixel);
    if (dst->format == DAV1D_HIP_SURFACE_RGB_PLANAR) {
        RgbArgs a = RgbArgs();
        for (int pl = 0; pl < 3; pl++) { a.s[pl] = planes[pl]; a.d[pl] = dst->data[pl]; a.dstride[pl] = dst->stride[pl]; }
        a.sstride[0] = (int) (src->p[0].stride / (ptrdiff_t) sizeof(pixel));
        a.sstride[1] = mono ? 0 : (int) (src->p[1].stride / (ptrdiff_t) sizeof(pixel));
        a.swide[0] = TILED || aligned_to(planes[0], src->p[0].stride, load_align);
        a.swide[1] = TILED || mono || (aligned_to(planes[1], src->p[1].stride, load_align) && aligned_to(planes[2], src->p[2].stride, load_align));
        const int store_align = 8 * (int) sizeof(T) > 16 ? 16 : 8 * (int) sizeof(T);
        a.dwide = 1;
        for (int pl = 0; pl < 3; pl++) a.dwide &= aligned_to(dst->data[pl], dst->stride[pl], store_align);
        a.w = w; a.cw = cw; a.row1 = row1; a.crow0 = crow0; a.crow1 = crow1;
        a.n_cx = (cw + 63) / 64;
        a.mid = 1 << (src->bpc - 1); a.max = (1 << src->bpc) - 1;
        a.identity = dst->matrix == 0; a.mono = mono;
        if (!a.identity) {
            const int m = dst->matrix == 1 ? 0 : dst->matrix == 9 ? 2 : 1;
            const int *const k = rgb_coef[m][!!dst->full_range][(src->bpc - 8) >> 1];
            a.cy = k[0]; a.crv = k[1]; a.cbu = k[2]; a.cgu = k[3]; a.cgv = k[4];
            a.yoff = dst->full_range ? 0 : 16 << (src->bpc - 8);
        }
        const int n_cy = ((crow1 + 7) >> 3) - (crow0 >> 3);
        const dim3 grid((unsigned) a.n_cx * (unsigned) n_cy);
        launch_rgb<pixel, TILED, Out>(a, out, ss_hor, ss_ver, grid, c->stream);
        return hip_rc(hipGetLastError());
    }
    CopyArgs a = CopyArgs();
    unsigned n_waves = 0;
    const bool semi = dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR;
    const int n_parts = mono ? 1 : semi ? 2 : 3;
    for (int k = 0; k < n_parts; k++) {
        SurfPart &p = a.part[k];
        p.interleave = semi && k == 1;
        p.s0 = planes[k]; p.s1 = p.interleave ? planes[2] : nullptr;
        p.d = dst->data[k]; p.dstride = dst->stride[k];
        p.sstride = (int) (src->p[k].stride / (ptrdiff_t) sizeof(pixel));
        p.w = k ? cw : w;
        p.y0 = k ? crow0 : row0; p.y1 = k ? crow1 : row1;
        p.n_cx = (p.w + 63) / 64;
        const int n_cy = ((p.y1 + 7) >> 3) - (p.y0 >> 3);
        p.n_waves = p.n_cx * ((n_cy + COPY_ROWS - 1) / COPY_ROWS);
        p.swide = TILED || (aligned_to(planes[k], src->p[k].stride, load_align) && (!p.interleave || aligned_to(planes[2], src->p[2].stride, load_align)));
        const int run = (p.interleave ? 16 : 8) * (int) sizeof(T);
        p.dwide = aligned_to(p.d, p.dstride, run > 16 ? 16 : run);
        n_waves += (unsigned) p.n_waves;
    }
    for (int k = n_parts; k < 3; k++) { a.part[k] = a.part[0]; a.part[k].n_waves = 0; }
    hipLaunchKernelGGL((surface_copy_kernel<pixel, TILED, Out>), dim3(n_waves), dim3(64), 0, c->stream, a, out);
    return hip_rc(hipGetLastError());
}

template <typename pixel, bool TILED>
int launch_sample(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes, const int row0, const int row1)
{
    if (dst->sample == DAV1D_HIP_SAMPLE_F32) {
        OutF32 o; o.scale = (float) (1.0 / (double) ((1 << src->bpc) - 1));
        return launch_surface<pixel, TILED, OutF32>(c, dst, src, planes, row0, row1, o);
    }
    if constexpr (sizeof(pixel) == 2) {
        if (dst->sample == DAV1D_HIP_SAMPLE_MSB16) {
            OutMsb16 o; o.shift = 16 - src->bpc;
            return launch_surface<pixel, TILED, OutMsb16>(c, dst, src, planes, row0, row1, o);
        }
    }
    return launch_surface<pixel, TILED, OutNative<pixel>>(c, dst, src, planes, row0, row1, OutNative<pixel>());
}

} // namespace

extern "C" int dav1d_hip_surface_export(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, int row0, int row1)
{
    if (!c || !dst || !src || !src->p[0].data) return -EINVAL;
    if (src->bpc != 8 && src->bpc != 10 && src->bpc != 12) return -EINVAL;
    if (src->layout < DAV1D_HIP_LAYOUT_I400 || src->layout > DAV1D_HIP_LAYOUT_I444) return -EINVAL;
    if (dst->format < DAV1D_HIP_SURFACE_PLANAR || dst->format > DAV1D_HIP_SURFACE_RGB_PLANAR) return -EINVAL;
    if (dst->sample < DAV1D_HIP_SAMPLE_NATIVE || dst->sample > DAV1D_HIP_SAMPLE_F32) return -EINVAL;
    if (dst->sample == DAV1D_HIP_SAMPLE_MSB16 && src->bpc == 8) return -EINVAL;
    const int w = src->p[0].w, h = src->p[0].h;
    if (w <= 0 || h <= 0 || dst->w != w || dst->h != h) return -EINVAL;
    const int mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    if (!mono && (!src->p[1].data || !src->p[2].data)) return -EINVAL;
    const ptrdiff_t ss = dst->sample == DAV1D_HIP_SAMPLE_F32 ? 4 : dst->sample == DAV1D_HIP_SAMPLE_MSB16 ? 2 : src->bpc > 8 ? 2 : 1;
    const bool rgb = dst->format == DAV1D_HIP_SURFACE_RGB_PLANAR;
    const int n_dst = rgb ? 3 : mono ? 1 : dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR ? 2 : 3;
    for (int k = 0; k < n_dst; k++) {
        const ptrdiff_t row_bytes = ss * (rgb || !k ? w : dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR ? 2 * src->p[1].w : src->p[k].w);
        if (!dst->data[k] || dst->stride[k] < row_bytes || dst->stride[k] % ss) return -EINVAL;
    }
    if (rgb) {
        if (dst->matrix == 0) { if (src->layout != DAV1D_HIP_LAYOUT_I444) return -EINVAL; }
        else if (dst->matrix != 1 && dst->matrix != 5 && dst->matrix != 6 && dst->matrix != 9) return -ENOTSUP;
    }
    if (row0 < 0) row0 = 0;
    if (row1 > h) row1 = h;
    if ((row0 & 1) || ((row1 & 1) && row1 < h)) return -EINVAL;       // a chroma row belongs to one band
    const bool tiled = src->twin_ok == DAV1D_HIP_TWIN_ONLY;
    void *planes[3];
    for (int pl = 0; pl < 3; pl++) {
        planes[pl] = pl && mono ? nullptr : tiled ? src->twin[pl] : src->p[pl].data;
        if ((!pl || !mono) && (!planes[pl] || src->p[pl].stride <= 0)) return -EINVAL;
        if ((!pl || !mono) && tiled && (src->p[pl].stride / (src->bpc > 8 ? 2 : 1)) % 8) return -EINVAL;
    }
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (row1 <= row0) return 0;
    (void) hipEventRecord(c->ev_t0, c->stream);
    int rc;
    if (src->bpc == 8) rc = tiled ? launch_sample<uint8_t, true>(c, dst, src, planes, row0, row1) : launch_sample<uint8_t, false>(c, dst, src, planes, row0, row1);
    else rc = tiled ? launch_sample<uint16_t, true>(c, dst, src, planes, row0, row1) : launch_sample<uint16_t, false>(c, dst, src, planes, row0, row1);
    (void) hipEventRecord(c->ev_t1, c->stream);
    c->last_ms_pending = !rc;
    return rc;
}
