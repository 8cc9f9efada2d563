// What the output units share (surface.hip: the plain export; surface_grain.hip: the export with film grain fused in; surface_scale.hip: the export
// with a crop and a scaler in front; surface_rgb.hip: tensor-ready RGB; surface_rgb_scale.hip: that behind the scaler; surface_batch.hip: many of those in one launch;
// surface_resize.hip: both with axes that may go up; surface_reduce.hip: both at thumbnail scale; surface_colour.hip and surface_colour_reduce.hip:
// tensor-ready RGB through a colour stage, at the picture's size and at any size): the 8-sample unit and
// its loads and stores, the output sample functors, the kernel arguments and how a call is checked and turned into them.  See surface.hip for the
// layout of a wave (8 rows x 8 units, a 64 x 8 cell of a plane), surface_call.h for the path of a call from its check to its launch and
// surface_batch.h for that of a batch.
#pragma once
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

// the colour terms of one RGB sample from the chroma terms of its column (tr, tg, tb) and its luma
template <typename Out>
__device__ __forceinline__ void rgb_of(const RgbArgs &a, const Out &out, const int Y, const int tr, const int tg, const int tb,
                                       typename Out::T &R, typename Out::T &G, typename Out::T &B)
{
    if (a.identity) { R = out(tr); G = out(Y); B = out(tb); return; }
    const int l = a.cy * (Y - a.yoff);
    R = out(dv::iclip((l + tr) >> 14, 0, a.max));
    G = out(dv::iclip((l + tg) >> 14, 0, a.max));
    B = out(dv::iclip((l + tb) >> 14, 0, a.max));
}
// ... and those chroma terms from cb = U - mid, cr = V - mid
__device__ __forceinline__ void rgb_chroma_terms(const RgbArgs &a, const int cb, const int cr, int &tr, int &tg, int &tb)
{
    tr = a.identity ? cr + a.mid : a.crv * cr + 8192;
    tg = a.identity ? 0 : 8192 - a.cgu * cb - a.cgv * cr;
    tb = a.identity ? cb + a.mid : a.cbu * cb + 8192;
}

inline bool aligned_to(const void *const p, const long long stride, const int a) { return !((uintptr_t) p % a) && !(stride % a); }

// ---- a call, checked: what dav1d_hip_surface_export refuses, in its order; then the rows clamped and the planes the kernels read
struct SurfaceCall {
    int row0, row1;
    bool tiled;
    void *planes[3];
};

// (`scaled`: the surface has a size of its own, dav1d_hip_surface_export_scaled — the size rule falls away, its planes and rows are the surface's)
// (`ext`: dav1d_hip_surface_export_rgb — the packed formats, one plane of 3 or 4 samples a pixel, and binary16 samples are known as well)
inline int surface_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, int row0, int row1, SurfaceCall *const call, const bool scaled,
                              const bool ext = false)
{
    if (!dst || !src || !src->p[0].data) return -EINVAL;
    if (src->bpc != 8 && src->bpc != 10 && src->bpc != 12) return -EINVAL;
    if (src->layout < DAV1D_HIP_LAYOUT_I400 || src->layout > DAV1D_HIP_LAYOUT_I444) return -EINVAL;
    if (dst->format < DAV1D_HIP_SURFACE_PLANAR || dst->format > (ext ? DAV1D_HIP_SURFACE_RGBA_PACKED : DAV1D_HIP_SURFACE_RGB_PLANAR)) return -EINVAL;
    if (dst->sample < DAV1D_HIP_SAMPLE_NATIVE || dst->sample > (ext ? DAV1D_HIP_SAMPLE_F16 : DAV1D_HIP_SAMPLE_F32)) return -EINVAL;
    if (dst->sample == DAV1D_HIP_SAMPLE_MSB16 && src->bpc == 8) return -EINVAL;
    const int w = src->p[0].w, h = src->p[0].h;
    if (w <= 0 || h <= 0) return -EINVAL;
    if (scaled ? dst->w <= 0 || dst->h <= 0 : dst->w != w || dst->h != h) return -EINVAL;
    const int mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    const int ss_hor = !mono && src->layout != DAV1D_HIP_LAYOUT_I444, dw = dst->w, dh = dst->h;
    if (!mono && (!src->p[1].data || !src->p[2].data)) return -EINVAL;
    const ptrdiff_t ss = dst->sample == DAV1D_HIP_SAMPLE_F32 ? 4 : dst->sample == DAV1D_HIP_SAMPLE_MSB16 || dst->sample == DAV1D_HIP_SAMPLE_F16 ? 2 : src->bpc > 8 ? 2 : 1;
    const bool rgb = dst->format >= DAV1D_HIP_SURFACE_RGB_PLANAR;
    const int packed = dst->format == DAV1D_HIP_SURFACE_RGB_PACKED ? 3 : dst->format == DAV1D_HIP_SURFACE_RGBA_PACKED ? 4 : 0;
    const int n_dst = packed ? 1 : rgb ? 3 : mono ? 1 : dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR ? 2 : 3;
    for (int k = 0; k < n_dst; k++) {
        const int cw = scaled ? (dw + ss_hor) >> ss_hor : src->p[k].w;
        const ptrdiff_t row_bytes = ss * (packed ? (ptrdiff_t) packed * dw : rgb || !k ? dw : dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR ? 2 * cw : cw);
        if (!dst->data[k] || dst->stride[k] < row_bytes || dst->stride[k] % ss) return -EINVAL;
    }
    if (rgb) {
        if (dst->matrix == 0) { if (src->layout != DAV1D_HIP_LAYOUT_I444) return -EINVAL; }
        else if (dst->matrix != 1 && dst->matrix != 5 && dst->matrix != 6 && dst->matrix != 9) return -ENOTSUP;
    }
    if (row0 < 0) row0 = 0;
    if (row1 > dh) row1 = dh;
    if ((row0 & 1) || ((row1 & 1) && row1 < dh)) return -EINVAL;      // a chroma row belongs to one band
    call->row0 = row0; call->row1 = row1;
    call->tiled = src->twin_ok == DAV1D_HIP_TWIN_ONLY;
    for (int pl = 0; pl < 3; pl++) {
        call->planes[pl] = pl && mono ? nullptr : call->tiled ? src->twin[pl] : src->p[pl].data;
        if ((!pl || !mono) && (!call->planes[pl] || src->p[pl].stride <= 0)) return -EINVAL;
        if ((!pl || !mono) && call->tiled && (src->p[pl].stride / (src->bpc > 8 ? 2 : 1)) % 8) return -EINVAL;
    }
    return 0;
}
inline int surface_call_check(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const int row0, const int row1,
                              SurfaceCall *const call, const bool scaled = false)
{
    if (!c) return -EINVAL;
    if (const int rc = surface_args_check(dst, src, row0, row1, call, scaled)) return rc;
    return pictures_on_device(c, src, 1);
}

// the geometry of a call (luma rows [row0, row1), the chroma rows that belong to them)
struct SurfaceGeom {
    int w, h, mono, ss_ver, ss_hor, cw, ch, crow0, crow1;
};
inline SurfaceGeom surface_geom(const Dav1dHipPicture *const src, const int row0, const int row1)
{
    SurfaceGeom g;
    g.w = src->p[0].w; g.h = src->p[0].h;
    g.mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    g.ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420; g.ss_hor = !g.mono && src->layout != DAV1D_HIP_LAYOUT_I444;
    g.cw = g.mono ? g.w : src->p[1].w; g.ch = g.mono ? g.h : src->p[1].h;
    g.crow0 = row0 >> g.ss_ver; g.crow1 = row1 >= g.h ? g.ch : row1 >> g.ss_ver;
    return g;
}

// the colour part of the arguments: the row of rgb_coef the surface asks for
inline void rgb_set_matrix(RgbArgs &a, const Dav1dHipSurface *const dst, const int bpc, const int mono)
{
    a.mid = 1 << (bpc - 1); a.max = (1 << bpc) - 1;
    a.identity = dst->matrix == 0; a.mono = mono;
    if (!a.identity) {
        const int m = dst->matrix == 1 ? 0 : dst->matrix == 9 ? 2 : 1;
        const int *const k = rgb_coef[m][!!dst->full_range][(bpc - 8) >> 1];
        a.cy = k[0]; a.crv = k[1]; a.cbu = k[2]; a.cgu = k[3]; a.cgv = k[4];
        a.yoff = dst->full_range ? 0 : 16 << (bpc - 8);
    }
}

// RGB: the kernel's arguments; *n_cells = the 64 x 8 chroma cells of the call (a wave each)
template <typename pixel, bool TILED, typename T>
RgbArgs make_rgb_args(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes, const int row0, const int row1,
                      unsigned *const n_cells)
{
    const SurfaceGeom g = surface_geom(src, row0, row1);
    const int load_align = 8 * (int) sizeof(pixel);
    RgbArgs a = RgbArgs();
    for (int pl = 0; pl < 3; pl++) { a.s[pl] = planes[pl]; a.d[pl] = dst->data[pl]; a.dstride[pl] = dst->stride[pl]; }
    a.sstride[0] = (int) (src->p[0].stride / (ptrdiff_t) sizeof(pixel));
    a.sstride[1] = g.mono ? 0 : (int) (src->p[1].stride / (ptrdiff_t) sizeof(pixel));
    a.swide[0] = TILED || aligned_to(planes[0], src->p[0].stride, load_align);
    a.swide[1] = TILED || g.mono || (aligned_to(planes[1], src->p[1].stride, load_align) && aligned_to(planes[2], src->p[2].stride, load_align));
    const int store_align = 8 * (int) sizeof(T) > 16 ? 16 : 8 * (int) sizeof(T);
    a.dwide = 1;
    for (int pl = 0; pl < 3; pl++) a.dwide &= aligned_to(dst->data[pl], dst->stride[pl], store_align);
    a.w = g.w; a.cw = g.cw; a.row1 = row1; a.crow0 = g.crow0; a.crow1 = g.crow1;
    a.n_cx = (g.cw + 63) / 64;
    rgb_set_matrix(a, dst, src->bpc, g.mono);
    const int n_cy = ((g.crow1 + 7) >> 3) - (g.crow0 >> 3);
    *n_cells = (unsigned) a.n_cx * (unsigned) n_cy;
    return a;
}

// planar / semi-planar: the parts; a wave takes `rows` cells under one another, the waves of a part are rounded up to a multiple of `group`
// (the waves of a workgroup then belong to one part); *n_waves = all of them
template <typename pixel, bool TILED, typename T>
CopyArgs make_copy_args(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes, const int row0, const int row1,
                        const int rows, const int group, unsigned *const n_waves)
{
    const SurfaceGeom g = surface_geom(src, row0, row1);
    const int load_align = 8 * (int) sizeof(pixel);
    CopyArgs a = CopyArgs();
    *n_waves = 0;
    const bool semi = dst->format == DAV1D_HIP_SURFACE_SEMIPLANAR;
    const int n_parts = g.mono ? 1 : semi ? 2 : 3;
    for (int k = 0; k < n_parts; k++) {
        SurfPart &p = a.part[k];
        p.interleave = semi && k == 1;
        p.s0 = planes[k]; p.s1 = p.interleave ? planes[2] : nullptr;
        p.d = dst->data[k]; p.dstride = dst->stride[k];
        p.sstride = (int) (src->p[k].stride / (ptrdiff_t) sizeof(pixel));
        p.w = k ? g.cw : g.w;
        p.y0 = k ? g.crow0 : row0; p.y1 = k ? g.crow1 : row1;
        p.n_cx = (p.w + 63) / 64;
        const int n_cy = ((p.y1 + 7) >> 3) - (p.y0 >> 3);
        p.n_waves = (p.n_cx * ((n_cy + rows - 1) / rows) + group - 1) / group * group;
        p.swide = TILED || (aligned_to(planes[k], src->p[k].stride, load_align) && (!p.interleave || aligned_to(planes[2], src->p[2].stride, load_align)));
        const int run = (p.interleave ? 16 : 8) * (int) sizeof(T);
        p.dwide = aligned_to(p.d, p.dstride, run > 16 ? 16 : run);
        *n_waves += (unsigned) p.n_waves;
    }
    for (int k = n_parts; k < 3; k++) { a.part[k] = a.part[0]; a.part[k].n_waves = 0; }
    return a;
}

// ---- the output samples of the tensor-ready RGB exports (surface_rgb.hip, surface_rgb_scale.hip)

// ---- output samples of channel ch (0, 1, 2 = R, G, B), and the opaque alpha of the sample type
template <typename Base> struct RgbInt {
    typedef typename Base::T T;
    Base b; T alpha;
    __device__ __forceinline__ T operator()(const int v, const int) const { return b(v); }
};
struct RgbF32 {
    typedef float T;
    float scale[3], bias[3]; T alpha;
    __device__ __forceinline__ T operator()(const int v, const int ch) const { return dv::mul_add_2r((float) v, scale[ch], bias[ch]); }
};
struct RgbF16 {
    typedef uint16_t T;
    float scale[3], bias[3]; T alpha;
    __device__ __forceinline__ T operator()(const int v, const int ch) const { return dv::f32_to_f16_bits(dv::mul_add_2r((float) v, scale[ch], bias[ch])); }
};

// N output samples to consecutive addresses, N * sizeof(T) any multiple of 8: vector stores of 16 bytes (8 where the run is no multiple of 16: 24 bytes
// of uint8 RGB) where the destination allows and the run is whole, else the first n one by one
template <typename T, int N>
__device__ __forceinline__ void store_packed(T *const dst, const T (&t)[N], const int n, const bool wide)
{
    constexpr int BYTES = N * (int) sizeof(T), CH = BYTES % 16 ? 8 : 16;
    static_assert(BYTES % CH == 0, "whole chunks");
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

// what the tensor-ready calls refuse beyond the export's own rules
inline int rgb_params_check(const Dav1dHipSurface *const dst, const Dav1dHipRgbParams &p)
{
    if (dst->format < DAV1D_HIP_SURFACE_RGB_PLANAR) return -EINVAL;
    if (p.chroma_pos < 0 || p.chroma_pos > 2) return -EINVAL;
    if (p.normalize && dst->sample != DAV1D_HIP_SAMPLE_F32 && dst->sample != DAV1D_HIP_SAMPLE_F16) return -EINVAL;
    return 0;
}

template <typename F> void set_float(F &o, const Dav1dHipRgbParams &p, const int bpc)
{
    for (int k = 0; k < 3; k++) {
        o.scale[k] = p.normalize ? p.scale[k] : (float) (1.0 / (double) ((1 << bpc) - 1));
        o.bias[k] = p.normalize ? p.bias[k] : 0.0f;          // (x + 0 is x: without normalisation this is OutF32's one multiply)
    }
}

// ---- the pixel work of the tensor-ready export (surface_rgb.hip has the account of the unit, the exchanges and the taps)

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

// One wave's share of a tensor-ready export: cell g (counted across, then down) of the call described by ax, all 64 lanes of the wave call.  `fn`
// turns the three clipped integers of a pixel into its three output samples (together: a colour matrix needs all of them) and has the opaque
// alpha.  The kernels of surface_rgb.hip (a cell a workgroup), surface_colour.hip and surface_colour_reduce.hip (a wave of a workgroup takes several cells in a loop: a
// lane without work returns from here, which is the `continue` of that loop) are this function.
template <typename pixel, bool TILED, int SSH, int SSV, typename Fn>
__device__ __forceinline__ void rgbx_cell(const RgbxArgs &ax, const int g, const Fn &fn)
{
    typedef typename Fn::T T;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const RgbArgs &a = ax.r;
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
                if (a.identity) { fn(tr[e], Y, tb[e], R[e], G[e], B[e]); continue; }
                const int l = dv::mul_i24(a.cy, Y - a.yoff);
                fn(dv::iclip((l + tr[e]) >> 14, 0, a.max), dv::iclip((l + tg[e]) >> 14, 0, a.max), dv::iclip((l + tb[e]) >> 14, 0, a.max), R[e], G[e], B[e]);
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
                for (int e = 0; e < 8; e++) { t[4 * e] = R[e]; t[4 * e + 1] = G[e]; t[4 * e + 2] = B[e]; t[4 * e + 3] = fn.alpha; }
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

// the arguments of rgbx_cell for luma rows [row0, row1) of a checked call; *n_cells = its 64 x 8 chroma cells
template <typename pixel, bool TILED, typename T>
RgbxArgs make_rgbx_args(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes, const Dav1dHipRgbParams &p,
                        const int row0, const int row1, unsigned *const n_cells)
{
    RgbxArgs ax = RgbxArgs();
    ax.r = make_rgb_args<pixel, TILED, T>(dst, src, planes, row0, row1, n_cells);
    const SurfaceGeom g = surface_geom(src, row0, row1);
    ax.ch = g.ch; ax.pos = p.chroma_pos;
    ax.hf = g.ss_hor && p.chroma_pos; ax.vf = g.ss_ver && p.chroma_pos;
    ax.packed = dst->format == DAV1D_HIP_SURFACE_RGB_PACKED ? 3 : dst->format == DAV1D_HIP_SURFACE_RGBA_PACKED ? 4 : 0;
    if (ax.packed) {          // one plane; a lane's run starts at a multiple of its size, so the chunk's alignment of base and stride decides
        const int run = 8 * ax.packed * (int) sizeof(T);
        ax.r.dwide = aligned_to(dst->data[0], dst->stride[0], run % 16 ? 8 : 16);
        ax.r.d[1] = ax.r.d[2] = nullptr;
    }
    return ax;
}

// ---- the area scaler S of DESIGN.md 10.2 (surface_scale.hip, surface_rgb_scale.hip): a workgroup of four waves scales a cell of a plane through LDS

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
    int up;                     // the resizing kernels only (surface_resize.hip): bit 0 / 1: the axis across / down goes up, through R of DESIGN.md 10.7
};

template <typename pixel> struct ScaleLds {
    alignas(16) pixel raw[SC_MAXR * SC_PITCH];
    uint32_t t[SC_OR * SC_PITCH];
    uint16_t wx[SC_TAPS][SC_OW], wy[SC_TAPS][SC_OR];
    uint16_t ix[SC_OW], iy[SC_OR];      // the first tap: column / row of the LDS window
    uint8_t nx[SC_OW], ny[SC_OR];       // taps
    union {                                 // the outputs: three planes of samples, or (surface_rgb_scale.hip) luma and a plane of chroma pairs u | v << 16
        alignas(16) uint16_t out[3][SC_OR * SC_OW];
        struct { uint16_t y[SC_OR * SC_OW]; uint32_t uv[SC_OR * SC_OW]; } pair;
    };
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

// A uniform value that the compiler shall not follow out of the loops around its use: what a division derives from its divisor is then made where
// the division stands, not once per kernel and carried in vector registers through the whole cell (the resizing kernels have twice the divisions
// of the scaling ones and would lose a wave per SIMD to that)
__device__ __forceinline__ int used_here(int v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(DAV1D_HIP_EMU)
    asm volatile("" : "+s"(v));
#endif
    return v;
}

// taps and weights of output `o` of an axis that goes up (s source samples to d > s), the resampler R of DESIGN.md 10.7: linear interpolation with
// half-sample centres in 12-bit weights, the two taps merged after the clamp to [0, s) — one or two taps of positive weight, 4096 in sum, on
// consecutive indices; *first = the first of them (never decreasing in o).  With q = (o s) / d and m = 2 (o s - q d) + s - d, which lies in (-d, 2 d):
// N = (2 o + 1) s - d = 2 d q + m, so i0 = floor(N / 2 d) is q - 1 with r = m + 2 d for a negative m, else q with r = m — one long division, as in S.
__device__ __forceinline__ int resize_weights(const int o, const int s, const int d_, int *const first, uint16_t *const w, const int wstride)
{
    const int d = used_here(d_);
    const uint64_t a = (uint64_t) o * (unsigned) s;
    const int q = (int) (a / (unsigned) d);
    const long long m = 2 * (long long) (a - (uint64_t) q * (unsigned) d) + s - d;
    const int i0 = m < 0 ? q - 1 : q;                           // -1 .. s - 1
    const uint64_t r = (uint64_t) (m < 0 ? m + 2LL * d : m);    // < 2 d
    // w1 = (r * 4096 + d) / (2 d) = ((r * 4096) / d + 1) >> 1: a division by d, like every other one of this axis
    const unsigned w1 = ((d < (1 << 18) ? (unsigned) r * 4096u / (unsigned) d : (unsigned) (r * 4096u / (unsigned) d)) + 1) >> 1;
    if (i0 < 0 || i0 >= s - 1 || w1 == 0 || w1 == 4096) {
        *first = i0 < 0 ? 0 : i0 >= s - 1 ? s - 1 : i0 + (w1 == 4096);
        w[0] = 4096;
        return 1;
    }
    *first = i0;
    w[0] = (uint16_t) (4096 - w1); w[wstride] = (uint16_t) w1;
    return 2;
}
// samples [*a0, *a1) of an axis of s samples that hold every tap of outputs [o0, o0 + n) of d, n > 0.  Through S: the hull of the taps.  `up`, through R:
// (o s) / d - 1 <= i0(o) <= (o s) / d, so from the sample before (o0 s) / d to the one behind ((o0 + n - 1) s) / d, clamped to the axis — at most n + 2
// samples, of which one at either end may go unused
__device__ __forceinline__ void scale_span(const bool up, const int o0, const int n, const int s, const int d_, int *const a0, int *const a1)
{
    const int d = used_here(d_);
    const uint64_t lo = (uint64_t) o0 * (unsigned) s, hi = up ? (uint64_t) (o0 + n - 1) * (unsigned) s : (uint64_t) (o0 + n) * (unsigned) s + (unsigned) d - 1;
    const int q0 = (int) (lo / (unsigned) d), q1 = (int) (hi / (unsigned) d);
    *a0 = up ? dv::imax(q0 - 1, 0) : q0;
    *a1 = up ? dv::imin(q1 + 2, s) : q1;
}

// Outputs [ox0, ox0 + nox) x [j0, j1) of plane p into out[(j - oyb) * SC_OW + (o - ox0)].  Every argument is uniform in the workgroup; all of
// its threads call.  nox <= SC_OW, oyb <= j0, j1 - oyb <= SC_OR.  HALF 0: `out` holds samples (uint16_t).  HALF 1 / 2: `out` holds pairs (uint32_t),
// the call sets the word to the sample / adds the sample as its upper half (U, then V of the same outputs: the same thread owns the word both times).
// RESIZE (surface_resize.hip): an axis whose bit of p.up is set takes its window and its weights from R instead of S; everything else is the same.
template <typename pixel, bool TILED, int HALF = 0, typename O = uint16_t, bool RESIZE = false>
__device__ __forceinline__ void scale_cell(ScaleLds<pixel> &L, const ScalePlane &p, const int ox0, const int nox, const int oyb, const int j0, const int j1,
                                           O *const out)
{
    typedef Piece<8 * sizeof(pixel)> piece_t;
    if (j1 <= j0 || nox <= 0) return;
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int ax0, ax1, ay0, ay1;
    const bool upx = RESIZE && (p.up & 1), upy = RESIZE && (p.up & 2);
    if (RESIZE) {
        scale_span(upx, ox0, nox, p.sw, p.dw, &ax0, &ax1);
        scale_span(upy, j0, j1 - j0, p.sh, p.dh, &ay0, &ay1);
        // (uniform, but out of the vector unit's long division: said here, the bounds and all that follows from them stay in scalar registers)
        ax0 = __builtin_amdgcn_readfirstlane(ax0 + p.x0); ax1 = __builtin_amdgcn_readfirstlane(ax1 + p.x0);
        ay0 = __builtin_amdgcn_readfirstlane(ay0 + p.y0); ay1 = __builtin_amdgcn_readfirstlane(ay1 + p.y0);
    } else {
        ax0 = p.x0 + (int) ((uint64_t) ox0 * (unsigned) p.sw / (unsigned) p.dw);
        ax1 = p.x0 + (int) (((uint64_t) (ox0 + nox) * (unsigned) p.sw + (unsigned) p.dw - 1) / (unsigned) p.dw);
        ay0 = p.y0 + (int) ((uint64_t) j0 * (unsigned) p.sh / (unsigned) p.dh);
        ay1 = p.y0 + (int) (((uint64_t) j1 * (unsigned) p.sh + (unsigned) p.dh - 1) / (unsigned) p.dh);
    }
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
        L.nx[tid] = (uint8_t) (upx ? resize_weights(ox0 + tid, p.sw, p.dw, &i0, &L.wx[0][tid], SC_OW) : scale_weights(ox0 + tid, p.sw, p.dw, &i0, &L.wx[0][tid], SC_OW));
        L.ix[tid] = (uint16_t) (p.x0 + i0 - ux0);
    } else if (tid >= SC_OW && tid < SC_OW + (j1 - j0)) {
        const int jr = j0 - oyb + tid - SC_OW;
        int i0;
        L.ny[jr] = (uint8_t) (upy ? resize_weights(oyb + jr, p.sh, p.dh, &i0, &L.wy[0][jr], SC_OR) : scale_weights(oyb + jr, p.sh, p.dh, &i0, &L.wy[0][jr], SC_OR));
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
        O &dst = out[(j + j0 - oyb) * SC_OW + o];
        if (HALF == 2) dst |= (O) (sum >> 20) << 16;
        else dst = (O) (sum >> 20);
    }
    __syncthreads();
}

struct ScaleGeom {
    int x0, y0, w, h;       // the crop
    int dw, dh;
    int mono, ss_hor, ss_ver;
};

// the crop and the ratio: what dav1d_hip_surface_export_scaled refuses beyond what the plain export does
// (`up_ok`: the resizing calls of surface_resize.hip, which serve dst->w > w and dst->h > h; `max_ratio`: the reducing calls of surface_reduce.h go past 8:1)
inline int scale_geom_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, ScaleGeom *const g,
                            const bool up_ok = false, const int max_ratio = 8)
{
    const int W = src->p[0].w, H = src->p[0].h;
    g->mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    g->ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420; g->ss_hor = !g->mono && src->layout != DAV1D_HIP_LAYOUT_I444;
    g->x0 = crop ? crop->x0 : 0; g->y0 = crop ? crop->y0 : 0; g->w = crop ? crop->w : W; g->h = crop ? crop->h : H;
    g->dw = dst->w; g->dh = dst->h;
    if (g->w <= 0 || g->h <= 0 || g->x0 < 0 || g->y0 < 0 || g->x0 > W - g->w || g->y0 > H - g->h) return -EINVAL;
    if ((g->ss_hor && (g->x0 & 1)) || (g->ss_ver && (g->y0 & 1))) return -EINVAL;
    if ((!up_ok && (g->dw > g->w || g->dh > g->h)) || g->w > (long long) max_ratio * g->dw || g->h > (long long) max_ratio * g->dh) return -ENOTSUP;
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
    p.up = (p.dw > p.sw) | (p.dh > p.sh) << 1;          // (never set where scale_geom_check ran without up_ok)
    return p;
}

// rows [0, n) of a plane's window of s rows that rows [0, r) of its d outputs read: through S the rows they cover; on an axis that goes up, through R,
// [0, min(s, i0(r - 1) + 2))
inline int resize_rows_of(const int r, const int s, const int d)
{
    if (r <= 0) return 0;
    if (d <= s) return (int) (((long long) r * s + d - 1) / d);
    const long long D = 2LL * d, N = (2LL * (r - 1) + 1) * s - d;
    const long long rows = (N + D) / D + 1;          // i0 + 2
    return (int) (rows > s ? s : rows);
}
// source luma rows from the top of the picture that destination rows [0, r1) of geometry g read, r1 > 0
inline int resize_rows_needed(const ScaleGeom &g, const int src_h, const int r1)
{
    long long need = g.y0 + resize_rows_of(r1, g.h, g.dh);
    if (!g.mono) {
        const int sh = (g.h + g.ss_ver) >> g.ss_ver, dch = (g.dh + g.ss_ver) >> g.ss_ver, cr1 = r1 >= g.dh ? dch : r1 >> g.ss_ver;
        const long long cneed = ((long long) (g.y0 >> g.ss_ver) + resize_rows_of(cr1, sh, dch)) << g.ss_ver;
        if (cneed > need) need = cneed;
    }
    return (int) (need > src_h ? src_h : need);
}
// What the *_rows_needed call of a sized family answers once its check (`rc`) has filled `call` and `g`: the source rows that destination rows
// [0, call.row1) read — with `ring` (the tensor-ready families at chroma_pos != 0) those of the chroma row below the band's last, which is made as well
inline int sized_rows_needed(const int rc, const SurfaceCall &call, const ScaleGeom &g, const bool ring, const Dav1dHipPicture *const src)
{
    if (rc) return rc;
    if (call.row1 <= 0) return 0;
    const int r = ring && g.ss_ver ? call.row1 + 2 : call.row1;
    return resize_rows_needed(g, src->p[0].h, r > g.dh ? g.dh : r);
}

// ---- tensor-ready RGB behind the scaler (surface_rgb_scale.hip has the account of the cell and its ring)

struct ScaleRgbxArgs {
    ScalePlane pl[3];
    RgbArgs c;              // d, dstride, dwide and the colour part
    int ssh, ssv;
    int row0, row1;         // destination luma rows
    int crow0, crow1;       // ... and chroma rows
    int n_cx;
    int cw, ch;             // the owned cell of the chroma planes (of the luma plane at 4:0:0)
    int hx, hyu, hyd;       // the ring: a column on the right, a row above, a row below (1 where the taps reach it)
    int pos;                // chroma_pos
    int packed;             // samples a pixel in data[0] (3, 4), 0: planes
};

// the 8 samples of a unit from their luma and the vertical tap sums P (pairs u | v << 16, sum 4) of the chroma columns under them: 8 columns at SSH 0,
// 4 and the neighbour to the right at SSH 1; `hf`: that neighbour takes part
template <int SSH, typename Out>
__device__ __forceinline__ void rgbx_unit(const RgbArgs &a, const Out &out, const uint16_t *const sy, const uint32_t (&P)[8], const bool hf,
                                          typename Out::T (&R)[8], typename Out::T (&G)[8], typename Out::T (&B)[8])
{
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int k = SSH ? e >> 1 : e;
        uint32_t s = 2 * P[k];
        if (SSH && (e & 1) && hf) s = P[k] + P[k + 1];
        s = ((s + 0x00040004u) >> 3) & 0x1fff1fffu;
        const int cb = (int) (s & 0xffff) - a.mid, cr = (int) (s >> 16) - a.mid;
        const int Y = sy[e];
        if (a.identity) { R[e] = out(cr + a.mid, 0); G[e] = out(Y, 1); B[e] = out(cb + a.mid, 2); continue; }
        const int l = dv::mul_i24(a.cy, Y - a.yoff);
        R[e] = out(dv::iclip((l + dv::mad_i24(a.crv, cr, 8192)) >> 14, 0, a.max), 0);
        G[e] = out(dv::iclip((l + dv::mad_i24(-a.cgv, cr, dv::mad_i24(-a.cgu, cb, 8192))) >> 14, 0, a.max), 1);
        B[e] = out(dv::iclip((l + dv::mad_i24(a.cbu, cb, 8192)) >> 14, 0, a.max), 2);
    }
}

// One workgroup's share of a scaled tensor-ready export: cell g (counted across, then down) of the call described by a.  Everything in a is uniform in the
// workgroup; all of its 256 threads call.  The kernels of surface_rgb_scale.hip (a: the kernel's own argument) and surface_batch.hip (a: the item's
// record in the batch's table) are this function behind a __shared__ ScaleLds.
template <typename pixel, bool TILED, typename Out, bool RESIZE = false>
__device__ __forceinline__ void scale_rgbx_cell(ScaleLds<pixel> &L, const ScaleRgbxArgs &a, const int g, const Out &out)
{
    typedef typename Out::T T;
    const ScalePlane &pc = a.pl[a.c.mono ? 0 : 1], &py = a.pl[0];
    const int cy = g / a.n_cx, cx = g - cy * a.n_cx;
    const int cx0 = cx * a.cw, cyb = (a.crow0 / a.ch + cy) * a.ch;
    const int ncx = dv::imin(a.cw, pc.dw - cx0), cj0 = dv::imax(cyb, a.crow0), cj1 = dv::imin(cyb + a.ch, a.crow1);
    // the cell and its ring, inside Q's chroma plane: at most pc.ow x pc.oh outputs
    const int hx0 = cx0, hx1 = dv::imin(cx0 + ncx + a.hx, pc.dw);
    const int hj0 = dv::imax(cj0 - a.hyu, 0), hj1 = dv::imin(cj1 + a.hyd, pc.dh);
    uint32_t *const pairs = L.pair.uv;
    if (!a.c.mono) {
        scale_cell<pixel, TILED, 1, uint32_t, RESIZE>(L, a.pl[1], hx0, hx1 - hx0, hj0, hj0, hj1, pairs);
        scale_cell<pixel, TILED, 2, uint32_t, RESIZE>(L, a.pl[2], hx0, hx1 - hx0, hj0, hj0, hj1, pairs);
    }
    const bool hf = a.hx != 0, vf = a.hyd != 0;
    const uint32_t grey = (uint32_t) a.c.mid * 0x10001u;
    // the luma of the cell
    const int lx0 = cx0 << a.ssh, lx1 = dv::imin((cx0 + ncx) << a.ssh, py.dw);
    const int ly0 = dv::imax(cj0 << a.ssv, a.row0), ly1 = dv::imin(cj1 << a.ssv, a.row1);
    for (int lyb = cyb << a.ssv; lyb < ly1; lyb += py.oh) {
        const int j0 = dv::imax(lyb, ly0), j1 = dv::imin(lyb + py.oh, ly1);
        if (j1 <= j0) continue;
        for (int lx = lx0; lx < lx1; lx += py.ow) {
            const int nox = dv::imin(py.ow, lx1 - lx);
            scale_cell<pixel, TILED, 0, uint16_t, RESIZE>(L, py, lx, nox, lyb, j0, j1, L.pair.y);
            const int nun = (nox + 7) >> 3;
            for (int it = (int) threadIdx.x; it < (j1 - j0) * nun; it += 256) {
                const int j = it / nun, u = it - j * nun, y = j0 + j, x = lx + u * 8, n = nox - u * 8;
                const uint16_t *const sy = &L.pair.y[(y - lyb) * SC_OW + u * 8];
                // the vertical taps: the lane's own chroma row and, at a filtered axis, the one above (chroma_pos 1, even luma row) or below it
                const int kr = y >> a.ssv, odd = y & 1;
                int w_own = 4, w_2nd = 0, r2 = kr;
                if (vf) {
                    if (a.pos == 1) { w_own = 3; w_2nd = 1; r2 = odd ? kr + 1 : kr - 1; }
                    else if (odd) { w_own = 2; w_2nd = 2; r2 = kr + 1; }
                    r2 = dv::imin(dv::imax(r2, 0), pc.dh - 1);
                }
                const int o_own = (kr - hj0) * SC_OW - hx0, o_2nd = (r2 - hj0) * SC_OW - hx0, kc = x >> a.ssh;
                uint32_t P[8];
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    if (a.c.mono) { P[m] = 4 * grey; continue; }
                    if (a.ssh && m > (hf ? 4 : 3)) { P[m] = 0; continue; }          // (the neighbour to the right is in LDS only where there is a ring)
                    const int col = dv::imin(kc + m, pc.dw - 1);          // right of the plane: its last column
                    P[m] = (uint32_t) w_own * pairs[o_own + col];
                    if (vf) P[m] += (uint32_t) w_2nd * pairs[o_2nd + col];
                }
                T R[8], G[8], B[8];
                if (a.ssh) rgbx_unit<1, Out>(a.c, out, sy, P, hf, R, G, B);
                else rgbx_unit<0, Out>(a.c, out, sy, P, false, R, G, B);
                if (a.packed == 3) {
                    T t[24];
#pragma unroll
                    for (int e = 0; e < 8; e++) { t[3 * e] = R[e]; t[3 * e + 1] = G[e]; t[3 * e + 2] = B[e]; }
                    store_packed<T, 24>((T *) ((uint8_t *) a.c.d[0] + (size_t) y * a.c.dstride[0]) + (size_t) x * 3, t, 3 * n, a.c.dwide);
                } else if (a.packed == 4) {
                    T t[32];
#pragma unroll
                    for (int e = 0; e < 8; e++) { t[4 * e] = R[e]; t[4 * e + 1] = G[e]; t[4 * e + 2] = B[e]; t[4 * e + 3] = out.alpha; }
                    store_packed<T, 32>((T *) ((uint8_t *) a.c.d[0] + (size_t) y * a.c.dstride[0]) + (size_t) x * 4, t, 4 * n, a.c.dwide);
                } else {
                    const size_t off = (size_t) x * sizeof(T);
                    store_run<T, 8>((T *) ((uint8_t *) a.c.d[0] + (size_t) y * a.c.dstride[0] + off), R, n, a.c.dwide);
                    store_run<T, 8>((T *) ((uint8_t *) a.c.d[1] + (size_t) y * a.c.dstride[1] + off), G, n, a.c.dwide);
                    store_run<T, 8>((T *) ((uint8_t *) a.c.d[2] + (size_t) y * a.c.dstride[2] + off), B, n, a.c.dwide);
                }
            }
        }
    }
}

// ---- the host side of the scaled tensor-ready export (surface_rgb_scale.hip: one call; surface_batch.hip: many in one launch)

// the union of what dav1d_hip_surface_export_rgb and dav1d_hip_surface_export_scaled refuse
inline int rgbx_scaled_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop,
                                  const Dav1dHipRgbParams &p, const int row0, const int row1, SurfaceCall *const call, ScaleGeom *const g,
                                  const bool up_ok = false, const int max_ratio = 8)
{
    if (const int rc = surface_args_check(dst, src, row0, row1, call, true, true)) return rc;
    if (const int rc = rgb_params_check(dst, p)) return rc;
    return scale_geom_check(dst, src, crop, g, up_ok, max_ratio);
}

// the kernel's arguments for destination luma rows [row0, row1) of a checked call; *n_groups = its workgroups (a cell of Q's chroma planes each)
template <typename pixel, bool TILED, typename T>
ScaleRgbxArgs make_scale_rgbx_args(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes, const ScaleGeom &g,
                                   const Dav1dHipRgbParams &p, const int row0, const int row1, unsigned *const n_groups)
{
    const int dch = (g.dh + g.ss_ver) >> g.ss_ver;
    const int crow0 = row0 >> g.ss_ver, crow1 = row1 >= g.dh ? dch : row1 >> g.ss_ver;
    ScaleRgbxArgs a = ScaleRgbxArgs();
    for (int pl = 0; pl < (g.mono ? 1 : 3); pl++) a.pl[pl] = make_scale_plane<pixel, TILED>(src, planes, g, pl);
    a.packed = dst->format == DAV1D_HIP_SURFACE_RGB_PACKED ? 3 : dst->format == DAV1D_HIP_SURFACE_RGBA_PACKED ? 4 : 0;
    // a lane's run starts at a multiple of its size, so the alignment of base and stride to a chunk decides
    const int run = 8 * (a.packed ? a.packed : 1) * (int) sizeof(T), store_align = run % 16 ? 8 : 16;
    a.c.dwide = 1;
    for (int pl = 0; pl < (a.packed ? 1 : 3); pl++) {
        a.c.d[pl] = dst->data[pl]; a.c.dstride[pl] = dst->stride[pl];
        a.c.dwide &= aligned_to(dst->data[pl], dst->stride[pl], store_align);
    }
    rgb_set_matrix(a.c, dst, src->bpc, g.mono);
    a.ssh = g.ss_hor; a.ssv = g.ss_ver; a.row0 = row0; a.row1 = row1;
    a.crow0 = g.mono ? row0 : crow0; a.crow1 = g.mono ? row1 : crow1;
    a.pos = p.chroma_pos;
    a.hx = g.ss_hor && p.chroma_pos; a.hyd = g.ss_ver && p.chroma_pos; a.hyu = g.ss_ver && p.chroma_pos == 1;
    const ScalePlane &pc = a.pl[g.mono ? 0 : 1];
    a.cw = pc.ow - 4 * a.hx; a.ch = pc.oh - a.hyu - a.hyd;
    a.n_cx = (pc.dw + a.cw - 1) / a.cw;
    const int n_cy = (a.crow1 + a.ch - 1) / a.ch - a.crow0 / a.ch;
    *n_groups = (unsigned) a.n_cx * (unsigned) n_cy;
    return a;
}

// the output functor of a sample type for pictures of `bpc` bits
inline void set_out(RgbF32 &o, const Dav1dHipRgbParams &p, const int bpc) { set_float(o, p, bpc); o.alpha = 1.0f; }
inline void set_out(RgbF16 &o, const Dav1dHipRgbParams &p, const int bpc) { set_float(o, p, bpc); o.alpha = 0x3c00; }
inline void set_out(RgbInt<OutMsb16> &o, const Dav1dHipRgbParams &, const int bpc) { o.b.shift = 16 - bpc; o.alpha = (uint16_t) (((1 << bpc) - 1) << o.b.shift); }
template <typename pixel> void set_out(RgbInt<OutNative<pixel>> &o, const Dav1dHipRgbParams &, const int bpc) { o.alpha = (pixel) ((1 << bpc) - 1); }

} // namespace
