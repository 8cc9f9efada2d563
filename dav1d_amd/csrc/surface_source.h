// The source-resolution loader of surface_linear.hip, shared with surface_stats.hip (10.13): the chroma under a luma unit of a crop
// window W at W's own size — the taps of chroma_pos down and across with cl() against W's chroma planes — as the tap sums rgbx_unit of
// surface_common.h takes.  Nothing here stores: what a kernel does with the integers of a unit is its own.
// `Item` is the record of the kernel that calls: cs[2], cstride, cswide, cpw (U and V, pixels per chroma row, one vector load per unit, visible
// samples per chroma row), cx0, cy0, ccw, cch (W's chroma planes), pos, hf, vf (chroma_pos; taps across / down other than replication) and c (RgbArgs:
// mono, mid).
#pragma once
#include "surface_common.h"

namespace {

struct RgbRaw { typedef int T; __device__ __forceinline__ int operator()(const int v, const int) const { return v; } };          // the integers of 10.3 themselves

// what a lane holds of the chroma under its luma unit between the loads and their use
template <typename pixel> struct LinChroma {
    Piece<8 * sizeof(pixel)> u0, v0, u1, v1;          // the unit of the lane's own chroma row, and of the second row of its taps down
    uint32_t h0, h1;                                  // the column behind the unit, u | v << 16, likewise
    int w_own, w_2nd;                                 // the taps down (sum 4)
};

// the loads of the luma unit at (x, y) of the picture, x a multiple of 8, y a row of W: every address lies inside W's chroma planes but for the
// columns of the unit itself that the alignment puts in front of or behind W (inside the plane; their luma has no weight)
template <typename pixel, bool TILED, int SSH, int SSV, typename Item>
__device__ __forceinline__ void lin_chroma_load(const Item &it, const int x, const int y, LinChroma<pixel> &k)
{
    const int kx = x >> SSH, ky = y >> SSV, cxu = SSH ? kx & ~7 : kx;
    int r2 = ky;
    k.w_own = 4; k.w_2nd = 0;
    if (SSV && it.vf) {
        const int odd = y & 1;          // (W starts at an even row)
        if (it.pos == 1) { k.w_own = 3; k.w_2nd = 1; r2 = odd ? ky + 1 : ky - 1; }
        else if (odd) { k.w_own = 2; k.w_2nd = 2; r2 = ky + 1; }
        r2 = dv::imin(dv::imax(r2, it.cy0), it.cy0 + it.cch - 1);
    }
    const int n = it.cpw - cxu;
    k.u0 = load8<pixel, TILED>(it.cs[0], it.cstride, cxu, ky, n, it.cswide);
    k.v0 = load8<pixel, TILED>(it.cs[1], it.cstride, cxu, ky, n, it.cswide);
    k.u1 = k.u0; k.v1 = k.v0;
    if (SSV && r2 != ky) {
        k.u1 = load8<pixel, TILED>(it.cs[0], it.cstride, cxu, r2, n, it.cswide);
        k.v1 = load8<pixel, TILED>(it.cs[1], it.cstride, cxu, r2, n, it.cswide);
    }
    k.h0 = k.h1 = 0;
    // the second half of a chroma unit: the column behind it is the next unit's first — inside W, or the clamp below replaces it
    if (SSH && it.hf && (x & 8) && kx + 4 < it.cx0 + it.ccw) {
        k.h0 = load1<pixel, TILED>(it.cs[0], it.cstride, kx + 4, ky) | load1<pixel, TILED>(it.cs[1], it.cstride, kx + 4, ky) << 16;
        k.h1 = k.h0;
        if (SSV && r2 != ky) k.h1 = load1<pixel, TILED>(it.cs[0], it.cstride, kx + 4, r2) | load1<pixel, TILED>(it.cs[1], it.cstride, kx + 4, r2) << 16;
    }
}

// the four samples of a half of a unit, chosen by value: a conditional between elements of the piece makes the compiler index it, in scratch memory
template <typename pixel>
__device__ __forceinline__ void half_of(const Piece<8 * sizeof(pixel)> &v, const bool second, uint32_t (&s)[4])
{
    const uint32_t m = second ? ~0u : 0u;
    if constexpr (sizeof(pixel) == 2) {
        const uint32_t d0 = v.a[0] ^ ((v.a[0] ^ v.a[2]) & m), d1 = v.a[1] ^ ((v.a[1] ^ v.a[3]) & m);
        s[0] = d0 & 0xffff; s[1] = d0 >> 16; s[2] = d1 & 0xffff; s[3] = d1 >> 16;
    } else {
        const uint32_t d = v.a[0] ^ ((v.a[0] ^ v.a[1]) & m);
        s[0] = d & 0xff; s[1] = (d >> 8) & 0xff; s[2] = (d >> 16) & 0xff; s[3] = d >> 24;
    }
}

// P[m]: the taps down (sum 4) on the chroma columns under the unit, U and V in the halves of a word — eight columns at SSH 0; four and the one
// behind them at SSH 1, cl()-clamped to W's last column
template <typename pixel, int SSH, typename Item>
__device__ __forceinline__ void lin_chroma_taps(const Item &it, const int x, const LinChroma<pixel> &k, uint32_t (&P)[8])
{
    if (it.c.mono) {
#pragma unroll
        for (int m = 0; m < 8; m++) P[m] = 4u * ((uint32_t) it.c.mid * 0x10001u);
        return;
    }
    const uint32_t wo = (uint32_t) k.w_own, w2 = (uint32_t) k.w_2nd;
    if (!SSH) {
#pragma unroll
        for (int m = 0; m < 8; m++) P[m] = wo * pair_of<pixel>(k.u0, k.v0, m) + w2 * pair_of<pixel>(k.u1, k.v1, m);
        return;
    }
    const bool second = x & 8;
    const int last = it.cx0 + it.ccw - 1 - (x >> 1);          // W's last chroma column, counted from the unit's first
    uint32_t uo[4], vo[4], us[4], vs[4];
    half_of<pixel>(k.u0, second, uo); half_of<pixel>(k.v0, second, vo);
    half_of<pixel>(k.u1, second, us); half_of<pixel>(k.v1, second, vs);
#pragma unroll
    for (int m = 0; m < 4; m++) P[m] = wo * (uo[m] | vo[m] << 16) + w2 * (us[m] | vs[m] << 16);
    P[4] = second ? wo * k.h0 + w2 * k.h1 : wo * pair_of<pixel>(k.u0, k.v0, 4) + w2 * pair_of<pixel>(k.u1, k.v1, 4);
#pragma unroll
    for (int m = 1; m < 5; m++) P[m] = m <= last ? P[m] : P[m - 1];          // (rgbx_unit<1> reads P[0 .. 4])
}

} // namespace
