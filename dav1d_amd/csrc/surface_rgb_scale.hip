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
#include "surface_common.h"

namespace {

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

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_scale_rgbx_kernel(const ScaleRgbxArgs a, const Out out)
{
    typedef typename Out::T T;
    __shared__ ScaleLds<pixel> L;
    const ScalePlane &pc = a.pl[a.c.mono ? 0 : 1], &py = a.pl[0];
    const int g = (int) blockIdx.x, cy = g / a.n_cx, cx = g - cy * a.n_cx;
    const int cx0 = cx * a.cw, cyb = (a.crow0 / a.ch + cy) * a.ch;
    const int ncx = dv::imin(a.cw, pc.dw - cx0), cj0 = dv::imax(cyb, a.crow0), cj1 = dv::imin(cyb + a.ch, a.crow1);
    // the cell and its ring, inside Q's chroma plane: at most pc.ow x pc.oh outputs
    const int hx0 = cx0, hx1 = dv::imin(cx0 + ncx + a.hx, pc.dw);
    const int hj0 = dv::imax(cj0 - a.hyu, 0), hj1 = dv::imin(cj1 + a.hyd, pc.dh);
    uint32_t *const pairs = L.pair.uv;
    if (!a.c.mono) {
        scale_cell<pixel, TILED, 1, uint32_t>(L, a.pl[1], hx0, hx1 - hx0, hj0, hj0, hj1, pairs);
        scale_cell<pixel, TILED, 2, uint32_t>(L, a.pl[2], hx0, hx1 - hx0, hj0, hj0, hj1, pairs);
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
            scale_cell<pixel, TILED>(L, py, lx, nox, lyb, j0, j1, L.pair.y);
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

// ---- the host side

template <typename pixel, bool TILED, typename Out>
int launch_rgbx_scaled(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                       const ScaleGeom &g, const Dav1dHipRgbParams &p, const int row0, const int row1, const Out &out)
{
    typedef typename Out::T T;
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
    hipLaunchKernelGGL((surface_scale_rgbx_kernel<pixel, TILED, Out>), dim3((unsigned) a.n_cx * (unsigned) n_cy), dim3(256), 0, c->stream, a, out);
    return hip_rc(hipGetLastError());
}

template <typename pixel, bool TILED>
int launch_rgbx_scaled_sample(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                              const ScaleGeom &g, const Dav1dHipRgbParams &p, const int row0, const int row1)
{
    const int max = (1 << src->bpc) - 1;
    if (dst->sample == DAV1D_HIP_SAMPLE_F32) {
        RgbF32 o; set_float(o, p, src->bpc); o.alpha = 1.0f;
        return launch_rgbx_scaled<pixel, TILED, RgbF32>(c, dst, src, planes, g, p, row0, row1, o);
    }
    if (dst->sample == DAV1D_HIP_SAMPLE_F16) {
        RgbF16 o; set_float(o, p, src->bpc); o.alpha = 0x3c00;
        return launch_rgbx_scaled<pixel, TILED, RgbF16>(c, dst, src, planes, g, p, row0, row1, o);
    }
    if constexpr (sizeof(pixel) == 2) {
        if (dst->sample == DAV1D_HIP_SAMPLE_MSB16) {
            RgbInt<OutMsb16> o; o.b.shift = 16 - src->bpc; o.alpha = (uint16_t) (max << o.b.shift);
            return launch_rgbx_scaled<pixel, TILED, RgbInt<OutMsb16>>(c, dst, src, planes, g, p, row0, row1, o);
        }
    }
    RgbInt<OutNative<pixel>> o; o.alpha = (pixel) max;
    return launch_rgbx_scaled<pixel, TILED, RgbInt<OutNative<pixel>>>(c, dst, src, planes, g, p, row0, row1, o);
}

// the union of what dav1d_hip_surface_export_rgb and dav1d_hip_surface_export_scaled refuse
int rgbx_scaled_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop,
                           const Dav1dHipRgbParams &p, const int row0, const int row1, SurfaceCall *const call, ScaleGeom *const g)
{
    if (const int rc = surface_args_check(dst, src, row0, row1, call, true, true)) return rc;
    if (const int rc = rgb_params_check(dst, p)) return rc;
    return scale_geom_check(dst, src, crop, g);
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_scaled(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                   const Dav1dHipRgbParams *params, int drow0, int drow1)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    SurfaceCall call;
    ScaleGeom g;
    if (!c) return -EINVAL;
    if (const int rc = rgbx_scaled_args_check(dst, src, crop, p, drow0, drow1, &call, &g)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    const int row0 = call.row0, row1 = call.row1;
    if (row1 <= row0) return 0;
    void *const *const planes = call.planes;
    (void) hipEventRecord(c->ev_t0, c->stream);
    int rc;
    if (src->bpc == 8) rc = call.tiled ? launch_rgbx_scaled_sample<uint8_t, true>(c, dst, src, planes, g, p, row0, row1) : launch_rgbx_scaled_sample<uint8_t, false>(c, dst, src, planes, g, p, row0, row1);
    else rc = call.tiled ? launch_rgbx_scaled_sample<uint16_t, true>(c, dst, src, planes, g, p, row0, row1) : launch_rgbx_scaled_sample<uint16_t, false>(c, dst, src, planes, g, p, row0, row1);
    (void) hipEventRecord(c->ev_t1, c->stream);
    c->last_ms_pending = !rc;
    return rc;
}

extern "C" int dav1d_hip_surface_rgb_scaled_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                        const Dav1dHipRgbParams *params, int drow1)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    SurfaceCall call;
    ScaleGeom g;
    if (const int rc = rgbx_scaled_args_check(dst, src, crop, p, 0, drow1, &call, &g)) return rc;
    if (call.row1 <= 0) return 0;
    // the ring: the chroma row below the band's last is scaled as well
    const int r = g.ss_ver && p.chroma_pos ? call.row1 + 2 : call.row1;
    return scale_rows_needed(g, src->p[0].h, r > g.dh ? g.dh : r);
}
