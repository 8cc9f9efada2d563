// Linear-light scaling for the colour-managed tensor export: dav1d_hip_surface_export_rgb_linear_reduced, its batch and
// dav1d_hip_surface_rgb_linear_rows_needed (include/dav1d_hip.h).  The crop window W is converted to integer R, G, B at its own size
// (10.3: sited chroma with cl() against W's chroma size, the integer matrix), every code is replaced by its light in fixed point (q of the handle,
// below 2^31), and the light is averaged with the 12-bit weights of R' (10.8) on both axes in one exact 64-bit sum per channel; only then come the
// matrix, enc, the normalisation and the store of 10.6.  No sum depends on its order, so kernel, emulated build and numpy agree byte for byte.
//
// One pass, no scratch picture.  The shape is reduce_cell's (surface_reduce.h): a workgroup of four waves owns ow outputs across and oh rows down;
// per output row a wave walks strips of 64 luma columns, 8 rows x 8 units of 8 samples from a row that is a multiple of 8.  Per unit a lane loads
// its luma, the chroma unit under it for the one or two chroma rows of its vertical taps and, for the odd luma columns of the unit's last pair, the
// next chroma column (one more load, clamped at the window's edge), runs rgbx_unit of surface_common.h on them — 10.3's up() and matrix, unchanged —
// reads q three times a pixel from LDS and adds wy * q to eight 64-bit sums per channel (a column's sum stays below 2^43).  The eight row lanes are
// folded with seven exchanges on two dwords each, the column sums go to LDS, and across a group of 2^k lanes per output adds wx * sum (below 2^55).
// The lane that ends up with A_R, A_G and A_B converts them (uint64 to binary32, ties to even, times 2^(e - 55)) and applies ColourFn::light and
// the store on the spot.  enc is read three times per OUTPUT sample: from global memory, through the caches.
// LDS: q (1 / 4 / 16 KiB, filled once per workgroup with 16-byte loads, one barrier behind the fill and before any lane can leave) in front of
// LinLds: three 64-bit column sums at LN_NCOL = 1024 (24 KiB; half of RD_NCOL, which is the trade) and the weight tables — 35.2 / 38.2 / 50.2 KiB.
#include "surface_reduce.h"
#include "surface_colour.h"
#include "surface_source.h"
#include <math.h>

namespace {

constexpr int LN_NCOL = 1024;       // source columns of a cell (from a multiple of 8)
constexpr int LN_OW = 256;          // outputs across a cell
constexpr int LN_TAPS = 264;        // taps down: 257 at 256:1
constexpr int LN_Q_MAX = 4 << 12;   // bytes of q at 12 bits

struct alignas(16) LinLds {
    uint64_t t[3][LN_NCOL];         // sum wy q of a column, per channel
    uint16_t w0[LN_NCOL], w1[LN_NCOL];
    int16_t oc[LN_NCOL];            // the first output a column feeds, from the cell's first
    uint16_t wy[LN_TAPS];
    uint16_t ix[LN_OW], nx[LN_OW];  // the first tap (column of the LDS row) and the taps of an output
    uint16_t wu[2][LN_OW];          // across, going up: R's weights
};

struct LinItem {
    ScalePlane p;                   // the luma plane and the crop window; ow x oh: the cell
    const void *cs[2];              // U, V
    int cstride, cswide, cpw;       // pixels per chroma row; one vector load per unit; visible samples per chroma row
    int cx0, cy0, ccw, cch;         // W's chroma planes: cl() clamps against these
    RgbArgs c;                      // d, dstride, dwide and the colour part
    int pos, hf, vf;                // chroma_pos; taps across / down other than replication
    int packed;                     // samples a pixel in data[0] (3, 4), 0: planes
    int row0, row1;                 // destination rows
    int n_cx;
};

__device__ __forceinline__ uint64_t shfl_xor_u64(const uint64_t v, const int m)
{
    const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) v, m), hi = (uint32_t) __shfl_xor((int) (uint32_t) (v >> 32), m);
    return (uint64_t) hi << 32 | lo;
}
// the eight row lanes of a column: seven exchanges, each halving what a lane still carries; lane r is left with column r of its unit
__device__ __forceinline__ uint64_t fold_rows(const uint64_t (&acc)[8], const int r)
{
    uint64_t a4[4], a2[2];
#pragma unroll
    for (int e = 0; e < 4; e++) a4[e] = (r & 4 ? acc[e + 4] : acc[e]) + shfl_xor_u64(r & 4 ? acc[e] : acc[e + 4], 32);
#pragma unroll
    for (int e = 0; e < 2; e++) a2[e] = (r & 2 ? a4[e + 2] : a4[e]) + shfl_xor_u64(r & 2 ? a4[e] : a4[e + 2], 16);
    return (r & 1 ? a2[1] : a2[0]) + shfl_xor_u64(r & 1 ? a2[0] : a2[1], 8);
}

// one output sample from its three sums: the light, steps 2 to 4 of 10.6, the store
template <typename Fn>
__device__ __forceinline__ void lin_emit(const LinItem &it, const Fn &fn, const int e, const int x, const int y, const uint64_t a0, const uint64_t a1, const uint64_t a2)
{
    typedef typename Fn::T T;
    T R, G, B;
    fn.light(ldexpf((float) a0, e - 55), ldexpf((float) a1, e - 55), ldexpf((float) a2, e - 55), R, G, B);
    const RgbArgs &a = it.c;
    if (it.packed == 3) {
        T *const d = (T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0]) + (size_t) x * 3;
        d[0] = R; d[1] = G; d[2] = B;
    } else if (it.packed == 4) {
        const T t[4] = { R, G, B, fn.alpha };
        store_packed<T, 4>((T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0]) + (size_t) x * 4, t, 4, a.dwide);
    } else {
        const size_t off = (size_t) x * sizeof(T);
        *(T *) ((uint8_t *) a.d[0] + (size_t) y * a.dstride[0] + off) = R;
        *(T *) ((uint8_t *) a.d[1] + (size_t) y * a.dstride[1] + off) = G;
        *(T *) ((uint8_t *) a.d[2] + (size_t) y * a.dstride[2] + off) = B;
    }
}

// Cell g (counted across, then down) of an item.  Everything in the item is uniform in the workgroup; all of its 256 threads call.
template <typename pixel, bool TILED, int SSH, int SSV, typename Fn>
__device__ __forceinline__ void linear_cell(LinLds &L, const uint32_t *const q, const int qmask, const LinItem &it, const int g, const Fn &fn, const int qe)
{
    typedef Piece<8 * sizeof(pixel)> piece_t;
    constexpr int NF = 2;          // row groups of a strip in flight
    const ScalePlane &p = it.p;
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane >> 3, c = lane & 7;
    const int cy = g / it.n_cx, cx = g - cy * it.n_cx;
    const int ox0 = cx * p.ow, nox = dv::imin(p.ow, p.dw - ox0);
    const int jc0 = it.row0 + cy * p.oh, jc1 = dv::imin(jc0 + p.oh, it.row1);
    const bool upx = p.up & 1, upy = p.up & 2;
    const unsigned sw = (unsigned) p.sw, dw = (unsigned) p.dw, sh = (unsigned) p.sh, dh = (unsigned) p.dh;
    // ---- the columns of the cell
    int ax0, ax1;
    if (upx) scale_span(true, ox0, nox, p.sw, p.dw, &ax0, &ax1);
    else {
        ax0 = (int) rd_div((uint64_t) ox0 * sw, dw);
        ax1 = (int) rd_div((uint64_t) (ox0 + nox) * sw + dw - 1, dw);
    }
    ax0 += p.x0; ax1 += p.x0;
    const int ux0 = ax0 & ~7, ncols = ax1 - ux0, nU = (ncols + 7) >> 3, nS = (nU + 7) >> 3;
    if (ncols > LN_NCOL || nox > LN_OW || nox <= 0) return;          // (not with the cells the host chooses; uniform, and behind the barrier of the fill)
    int lg = 0;          // across, going down: log2 of the lanes that share an output
    while (lg < 6 && (1 << lg) < (p.sw + p.dw - 1) / p.dw + 1) lg++;
    // ---- the weights across
    if (upx) {
        for (int o = tid; o < nox; o += 256) {
            int i0;
            L.nx[o] = (uint16_t) resize_weights(ox0 + o, p.sw, p.dw, &i0, &L.wu[0][o], LN_OW);
            L.ix[o] = (uint16_t) (p.x0 + i0 - ux0);
        }
    } else {
        for (int ci = tid; ci < ncols; ci += 256) {
            const int i = ux0 + ci - p.x0;
            unsigned w0 = 0, w1 = 0;
            int oc = 0x7fff;
            if (i >= 0 && i < p.sw) {
                const uint64_t lo = (uint64_t) (unsigned) i * dw;
                const unsigned o = rd_div(lo, sw);
                w0 = rd_weight((unsigned) i, o, sw, dw);
                const uint64_t b = (uint64_t) (o + 1) * sw;
                if (lo + dw > b) w1 = rd_cum((unsigned) (lo + dw - b), sw);
                oc = (int) o - ox0;
            }
            L.w0[ci] = (uint16_t) w0; L.w1[ci] = (uint16_t) w1; L.oc[ci] = (int16_t) oc;
        }
        for (int o = tid; o < nox; o += 256) {
            const uint64_t a = (uint64_t) (ox0 + o) * sw;
            const int i0 = (int) rd_div(a, dw), i1 = (int) rd_div(a + sw + dw - 1, dw) - 1;
            L.ix[o] = (uint16_t) (p.x0 + i0 - ux0);
            L.nx[o] = (uint16_t) (i1 - i0 + 1);
        }
    }
    for (int j = jc0; j < jc1; j++) {
        // ---- the taps down of this row
        int i0, n;
        if (upy) {
            uint16_t w[2];
            n = resize_weights(j, p.sh, p.dh, &i0, w, 1);
            if (tid < n) L.wy[tid] = w[tid ? 1 : 0];
        } else {
            const uint64_t a = (uint64_t) (unsigned) j * sh;
            i0 = (int) rd_div(a, dh);
            n = (int) rd_div(a + sh + dh - 1, dh) - i0;
            for (int k = tid; k < n; k += 256) L.wy[k] = (uint16_t) rd_weight((unsigned) (i0 + k), (unsigned) j, sh, dh);
        }
        i0 = __builtin_amdgcn_readfirstlane(i0); n = __builtin_amdgcn_readfirstlane(n);
        __syncthreads();          // (the weights; and the pass across of the row before is through with L.t)
        // ---- down: a wave walks a strip of 64 columns, 8 rows x 8 units at a time from a multiple of 8
        const int ya0 = p.y0 + i0, ya1 = ya0 + n, ry0 = ya0 & ~7;
        for (int strip = wave; strip < nS; strip += 4) {
            const int unit = strip * 8 + c, x = ux0 + unit * 8;
            const bool col_ok = unit < nU;
            uint64_t acc[3][8];
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
#pragma unroll
                for (int e = 0; e < 8; e++) acc[ch][e] = 0;
            for (int yb = ry0; yb < ya1; yb += 8 * NF) {
                piece_t v[NF];
                LinChroma<pixel> k[NF];
#pragma unroll
                for (int u = 0; u < NF; u++) {
                    const int y = yb + u * 8 + r;
                    if (col_ok && y >= ya0 && y < ya1) {
                        v[u] = load8<pixel, TILED>(p.s, p.sstride, x, y, p.pw - x, p.swide);
                        if (!it.c.mono) lin_chroma_load<pixel, TILED, SSH, SSV>(it, x, y, k[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < NF; u++) {
                    const int y = yb + u * 8 + r;
                    if (col_ok && y >= ya0 && y < ya1) {
                        const uint32_t w = L.wy[y - ya0];
                        uint32_t P[8];
                        lin_chroma_taps<pixel, SSH>(it, x, k[u], P);
                        uint16_t sy[8];
#pragma unroll
                        for (int e = 0; e < 8; e++) sy[e] = (uint16_t) sample_of<pixel>(v[u], e);
                        int R[8], G[8], B[8];
                        rgbx_unit<SSH, RgbRaw>(it.c, RgbRaw(), sy, P, it.hf != 0, R, G, B);
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            acc[0][e] += (uint64_t) w * q[R[e] & qmask];
                            acc[1][e] += (uint64_t) w * q[G[e] & qmask];
                            acc[2][e] += (uint64_t) w * q[B[e] & qmask];
                        }
                    }
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const uint64_t a1 = fold_rows(acc[ch], r);          // (every lane of the wave takes part)
                if (col_ok) L.t[ch][unit * 8 + r] = a1;
            }
        }
        __syncthreads();
        // ---- across
        if (upx) {
            for (int o = tid; o < nox; o += 256) {
                const int ic = L.ix[o];
                uint64_t a[3];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    a[ch] = (uint64_t) L.wu[0][o] * L.t[ch][ic];
                    if (L.nx[o] > 1) a[ch] += (uint64_t) L.wu[1][o] * L.t[ch][ic + 1];
                }
                lin_emit(it, fn, qe, ox0 + o, j, a[0], a[1], a[2]);
            }
        } else {
            // a group of G lanes per output, G the power of two that holds the taps (64 at most), 64 / G outputs of a wave at a time
            for (int ob = wave * (64 >> lg); ob < nox; ob += 4 * (64 >> lg)) {
                const int o = ob + (lane >> lg), gl = lane & ((1 << lg) - 1);
                const bool ok = o < nox;
                const int ic = ok ? L.ix[o] : 0, nt = ok ? L.nx[o] : 0;
                uint64_t a[3] = { 0, 0, 0 };
                for (int k = gl; k < nt; k += 1 << lg) {
                    const int col = ic + k;
                    const uint64_t w = L.oc[col] == o ? L.w0[col] : L.w1[col];
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) a[ch] += w * L.t[ch][col];
                }
                for (int m = (1 << lg) >> 1; m >= 1; m >>= 1) {
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) a[ch] += shfl_xor_u64(a[ch], m);
                }
                if (ok && gl == 0) lin_emit(it, fn, qe, ox0 + o, j, a[0], a[1], a[2]);
            }
        }
    }
}

template <typename pixel, bool TILED, int SSH, int SSV, typename Out>
__global__ __launch_bounds__(256) void surface_linear_kernel(const LinItem *const __restrict__ items, const uint32_t *const __restrict__ first, const int n,
                                                             const ColourArgs k, const uint16_t *const __restrict__ enc, const int qe, const Out out)
{
#ifdef DAV1D_HIP_EMU
    static uint4 lds[(LN_Q_MAX + sizeof(LinLds)) / 16];            // (the shim has no dynamic LDS: the largest)
#else
    extern __shared__ uint4 lds[];
#endif
    const int tid = (int) threadIdx.x;
    for (int i = tid; i < k.n16; i += 256) lds[i] = k.tables[i];          // q
    __syncthreads();          // (before any lane can leave)
    LinLds &L = *reinterpret_cast<LinLds *>(lds + k.n16);
    const ColourFn<Out, true> fn = { nullptr, k.has_enc ? enc : nullptr, k, out, out.alpha };          // (step 1b behind a branch on k.gain, uniform in the launch)
    const uint32_t g = blockIdx.x;
    const int lo = item_of(first, n, g);
    LinItem it = items[lo];
    it.p.s = in_device_memory(it.p.s);
    for (int pl = 0; pl < 2; pl++) it.cs[pl] = in_device_memory(it.cs[pl]);
    for (int pl = 0; pl < 3; pl++) it.c.d[pl] = in_device_memory(it.c.d[pl]);
    linear_cell<pixel, TILED, SSH, SSV>(L, reinterpret_cast<const uint32_t *>(lds), k.n_lin - 1, it, (int) (g - first[lo]), fn, qe);
}

// ---- the host side

struct LinPlan {
    SurfaceCall call;
    ScaleGeom g;
};

// the record of a checked item and its workgroups: as many outputs across as LN_NCOL columns hold; four rows, which share the weights across —
// fewer where a large window would otherwise be left to a few hundred workgroups (job_cell of surface_reduce.h)
template <typename pixel, bool TILED, typename T>
unsigned linear_item_fill(LinItem &it, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const LinPlan &pl, const Dav1dHipRgbParams &prm)
{
    const ScaleGeom &g = pl.g;
    void *const *const planes = pl.call.planes;
    it = LinItem();
    ScalePlane &p = it.p;
    p = make_scale_plane<pixel, TILED>(src, planes, g, 0);
    const long long ow = p.up & 1 ? LN_OW : (long long) (LN_NCOL - 9) * p.dw / p.sw;          // ceil(ow sw / dw) + 1 columns and up to 7 in front
    p.ow = (int) (ow > LN_OW ? LN_OW : ow < 1 ? 1 : ow);
    it.n_cx = (p.dw + p.ow - 1) / p.ow;
    it.row0 = pl.call.row0; it.row1 = pl.call.row1;
    const int rows = it.row1 - it.row0;
    const bool large = (long long) p.sw * p.sh >= 1 << 20;
    p.oh = !large || (long long) it.n_cx * ((rows + 3) / 4) >= 512 ? 4 : (long long) it.n_cx * ((rows + 1) / 2) >= 512 ? 2 : 1;
    if (!g.mono) {
        const int load_align = 8 * (int) sizeof(pixel);
        it.cs[0] = planes[1]; it.cs[1] = planes[2];
        it.cstride = (int) (src->p[1].stride / (ptrdiff_t) sizeof(pixel));
        it.cswide = TILED || (aligned_to(planes[1], src->p[1].stride, load_align) && aligned_to(planes[2], src->p[2].stride, load_align));
        it.cpw = src->p[1].w;
    }
    it.cx0 = g.x0 >> g.ss_hor; it.cy0 = g.y0 >> g.ss_ver;
    it.ccw = (g.w + g.ss_hor) >> g.ss_hor; it.cch = (g.h + g.ss_ver) >> g.ss_ver;
    it.packed = dst->format == DAV1D_HIP_SURFACE_RGB_PACKED ? 3 : dst->format == DAV1D_HIP_SURFACE_RGBA_PACKED ? 4 : 0;
    for (int k = 0; k < (it.packed ? 1 : 3); k++) { it.c.d[k] = dst->data[k]; it.c.dstride[k] = dst->stride[k]; }
    it.c.dwide = it.packed == 4 && aligned_to(dst->data[0], dst->stride[0], 4 * (int) sizeof(T));          // a pixel of four samples in one store
    rgb_set_matrix(it.c, dst, src->bpc, g.mono);
    it.pos = prm.chroma_pos; it.hf = g.ss_hor && prm.chroma_pos; it.vf = g.ss_ver && prm.chroma_pos;
    return (unsigned) it.n_cx * (unsigned) ((rows + p.oh - 1) / p.oh);
}

template <typename pixel, typename Out, bool TILED>
void linear_launch(hipStream_t st, const int cls, const dim3 grid, const unsigned lds, const LinItem *const items, const uint32_t *const first, const int n,
                   const ColourArgs &k, const uint16_t *const enc, const int qe, const Out &out)
{
    const dim3 wg(256);
    if (cls == 0) hipLaunchKernelGGL((surface_linear_kernel<pixel, TILED, 0, 0, Out>), grid, wg, lds, st, items, first, n, k, enc, qe, out);
    else if (cls == 1) hipLaunchKernelGGL((surface_linear_kernel<pixel, TILED, 1, 0, Out>), grid, wg, lds, st, items, first, n, k, enc, qe, out);
    else hipLaunchKernelGGL((surface_linear_kernel<pixel, TILED, 1, 1, Out>), grid, wg, lds, st, items, first, n, k, enc, qe, out);
}

// the checked items of a call (n of them; 1: the single call): a class per instance of the kernel — 4:4:4 and 4:0:0, 4:2:2, 4:2:0 of the raster
// sources, then of the twin-only ones
template <typename pixel, typename Out>
int linear_run(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, const LinPlan *const plan,
               const Dav1dHipRgbParams &p, const Dav1dHipColour *const h)
{
    typedef typename Out::T T;
    auto tb = batch_table<LinItem, 6>(c, n, [&](const int i) { return 3 * (int) plan[i].call.tiled + plan[i].g.ss_hor + plan[i].g.ss_ver; });
    if (const int rc = tb.open(0)) return rc;
    tb.fill([&](const int i, const int t, LinItem &it) {
        return t >= 3 ? linear_item_fill<pixel, true, T>(it, &dst[i], src[i], plan[i], p) : linear_item_fill<pixel, false, T>(it, &dst[i], src[i], plan[i], p);
    });
    Out out;
    ColourArgs k;
    colour_launch_args(p, h, out, k);
    const unsigned q_bytes = 4u << h->bpc;
    k.tables = reinterpret_cast<const uint4 *>(h->dev + h->bytes); k.n16 = (int) (q_bytes / 16);          // q takes the tables' place
    const uint16_t *const enc = reinterpret_cast<const uint16_t *>(h->dev + q_bytes);                       // (behind lin, which is as large as q)
    const unsigned lds = q_bytes + (unsigned) sizeof(LinLds);
    return tb.run(1, [](const uint8_t *) { return 0; }, [&](const int t, const LinItem *const items, const uint32_t *const first, const int n_t, const uint32_t groups) {
        if (t >= 3) linear_launch<pixel, Out, true>(c->stream, t - 3, dim3(groups), lds, items, first, n_t, k, enc, h->qe, out);
        else linear_launch<pixel, Out, false>(c->stream, t, dim3(groups), lds, items, first, n_t, k, enc, h->qe, out);
    });
}

int linear_run_sample(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, const LinPlan *const plan,
                      const Dav1dHipRgbParams &p, const Dav1dHipColour *const h)
{
    return with_pixel(h->bpc, [&](auto px) {
        return with_float_out(dst[0].sample, [&](auto out) { return linear_run<decltype(px), decltype(out)>(c, n, dst, src, plan, p, h); });
    });
}

// what the calls refuse without looking at a context or a handle ...
int linear_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, const Dav1dHipRgbParams &p,
                      const int filter, const int row0, const int row1, LinPlan *const plan)
{
    return reduced_args_check(dst, src, crop, p, filter, row0, row1, &plan->call, &plan->g);
}

// ... and the single call, in its order (include/dav1d_hip.h)
int linear_check(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop,
                 const Dav1dHipRgbParams &p, const Dav1dHipColour *const colour, const int filter, const int row0, const int row1, LinPlan *const plan)
{
    if (const int rc = linear_args_check(dst, src, crop, p, filter, row0, row1, plan)) return rc;
    if (!colour) return -EINVAL;
    if (dst->sample != DAV1D_HIP_SAMPLE_F32 && dst->sample != DAV1D_HIP_SAMPLE_F16) return -EINVAL;
    if (colour->bpc != src->bpc) return -EINVAL;
    if (!colour->has_q) return -EINVAL;          // a lin with a negative entry: light is not negative
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (colour->device != c->device) return -EXDEV;
    return 0;
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_linear_reduced(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                           const Dav1dHipRgbParams *params, const Dav1dHipColour *colour, int filter, int drow0, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    if (!c) return -EINVAL;
    LinPlan *const plan = take_plans<LinPlan>(c, 1);
    if (!plan) return -ENOMEM;
    if (const int rc = linear_check(c, dst, src, crop, p, colour, filter, drow0, drow1, plan)) return rc;
    if (plan->call.row1 <= plan->call.row0) return 0;
    return linear_run_sample(c, 1, dst, &src, plan, p, colour);
}

extern "C" int dav1d_hip_surface_export_rgb_linear_reduced_batch(Dav1dHipContext *c, int n, const Dav1dHipSurface *dst, const Dav1dHipPicture *const *src,
                                                                 const Dav1dHipSurfaceRect *crop, const Dav1dHipRgbParams *params, const Dav1dHipColour *colour,
                                                                 int filter, int *bad_item)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    LinPlan *plan;
    const int whole_rc = filter != DAV1D_HIP_RESIZE_BILINEAR ? -ENOTSUP : !colour ? -EINVAL : 0;          // the call as a whole: its filter, then its handle
    const int rc = batch_plans(c, n, dst, src, whole_rc, false, bad_item, &plan, [&](const int i, LinPlan &pl) {
        return linear_check(c, &dst[i], src[i], crop ? &crop[i] : nullptr, p, colour, filter, 0, dst[i].h, &pl);
    });
    return plan ? linear_run_sample(c, n, dst, src, plan, p, colour) : rc;
}

extern "C" int dav1d_hip_surface_rgb_linear_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                        const Dav1dHipRgbParams *params, int filter, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    LinPlan plan;
    if (const int rc = linear_args_check(dst, src, crop, p, filter, 0, drow1, &plan)) return rc;
    if (dst->sample != DAV1D_HIP_SAMPLE_F32 && dst->sample != DAV1D_HIP_SAMPLE_F16) return -EINVAL;
    if (plan.call.row1 <= 0) return 0;
    const ScaleGeom &g = plan.g;
    const int n = g.y0 + resize_rows_of(plan.call.row1, g.h, g.dh);          // the luma rows the taps down take
    if (!p.chroma_pos || !g.ss_ver) return n;
    return n + 2 < g.y0 + g.h ? n + 2 : g.y0 + g.h;          // the chroma row below the last one's own
}
