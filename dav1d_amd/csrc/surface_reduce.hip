// Tensor-ready RGB at thumbnail scale: dav1d_hip_surface_export_rgb_reduced, dav1d_hip_surface_rgb_reduced_rows_needed and
// dav1d_hip_surface_export_rgb_reduced_batch (include/dav1d_hip.h).  They write what dav1d_hip_surface_export_rgb writes from the
// picture Q whose planes are R' of the crop windows: R of DESIGN.md 10.7 with the area rule S served at every ratio up to 256:1 per axis.
//
// The scaler of surface_common.h holds the source window of a cell in LDS (257 x 33 samples: 9 taps an axis) and cannot serve these ratios.  Here
//   reducer a streaming kernel writes Q's planes (native integers, rows padded to 16 bytes) into scratch memory of the context.  A workgroup owns a cell
//           of a Q plane, ow x oh outputs whose source columns fit RD_NCOL.  Per output row it walks the source rows of the vertical taps once: a wave
//           takes a strip of 64 columns, 8 rows x 8 units of 8 samples at a time (whole 128-byte lines: eight tiles of a twin, eight pieces of raster
//           rows at 10 / 12 bits), four such loads in flight, and keeps sum wy P per column in registers (below 2^24); the eight row lanes of a
//           column are added with seven exchanges (each lane ends with one column) and t = (sum + 8) >> 4 goes to one LDS row.  The pass across reads that row: a group of lanes per
//           output, a lane per tap, up to six exchanges (integer sums: any order).  The source row on the border of two output rows is read for both.
//   weights across, per source column and made once per cell: the first output it feeds and its weights for that one and the next (a sample is no
//           wider than an output, so there is no third).  S's cumulative rule: with c(x) = (x * 4096 + s / 2) / s the weight of sample i for output
//           o is c(min((i + 1) d, (o + 1) s) - o s) - c(max(i d, o s) - o s), which is scale_weights' q - prev.  Down, per output row: the same rule
//           per tap.  An axis that goes up takes R's one or two taps (resize_weights).
//   export  Q, described as a raster picture, goes through scale_rgbx_cell at d == s (S is the identity there), which is dav1d_hip_surface_export_rgb
//           of Q: the kernel of surface_resize.hip's batch behind its table.  Items of a batch that no axis takes past 8:1 run in that same launch
//           from their own source and crop, so they get dav1d_hip_surface_export_rgb_resized's bytes.
// Everything runs on the context's stream between the two timing events: at most two reducer launches (raster / twin-only sources) and two export
// launches.  The scratch grows on demand and is kept; an outgrown one is retired, not freed (launches in flight may read it), until dav1d_hip_close.
#include "surface_batch.h"

namespace {

constexpr int RD_NCOL = 2048;       // source columns of a cell (from a multiple of 8)
constexpr int RD_OW = 256;          // outputs across a cell
constexpr int RD_TAPS = 264;        // taps down: 257 at 256:1

struct ReduceJob {                  // a Q plane of an item
    ScalePlane p;                   // (ow x oh: the cell)
    void *q;
    int qstride;                    // pixels
    int j0, j1;                     // rows of Q to make
    int n_cx;
    uint32_t first;                 // workgroups of the jobs before this one
};

struct ReduceLds {
    uint32_t t[RD_NCOL];
    uint16_t w0[RD_NCOL], w1[RD_NCOL];
    int16_t oc[RD_NCOL];            // the first output a column feeds, from the cell's first
    uint16_t wy[RD_TAPS];
    uint16_t ix[RD_OW], nx[RD_OW];  // the first tap (column of the LDS row) and the taps of an output
    uint16_t wu[2][RD_OW];          // across, going up: R's weights
};

__device__ __forceinline__ unsigned rd_div(const uint64_t a, const unsigned b) { return (a >> 32) ? (unsigned) (a / b) : (unsigned) a / b; }
__device__ __forceinline__ unsigned rd_cum(const unsigned cov, const unsigned s) { return (cov * 4096u + (s >> 1)) / s; }      // cov <= s < 2^20

// the weight of sample i of an axis (s samples to d <= s) for output o, which it overlaps
__device__ __forceinline__ unsigned rd_weight(const unsigned i, const unsigned o, const unsigned s, const unsigned d)
{
    const uint64_t a = (uint64_t) o * s, b = a + s, lo = (uint64_t) i * d, hi = lo + d;
    return rd_cum((unsigned) ((hi < b ? hi : b) - a), s) - (lo > a ? rd_cum((unsigned) (lo - a), s) : 0u);
}

// Cell g (counted across, then down) of a job.  Everything in the job is uniform in the workgroup; all of its 256 threads call.
template <typename pixel, bool TILED>
__device__ __forceinline__ void reduce_cell(ReduceLds &L, const ReduceJob &job, const int g)
{
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const ScalePlane &p = job.p;
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane >> 3, c = lane & 7;
    const int cy = g / job.n_cx, cx = g - cy * job.n_cx;
    const int ox0 = cx * p.ow, nox = dv::imin(p.ow, p.dw - ox0);
    const int jc0 = job.j0 + cy * p.oh, jc1 = dv::imin(jc0 + p.oh, job.j1);
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
    if (ncols > RD_NCOL || nox > RD_OW) return;          // (not with the cells the host chooses)
    int lg = 0;          // across, going down: log2 of the lanes that share an output
    while (lg < 6 && (1 << lg) < (p.sw + p.dw - 1) / p.dw + 1) lg++;
    // ---- the weights across
    if (upx) {
        for (int o = tid; o < nox; o += 256) {
            int i0;
            L.nx[o] = (uint16_t) resize_weights(ox0 + o, p.sw, p.dw, &i0, &L.wu[0][o], RD_OW);
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
            unsigned acc[8];
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] = 0;
            for (int yb = ry0; yb < ya1; yb += 32) {
                piece_t v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int y = yb + u * 8 + r;
                    if (col_ok && y >= ya0 && y < ya1) v[u] = load8<pixel, TILED>(p.s, p.sstride, x, y, p.pw - x, p.swide);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int y = yb + u * 8 + r;
                    if (col_ok && y >= ya0 && y < ya1) {
                        const unsigned w = L.wy[y - ya0];
#pragma unroll
                        for (int e = 0; e < 8; e++) acc[e] = dv::mad_u24(w, (unsigned) sample_of<pixel>(v[u], e), acc[e]);
                    }
                }
            }
            // the eight row lanes of a column: seven exchanges, each halving what a lane still carries; lane r is left with column r of its unit
            unsigned a4[4], a2[2];
#pragma unroll
            for (int e = 0; e < 4; e++) a4[e] = (r & 4 ? acc[e + 4] : acc[e]) + (unsigned) __shfl_xor((int) (r & 4 ? acc[e] : acc[e + 4]), 32);
#pragma unroll
            for (int e = 0; e < 2; e++) a2[e] = (r & 2 ? a4[e + 2] : a4[e]) + (unsigned) __shfl_xor((int) (r & 2 ? a4[e] : a4[e + 2]), 16);
            const unsigned a1 = (r & 1 ? a2[1] : a2[0]) + (unsigned) __shfl_xor((int) (r & 1 ? a2[0] : a2[1]), 8);
            if (col_ok) L.t[unit * 8 + r] = (a1 + 8) >> 4;
        }
        __syncthreads();
        // ---- across
        pixel *const qrow = (pixel *) job.q + (size_t) j * job.qstride + ox0;
        if (upx) {
            for (int o = tid; o < nox; o += 256) {
                const int ic = L.ix[o];
                unsigned sum = dv::mad_u24(L.wu[0][o], L.t[ic], 1u << 19);
                if (L.nx[o] > 1) sum = dv::mad_u24(L.wu[1][o], L.t[ic + 1], sum);
                qrow[o] = (pixel) (sum >> 20);
            }
        } else {
            // a group of G lanes per output, G the power of two that holds the taps (64 at most), 64 / G outputs of a wave at a time
            for (int ob = wave * (64 >> lg); ob < nox; ob += 4 * (64 >> lg)) {
                const int o = ob + (lane >> lg), gl = lane & ((1 << lg) - 1);
                const bool ok = o < nox;
                const int ic = ok ? L.ix[o] : 0, nt = ok ? L.nx[o] : 0;
                unsigned sum = 0;
                for (int k = gl; k < nt; k += 1 << lg) {
                    const int col = ic + k;
                    const unsigned w = L.oc[col] == o ? L.w0[col] : L.w1[col];
                    sum = dv::mad_u24(w, L.t[col], sum);
                }
                for (int m = (1 << lg) >> 1; m >= 1; m >>= 1) sum += (unsigned) __shfl_xor((int) sum, m);
                if (ok && gl == 0) qrow[o] = (pixel) ((sum + (1u << 19)) >> 20);
            }
        }
    }
}

template <typename pixel, bool TILED>
__global__ __launch_bounds__(256) void surface_reduce_kernel(const ReduceJob *const __restrict__ jobs, const int n)
{
    __shared__ ReduceLds L;
    const uint32_t g = blockIdx.x;
    int lo = 0, hi = n;          // jobs[lo].first <= g < jobs[hi].first
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].first <= g) lo = mid;
        else hi = mid;
    }
    ReduceJob job = jobs[lo];
    job.p.s = in_device_memory(job.p.s); job.q = in_device_memory(job.q);
    reduce_cell<pixel, TILED>(L, job, (int) (g - job.first));
}

// the export of the batch: surface_batch.h's kernel under a name of this unit
template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256, sizeof(pixel) == 1 ? 5 : 4) void surface_reduced_rgbx_kernel(const BatchItem<Out> *const __restrict__ items, const uint32_t *const __restrict__ first,
                                                                                                const int n)
{
    __shared__ ScaleLds<pixel> L;
    const uint32_t g = blockIdx.x;
    int lo = 0, hi = n;          // first[lo] <= g < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    const BatchItem<Out> &it = items[lo];
    ScaleRgbxArgs a = it.a;
    for (int pl = 0; pl < 3; pl++) { a.pl[pl].s = in_device_memory(a.pl[pl].s); a.c.d[pl] = in_device_memory(a.c.d[pl]); }
    scale_rgbx_cell<pixel, TILED, Out, true>(L, a, (int) (g - first[lo]), it.out);
}

// ---- the host side

// what the checks found about an item, and the picture Q of one that is reduced
struct ReducePlan {
    SurfaceCall call;
    ScaleGeom g;
    int reduce;
    Dav1dHipPicture q;
    size_t q_off[3];
};

inline size_t round_up(const size_t v, const size_t a) { return (v + a - 1) / a * a; }

// the crop and the ratio: scale_geom_check with these calls' rule
int reduce_geom_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, ScaleGeom *const g)
{
    const int W = src->p[0].w, H = src->p[0].h;
    g->mono = src->layout == DAV1D_HIP_LAYOUT_I400;
    g->ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420; g->ss_hor = !g->mono && src->layout != DAV1D_HIP_LAYOUT_I444;
    g->x0 = crop ? crop->x0 : 0; g->y0 = crop ? crop->y0 : 0; g->w = crop ? crop->w : W; g->h = crop ? crop->h : H;
    g->dw = dst->w; g->dh = dst->h;
    if (g->w <= 0 || g->h <= 0 || g->x0 < 0 || g->y0 < 0 || g->x0 > W - g->w || g->y0 > H - g->h) return -EINVAL;
    if ((g->ss_hor && (g->x0 & 1)) || (g->ss_ver && (g->y0 & 1))) return -EINVAL;
    if (g->w > (long long) DAV1D_HIP_SURFACE_REDUCE_MAX * g->dw || g->h > (long long) DAV1D_HIP_SURFACE_REDUCE_MAX * g->dh) return -ENOTSUP;
    return 0;
}

// what dav1d_hip_surface_export_rgb_resized refuses, in its order, with the ratio rule of these calls
int reduced_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, const Dav1dHipRgbParams &p,
                       const int filter, const int row0, const int row1, SurfaceCall *const call, ScaleGeom *const g)
{
    if (const int rc = surface_args_check(dst, src, row0, row1, call, true, true)) return rc;
    if (const int rc = rgb_params_check(dst, p)) return rc;
    if (const int rc = reduce_geom_check(dst, src, crop, g)) return rc;
    return filter == DAV1D_HIP_RESIZE_BILINEAR ? 0 : -ENOTSUP;
}

// Q of a checked item at `off` of the scratch (its base is set later): the planes' places; returns the end
size_t plan_q(ReducePlan &pl, const Dav1dHipPicture *const src, size_t off)
{
    const ScaleGeom &g = pl.g;
    const size_t ps = src->bpc > 8 ? 2 : 1;
    pl.q = Dav1dHipPicture();
    pl.q.bpc = src->bpc; pl.q.layout = src->layout;
    for (int k = 0; k < (g.mono ? 1 : 3); k++) {
        const int w = k ? (g.dw + g.ss_hor) >> g.ss_hor : g.dw, h = k ? (g.dh + g.ss_ver) >> g.ss_ver : g.dh;
        pl.q.p[k].w = w; pl.q.p[k].h = h;
        pl.q.p[k].stride = (ptrdiff_t) round_up((size_t) w * ps, 16);
        pl.q_off[k] = off;
        off = round_up(off + (size_t) pl.q.p[k].stride * h, 256);
    }
    return off;
}

// the cell of a job: as many outputs across as RD_NCOL columns hold; four rows, which share the weights across — fewer where a large window would
// otherwise be left to a few hundred workgroups
void job_cell(ReduceJob &j)
{
    ScalePlane &p = j.p;
    long long ow = p.up & 1 ? RD_OW : (long long) (RD_NCOL - 9) * p.dw / p.sw;          // ceil(ow sw / dw) + 1 columns and up to 7 in front
    p.ow = (int) (ow > RD_OW ? RD_OW : ow < 1 ? 1 : ow);
    j.n_cx = (p.dw + p.ow - 1) / p.ow;
    const int rows = j.j1 - j.j0;
    const bool large = (long long) p.sw * p.sh >= 1 << 20;
    p.oh = !large || (long long) j.n_cx * ((rows + 3) / 4) >= 512 ? 4 : (long long) j.n_cx * ((rows + 1) / 2) >= 512 ? 2 : 1;
}

template <typename pixel, typename Out>
int reduced_run(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                const Dav1dHipRgbParams &p, const size_t q_bytes)
{
    typedef BatchItem<Out> Item;
    int n_red = 0, n_exp[2] = { 0, 0 };
    for (int i = 0; i < n; i++) { n_red += plan[i].reduce; n_exp[!plan[i].reduce && plan[i].call.tiled]++; }
    if (q_bytes > c->reduce_cap) {
        size_t want = 1 << 20;
        while (want < q_bytes) want <<= 1;
        void *d = nullptr;
        if (hipMalloc(&d, want) != hipSuccess) { (void) hipGetLastError(); return -ENOMEM; }
        try {
            if (c->reduce_scratch) c->batch_retired_dev.push_back(c->reduce_scratch);
        } catch (...) {
            (void) hipFree(d);
            return -ENOMEM;
        }
        c->reduce_scratch = (uint8_t *) d; c->reduce_cap = want;
    }
    // the tables: the items of the export (raster, then twin-only), their two prefixes, the jobs of the reducer (raster, then twin-only)
    const size_t first_at = (size_t) n * sizeof(Item), jobs_at = round_up(first_at + (size_t) (n + 2) * sizeof(uint32_t), 16);
    const size_t bytes = jobs_at + (size_t) (3 * n_red + 2) * sizeof(ReduceJob);
    Dav1dHipContext::BatchStage *s;
    if (const int rc = batch_stage_take(c, bytes, &s)) return rc;
    Item *const items = (Item *) s->host;
    uint32_t *const first = (uint32_t *) (s->host + first_at);
    ReduceJob *const jobs = (ReduceJob *) (s->host + jobs_at);
    // ---- the reducer's jobs
    int n_jobs[2] = { 0, 0 }, job0[2];
    uint32_t cells[2] = { 0, 0 };
    for (int t = 0; t < 2; t++) {
        job0[t] = t ? n_jobs[0] + 1 : 0;
        for (int i = 0; i < n; i++) {
            ReducePlan &pl = plan[i];
            if (!pl.reduce || pl.call.tiled != (bool) t) continue;
            const ScaleGeom &g = pl.g;
            const int hyd = g.ss_ver && p.chroma_pos, hyu = g.ss_ver && p.chroma_pos == 1;
            const int dch = (g.dh + g.ss_ver) >> g.ss_ver;
            const int crow0 = pl.call.row0 >> g.ss_ver, crow1 = pl.call.row1 >= g.dh ? dch : pl.call.row1 >> g.ss_ver;
            for (int k = 0; k < (g.mono ? 1 : 3); k++) {
                pl.q.p[k].data = c->reduce_scratch + pl.q_off[k];
                ReduceJob &j = jobs[job0[t] + n_jobs[t]];
                j = ReduceJob();
                j.p = t ? make_scale_plane<pixel, true>(src[i], pl.call.planes, g, k) : make_scale_plane<pixel, false>(src[i], pl.call.planes, g, k);
                j.q = pl.q.p[k].data; j.qstride = (int) (pl.q.p[k].stride / (ptrdiff_t) sizeof(pixel));
                j.j0 = k ? (crow0 > hyu ? crow0 - hyu : 0) : pl.call.row0; j.j1 = k ? (crow1 + hyd < dch ? crow1 + hyd : dch) : pl.call.row1;
                if (j.j1 <= j.j0) continue;
                job_cell(j);
                j.first = cells[t];
                cells[t] += (uint32_t) j.n_cx * (uint32_t) ((j.j1 - j.j0 + j.p.oh - 1) / j.p.oh);
                n_jobs[t]++;
            }
        }
        jobs[job0[t] + n_jobs[t]] = ReduceJob();
        jobs[job0[t] + n_jobs[t]].first = cells[t];
    }
    // ---- the items of the export: a reduced item is read from its Q, in raster order (counted with the raster items above)
    const int slice0[2] = { 0, n_exp[0] }, first0[2] = { 0, n_exp[0] + 1 };
    int fill[2] = { 0, 0 };
    uint32_t groups[2] = { 0, 0 };
    for (int i = 0; i < n; i++) {
        const ReducePlan &pl = plan[i];
        const int t = !pl.reduce && pl.call.tiled, k = fill[t]++;
        Item &it = items[slice0[t] + k];
        unsigned ng;
        if (pl.reduce) {
            ScaleGeom gq = pl.g;
            gq.x0 = gq.y0 = 0; gq.w = gq.dw; gq.h = gq.dh;
            void *const planes[3] = { pl.q.p[0].data, pl.q.p[1].data, pl.q.p[2].data };
            it.a = make_scale_rgbx_args<pixel, false, typename Out::T>(&dst[i], &pl.q, planes, gq, p, pl.call.row0, pl.call.row1, &ng);
        } else {
            it.a = t ? make_scale_rgbx_args<pixel, true, typename Out::T>(&dst[i], src[i], pl.call.planes, pl.g, p, pl.call.row0, pl.call.row1, &ng)
                     : make_scale_rgbx_args<pixel, false, typename Out::T>(&dst[i], src[i], pl.call.planes, pl.g, p, pl.call.row0, pl.call.row1, &ng);
        }
        it.out = Out();
        set_out(it.out, p, src[i]->bpc);
        first[first0[t] + k] = groups[t];
        groups[t] += ng;
    }
    for (int t = 0; t < 2; t++) first[first0[t] + n_exp[t]] = groups[t];
    HIP_TRY(hipMemcpyAsync(s->dev, s->host, bytes, hipMemcpyHostToDevice, c->stream));
    const Item *const d_items = (const Item *) s->dev;
    const uint32_t *const d_first = (const uint32_t *) (s->dev + first_at);
    const ReduceJob *const d_jobs = (const ReduceJob *) (s->dev + jobs_at);
    (void) hipEventRecord(c->ev_t0, c->stream);
    int rc = 0;
    if (cells[0]) {
        hipLaunchKernelGGL((surface_reduce_kernel<pixel, false>), dim3(cells[0]), dim3(256), 0, c->stream, d_jobs + job0[0], n_jobs[0]);
        rc = hip_rc(hipGetLastError());
    }
    if (cells[1] && !rc) {
        hipLaunchKernelGGL((surface_reduce_kernel<pixel, true>), dim3(cells[1]), dim3(256), 0, c->stream, d_jobs + job0[1], n_jobs[1]);
        rc = hip_rc(hipGetLastError());
    }
    if (groups[0] && !rc) {
        hipLaunchKernelGGL((surface_reduced_rgbx_kernel<pixel, false, Out>), dim3(groups[0]), dim3(256), 0, c->stream, d_items, d_first, n_exp[0]);
        rc = hip_rc(hipGetLastError());
    }
    if (groups[1] && !rc) {
        hipLaunchKernelGGL((surface_reduced_rgbx_kernel<pixel, true, Out>), dim3(groups[1]), dim3(256), 0, c->stream, d_items + slice0[1], d_first + first0[1], n_exp[1]);
        rc = hip_rc(hipGetLastError());
    }
    (void) hipEventRecord(c->ev_t1, c->stream);
    (void) hipEventRecord(s->done, c->stream);
    s->busy = true;
    c->last_ms_pending = !rc;
    return rc;
}

template <typename pixel>
int reduced_run_sample(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                       const Dav1dHipRgbParams &p, const size_t q_bytes)
{
    if (dst[0].sample == DAV1D_HIP_SAMPLE_F32) return reduced_run<pixel, RgbF32>(c, n, dst, src, plan, p, q_bytes);
    if (dst[0].sample == DAV1D_HIP_SAMPLE_F16) return reduced_run<pixel, RgbF16>(c, n, dst, src, plan, p, q_bytes);
    if constexpr (sizeof(pixel) == 2) {
        if (dst[0].sample == DAV1D_HIP_SAMPLE_MSB16) return reduced_run<pixel, RgbInt<OutMsb16>>(c, n, dst, src, plan, p, q_bytes);
    }
    return reduced_run<pixel, RgbInt<OutNative<pixel>>>(c, n, dst, src, plan, p, q_bytes);
}

// the plans of a call live in the context's batch_plan
ReducePlan *take_plans(Dav1dHipContext *const c, const int n)
{
    try {
        if (c->batch_plan.size() < (size_t) n * sizeof(ReducePlan) + alignof(ReducePlan)) c->batch_plan.resize((size_t) n * sizeof(ReducePlan) + alignof(ReducePlan));
    } catch (...) {
        return nullptr;
    }
    return (ReducePlan *) round_up((size_t) (uintptr_t) c->batch_plan.data(), alignof(ReducePlan));
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_reduced(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                    const Dav1dHipRgbParams *params, int filter, int drow0, int drow1)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    if (!c) return -EINVAL;
    ReducePlan *const plan = take_plans(c, 1);
    if (!plan) return -ENOMEM;
    if (const int rc = reduced_args_check(dst, src, crop, p, filter, drow0, drow1, &plan->call, &plan->g)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (plan->call.row1 <= plan->call.row0) return 0;
    plan->reduce = plan->g.w > 8LL * plan->g.dw || plan->g.h > 8LL * plan->g.dh;
    const size_t q_bytes = plan->reduce ? plan_q(*plan, src, 0) : 0;
    return src->bpc == 8 ? reduced_run_sample<uint8_t>(c, 1, dst, &src, plan, p, q_bytes) : reduced_run_sample<uint16_t>(c, 1, dst, &src, plan, p, q_bytes);
}

extern "C" int dav1d_hip_surface_rgb_reduced_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                         const Dav1dHipRgbParams *params, int filter, int drow1)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    SurfaceCall call;
    ScaleGeom g;
    if (const int rc = reduced_args_check(dst, src, crop, p, filter, 0, drow1, &call, &g)) return rc;
    if (call.row1 <= 0) return 0;
    // the ring: the chroma row below the band's last is made as well
    const int r = g.ss_ver && p.chroma_pos ? call.row1 + 2 : call.row1;
    return resize_rows_needed(g, src->p[0].h, r > g.dh ? g.dh : r);
}

extern "C" int dav1d_hip_surface_export_rgb_reduced_batch(Dav1dHipContext *c, int n, const Dav1dHipSurface *dst, const Dav1dHipPicture *const *src,
                                                          const Dav1dHipSurfaceRect *crop, const Dav1dHipRgbParams *params, int filter, int *bad_item)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    if (bad_item) *bad_item = -1;
    if (!c || n < 0 || n > DAV1D_HIP_SURFACE_BATCH_MAX) return -EINVAL;
    if (filter != DAV1D_HIP_RESIZE_BILINEAR) return -ENOTSUP;          // the call as a whole
    if (!n) return 0;
    if (!dst || !src) return -EINVAL;
    for (int i = 0; i < n; i++)
        if (!src[i]) { if (bad_item) *bad_item = i; return -EINVAL; }
    ReducePlan *const plan = take_plans(c, n);
    if (!plan) return -ENOMEM;
    size_t q_bytes = 0;
    for (int i = 0; i < n; i++) {
        ReducePlan &pl = plan[i];
        int rc = reduced_args_check(&dst[i], src[i], crop ? &crop[i] : nullptr, p, filter, 0, dst[i].h, &pl.call, &pl.g);
        if (!rc) rc = pictures_on_device(c, src[i], 1);
        // one kernel instance for the batch: format, sample and pixel size are item 0's
        if (!rc && (dst[i].format != dst[0].format || dst[i].sample != dst[0].sample || (src[i]->bpc == 8) != (src[0]->bpc == 8))) rc = -EINVAL;
        if (rc) { if (bad_item) *bad_item = i; return rc; }
        pl.reduce = pl.g.w > 8LL * pl.g.dw || pl.g.h > 8LL * pl.g.dh;
        if (pl.reduce) q_bytes = plan_q(pl, src[i], q_bytes);
    }
    return src[0]->bpc == 8 ? reduced_run_sample<uint8_t>(c, n, dst, src, plan, p, q_bytes) : reduced_run_sample<uint16_t>(c, n, dst, src, plan, p, q_bytes);
}
