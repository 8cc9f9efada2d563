// The reducer of the thumbnail-scale exports (surface_reduce.hip: DESIGN.md 10.8; surface_colour_reduce.hip: DESIGN.md 10.9): the streaming kernel that
// writes the planes of a reduced picture Q into scratch memory of the context, its jobs, and the host side the two units share — the checks, Q's layout,
// the scratch, the job table and the launches.  surface_reduce.hip has the account of the kernel.
#pragma once
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
    int lo = 0, hi = n;          // jobs[lo].first <= g < jobs[hi].first (item_of of surface_batch.h over a field: its own loop, which keeps this kernel's code)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].first <= g) lo = mid;
        else hi = mid;
    }
    ReduceJob job = jobs[lo];
    job.p.s = in_device_memory(job.p.s); job.q = in_device_memory(job.q);
    reduce_cell<pixel, TILED>(L, job, (int) (g - job.first));
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

// what dav1d_hip_surface_export_rgb_resized refuses, in its order, with the ratio rule of these calls
int reduced_args_check(const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop, const Dav1dHipRgbParams &p,
                       const int filter, const int row0, const int row1, SurfaceCall *const call, ScaleGeom *const g)
{
    if (const int rc = rgbx_scaled_args_check(dst, src, crop, p, row0, row1, call, g, true, DAV1D_HIP_SURFACE_REDUCE_MAX)) return rc;
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

// the context's scratch holds q_bytes: grown on demand, an outgrown one is retired, not freed (launches in flight may read it)
inline int reduce_scratch_take(Dav1dHipContext *const c, const size_t q_bytes)
{
    if (q_bytes <= c->reduce_cap) return 0;
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
    return 0;
}

// the reducer's jobs of a call: those of the raster sources, an end mark, those of the twin-only sources, an end mark
struct ReduceJobs {
    int n[2], job0[2];
    uint32_t cells[2];          // workgroups
};

// Fills `jobs` (room for three per reduced item and two more) from the plans whose `reduce` is set and gives Q's planes their addresses in the
// scratch.  The rows: the band's luma rows; its chroma rows and, where the taps of chroma_pos go down, the ring — the row below, and the row above
// at chroma_pos 1 (`ring_above`: at chroma_pos 2 as well, for an export that loads it there).
template <typename pixel>
ReduceJobs reduce_jobs_fill(Dav1dHipContext *const c, const int n, const Dav1dHipPicture *const *const src, ReducePlan *const plan, const Dav1dHipRgbParams &p,
                            const bool ring_above, ReduceJob *const jobs)
{
    ReduceJobs r = ReduceJobs();
    for (int t = 0; t < 2; t++) {
        r.job0[t] = t ? r.n[0] + 1 : 0;
        for (int i = 0; i < n; i++) {
            ReducePlan &pl = plan[i];
            if (!pl.reduce || pl.call.tiled != (bool) t) continue;
            const ScaleGeom &g = pl.g;
            const int hyd = g.ss_ver && p.chroma_pos, hyu = g.ss_ver && (ring_above ? p.chroma_pos != 0 : p.chroma_pos == 1);
            const int dch = (g.dh + g.ss_ver) >> g.ss_ver;
            const int crow0 = pl.call.row0 >> g.ss_ver, crow1 = pl.call.row1 >= g.dh ? dch : pl.call.row1 >> g.ss_ver;
            for (int k = 0; k < (g.mono ? 1 : 3); k++) {
                pl.q.p[k].data = c->reduce_scratch + pl.q_off[k];
                ReduceJob &j = jobs[r.job0[t] + r.n[t]];
                j = ReduceJob();
                j.p = t ? make_scale_plane<pixel, true>(src[i], pl.call.planes, g, k) : make_scale_plane<pixel, false>(src[i], pl.call.planes, g, k);
                j.q = pl.q.p[k].data; j.qstride = (int) (pl.q.p[k].stride / (ptrdiff_t) sizeof(pixel));
                j.j0 = k ? (crow0 > hyu ? crow0 - hyu : 0) : pl.call.row0; j.j1 = k ? (crow1 + hyd < dch ? crow1 + hyd : dch) : pl.call.row1;
                if (j.j1 <= j.j0) continue;
                job_cell(j);
                j.first = r.cells[t];
                r.cells[t] += (uint32_t) j.n_cx * (uint32_t) ((j.j1 - j.j0 + j.p.oh - 1) / j.p.oh);
                r.n[t]++;
            }
        }
        jobs[r.job0[t] + r.n[t]] = ReduceJob();
        jobs[r.job0[t] + r.n[t]].first = r.cells[t];
    }
    return r;
}

// at most two launches on the context's stream: the raster sources, the twin-only ones
template <typename pixel>
int reduce_jobs_launch(Dav1dHipContext *const c, const ReduceJob *const d_jobs, const ReduceJobs &r)
{
    int rc = 0;
    if (r.cells[0]) {
        hipLaunchKernelGGL((surface_reduce_kernel<pixel, false>), dim3(r.cells[0]), dim3(256), 0, c->stream, d_jobs + r.job0[0], r.n[0]);
        rc = hip_rc(hipGetLastError());
    }
    if (r.cells[1] && !rc) {
        hipLaunchKernelGGL((surface_reduce_kernel<pixel, true>), dim3(r.cells[1]), dim3(256), 0, c->stream, d_jobs + r.job0[1], r.n[1]);
        rc = hip_rc(hipGetLastError());
    }
    return rc;
}

} // namespace
