// Tensor-ready RGB at thumbnail scale: dav1d_hip_surface_export_rgb_reduced, dav1d_hip_surface_rgb_reduced_rows_needed and
// dav1d_hip_surface_export_rgb_reduced_batch (include/dav1d_hip.h).  They write what dav1d_hip_surface_export_rgb writes from the
// picture Q whose planes are R' of the crop windows: R of DESIGN.md 10.7 with the area rule S served at every ratio up to 256:1 per axis.
//
// The scaler of surface_common.h holds the source window of a cell in LDS (257 x 33 samples: 9 taps an axis) and cannot serve these ratios.  Here
//   reducer (surface_reduce.h, shared with surface_colour_reduce.hip) a streaming kernel writes Q's planes (native integers, rows padded to 16 bytes) into scratch memory of the context.  A workgroup owns a cell
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
#include "surface_reduce.h"

namespace {

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

template <typename pixel, typename Out>
int reduced_run(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                const Dav1dHipRgbParams &p, const size_t q_bytes)
{
    typedef BatchItem<Out> Item;
    int n_red = 0, n_exp[2] = { 0, 0 };
    for (int i = 0; i < n; i++) { n_red += plan[i].reduce; n_exp[!plan[i].reduce && plan[i].call.tiled]++; }
    if (const int rc = reduce_scratch_take(c, q_bytes)) return rc;
    // the tables: the items of the export (raster, then twin-only), their two prefixes, the jobs of the reducer (raster, then twin-only)
    const size_t first_at = (size_t) n * sizeof(Item), jobs_at = round_up(first_at + (size_t) (n + 2) * sizeof(uint32_t), 16);
    const size_t bytes = jobs_at + (size_t) (3 * n_red + 2) * sizeof(ReduceJob);
    Dav1dHipContext::BatchStage *s;
    if (const int rc = batch_stage_take(c, bytes, &s)) return rc;
    Item *const items = (Item *) s->host;
    uint32_t *const first = (uint32_t *) (s->host + first_at);
    ReduceJob *const jobs = (ReduceJob *) (s->host + jobs_at);
    const ReduceJobs rj = reduce_jobs_fill<pixel>(c, n, src, plan, p, false, jobs);
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
    int rc = reduce_jobs_launch<pixel>(c, d_jobs, rj);
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
