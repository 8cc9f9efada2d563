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

// ---- the host side

// the checked items of a call (n of them; 1: the single call), those past 8:1 through their Q
template <typename pixel, typename Out>
int reduced_run(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                const Dav1dHipRgbParams &p)
{
    typedef BatchItem<Out> Item;
    int n_red = 0;
    size_t q_bytes = 0;
    for (int i = 0; i < n; i++) {
        ReducePlan &pl = plan[i];
        pl.reduce = pl.g.w > 8LL * pl.g.dw || pl.g.h > 8LL * pl.g.dh;
        if (pl.reduce) { q_bytes = plan_q(pl, src[i], q_bytes); n_red++; }
    }
    if (const int rc = reduce_scratch_take(c, q_bytes)) return rc;
    // the items of the export: raster ones — a reduced item is read from its Q, whatever its source — then twin-only ones; behind the table the jobs
    // of the reducer
    auto tb = batch_table<Item, 2>(c, n, [&](const int i) { return (int) (!plan[i].reduce && plan[i].call.tiled); });
    if (const int rc = tb.open((size_t) (3 * n_red + 2) * sizeof(ReduceJob))) return rc;
    const ReduceJobs rj = reduce_jobs_fill<pixel>(c, n, src, plan, p, false, (ReduceJob *) tb.extra());
    tb.fill([&](const int i, const int t, Item &it) {
        const ReducePlan &pl = plan[i];
        if (!pl.reduce) return rgbx_item_fill<pixel>(it, t, &dst[i], src[i], pl.call.planes, pl.g, p, pl.call.row0, pl.call.row1);
        ScaleGeom gq = pl.g;
        gq.x0 = gq.y0 = 0; gq.w = gq.dw; gq.h = gq.dh;
        void *const planes[3] = { pl.q.p[0].data, pl.q.p[1].data, pl.q.p[2].data };
        return rgbx_item_fill<pixel>(it, false, &dst[i], &pl.q, planes, gq, p, pl.call.row0, pl.call.row1);
    });
    return tb.run(1, [&](const uint8_t *const d_jobs) { return reduce_jobs_launch<pixel>(c, (const ReduceJob *) d_jobs, rj); },
                  [&](const int t, const Item *const items, const uint32_t *const first, const int n_t, const uint32_t groups) {
                      launch_rgbx_batch<pixel, Out, true>(c->stream, t, items, first, n_t, groups);
                  });
}

int reduced_run_sample(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                       const Dav1dHipRgbParams &p)
{
    return with_pixel(src[0]->bpc, [&](auto px) {
        typedef decltype(px) pixel;
        return with_rgb_out<pixel>(dst[0].sample, p, src[0]->bpc, [&](const auto &o) {          // (the type: every item gets the functor of its own depth)
            return reduced_run<pixel, std::decay_t<decltype(o)>>(c, n, dst, src, plan, p);
        });
    });
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_reduced(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                    const Dav1dHipRgbParams *params, int filter, int drow0, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    if (!c) return -EINVAL;
    ReducePlan *const plan = take_plans<ReducePlan>(c, 1);
    if (!plan) return -ENOMEM;
    if (const int rc = reduced_args_check(dst, src, crop, p, filter, drow0, drow1, &plan->call, &plan->g)) return rc;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (plan->call.row1 <= plan->call.row0) return 0;
    return reduced_run_sample(c, 1, dst, &src, plan, p);
}

extern "C" int dav1d_hip_surface_rgb_reduced_rows_needed(const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                         const Dav1dHipRgbParams *params, int filter, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    ScaleGeom g;
    return sized_rows_needed(reduced_args_check(dst, src, crop, p, filter, 0, drow1, &call, &g), call, g, p.chroma_pos != 0, src);
}

extern "C" int dav1d_hip_surface_export_rgb_reduced_batch(Dav1dHipContext *c, int n, const Dav1dHipSurface *dst, const Dav1dHipPicture *const *src,
                                                          const Dav1dHipSurfaceRect *crop, const Dav1dHipRgbParams *params, int filter, int *bad_item)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    ReducePlan *plan;
    const int rc = batch_plans(c, n, dst, src, filter == DAV1D_HIP_RESIZE_BILINEAR ? 0 : -ENOTSUP, true, bad_item, &plan, [&](const int i, ReducePlan &pl) {
        const int rc = reduced_args_check(&dst[i], src[i], crop ? &crop[i] : nullptr, p, filter, 0, dst[i].h, &pl.call, &pl.g);
        return rc ? rc : pictures_on_device(c, src[i], 1);
    });
    return plan ? reduced_run_sample(c, n, dst, src, plan, p) : rc;
}
