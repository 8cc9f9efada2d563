// Colour-managed tensor export at any size: dav1d_hip_surface_export_rgb_colour_reduced and dav1d_hip_surface_export_rgb_colour_reduced_batch
// (include/dav1d_hip.h).  They write what dav1d_hip_surface_export_rgb_colour writes from the picture Q whose planes are R' of the crop
// windows: any crop to any size within 256:1, many items per launch, the colour stage on Q's code values.
//
// The one-pass form does not fit: ScaleLds (28592 / 39472 bytes) next to the colour tables (up to 47120 bytes, read at addresses the picture chooses)
// leaves one workgroup per CU.  So Q goes through the scratch memory of the context for EVERY item, whatever its ratio:
//   Q       surface_reduce_kernel of surface_reduce.h, unchanged, writes the planes (native integers, rows padded to 16 bytes, planes from 256-byte
//           offsets: plan_q).  It is general in the ratio — S's cumulative weights for any s >= d, R's taps on an axis that goes up — and serves
//           d == s, ratios under 8:1 and both axes going up here, where 10.8 launches it above 8:1 only.
//   export  surface_colour_batch_kernel: 10.6's kernel behind 10.5's item table.  Four waves a workgroup, the tables in dynamic LDS, filled once with
//           16-byte loads, one __syncthreads behind the fill and before any lane can leave; the item of a workgroup is found by bisection over a prefix
//           table of workgroups, and wave k of an item's workgroup g takes its cells (g C + i) 4 + k, i < C, through rgbx_cell with ColourFn on Q, so
//           the sited-chroma taps, the exchanges and the stores are 10.3's.  Q is raster whatever the source was: there is no TILED instance.  SSH and
//           SSV are template arguments as in 10.6, so a batch whose items mix 4:2:0, 4:2:2 and 4:4:4 / 4:0:0 is exported by a launch per class that is
//           present: one in the single call and in a batch of one layout, three at the most whatever n is.
// rgbx_cell loads units of 8 samples and, where the chroma taps go down, the chroma row above and the one below a band whatever chroma_pos is (at
// chroma_pos 2 the row above is loaded and not used).  Q's rows are padded to a unit, so a load never leaves its row, and the reducer makes both ring
// rows here at either chroma_pos (10.8 makes the one above at chroma_pos 1 only): no load reads a row of Q that this call did not write.
// Everything runs on the context's stream between the two timing events; scratch and tables are 10.8's and 10.5's.
#include "surface_reduce.h"
#include "surface_colour.h"

namespace {

struct ColourItem {
    RgbxArgs ax;                // of Q
    unsigned n_cells;           // its 64 x 8 chroma cells
};

template <typename pixel, int SSH, int SSV, typename Out, bool TONED>
__global__ __launch_bounds__(256) void surface_colour_batch_kernel(const ColourItem *const __restrict__ items, const uint32_t *const __restrict__ first, const int n,
                                                                   const ColourArgs k, const Out out)
{
#ifdef DAV1D_HIP_EMU
    static uint4 lds[LDS_MAX / 16];            // (the shim has no dynamic LDS: the largest)
#else
    extern __shared__ uint4 lds[];
#endif
    const int tid = (int) threadIdx.x;
    for (int i = tid; i < k.n16; i += 256) lds[i] = k.tables[i];
    __syncthreads();
    const float *const lin = reinterpret_cast<const float *>(lds);
    const ColourFn<Out, TONED> fn = { lin, k.has_enc ? reinterpret_cast<const uint16_t *>(lin + k.n_lin) : nullptr, k, out, out.alpha };
    const uint32_t g = blockIdx.x;
    int lo = 0, hi = n;          // first[lo] <= g < first[hi] (item_of of surface_batch.h, written out: through the helper this kernel's code comes out another)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    RgbxArgs ax = items[lo].ax;
    const unsigned n_cells = items[lo].n_cells;
    for (int pl = 0; pl < 3; pl++) { ax.r.s[pl] = in_device_memory(ax.r.s[pl]); ax.r.d[pl] = in_device_memory(ax.r.d[pl]); }
    const unsigned cell0 = (g - first[lo]) * (unsigned) k.C * 4u + (unsigned) (tid >> 6);
    for (int i = 0; i < k.C; i++) {
        const unsigned cell = cell0 + 4u * (unsigned) i;
        if (cell >= n_cells) break;          // (uniform in the wave; nothing is synchronised across waves from here on)
        rgbx_cell<pixel, false, SSH, SSV>(ax, (int) cell, fn);
    }
}

// ---- the host side

// 0: 4:4:4 and 4:0:0, 1: 4:2:2, 2: 4:2:0 — the instance of the export kernel
inline int class_of(const ScaleGeom &g) { return g.ss_hor + g.ss_ver; }

// the checked items of a call (n of them; 1: the single call), every one through its Q
template <typename pixel, typename Out, bool TONED>
int colour_reduced_run(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                       const Dav1dHipRgbParams &p, const Dav1dHipColour *const h)
{
    typedef typename Out::T T;
    size_t q_bytes = 0;
    for (int i = 0; i < n; i++) q_bytes = plan_q(plan[i], src[i], q_bytes);
    if (const int rc = reduce_scratch_take(c, q_bytes)) return rc;
    // the items of the export, a class per instance of its kernel; behind the table the jobs of the reducer
    auto tb = batch_table<ColourItem, 3>(c, n, [&](const int i) { return class_of(plan[i].g); });
    if (const int rc = tb.open((size_t) (3 * n + 2) * sizeof(ReduceJob))) return rc;
    const ReduceJobs rj = reduce_jobs_fill<pixel>(c, n, src, plan, p, true, (ReduceJob *) tb.extra());          // (Q's planes get their addresses here)
    const unsigned total = tb.fill([&](const int i, int, ColourItem &it) {
        const ReducePlan &pl = plan[i];
        void *const planes[3] = { pl.q.p[0].data, pl.q.p[1].data, pl.q.p[2].data };
        it.ax = make_rgbx_args<pixel, false, T>(&dst[i], &pl.q, planes, p, pl.call.row0, pl.call.row1, &it.n_cells);
        return it.n_cells;
    });
    Out out;
    ColourArgs k;
    colour_launch_args(p, h, out, k);
    k.n_cells = total;
    k.C = c->colour_cells ? c->colour_cells : cells_per_wave(total, h->bytes);
    return tb.run(4u * (unsigned) k.C, [&](const uint8_t *const d_jobs) { return reduce_jobs_launch<pixel>(c, (const ReduceJob *) d_jobs, rj); },
                  [&](const int t, const ColourItem *const items, const uint32_t *const first, const int n_t, const uint32_t groups) {
                      const dim3 grid(groups), wg(256);
                      hipStream_t st = c->stream;
                      if (t == 0) hipLaunchKernelGGL((surface_colour_batch_kernel<pixel, 0, 0, Out, TONED>), grid, wg, h->bytes, st, items, first, n_t, k, out);
                      else if (t == 1) hipLaunchKernelGGL((surface_colour_batch_kernel<pixel, 1, 0, Out, TONED>), grid, wg, h->bytes, st, items, first, n_t, k, out);
                      else hipLaunchKernelGGL((surface_colour_batch_kernel<pixel, 1, 1, Out, TONED>), grid, wg, h->bytes, st, items, first, n_t, k, out);
                  });
}

int colour_reduced_run_sample(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, ReducePlan *const plan,
                              const Dav1dHipRgbParams &p, const Dav1dHipColour *const h)
{
    return with_pixel(h->bpc, [&](auto px) {
        return with_float_out(dst[0].sample, [&](auto out) {
            if (h->has_tone) return colour_reduced_run<decltype(px), decltype(out), true>(c, n, dst, src, plan, p, h);
            return colour_reduced_run<decltype(px), decltype(out), false>(c, n, dst, src, plan, p, h);
        });
    });
}

// what the single call refuses, in its order (include/dav1d_hip.h)
int colour_reduced_check(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, const Dav1dHipSurfaceRect *const crop,
                         const Dav1dHipRgbParams &p, const Dav1dHipColour *const colour, const int filter, const int row0, const int row1, ReducePlan *const plan)
{
    if (const int rc = reduced_args_check(dst, src, crop, p, filter, row0, row1, &plan->call, &plan->g)) return rc;
    if (!colour) return -EINVAL;
    if (dst->sample != DAV1D_HIP_SAMPLE_F32 && dst->sample != DAV1D_HIP_SAMPLE_F16) return -EINVAL;
    if (colour->bpc != src->bpc) return -EINVAL;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (colour->device != c->device) return -EXDEV;
    plan->reduce = 1;
    return 0;
}

} // namespace

extern "C" int dav1d_hip_surface_export_rgb_colour_reduced(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                                           const Dav1dHipRgbParams *params, const Dav1dHipColour *colour, int filter, int drow0, int drow1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    if (!c) return -EINVAL;
    ReducePlan *const plan = take_plans<ReducePlan>(c, 1);
    if (!plan) return -ENOMEM;
    if (const int rc = colour_reduced_check(c, dst, src, crop, p, colour, filter, drow0, drow1, plan)) return rc;
    if (plan->call.row1 <= plan->call.row0) return 0;
    return colour_reduced_run_sample(c, 1, dst, &src, plan, p, colour);
}

extern "C" int dav1d_hip_surface_export_rgb_colour_reduced_batch(Dav1dHipContext *c, int n, const Dav1dHipSurface *dst, const Dav1dHipPicture *const *src,
                                                                 const Dav1dHipSurfaceRect *crop, const Dav1dHipRgbParams *params, const Dav1dHipColour *colour,
                                                                 int filter, int *bad_item)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    ReducePlan *plan;
    // the call as a whole: its filter, then its handle.  (An item whose bpc is not the handle's is refused by the single call's rule, which is
    // stricter than the pixel size of 10.5.)
    const int whole_rc = filter != DAV1D_HIP_RESIZE_BILINEAR ? -ENOTSUP : !colour ? -EINVAL : 0;
    const int rc = batch_plans(c, n, dst, src, whole_rc, false, bad_item, &plan, [&](const int i, ReducePlan &pl) {
        return colour_reduced_check(c, &dst[i], src[i], crop ? &crop[i] : nullptr, p, colour, filter, 0, dst[i].h, &pl);
    });
    return plan ? colour_reduced_run_sample(c, n, dst, src, plan, p, colour) : rc;
}
