// What the batched exports share (surface_batch.hip has the account of the table, the search, the picture states and the staging ring): the kernels of
// the scaled and resized batches, and the host side of every batch — the front of an entry point (batch_plans), the plans it keeps (take_plans) and the
// table of a launch from its staging slot to the events behind it (BatchTable).  surface_resize.hip, surface_reduce.hip and
// surface_colour_reduce.hip run their batches through the same.
#pragma once
#include "surface_call.h"

namespace {

template <typename Out> struct BatchItem {
    ScaleRgbxArgs a;
    Out out;
};

// what the checks found about an item: its rows, planes and picture state, and its geometry
struct BatchPlan {
    SurfaceCall call;
    ScaleGeom g;
};

// A pointer that arrives as a kernel argument is known to point into device memory; one read from a table is not, and its loads and stores would be
// flat ones, which wait on the LDS counter as well.  Made anew as a pointer of the global address space, it says so.
template <typename P> __device__ __forceinline__ P *in_device_memory(P *const p)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(DAV1D_HIP_EMU)
    return (P *) (__attribute__((address_space(1))) P *) (uintptr_t) p;          // (a flat address of device memory is its global address)
#else
    return p;
#endif
}

// the item of workgroup g: the last k with first[k] <= g, of a prefix with first[0] = 0 and first[n] = all workgroups
__device__ __forceinline__ int item_of(const uint32_t *const first, const int n, const uint32_t g)
{
    int lo = 0, hi = n;          // first[lo] <= g < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_scale_rgbx_batch_kernel(const BatchItem<Out> *const __restrict__ items, const uint32_t *const __restrict__ first,
                                                                       const int n)
{
    __shared__ ScaleLds<pixel> L;
    const uint32_t g = blockIdx.x;
    const int lo = item_of(first, n, g);
    const BatchItem<Out> &it = items[lo];
    ScaleRgbxArgs a = it.a;
    for (int pl = 0; pl < 3; pl++) { a.pl[pl].s = in_device_memory(a.pl[pl].s); a.c.d[pl] = in_device_memory(a.c.d[pl]); }
    scale_rgbx_cell<pixel, TILED, Out>(L, a, (int) (g - first[lo]), it.out);
}

// the same search in front of the resizing body (surface_resize.hip: an axis of an item may go up; surface_reduce.hip: Q at its own size); a kernel of
// its own, so that the one above keeps its code to the register
template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256, sizeof(pixel) == 1 ? 5 : 4) void surface_resize_rgbx_batch_kernel(const BatchItem<Out> *const __restrict__ items, const uint32_t *const __restrict__ first,
                                                                        const int n)
{
    __shared__ ScaleLds<pixel> L;
    const uint32_t g = blockIdx.x;
    const int lo = item_of(first, n, g);
    const BatchItem<Out> &it = items[lo];
    ScaleRgbxArgs a = it.a;
    for (int pl = 0; pl < 3; pl++) { a.pl[pl].s = in_device_memory(a.pl[pl].s); a.c.d[pl] = in_device_memory(a.c.d[pl]); }
    scale_rgbx_cell<pixel, TILED, Out, true>(L, a, (int) (g - first[lo]), it.out);
}

// ---- the host side

inline size_t round_up(const size_t v, const size_t a) { return (v + a - 1) / a * a; }

// the plans of a call live in the context's batch_plan (it grows to the largest batch); nullptr: no memory
template <typename Plan> Plan *take_plans(Dav1dHipContext *const c, const int n)
{
    try {
        if (c->batch_plan.size() < (size_t) n * sizeof(Plan) + alignof(Plan)) c->batch_plan.resize((size_t) n * sizeof(Plan) + alignof(Plan));
    } catch (...) {
        return nullptr;
    }
    return (Plan *) round_up((size_t) (uintptr_t) c->batch_plan.data(), alignof(Plan));
}

// The front of a batch entry point, in the order the header promises: the count; `whole_rc`, what the call as a whole refuses (its filter, a missing
// handle); the empty batch; the arrays; then per item check(i, plan) — the family's checks and pictures_on_device — and the rule of one kernel
// instance for the batch: format and sample are item 0's, and with `same_pixel` the pixel size (the colour-managed batch checks the depth itself, against
// its handle).  *plans: the checked plans, nullptr where there is nothing to run (the call then returns what this returns).
template <typename Plan, typename Check>
int batch_plans(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src, const int whole_rc,
                const bool same_pixel, int *const bad_item, Plan **const plans, Check &&check)
{
    *plans = nullptr;
    if (bad_item) *bad_item = -1;
    if (!c || n < 0 || n > DAV1D_HIP_SURFACE_BATCH_MAX) return -EINVAL;
    if (whole_rc) return whole_rc;
    if (!n) return 0;
    if (!dst || !src) return -EINVAL;
    for (int i = 0; i < n; i++)
        if (!src[i]) { if (bad_item) *bad_item = i; return -EINVAL; }
    Plan *const plan = take_plans<Plan>(c, n);
    if (!plan) return -ENOMEM;
    for (int i = 0; i < n; i++) {
        int rc = check(i, plan[i]);
        if (!rc && (dst[i].format != dst[0].format || dst[i].sample != dst[0].sample || (same_pixel && (src[i]->bpc == 8) != (src[0]->bpc == 8)))) rc = -EINVAL;
        if (rc) { if (bad_item) *bad_item = i; return rc; }
    }
    *plans = plan;
    return 0;
}

// a staging slot of at least `bytes`, free to be written: the one used longest ago, waited for if its batch has not run yet
inline int batch_stage_take(Dav1dHipContext *const c, const size_t bytes, Dav1dHipContext::BatchStage **const out)
{
    Dav1dHipContext::BatchStage &s = c->batch_stage[c->batch_next++ % Dav1dHipContext::N_BATCH_STAGE];
    if (!s.made) {
        HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        s.made = true;
    }
    if (s.busy) {
        HIP_TRY(hipEventSynchronize(s.done));
        s.busy = false;
    }
    if (s.cap < bytes) {
        if (s.host) c->batch_retired_host.push_back(s.host);
        if (s.dev) c->batch_retired_dev.push_back(s.dev);
        s.host = s.dev = nullptr; s.cap = 0;
        size_t want = 1 << 14;
        while (want < bytes) want <<= 1;
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, want, hipHostMallocDefault));
        const hipError_t e = hipMalloc(&d, want);
        if (e != hipSuccess) { (void) hipHostFree(h); return hip_rc(e); }
        s.host = (uint8_t *) h; s.dev = (uint8_t *) d; s.cap = want;
    }
    *out = &s;
    return 0;
}

// The table of a batched launch, from its staging slot to the events behind the launches.  The items are sorted by class (cls(i) < NCLS: the kernel
// instance that exports item i), each class with a prefix of its own:
//     [ items of class 0, 1, .. | first: n_cls[0] + 1 words, n_cls[1] + 1 words, .. | extra, from a multiple of 16 bytes ]
// open, fill, run, in that order; whatever the caller puts into extra() goes between open and run.
template <typename Item, int NCLS, typename Classify> struct BatchTable {
    Dav1dHipContext *const c;
    const int n;
    const Classify cls;
    Dav1dHipContext::BatchStage *s;
    size_t first_at, extra_at, bytes;
    int n_cls[NCLS], slice0[NCLS], first0[NCLS];

    Item *items() const { return (Item *) s->host; }
    uint32_t *first() const { return (uint32_t *) (s->host + first_at); }
    uint8_t *extra() const { return s->host + extra_at; }

    int open(const size_t extra_bytes)
    {
        for (int t = 0; t < NCLS; t++) n_cls[t] = 0;
        for (int i = 0; i < n; i++) n_cls[cls(i)]++;
        for (int t = 0, at = 0; t < NCLS; at += n_cls[t++]) { slice0[t] = at; first0[t] = at + t; }
        first_at = (size_t) n * sizeof(Item);
        extra_at = first_at + (size_t) (n + NCLS) * sizeof(uint32_t);
        if (extra_bytes) extra_at = round_up(extra_at, 16);
        bytes = extra_at + extra_bytes;
        return batch_stage_take(c, bytes, &s);
    }
    // fill(i, class, item) writes the record of item i and returns what it counts, workgroups or cells; returns the count of all
    template <typename Fill> unsigned fill(Fill &&fill)
    {
        int k[NCLS] = {};
        unsigned total = 0;
        for (int i = 0; i < n; i++) {
            const int t = cls(i), at = k[t]++;
            const unsigned count = fill(i, t, items()[slice0[t] + at]);
            first()[first0[t] + at] = count;
            total += count;
        }
        return total;
    }
    // The prefixes (a workgroup per `per` of what an item counted), the upload, and between the timing events before(extra on the device) and
    // launch(class, its items, its prefix, its items' number, its workgroups) for every class that has any; the slot is busy until they ran.
    template <typename Before, typename Launch> int run(const unsigned per, Before &&before, Launch &&launch)
    {
        uint32_t groups[NCLS];
        for (int t = 0; t < NCLS; t++) {
            uint32_t *const f = first() + first0[t];
            groups[t] = 0;
            for (int j = 0; j < n_cls[t]; j++) {
                const uint32_t ng = (f[j] + per - 1) / per;
                f[j] = groups[t];
                groups[t] += ng;
            }
            f[n_cls[t]] = groups[t];
        }
        HIP_TRY(hipMemcpyAsync(s->dev, s->host, bytes, hipMemcpyHostToDevice, c->stream));
        const CallTimer timer(c);
        int rc = before((const uint8_t *) s->dev + extra_at);
        for (int t = 0; t < NCLS; t++) {
            if (!groups[t] || rc) continue;
            launch(t, (const Item *) s->dev + slice0[t], (const uint32_t *) (s->dev + first_at) + first0[t], n_cls[t], groups[t]);
            rc = hip_rc(hipGetLastError());
        }
        timer.done(rc);
        (void) hipEventRecord(s->done, c->stream);
        s->busy = true;
        return rc;
    }
};
template <typename Item, int NCLS, typename Classify> BatchTable<Item, NCLS, Classify> batch_table(Dav1dHipContext *const c, const int n, const Classify cls)
{
    return BatchTable<Item, NCLS, Classify>{ c, n, cls };
}

// the record of an item of the scaled, resized and reduced batches, and its workgroups
template <typename pixel, typename Out>
unsigned rgbx_item_fill(BatchItem<Out> &it, const bool tiled, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                        const ScaleGeom &g, const Dav1dHipRgbParams &p, const int row0, const int row1)
{
    unsigned ng;
    it.a = tiled ? make_scale_rgbx_args<pixel, true, typename Out::T>(dst, src, planes, g, p, row0, row1, &ng)
                 : make_scale_rgbx_args<pixel, false, typename Out::T>(dst, src, planes, g, p, row0, row1, &ng);
    it.out = Out();
    set_out(it.out, p, src->bpc);
    return ng;
}

// ... and the launch of a class of them: raster sources, or twin-only ones
template <typename pixel, typename Out, bool RESIZE>
void launch_rgbx_batch(hipStream_t st, const bool tiled, const BatchItem<Out> *const items, const uint32_t *const first, const int n, const uint32_t groups)
{
    const dim3 grid(groups), wg(256);
    if constexpr (RESIZE) {
        if (tiled) hipLaunchKernelGGL((surface_resize_rgbx_batch_kernel<pixel, true, Out>), grid, wg, 0, st, items, first, n);
        else hipLaunchKernelGGL((surface_resize_rgbx_batch_kernel<pixel, false, Out>), grid, wg, 0, st, items, first, n);
    } else {
        if (tiled) hipLaunchKernelGGL((surface_scale_rgbx_batch_kernel<pixel, true, Out>), grid, wg, 0, st, items, first, n);
        else hipLaunchKernelGGL((surface_scale_rgbx_batch_kernel<pixel, false, Out>), grid, wg, 0, st, items, first, n);
    }
}

// dav1d_hip_surface_export_rgb_scaled_batch (RESIZE false) and dav1d_hip_surface_export_rgb_resized_batch (true: an item may go up)
template <bool RESIZE>
int export_batch_call(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src,
                      const Dav1dHipSurfaceRect *const crop, const Dav1dHipRgbParams *const params, const int whole_rc, int *const bad_item)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    BatchPlan *plan;
    const int rc = batch_plans(c, n, dst, src, whole_rc, true, bad_item, &plan, [&](const int i, BatchPlan &pl) {
        const int rc = rgbx_scaled_args_check(&dst[i], src[i], crop ? &crop[i] : nullptr, p, 0, dst[i].h, &pl.call, &pl.g, RESIZE);
        return rc ? rc : pictures_on_device(c, src[i], 1);
    });
    if (!plan) return rc;
    return with_pixel(src[0]->bpc, [&](auto px) {
        typedef decltype(px) pixel;
        return with_rgb_out<pixel>(dst[0].sample, p, src[0]->bpc, [&](const auto &o) {          // (the type: every item gets the functor of its own depth)
            typedef std::decay_t<decltype(o)> Out;
            typedef BatchItem<Out> Item;
            auto tb = batch_table<Item, 2>(c, n, [&](const int i) { return (int) plan[i].call.tiled; });          // raster items, then twin-only ones
            if (const int rc = tb.open(0)) return rc;
            tb.fill([&](const int i, const int t, Item &it) {
                return rgbx_item_fill<pixel>(it, t, &dst[i], src[i], plan[i].call.planes, plan[i].g, p, plan[i].call.row0, plan[i].call.row1);
            });
            return tb.run(1, [](const uint8_t *) { return 0; }, [&](const int t, const Item *const items, const uint32_t *const first, const int n_t, const uint32_t groups) {
                launch_rgbx_batch<pixel, Out, RESIZE>(c->stream, t, items, first, n_t, groups);
            });
        });
    });
}

} // namespace
