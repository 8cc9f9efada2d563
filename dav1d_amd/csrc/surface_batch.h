// The batched scaled tensor-ready export behind its two entry points (surface_batch.hip has the account of the table, the search, the picture
// states and the staging ring; surface_resize.hip runs the same from its own entry point, with the body that lets an axis go up).
#pragma once
#include "surface_common.h"

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

template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256) void surface_scale_rgbx_batch_kernel(const BatchItem<Out> *const __restrict__ items, const uint32_t *const __restrict__ first,
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
    scale_rgbx_cell<pixel, TILED, Out>(L, a, (int) (g - first[lo]), it.out);
}

// the same search in front of the resizing body (surface_resize.hip: an axis of an item may go up); a kernel of its own, so that the one above
// keeps its code to the register
template <typename pixel, bool TILED, typename Out>
__global__ __launch_bounds__(256, sizeof(pixel) == 1 ? 5 : 4) void surface_resize_rgbx_batch_kernel(const BatchItem<Out> *const __restrict__ items, const uint32_t *const __restrict__ first,
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

template <typename pixel, typename Out, bool RESIZE>
int export_batch(Dav1dHipContext *const c, const int n, const int n_raster, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src,
                 const BatchPlan *const plan, const Dav1dHipRgbParams &p)
{
    typedef BatchItem<Out> Item;
    // records: the raster items, then the twin-only ones; behind them the two prefixes
    const size_t first_at = (size_t) n * sizeof(Item), bytes = first_at + (size_t) (n + 2) * sizeof(uint32_t);
    Dav1dHipContext::BatchStage *s;
    if (const int rc = batch_stage_take(c, bytes, &s)) return rc;
    Item *const items = (Item *) s->host;
    uint32_t *const first = (uint32_t *) (s->host + first_at);
    const int n_slice[2] = { n_raster, n - n_raster }, slice0[2] = { 0, n_raster }, first0[2] = { 0, n_raster + 1 };
    int fill[2] = { 0, 0 };
    uint32_t groups[2] = { 0, 0 };
    for (int i = 0; i < n; i++) {
        const SurfaceCall &call = plan[i].call;
        const ScaleGeom &g = plan[i].g;
        const int t = call.tiled, k = fill[t]++;
        Item &it = items[slice0[t] + k];
        unsigned ng;
        it.a = t ? make_scale_rgbx_args<pixel, true, typename Out::T>(&dst[i], src[i], call.planes, g, p, call.row0, call.row1, &ng)
                 : make_scale_rgbx_args<pixel, false, typename Out::T>(&dst[i], src[i], call.planes, g, p, call.row0, call.row1, &ng);
        it.out = Out();
        set_out(it.out, p, src[i]->bpc);
        first[first0[t] + k] = groups[t];
        groups[t] += ng;
    }
    for (int t = 0; t < 2; t++) first[first0[t] + n_slice[t]] = groups[t];
    HIP_TRY(hipMemcpyAsync(s->dev, s->host, bytes, hipMemcpyHostToDevice, c->stream));
    const Item *const d_items = (const Item *) s->dev;
    const uint32_t *const d_first = (const uint32_t *) (s->dev + first_at);
    (void) hipEventRecord(c->ev_t0, c->stream);
    int rc = 0;
    if (n_slice[0]) {
        if constexpr (RESIZE) hipLaunchKernelGGL((surface_resize_rgbx_batch_kernel<pixel, false, Out>), dim3(groups[0]), dim3(256), 0, c->stream, d_items, d_first, n_slice[0]);
        else hipLaunchKernelGGL((surface_scale_rgbx_batch_kernel<pixel, false, Out>), dim3(groups[0]), dim3(256), 0, c->stream, d_items, d_first, n_slice[0]);
        rc = hip_rc(hipGetLastError());
    }
    if (n_slice[1] && !rc) {
        if constexpr (RESIZE) hipLaunchKernelGGL((surface_resize_rgbx_batch_kernel<pixel, true, Out>), dim3(groups[1]), dim3(256), 0, c->stream, d_items + slice0[1], d_first + first0[1],
                                                 n_slice[1]);
        else hipLaunchKernelGGL((surface_scale_rgbx_batch_kernel<pixel, true, Out>), dim3(groups[1]), dim3(256), 0, c->stream, d_items + slice0[1], d_first + first0[1],
                                n_slice[1]);
        rc = hip_rc(hipGetLastError());
    }
    (void) hipEventRecord(c->ev_t1, c->stream);
    (void) hipEventRecord(s->done, c->stream);
    s->busy = true;
    c->last_ms_pending = !rc;
    return rc;
}

template <typename pixel, bool RESIZE>
int export_batch_sample(Dav1dHipContext *const c, const int n, const int n_raster, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src,
                        const BatchPlan *const plan, const Dav1dHipRgbParams &p)
{
    if (dst[0].sample == DAV1D_HIP_SAMPLE_F32) return export_batch<pixel, RgbF32, RESIZE>(c, n, n_raster, dst, src, plan, p);
    if (dst[0].sample == DAV1D_HIP_SAMPLE_F16) return export_batch<pixel, RgbF16, RESIZE>(c, n, n_raster, dst, src, plan, p);
    if constexpr (sizeof(pixel) == 2) {
        if (dst[0].sample == DAV1D_HIP_SAMPLE_MSB16) return export_batch<pixel, RgbInt<OutMsb16>, RESIZE>(c, n, n_raster, dst, src, plan, p);
    }
    return export_batch<pixel, RgbInt<OutNative<pixel>>, RESIZE>(c, n, n_raster, dst, src, plan, p);
}

// dav1d_hip_surface_export_rgb_scaled_batch (RESIZE false) and dav1d_hip_surface_export_rgb_resized_batch (true: an item may go up)
template <bool RESIZE>
int export_batch_call(Dav1dHipContext *const c, const int n, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const *const src,
                      const Dav1dHipSurfaceRect *const crop, const Dav1dHipRgbParams *const params, int *const bad_item)
{
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    if (params) p = *params;
    if (bad_item) *bad_item = -1;
    if (!c || n < 0 || n > DAV1D_HIP_SURFACE_BATCH_MAX) return -EINVAL;
    if (!n) return 0;
    if (!dst || !src) return -EINVAL;
    for (int i = 0; i < n; i++)
        if (!src[i]) { if (bad_item) *bad_item = i; return -EINVAL; }
    try {
        if (c->batch_plan.size() < (size_t) n * sizeof(BatchPlan)) c->batch_plan.resize((size_t) n * sizeof(BatchPlan));
    } catch (...) {
        return -ENOMEM;
    }
    BatchPlan *const plan = (BatchPlan *) c->batch_plan.data();
    int n_raster = 0;
    for (int i = 0; i < n; i++) {
        SurfaceCall &call = plan[i].call;
        int rc = rgbx_scaled_args_check(&dst[i], src[i], crop ? &crop[i] : nullptr, p, 0, dst[i].h, &call, &plan[i].g, RESIZE);
        if (!rc) rc = pictures_on_device(c, src[i], 1);
        // one kernel instance for the batch: format, sample and pixel size are item 0's
        if (!rc && (dst[i].format != dst[0].format || dst[i].sample != dst[0].sample || (src[i]->bpc == 8) != (src[0]->bpc == 8))) rc = -EINVAL;
        if (rc) { if (bad_item) *bad_item = i; return rc; }
        n_raster += !call.tiled;
    }
    return src[0]->bpc == 8 ? export_batch_sample<uint8_t, RESIZE>(c, n, n_raster, dst, src, plan, p) : export_batch_sample<uint16_t, RESIZE>(c, n, n_raster, dst, src, plan, p);
}

} // namespace
