// Host side of the C ABI: the *_batch calls of CDEF, deblocking, warped and scaled motion compensation, resize, emu_edge, loop restoration, film grain.
#include "capi.h"
#include <string.h>
#include <new>
#include <algorithm>

// --------------------------------------------------------------------- cdef

int dav1d_hip_cdef_run_groups(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src, const Dav1dHipCdefTask *tasks,
                              size_t n, const CdefGroup *groups, size_t n_groups, size_t n_raw, int damping, uint32_t *dirvar) {
    if (!raster_dst_ok(dst)) return -EINVAL;
    if (const int rv_ = raster_planes_valid(c, src, 1)) return rv_;      // (a source that lives in its tiled twin only: raster planes first)
    const size_t tb = (n * sizeof(Dav1dHipCdefTask) + 255) & ~(size_t) 255;
    TaskBuf dev_buf(c, tb + n_groups * sizeof(CdefGroup) + 256);
    uint8_t *const dev = reinterpret_cast<uint8_t *>(dev_buf.p);
    if (!dev) return -ENOMEM;
    int rc = dav1d_hip_upload(c, dev, tasks, n * sizeof(Dav1dHipCdefTask));
    if (!rc && n_groups) rc = dav1d_hip_upload(c, dev + tb, groups, n_groups * sizeof(CdefGroup));
    const DevPlanes dp = dev_planes(dst), sp = dev_planes(src);
    const Dav1dHipCdefTask *d_tasks = reinterpret_cast<const Dav1dHipCdefTask *>(dev);
    KernelTimer kt(c);
    if (!rc) rc = dav1d_hip_launch_cdef_groups(&dp, &sp, dst->bpc, dst->layout, d_tasks, reinterpret_cast<const CdefGroup *>(dev + tb),
                                               (int) n_groups, damping, dirvar, c->stream);
    if (!rc && n_raw) rc = dav1d_hip_launch_cdef(&dp, &sp, dst->bpc, dst->layout, d_tasks, (int) n, damping, dirvar, 1, c->stream);
    kt.stop();
    hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" int dav1d_hip_cdef_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src,
                                    const Dav1dHipCdefTask *tasks, size_t n, int damping, uint32_t *dirvar) {
    if (!raster_dst_ok(dst) || !src || (!tasks && n) || dst->bpc != src->bpc || dst->layout != src->layout) return -EINVAL;
    if (!n) return 0;
    // one pass over the list (half a million units per 8K frame): the field checks as one OR-reduction
    unsigned bad = 0;
    for (size_t i = 0; i < n; i++) bad |= (unsigned) (tasks[i].edges > 15) | (unsigned) (tasks[i].plane > 2) | (unsigned) (tasks[i].dir > 7);
    if (bad) return -EINVAL;
    if (const int rv_ = raster_planes_valid(c, src, 1)) return rv_;      // (a source that lives in its tiled twin only: raster planes first)
    const DevPlanes dp = dev_planes(dst), sp = dev_planes(src);
    if (dav1d_hip_cdef_strip_ok(&dp, &sp, dst->bpc) && !c->cdef_unit_kernel) {
        // units that sit side by side share a wave (strip kernel); DSP-level RAW tasks keep the one-unit kernel
        std::vector<CdefGroup> groups;
        groups.reserve(n / 8 + 16);
        const size_t n_raw = dav1d_hip_cdef_make_groups(tasks, n, 0, groups);
        return dav1d_hip_cdef_run_groups(c, dst, src, tasks, n, groups.data(), groups.size(), n_raw, damping, dirvar);
    }
    TaskBuf dev_buf(c, n * sizeof(Dav1dHipCdefTask));
    Dav1dHipCdefTask *const dev = reinterpret_cast<Dav1dHipCdefTask *>(dev_buf.p);
    if (!dev) return -ENOMEM;
    int rc = dav1d_hip_upload(c, dev, tasks, n * sizeof(*dev));
    KernelTimer kt(c);
    if (!rc) rc = dav1d_hip_launch_cdef(&dp, &sp, dst->bpc, dst->layout, dev, (int) n, damping, dirvar, 0, c->stream);
    kt.stop();
    hipStreamSynchronize(c->stream);
    return rc;
}

// -------------------------------------------------------------- loop filter

extern "C" int dav1d_hip_lf_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipLfTask *tasks, size_t n,
                                  const uint8_t *lvl, ptrdiff_t b4_stride, const uint8_t lut_e[64], const uint8_t lut_i[64]) {
    if (!raster_dst_ok(dst) || (!tasks && n) || !lvl || !lut_e || !lut_i) return -EINVAL;
    if (!n) return 0;
    std::vector<Dav1dHipLfTask> sorted;
    sorted.reserve(n);
    size_t n0 = 0;
    for (int d = 0; d < 2; d++) {
        for (size_t i = 0; i < n; i++) {
            if (tasks[i].plane > 2 || tasks[i].dir > 1 || tasks[i].lvl_comp > 3) return -EINVAL;
            if (tasks[i].dir == d) sorted.push_back(tasks[i]);
        }
        if (d == 0) n0 = sorted.size();
    }
    TaskBuf dev_buf(c, n * sizeof(Dav1dHipLfTask));
    Dav1dHipLfTask *const dev = reinterpret_cast<Dav1dHipLfTask *>(dev_buf.p);
    if (!dev) return -ENOMEM;
    int rc = dav1d_hip_upload(c, dev, sorted.data(), n * sizeof(*dev));
    const DevPlanes dp = dev_planes(dst);
    // pass 1: every vertical edge; pass 2 (same stream, so after pass 1): every horizontal edge
    KernelTimer kt(c);
    if (!rc) rc = dav1d_hip_launch_lf(&dp, dst->bpc, 0, dev, (int) n0, lvl, (int) b4_stride, lut_e, lut_i, c->stream);
    if (!rc) rc = dav1d_hip_launch_lf(&dp, dst->bpc, 1, dev + n0, (int) (n - n0), lvl, (int) b4_stride, lut_e, lut_i, c->stream);
    kt.stop();
    hipStreamSynchronize(c->stream);
    return rc;
}

// ------------------------------------------------- mc: warp, scaled, resize, emu_edge

template <typename T, typename Launch>
static int run_task_batch(Dav1dHipContext *c, const T *tasks, size_t n, Launch launch) {
    TaskBuf dev_buf(c, n * sizeof(T));
    T *const dev = reinterpret_cast<T *>(dev_buf.p);
    if (!dev) return -ENOMEM;
    int rc = dav1d_hip_upload(c, dev, tasks, n * sizeof(T));
    if (!rc) rc = launch(dev);
    hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" int dav1d_hip_warp_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *refs, int n_refs,
                                    const Dav1dHipWarpTask *tasks, size_t n, int16_t *prep) {
    if (!raster_dst_ok(dst) || !refs || n_refs < 1 || n_refs > 8 || (!tasks && n)) return -EINVAL;
    if (!n) return 0;
    for (size_t i = 0; i < n; i++) {
        const Dav1dHipWarpTask &t = tasks[i];
        if (t.kind > DAV1D_HIP_MC_PREP || t.plane > 2 || t.ref >= n_refs) return -EINVAL;
        if (t.kind == DAV1D_HIP_MC_PREP && !prep) return -EINVAL;
    }
    DevPlanes rp[8];
    if (const int rv = raster_planes_valid(c, refs, n_refs)) return rv;          // (the warp kernels read raster planes)
    for (int i = 0; i < n_refs; i++) { if (refs[i].bpc != dst->bpc) return -EINVAL; rp[i] = dev_planes(&refs[i]); }
    const DevPlanes dp = dev_planes(dst);
    return run_task_batch(c, tasks, n, [&](const Dav1dHipWarpTask *dev) {
        return dav1d_hip_launch_warp(&dp, rp, n_refs, dst->bpc, dev, (int) n, prep, c->stream); });
}

extern "C" int dav1d_hip_mc_scaled_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *refs, int n_refs,
                                         const Dav1dHipMcScaledTask *tasks, size_t n, int16_t *prep) {
    if (!raster_dst_ok(dst) || !refs || n_refs < 1 || n_refs > 8 || (!tasks && n)) return -EINVAL;
    if (!n) return 0;
    for (size_t i = 0; i < n; i++) {
        const Dav1dHipMcScaledTask &t = tasks[i];
        if (t.kind > DAV1D_HIP_MC_PUT_TMP || t.plane > 2 || t.ref >= n_refs || t.filter_2d > 9) return -EINVAL;
        if (t.w < 2 || t.w > 128 || t.h < 2 || t.h > 128 || t.mx < 0 || t.mx > 1023 || t.my < 0 || t.my > 1023 || t.dx < 0 || t.dy < 0)
            return -EINVAL;
        if (t.kind != DAV1D_HIP_MC_PUT && !prep) return -EINVAL;
    }
    DevPlanes rp[8];
    if (const int rv = raster_planes_valid(c, refs, n_refs)) return rv;          // (so do the scaled ones)
    for (int i = 0; i < n_refs; i++) { if (refs[i].bpc != dst->bpc) return -EINVAL; rp[i] = dev_planes(&refs[i]); }
    const DevPlanes dp = dev_planes(dst);
    return run_task_batch(c, tasks, n, [&](const Dav1dHipMcScaledTask *dev) {
        return dav1d_hip_launch_mc_scaled(&dp, rp, n_refs, dst->bpc, dev, (int) n, prep, c->stream); });
}

extern "C" int dav1d_hip_resize(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src, int plane, int dst_w, int y0,
                                int h, int src_w, int dx, int mx0) {
    if (!raster_dst_ok(dst) || !src || dst->bpc != src->bpc || plane < 0 || plane > 2 || dst_w < 1 || src_w < 1 || h < 0 || y0 < 0) return -EINVAL;
    if (mx0 < 0 || mx0 > 0x3fff || dx < 0) return -EINVAL;
    if (!h) return 0;
    if (const int rv_ = raster_planes_valid(c, src, 1)) return rv_;      // (a source that lives in its tiled twin only: raster planes first)
    const DevPlanes dp = dev_planes(dst), sp = dev_planes(src);
    if (y0 + h > dp.h[plane] || y0 + h > sp.h[plane] || dst_w > dp.w[plane]) return -EINVAL;
    const int rc = dav1d_hip_launch_resize(&dp, &sp, dst->bpc, plane, dst_w, y0, h, src_w, dx, mx0, c->stream);
    hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" int dav1d_hip_emu_edge(Dav1dHipContext *c, int bpc, intptr_t bw, intptr_t bh, intptr_t iw, intptr_t ih, intptr_t x, intptr_t y,
                                  void *dst, ptrdiff_t dst_stride, const void *ref, ptrdiff_t ref_stride) {
    if (!dst || !ref || bw < 1 || bh < 1 || iw < 1 || ih < 1 || (bpc != 8 && bpc != 10 && bpc != 12)) return -EINVAL;
    const int rc = dav1d_hip_launch_emu_edge(dst, dst_stride, ref, ref_stride, (int) bw, (int) bh, (int) iw, (int) ih, (int) x, (int) y, bpc,
                                             c->stream);
    hipStreamSynchronize(c->stream);
    return rc;
}

// --------------------------------------------------------- loop restoration

extern "C" int dav1d_hip_lr_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src,
                                  const Dav1dHipPicture *lpf, const Dav1dHipLrTask *tasks, size_t n) {
    if (!raster_dst_ok(dst) || !src || !lpf || (!tasks && n) || dst->bpc != src->bpc || lpf->bpc != src->bpc) return -EINVAL;
    if (!n) return 0;
    for (size_t i = 0; i < n; i++) {
        const Dav1dHipLrTask &t = tasks[i];
        if (t.plane > 2 || t.edges > 15 || !t.w || t.w > 384 || !t.h || t.h > 64) return -EINVAL;
        if (t.type > DAV1D_HIP_LR_SGR_MIX) return -EINVAL;
    }
    // (a source or a row store that lives in its tiled twin only: raster planes first, before anything is uploaded)
    if (const int rv_ = raster_planes_valid(c, src, 1)) return rv_;
    if (const int rv_ = raster_planes_valid(c, lpf, 1)) return rv_;
    // Wiener tasks first, self-guided tasks second: one launch each (tasks write disjoint stripes)
    std::vector<Dav1dHipLrTask> sorted;
    sorted.reserve(n);
    for (size_t i = 0; i < n; i++) if (tasks[i].type <= DAV1D_HIP_LR_WIENER5) sorted.push_back(tasks[i]);
    const size_t nw = sorted.size();
    for (size_t i = 0; i < n; i++) if (tasks[i].type > DAV1D_HIP_LR_WIENER5) sorted.push_back(tasks[i]);
    // self-guided: the units of a row share waves (lr.hip)
    std::vector<uint32_t> waves;
    dav1d_hip_sgr_make_rows(sorted.data() + nw, n - nw, waves);
    const size_t o_waves = (n * sizeof(Dav1dHipLrTask) + 15) & ~(size_t) 15;
    TaskBuf devb_buf(c, o_waves + waves.size() * 4 + 16);
    uint8_t *const devb = reinterpret_cast<uint8_t *>(devb_buf.p);
    if (!devb) return -ENOMEM;
    Dav1dHipLrTask *const dev = reinterpret_cast<Dav1dHipLrTask *>(devb);
    int rc = dav1d_hip_upload(c, dev, sorted.data(), n * sizeof(*dev));
    if (!rc && !waves.empty()) rc = dav1d_hip_upload(c, devb + o_waves, waves.data(), waves.size() * 4);
    const DevPlanes dp = dev_planes(dst), sp = dev_planes(src), lp = dev_planes(lpf);
    KernelTimer kt(c);
    int max_w = 0;
    for (size_t i = 0; i < nw; i++) max_w = std::max(max_w, (int) sorted[i].w);
    if (!rc) rc = dav1d_hip_launch_wiener(&dp, &sp, &lp, dst->bpc, dev, (int) nw, max_w, c->stream);
    if (!rc) rc = dav1d_hip_launch_sgr(&dp, &sp, &lp, dst->bpc, dev + nw, devb + o_waves, (int) (waves.size() / 4), c->stream);
    kt.stop();
    hipStreamSynchronize(c->stream);
    return rc;
}

// --------------------------------------------------------------- film grain

// generate_scaling, reference src/fg_apply_tmpl.c:41-95 (piecewise-linear LUT over the scaling points;
// high bit depth interpolates between the 8-bit grid points)
static void fg_generate_scaling(const int bitdepth, const uint8_t points[][2], const int num, uint8_t *scaling) {
    const int shift_x = bitdepth - 8, scaling_size = 1 << bitdepth;
    if (num == 0) { memset(scaling, 0, scaling_size); return; }
    memset(scaling, points[0][1], (size_t) points[0][0] << shift_x);
    for (int i = 0; i < num - 1; i++) {
        const int bx = points[i][0], by = points[i][1], ex = points[i + 1][0], ey = points[i + 1][1];
        const int dx = ex - bx, dy = ey - by;
        const int delta = dy * ((0x10000 + (dx >> 1)) / dx);
        for (int x = 0, d = 0x8000; x < dx; x++) { scaling[(bx + x) << shift_x] = (uint8_t) (by + (d >> 16)); d += delta; }
    }
    const int n = points[num - 1][0] << shift_x;
    memset(&scaling[n], points[num - 1][1], scaling_size - n);
    if (shift_x) {
        const int pad = 1 << shift_x, rnd = pad >> 1;
        for (int i = 0; i < num - 1; i++) {
            const int bx = points[i][0] << shift_x, ex = points[i + 1][0] << shift_x, dx = ex - bx;
            for (int x = 0; x < dx; x += pad) {
                const int range = scaling[bx + x + pad] - scaling[bx + x];
                for (int k = 1, r = rnd; k < pad; k++) { r += range; scaling[bx + x + k] = (uint8_t) (scaling[bx + x] + (r >> shift_x)); }
            }
        }
    }
}

extern "C" int dav1d_hip_fg_generate_grain(Dav1dHipContext *c, const Dav1dHipFilmGrainData *data, int bpc, int layout, int16_t *host_lut) {
    if (!data || !host_lut || (bpc != 8 && bpc != 10 && bpc != 12)) return -EINVAL;
    const size_t bytes = 3 * 74 * 82 * sizeof(int16_t);
    TaskBuf dev_buf(c, bytes);
    int16_t *const dev = reinterpret_cast<int16_t *>(dev_buf.p);
    if (!dev) return -ENOMEM;
    hipMemsetAsync(dev, 0, bytes, c->stream);
    int rc = dav1d_hip_launch_fg_gen(dev, data, bpc, layout, c->stream);
    if (!rc) rc = dav1d_hip_download(c, host_lut, dev, bytes);
    return rc;
}

// Grain templates + scaling tables of one frame (dav1d_prep_grain, src/fg_apply_tmpl.c:97-163 up to the row loop): they depend
// on the frame header only, so they are generated on a side stream as soon as the parameters are known — a lone wave per
// template, ~0.23 ms of latency that then hides behind the reconstruction of the frame — and dav1d_hip_fg_apply_prepared
// (the dav1d_apply_grain_row part) only waits for their event.
static int fg_prepare_on(Dav1dHipContext *c, Dav1dHipGrain **out, const Dav1dHipFilmGrainData *data, int bpc, int layout, hipStream_t stream) {
    if (!c || !out || !data || (bpc != 8 && bpc != 10 && bpc != 12) || layout < 0 || layout > 3) return -EINVAL;
    *out = nullptr;
    Dav1dHipGrain *g = new (std::nothrow) Dav1dHipGrain();
    if (!g) return -ENOMEM;
    g->dev = nullptr; g->bpc = bpc; g->layout = layout; g->data = *data;
    g->scaling_size = (size_t) 1 << bpc;
    g->lut_bytes = (3 * 74 * 82 * sizeof(int16_t) + 255) & ~(size_t) 255;      // keeps the scaling tables 16-byte aligned
    g->side = stream;
    if (hipEventCreateWithFlags(&g->ready, hipEventDisableTiming) != hipSuccess) { delete g; return -ENOMEM; }
    if (hipMalloc((void **) &g->dev, g->lut_bytes + 3 * g->scaling_size) != hipSuccess) { hipEventDestroy(g->ready); delete g; return -ENOMEM; }
    g->sc.assign(3 * g->scaling_size, 0);
    if (data->num_y_points || data->chroma_scaling_from_luma) fg_generate_scaling(bpc, data->y_points, data->num_y_points, &g->sc[0]);
    for (int i = 0; i < 2; i++)
        if (data->num_uv_points[i]) fg_generate_scaling(bpc, data->uv_points[i], data->num_uv_points[i], &g->sc[(size_t) (1 + i) * g->scaling_size]);
    int rc = hip_rc(hipMemsetAsync(g->dev, 0, g->lut_bytes, g->side));
    if (!rc) rc = hip_rc(hipMemcpyAsync(g->dev + g->lut_bytes, g->sc.data(), g->sc.size(), hipMemcpyHostToDevice, g->side));
    if (!rc) rc = dav1d_hip_launch_fg_gen((int16_t *) g->dev, data, bpc, layout, g->side);
    if (!rc) rc = hip_rc(hipEventRecord(g->ready, g->side));
    if (rc) { hipStreamSynchronize(g->side); hipFree(g->dev); hipEventDestroy(g->ready); delete g; return rc; }
    *out = g;
    return 0;
}

extern "C" int dav1d_hip_fg_prepare(Dav1dHipContext *c, Dav1dHipGrain **out, const Dav1dHipFilmGrainData *data, int bpc, int layout) {
    if (!c) return -EINVAL;
    return fg_prepare_on(c, out, data, bpc, layout, c->concurrent ? c->side[Dav1dHipContext::N_SIDE - 1] : c->stream);
}

extern "C" void dav1d_hip_fg_grain_destroy(Dav1dHipContext *c, Dav1dHipGrain *g) {
    if (!g) return;
    hipStreamSynchronize(g->side);
    if (c) hipStreamSynchronize(c->stream);
    hipFree(g->dev);
    for (const Dav1dHipGrain::Offsets &o : g->offs) hipFree(o.dev);       // (the fused export's tables: surface_grain.hip)
    hipEventDestroy(g->ready);
    delete g;
}

// the application proper on the context's stream (no timing, no synchronisation); offs: scratch for the per-block offsets
static int fg_apply_core(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src, const Dav1dHipGrain *g, int is_id,
                         uint8_t *offs) {
    const Dav1dHipFilmGrainData *data = &g->data;
    const int bpc = src->bpc;
    // (a source that lives in its tiled twin only: raster planes first — the plane copies below read them as the kernel does)
    if (const int rv_ = raster_planes_valid(c, src, 1)) return rv_;
    int rc = 0;
    // planes that get no grain are copied (dav1d_prep_grain, src/fg_apply_tmpl.c:127-163)
    const int ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420;
    for (int pl = 0; pl < 3 && !rc; pl++) {
        if (pl && src->layout == DAV1D_HIP_LAYOUT_I400) break;
        const bool grain = pl ? (data->num_uv_points[pl - 1] || data->chroma_scaling_from_luma) : data->num_y_points != 0;
        if (grain) continue;
        const int rows = pl ? (src->p[0].h + ss_ver) >> ss_ver : src->p[0].h;
        const size_t rb = (size_t) src->p[pl].w * (bpc > 8 ? 2 : 1);
        rc = hip_rc(hipMemcpy2DAsync(dst->p[pl].data, dst->p[pl].stride, src->p[pl].data, src->p[pl].stride, rb, rows,
                                     hipMemcpyDeviceToDevice, c->stream));
    }
    const DevPlanes dp = dev_planes(dst), sp = dev_planes(src);
    if (!rc) rc = dav1d_hip_launch_fg_apply(&dp, &sp, (const int16_t *) g->dev, g->dev + g->lut_bytes, (int) g->scaling_size, data, bpc, src->layout,
                                            is_id, offs, c->stream);
    return rc;
}

// scratch for the per-block offsets of one application (fg_apply_core's offs): p is NULL when there is no memory
static TaskBuf fg_offsets_scratch(Dav1dHipContext *c, const Dav1dHipPicture *src) { return TaskBuf(c, (size_t) ((src->p[0].w + 31) / 32) * ((src->p[0].h + 31) / 32) + 16); }

static int fg_args_ok(const Dav1dHipPicture *dst, const Dav1dHipPicture *src) {
    return raster_dst_ok(dst) && src && dst->bpc == src->bpc && dst->layout == src->layout;
}

extern "C" int dav1d_hip_fg_apply_prepared(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src,
                                           const Dav1dHipGrain *g, int is_id) {
    if (!c || !g || !fg_args_ok(dst, src) || src->bpc != g->bpc || src->layout != g->layout) return -EINVAL;
    const TaskBuf offs_buf = fg_offsets_scratch(c, src);
    if (!offs_buf.p) return -ENOMEM;
    int rc = hip_rc(hipStreamWaitEvent(c->stream, g->ready, 0));
    KernelTimer kt(c);
    if (!rc) rc = fg_apply_core(c, dst, src, g, is_id, offs_buf.p);
    kt.stop();
    hipStreamSynchronize(c->stream);
    return rc;
}

// dav1d_apply_grain in one call: templates and application back to back on the context's stream
extern "C" int dav1d_hip_fg_apply(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *src,
                                  const Dav1dHipFilmGrainData *data, int is_id) {
    if (!c || !data || !fg_args_ok(dst, src)) return -EINVAL;
    const TaskBuf offs_buf = fg_offsets_scratch(c, src);
    if (!offs_buf.p) return -ENOMEM;
    Dav1dHipGrain *g = nullptr;
    KernelTimer kt(c);
    int rc = fg_prepare_on(c, &g, data, src->bpc, src->layout, c->stream);
    if (!rc) rc = fg_apply_core(c, dst, src, g, is_id, offs_buf.p);
    kt.stop();
    hipStreamSynchronize(c->stream);
    dav1d_hip_fg_grain_destroy(c, g);
    return rc;
}
