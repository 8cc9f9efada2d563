// Host side of the C ABI: pictures — allocation and the context's pool, tiled twins, host pictures, copies between devices, plane transfers.
#include "capi.h"
#include <string.h>

extern "C" {

int dav1d_hip_picture_alloc(Dav1dHipContext *c, Dav1dHipPicture *pic, int w, int h, int layout, int bpc) {
    if (!pic || w <= 0 || h <= 0 || (bpc != 8 && bpc != 10 && bpc != 12) || layout < 0 || layout > 3)
        return -EINVAL;
    // geometry of the reference's default allocator, src/picture.c:46-78
    const int hbd = bpc > 8;
    const int aligned_w = (w + 127) & ~127, aligned_h = (h + 127) & ~127;
    const int has_chroma = layout != DAV1D_HIP_LAYOUT_I400;
    const int ss_ver = layout == DAV1D_HIP_LAYOUT_I420;
    const int ss_hor = layout != DAV1D_HIP_LAYOUT_I444;
    ptrdiff_t y_stride = (ptrdiff_t) aligned_w << hbd;
    ptrdiff_t uv_stride = has_chroma ? y_stride >> ss_hor : 0;
    if (!(y_stride & 1023)) y_stride += 64;
    if (!(uv_stride & 1023) && has_chroma) uv_stride += 64;
    const size_t y_sz = (size_t) y_stride * aligned_h;
    const size_t uv_sz = (size_t) uv_stride * (aligned_h >> ss_ver);
    const size_t total = y_sz + 2 * uv_sz + 64;
    void *buf = nullptr;
    HIP_TRY(hipMalloc(&buf, total));
    HIP_TRY(hipMemsetAsync(buf, 0, total, c->stream));
    memset(pic, 0, sizeof(*pic));
    pic->alloc = buf;
    pic->alloc_size = total;
    pic->bpc = bpc;
    pic->layout = layout;
    pic->p[0].data = buf;
    pic->p[0].stride = y_stride;
    pic->p[0].w = w;
    pic->p[0].h = h;
    for (int i = 1; i < 3; i++) {
        pic->p[i].data = has_chroma ? (uint8_t *) buf + y_sz + (i - 1) * uv_sz : nullptr;
        pic->p[i].stride = uv_stride;
        pic->p[i].w = has_chroma ? (w + ss_hor) >> ss_hor : 0;
        pic->p[i].h = has_chroma ? (h + ss_ver) >> ss_ver : 0;
    }
    if (c->ref_twin >= 2) {
        const int rc = dav1d_hip_picture_twin_alloc(c, pic);
        if (rc) { (void) hipFree(buf); memset(pic, 0, sizeof(*pic)); return rc; }
    }
    return 0;
}

int dav1d_hip_picture_take(Dav1dHipContext *c, Dav1dHipPicture *pic, int w, int h, int layout, int bpc) {
    {
        std::lock_guard<std::mutex> lk(c->pool_mtx);
        for (size_t i = 0; i < c->free_pictures.size(); i++) {
            const Dav1dHipPicture &q = c->free_pictures[i];
            if (q.p[0].w == w && q.p[0].h == h && q.layout == layout && q.bpc == bpc && !q.twin_alloc == !(c->ref_twin >= 2)) {
                *pic = q;
                c->free_pictures[i] = c->free_pictures.back();
                c->free_pictures.pop_back();
                pic->twin_ok = 0;
                // as a fresh allocation would be: zero, padding included
                return hip_rc(hipMemsetAsync(pic->alloc, 0, pic->alloc_size, c->stream));
            }
        }
    }
    return dav1d_hip_picture_alloc(c, pic, w, h, layout, bpc);
}

void dav1d_hip_picture_give(Dav1dHipContext *c, Dav1dHipPicture *pic) {
    if (!pic->alloc) return;
    {
        std::lock_guard<std::mutex> lk(c->pool_mtx);
        if (c->free_pictures.size() < 16) { c->free_pictures.push_back(*pic); memset(pic, 0, sizeof(*pic)); return; }
    }
    (void) dav1d_hip_picture_free(c, pic);
}

extern "C" int dav1d_hip_launch_retile(const DevPlanes *src, void *const twin[3], int bpc, void *stream);

// Rows of plane pl that exist in memory: a plane of dav1d_hip_picture_alloc (and of dav1d's own allocator, src/picture.c:46-63) is padded to
// a multiple of 128 luma rows — blocks on the picture's bottom edge reconstruct into that padding — a caller-wrapped plane only promises its
// visible rows.
static inline int picture_plane_rows(const Dav1dHipPicture *pic, int pl, bool padded) {
    if (!padded) return pic->p[pl].h;
    const int ss_ver = pic->layout == DAV1D_HIP_LAYOUT_I420;
    const int ah = (pic->p[0].h + 127) & ~127;
    return pl ? ah >> ss_ver : ah;
}
// the picture's planes for the retile / untile passes: every row the allocation holds when the library made it
static inline DevPlanes twin_pass_planes(const Dav1dHipPicture *pic) {
    DevPlanes d = dev_planes(pic);
    for (int pl = 0; pl < 3; pl++) if (pic->p[pl].data) d.h[pl] = picture_plane_rows(pic, pl, pic->alloc != nullptr);
    return d;
}

// Storage for the tiled twin: per plane stride x (rows padded as dav1d's allocator pads them: blocks on the bottom edge write below the
// visible rows, in the twin as in the raster plane) bytes, the planes one after the other.
int dav1d_hip_picture_twin_alloc(Dav1dHipContext *c, Dav1dHipPicture *pic) {
    if (!c || !pic || !pic->p[0].data) return -EINVAL;
    if (pic->twin_alloc) return 0;
    const int bps = pic->bpc > 8 ? 2 : 1;
    size_t off[3] = { 0, 0, 0 }, total = 0;
    for (int i = 0; i < 3; i++) {
        if (!pic->p[i].data) continue;
        if (pic->p[i].stride <= 0 || (pic->p[i].stride / bps) % 8 || pic->p[i].stride % 16) return -EINVAL;
        off[i] = total;
        total += (size_t) pic->p[i].stride * (size_t) picture_plane_rows(pic, i, true);
        total = (total + 255) & ~(size_t) 255;
    }
    void *buf = nullptr;
    HIP_TRY(hipMalloc(&buf, total + 256));
    HIP_TRY(hipMemsetAsync(buf, 0, total + 256, c->stream));
    pic->twin_alloc = buf;
    for (int i = 0; i < 3; i++) pic->twin[i] = pic->p[i].data ? (uint8_t *) buf + off[i] : nullptr;
    pic->twin_ok = 0;
    return 0;
}

extern "C" int dav1d_hip_launch_untile(const DevPlanes *dst, void *const twin[3], int bpc, const int row0[3], const int row1[3], int plane_mask, void *stream);

// The same on a side stream of the context: the copy starts when the work enqueued so far is through and runs NEXT TO whatever the
// caller enqueues afterwards (the next frame's launches: they are bound by request latency and arithmetic, the copy by bandwidth).
// Launches of this context that read twins wait for it (ref_planes); dav1d_hip_sync does too.
int dav1d_hip_picture_retile_overlapped(Dav1dHipContext *c, Dav1dHipPicture *pic) {
    if (!c || !pic) return -EINVAL;
    if (!c->concurrent) return dav1d_hip_picture_retile(c, pic);
    if (const int rc = twin_on_demand(c, pic)) return rc;
    hipStream_t side = c->side[Dav1dHipContext::N_SIDE - 1];
    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(side, c->ev_fork, 0));
    if (pic->twin_ok == DAV1D_HIP_TWIN_ONLY) return 0;          // the twin IS the picture
    const DevPlanes sp = twin_pass_planes(pic);
    const int rc = dav1d_hip_launch_retile(&sp, pic->twin, pic->bpc, side);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_retile, side));
    c->retile_pending = true;
    pic->twin_ok = 1;
    return 0;
}

int dav1d_hip_picture_retile(Dav1dHipContext *c, Dav1dHipPicture *pic) {
    if (!c || !pic) return -EINVAL;
    if (const int rc = twin_on_demand(c, pic)) return rc;
    if (pic->twin_ok == DAV1D_HIP_TWIN_ONLY) return 0;          // the twin IS the picture
    const DevPlanes sp = twin_pass_planes(pic);
    const int rc = dav1d_hip_launch_retile(&sp, pic->twin, pic->bpc, c->stream);
    if (!rc) pic->twin_ok = 1;
    return rc;
}

// The other way: a picture that lives in its twin only (twin_ok == DAV1D_HIP_TWIN_ONLY: what dav1d_hip_recon_list_run_tiled leaves) gets
// its raster planes back, on the context's stream; twin_ok becomes 1 (both valid).  No-op for any other picture.
int dav1d_hip_picture_untile(Dav1dHipContext *c, Dav1dHipPicture *pic) {
    if (!c || !pic) return -EINVAL;
    if (pic->twin_ok != DAV1D_HIP_TWIN_ONLY) return 0;
    if (!pic->twin[0]) return -EINVAL;
    const DevPlanes dp = twin_pass_planes(pic);
    const int rc = dav1d_hip_launch_untile(&dp, pic->twin, pic->bpc, nullptr, nullptr, 7, c->stream);
    if (!rc) pic->twin_ok = 1;
    return rc;
}

// Host side of a Dav1dPicAllocator: pinned planes with the geometry of the device picture (= the reference's default allocator,
// src/picture.c:46-82)
int dav1d_hip_host_picture_alloc(Dav1dHipContext *c, Dav1dHipHostPicture *hp, int w, int h, int layout, int bpc) {
    if (!c || !hp) return -EINVAL;
    memset(hp, 0, sizeof(*hp));
    const int rc = dav1d_hip_picture_alloc(c, &hp->dev, w, h, layout, bpc);
    if (rc) return rc;
    void *buf = nullptr;
    if (hipHostMalloc(&buf, hp->dev.alloc_size, hipHostMallocDefault) != hipSuccess) {
        (void) dav1d_hip_picture_free(c, &hp->dev);
        memset(hp, 0, sizeof(*hp));
        return -ENOMEM;
    }
    hp->alloc = buf;
    hp->alloc_size = hp->dev.alloc_size;
    for (int i = 0; i < 3; i++)
        hp->data[i] = hp->dev.p[i].data ? (uint8_t *) buf + ((const uint8_t *) hp->dev.p[i].data - (const uint8_t *) hp->dev.alloc) : nullptr;
    hp->stride[0] = hp->dev.p[0].stride;
    hp->stride[1] = hp->dev.p[1].stride;
    __atomic_fetch_add(&dav1d_hip_live[3], 1, __ATOMIC_RELAXED);
    return 0;
}

int dav1d_hip_host_picture_release(Dav1dHipContext *c, Dav1dHipHostPicture *hp) {
    if (!c || !hp) return -EINVAL;
    (void) hipStreamSynchronize(c->copy_stream);
    int rc = 0;
    if (hp->alloc) { rc = hip_rc(hipHostFree(hp->alloc)); __atomic_fetch_sub(&dav1d_hip_live[3], 1, __ATOMIC_RELAXED); }
    const int rc2 = dav1d_hip_picture_free(c, &hp->dev);
    memset(hp, 0, sizeof(*hp));
    return rc ? rc : rc2;
}

int dav1d_hip_host_picture_fetch(Dav1dHipContext *c, const Dav1dHipHostPicture *hp, const Dav1dHipPicture *src, int row0, int row1) {
    if (!c || !hp || !hp->alloc) return -EINVAL;
    if (!src) src = &hp->dev;
    if (src->bpc != hp->dev.bpc || src->layout != hp->dev.layout || src->p[0].w != hp->dev.p[0].w || src->p[0].h != hp->dev.p[0].h) return -EINVAL;
    if (row0 < 0) row0 = 0;
    if (row1 > src->p[0].h) row1 = src->p[0].h;
    if (row1 <= row0) return 0;
    const int ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420, bps = src->bpc > 8 ? 2 : 1;
    if (src->twin_ok == DAV1D_HIP_TWIN_ONLY) {
        // the picture lives in its twin: the rows of this band become raster rows here, on their way out (the raster planes are the
        // staging; src is const, so the picture stays DAV1D_HIP_TWIN_ONLY and a later band / fetch does its own rows again)
        if (!src->twin[0]) return -EINVAL;
        int r0[3], r1[3];
        for (int pl = 0; pl < 3; pl++) {
            const int sv = pl ? ss_ver : 0;
            r0[pl] = row0 >> sv; r1[pl] = row1 >= src->p[0].h ? src->p[pl].h : row1 >> sv;
        }
        const DevPlanes dp = dev_planes(src);
        int rc = dav1d_hip_launch_untile(&dp, src->twin, src->bpc, r0, r1, 7, c->stream);
        if (!rc) rc = hip_rc(hipEventRecord(c->ev_untile, c->stream));
        if (!rc) rc = hip_rc(hipStreamWaitEvent(c->copy_stream, c->ev_untile, 0));
        if (rc) return rc;
    }
    for (int pl = 0; pl < 3; pl++) {
        if (!src->p[pl].data || !hp->data[pl]) continue;
        const int sv = pl ? ss_ver : 0;
        // chroma rows under luma rows [row0, row1): a band boundary is even, the last band ends with the picture
        const int r0 = row0 >> sv, r1 = row1 >= src->p[0].h ? src->p[pl].h : row1 >> sv;
        if (r1 <= r0) continue;
        const ptrdiff_t hs = hp->stride[pl ? 1 : 0];
        const hipError_t e = hipMemcpy2DAsync((uint8_t *) hp->data[pl] + (size_t) r0 * hs, hs,
                                              (const uint8_t *) src->p[pl].data + (size_t) r0 * src->p[pl].stride, src->p[pl].stride,
                                              (size_t) src->p[pl].w * bps, r1 - r0, hipMemcpyDeviceToHost, c->copy_stream);
        if (e != hipSuccess) return hip_rc(e);
    }
    return 0;
}

int dav1d_hip_host_picture_wait(Dav1dHipContext *c) {
    if (!c) return -EINVAL;
    return hip_rc(hipStreamSynchronize(c->copy_stream));
}

int dav1d_hip_picture_free(Dav1dHipContext *c, Dav1dHipPicture *pic) {
    if (!pic || (!pic->alloc && !pic->twin_alloc)) return 0;
    if (c) hipStreamSynchronize(c->stream); else (void) hipDeviceSynchronize();        // (a picture that outlived its context)
    int rc = pic->alloc ? hip_rc(hipFree(pic->alloc)) : 0;
    if (pic->twin_alloc) { const int rc2 = hip_rc(hipFree(pic->twin_alloc)); if (!rc) rc = rc2; }
    memset(pic, 0, sizeof(*pic));
    return rc;
}

// `dst` (a picture of dst_c's device with src's geometry: dav1d_hip_picture_alloc under the same ref_twin option) becomes a copy of `src`
// (src_c's device): the raster planes unless src lives in its twin only, the twin when src has a valid one and dst the storage.  The copy is
// enqueued on dst_c's stream behind everything src_c's stream holds now (an event across the devices), over xGMI when the devices are peers
// (hipMemcpyPeerAsync stages through the host when they are not): a launch of dst_c that follows reads the copy.
int dav1d_hip_picture_copy_peer(Dav1dHipContext *dst_c, Dav1dHipPicture *dst, Dav1dHipContext *src_c, const Dav1dHipPicture *src) {
    if (!dst_c || !dst || !src_c || !src || !dst->p[0].data || !src->p[0].data) return -EINVAL;
    if (dst->bpc != src->bpc || dst->layout != src->layout) return -EINVAL;
    for (int pl = 0; pl < 3; pl++)
        if (dst->p[pl].w != src->p[pl].w || dst->p[pl].h != src->p[pl].h || dst->p[pl].stride != src->p[pl].stride || !dst->p[pl].data != !src->p[pl].data) return -EINVAL;
    const bool twin = src->twin_ok && src->twin[0] && dst->twin[0];
    if (src->twin_ok == DAV1D_HIP_TWIN_ONLY && !twin) return -EINVAL;
    // behind the source's work
    // (an event of this call's own: several devices may be copying from one source at a time, and src_c's thread goes on enqueuing.  A twin
    // made by dav1d_hip_picture_retile_overlapped is on a side stream: its maker waits for it — dav1d_hip_sync — before handing it out.)
    hipEvent_t ev;
    if (hipSetDevice(src_c->device) != hipSuccess) return -ENODEV;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, src_c->stream);
    if (hipSetDevice(dst_c->device) != hipSuccess) { (void) hipEventDestroy(ev); return -ENODEV; }
    if (e == hipSuccess) e = hipStreamWaitEvent(dst_c->stream, ev, 0);
    (void) hipEventDestroy(ev);             // (released once the wait has passed it)
    HIP_TRY(e);
    const bool padded = src->alloc != nullptr && dst->alloc != nullptr;
    for (int pl = 0; pl < 3; pl++) {
        if (!src->p[pl].data) continue;
        const size_t bytes = (size_t) src->p[pl].stride * (size_t) picture_plane_rows(src, pl, padded);
        if (src->twin_ok != DAV1D_HIP_TWIN_ONLY)
            HIP_TRY(hipMemcpyPeerAsync(dst->p[pl].data, dst_c->device, src->p[pl].data, src_c->device, bytes, dst_c->stream));
        if (twin)
            HIP_TRY(hipMemcpyPeerAsync(dst->twin[pl], dst_c->device, src->twin[pl], src_c->device, bytes, dst_c->stream));
    }
    dst->twin_ok = twin ? src->twin_ok : 0;
    return 0;
}

// Luma rows [y0, y1) of src's RASTER planes (the chroma rows under them) to dst on another device, on dst_c's stream.  The caller says the rows are
// final on the source device (dav1d_hip_frame_set_progress_callback reported them): nothing of src_c's stream is waited for, so the bands of a
// picture can cross while the frame that makes it is still ending (dav1d_glue.c).  y0 a multiple of 8; dst's twin is stale afterwards.
int dav1d_hip_picture_copy_peer_rows(Dav1dHipContext *dst_c, Dav1dHipPicture *dst, Dav1dHipContext *src_c, const Dav1dHipPicture *src, int y0, int y1) {
    if (!dst_c || !dst || !src_c || !src || !dst->p[0].data || !src->p[0].data) return -EINVAL;
    if (dst->bpc != src->bpc || dst->layout != src->layout || src->twin_ok == DAV1D_HIP_TWIN_ONLY) return -EINVAL;
    for (int pl = 0; pl < 3; pl++)
        if (dst->p[pl].w != src->p[pl].w || dst->p[pl].h != src->p[pl].h || dst->p[pl].stride != src->p[pl].stride || !dst->p[pl].data != !src->p[pl].data) return -EINVAL;
    if (y0 < 0 || (y0 & 7) || y1 < y0 || y1 > src->p[0].h) return -EINVAL;
    if (y1 == y0) return 0;
    if (hipSetDevice(dst_c->device) != hipSuccess) return -ENODEV;
    const bool padded = src->alloc != nullptr && dst->alloc != nullptr;
    const bool last = y1 == src->p[0].h;           // (the padding rows below the picture travel with its last band, as dav1d_hip_picture_copy_peer sends them)
    const int ss_ver = src->layout == DAV1D_HIP_LAYOUT_I420;
    for (int pl = 0; pl < 3; pl++) {
        if (!src->p[pl].data) continue;
        const int sv = pl ? ss_ver : 0;
        const int r0 = y0 >> sv, r1 = last ? picture_plane_rows(src, pl, padded) : (y1 + sv) >> sv;
        if (r1 <= r0) continue;
        const size_t off = (size_t) src->p[pl].stride * (size_t) r0, bytes = (size_t) src->p[pl].stride * (size_t) (r1 - r0);
        HIP_TRY(hipMemcpyPeerAsync((char *) dst->p[pl].data + off, dst_c->device, (const char *) src->p[pl].data + off, src_c->device, bytes, dst_c->stream));
    }
    dst->twin_ok = 0;
    return 0;
}

static void plane_extent(const Dav1dHipPicture *pic, int plane, int padded, size_t *row_bytes, int *rows) {
    const int bps = pic->bpc > 8 ? 2 : 1;
    if (padded) {
        const int ss_ver = plane && pic->layout == DAV1D_HIP_LAYOUT_I420;
        const int ss_hor = plane && pic->layout != DAV1D_HIP_LAYOUT_I444;
        const int aw = ((pic->p[0].w + 127) & ~127) >> ss_hor, ah = ((pic->p[0].h + 127) & ~127) >> ss_ver;
        *row_bytes = (size_t) aw * bps;
        *rows = ah;
    } else {
        *row_bytes = (size_t) pic->p[plane].w * bps;
        *rows = pic->p[plane].h;
    }
}

int dav1d_hip_plane_upload(Dav1dHipContext *c, const Dav1dHipPicture *pic, int plane,
                           const void *host, ptrdiff_t host_stride, int padded) {
    if (!pic || plane < 0 || plane > 2 || !pic->p[plane].data) return -EINVAL;
    size_t rb; int rows;
    plane_extent(pic, plane, padded, &rb, &rows);
    HIP_TRY(hipMemcpy2DAsync(pic->p[plane].data, pic->p[plane].stride, host, host_stride, rb, rows,
                             hipMemcpyHostToDevice, c->stream));
    return hip_rc(hipStreamSynchronize(c->stream));
}

int dav1d_hip_plane_download(Dav1dHipContext *c, const Dav1dHipPicture *pic, int plane,
                             void *host, ptrdiff_t host_stride, int padded) {
    if (!pic || plane < 0 || plane > 2 || !pic->p[plane].data) return -EINVAL;
    size_t rb; int rows;
    plane_extent(pic, plane, padded, &rb, &rows);
    if (pic->twin_ok == DAV1D_HIP_TWIN_ONLY) {
        // the picture lives in its twin: this plane's raster rows are made here (pic is const: the flag stays, the next call does it again)
        if (!pic->twin[plane]) return -EINVAL;
        const DevPlanes dp = twin_pass_planes(pic);
        const int rc = dav1d_hip_launch_untile(&dp, pic->twin, pic->bpc, nullptr, nullptr, 1 << plane, c->stream);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpy2DAsync(host, host_stride, pic->p[plane].data, pic->p[plane].stride, rb, rows,
                             hipMemcpyDeviceToHost, c->stream));
    return hip_rc(hipStreamSynchronize(c->stream));
}

} // extern "C"
