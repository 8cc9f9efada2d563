// Host side of the C ABI: recon lists (predictions and residuals of a frame pipelined over the context's streams).
#include "lists.h"
#include <stdio.h>
#include <stdlib.h>
#include <new>
#include <algorithm>

// ------------------------------------------------------------------ recon list: predictions and residuals pipelined
//
// dav1d_hip_inter_list_run followed by dav1d_hip_itx_list_run makes every residual wait for every prediction.  The residual
// launch of one transform size only needs the prediction launches whose tiles lie under its blocks; which ones those are is
// worked out here once, on a 4x4-cell map of the picture.  At run time the prediction launches go down the context's stream
// in the order largest tile shape first, each followed by an event; the residual launches go down a side stream, largest
// transform first, each waiting for the events of its own predecessors only.  The memory-bound predictions of the small
// shapes then overlap with the arithmetic-bound 64- and 32-point transforms instead of queueing in front of them.

// DAV1D_HIP_RECON_FUSE: which square block sizes get paired (transform block + the prediction block of the same rectangle in
// one wave, recon.hip): bit 0 4x4, bit 1 8x8, bit 2 16x16, bit 3 32x32, bit 4 64x64; 0 none.  Measured on MI355X (8K 10-bit
// frame, ms per frame, round 2 after the paired kernel's LDS regions were overlaid): 8x8 + 16x16 (6) 0.325-0.339,
// 8x8 + 16x16 + 32x32 (14, the default) 0.317-0.327.  Round 1 (three separate LDS arrays): none 0.362, 6 0.311 (older clock),
// 4x4 + 8x8 0.318, all 0.411.  What pays is that the paired launches move a quarter less HBM traffic AND run next to the
// pipelined launches of the other sizes on streams of their own; 4x4 and 64x64 pairs lose to their separate kernels.
// Round 6: the 4x4 pairs too (15, the default now): their launch fits five LDS pieces since the records pass through the window
// buffer (48 us against 37 + 23 for the two launches it replaces) and it runs on the MAIN stream, out of the way of the side streams'
// chains; with two frame contexts and two paired streams 0.2295 against 0.2424 ms per frame (profiles/r06/streams.txt).
int recon_fuse_mask(const Dav1dHipContext *c) { return c->recon_fuse & 31; }

extern "C" {

int dav1d_hip_recon_list_create(Dav1dHipContext *c, Dav1dHipReconList **out, const Dav1dHipPicture *geometry,
                                const Dav1dHipMcTask *mc, size_t n_mc, const Dav1dHipCompTask *comp, size_t n_comp,
                                const Dav1dHipItxTask *itx, size_t n_itx) {
    if (!c || !out || !geometry) return -EINVAL;
    *out = nullptr;
    if ((!itx && n_itx) || n_itx > 0xffffffffu) return -EINVAL;
    for (size_t i = 0; i < n_itx; i++) if (!itx_task_ok(itx[i])) return -EINVAL;
    Dav1dHipReconList *l = new (std::nothrow) Dav1dHipReconList();
    if (!l) return -ENOMEM;
    const Dav1dHipItxTask *const itx_all = itx;
    const size_t n_itx_all = n_itx;
    l->inter = nullptr; l->itx = nullptr; l->wide_ok = false;
    for (int k = 0; k < 5; k++) { l->f_tiles[k] = nullptr; l->f_tasks[k] = nullptr; l->f_n[k] = 0; }
    l->f_max_ref = 0;
    ReconPairing pair;
    const bool fuse = recon_fuse_mask(c) != 0;
    if (fuse) {
        pair.mask = recon_fuse_mask(c);
        pair.itx = itx;
        bool any_blend = false;
        for (size_t i = 0; i < n_comp && !any_blend; i++) any_blend = comp[i].kind >= DAV1D_HIP_COMP_BLEND;
        for (int p = 0; p < 3; p++) {
            const int bps = geometry->bpc > 8 ? 2 : 1;
            pair.stride_px[p] = geometry->p[p].data ? (int) (geometry->p[p].stride / bps) : 0;
            pair.cell_stride[p] = (pair.stride_px[p] + 3) >> 2;
            if (any_blend && pair.stride_px[p]) pair.blend_cells[p].assign((size_t) pair.cell_stride[p] * (size_t) ((geometry->p[p].h + 127 + 3) >> 2), 0);
        }
        pair.taken.assign(n_itx, 0);
        for (size_t i = 0; i < n_itx; i++)
            if (itx[i].tx <= 4 && (pair.mask >> itx[i].tx & 1)) pair.by_pos[(uint64_t) itx[i].plane << 32 | itx[i].dst_off] = (uint32_t) i;
    }
    int rc = inter_list_create_geo(c, &l->inter, mc, n_mc, comp, n_comp, geometry, fuse ? &pair : nullptr);
    std::vector<Dav1dHipItxTask> rest;
    if (!rc && fuse) {
        rest.reserve(n_itx);
        for (size_t i = 0; i < n_itx; i++) if (!pair.taken[i]) rest.push_back(itx[i]);
        itx = rest.data();
        n_itx = rest.size();
    }
    if (!rc) rc = dav1d_hip_itx_list_create(c, &l->itx, itx, n_itx);
    // ---- the paired blocks of each size: ordered by where their first tile reads (as the tiles of mc lists are), then
    // grouped by the transform's code path inside windows of 128 waves (as the blocks of itx lists are); uploaded
    for (int k = 0; k < 5 && !rc && fuse; k++) {
        const size_t nblk = pair.itx_idx[k].size();
        if (!nblk) continue;
        const int tpb = k < 3 ? 1 : k == 3 ? 2 : 4, bpw = k == 0 ? 16 : k == 1 ? 8 : k == 2 ? 4 : k == 3 ? 2 : 1;
        if (pair.tiles[k].size() != nblk * tpb) { rc = -EINVAL; break; }
        std::vector<uint32_t> ord(nblk);
        std::vector<uint64_t> skey(nblk);
        for (size_t i = 0; i < nblk; i++) {
            ord[i] = (uint32_t) i;
            const McTile &t = pair.tiles[k][i * tpb];
            const uint64_t y = (uint64_t) (t.r[0].src_y + 4096) & 0xffff, x = (uint64_t) (t.r[0].src_x + 4096) & 0xffff;
            skey[i] = ((uint64_t) t.r[0].ref << 56) | ((uint64_t) t.plane << 52) | ((y >> 6) << 32) | x;
        }
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t p, uint32_t q) { return skey[p] < skey[q]; });
        const size_t win = (size_t) 128 * bpw;
        for (size_t lo = 0; lo < nblk; lo += win)
            std::stable_sort(ord.begin() + lo, ord.begin() + std::min(lo + win, nblk), [&](uint32_t p, uint32_t q) {
                const McTile &tp = pair.tiles[k][p * tpb], &tq = pair.tiles[k][q * tpb];
                // ... and the parity of the first reference column: with tiled references the horizontal pass picks its tap pairs by it
                // (mc_body.h, TILED), and a wave whose tiles agree runs one of the two forms instead of both
                const int kp = (itx_path_key(pair.itx[pair.itx_idx[k][p]]) * 8 + tp.kind) * 2 + (tp.r[0].src_x & 1);
                const int kq = (itx_path_key(pair.itx[pair.itx_idx[k][q]]) * 8 + tq.kind) * 2 + (tq.r[0].src_x & 1);
                return kp < kq;
            });
        std::vector<McTile> tiles(nblk * tpb);
        std::vector<Dav1dHipItxTask> tasks(nblk);
        for (size_t i = 0; i < nblk; i++) {
            for (int j = 0; j < tpb; j++) {
                const McTile &t = tiles[i * tpb + j] = pair.tiles[k][(size_t) ord[i] * tpb + j];
                const bool two = t.kind == MCT_AVG || t.kind == MCT_WAVG;
                l->f_max_ref = std::max(l->f_max_ref, std::max((int) t.r[0].ref, two ? (int) t.r[1].ref : 0));
            }
            tasks[i] = pair.itx[pair.itx_idx[k][ord[i]]];
            itx_fill_prefix(tasks[i]);
        }
        if (hipMalloc((void **) &l->f_tiles[k], tiles.size() * sizeof(McTile)) != hipSuccess ||
            hipMalloc((void **) &l->f_tasks[k], tasks.size() * sizeof(Dav1dHipItxTask)) != hipSuccess) { rc = -ENOMEM; break; }
        rc = dav1d_hip_upload(c, l->f_tiles[k], tiles.data(), tiles.size() * sizeof(McTile));
        if (!rc) rc = dav1d_hip_upload(c, l->f_tasks[k], tasks.data(), tasks.size() * sizeof(Dav1dHipItxTask));
        l->f_n[k] = nblk;
    }
    if (rc) { dav1d_hip_recon_list_destroy(c, l); return rc; }
    for (int b = 0; b < 19; b++) l->dep[b] = 0;
    for (int p = 0; p < 3; p++) l->stride_px[p] = l->inter->stride_px[p];
    l->wide_ok = true;
    for (size_t i = 0; i < n_itx_all && l->wide_ok; i++) {
        const Dav1dHipItxTask &t = itx_all[i];
        const int sp = l->stride_px[t.plane];
        l->wide_ok = sp > 0 && (int) (t.dst_off % (uint32_t) sp) % std::min((int) k_tx_w[t.tx], 8) == 0 && sp % 8 == 0;
    }
    for (size_t i = 0; i < n_itx; i++) {
        const Dav1dHipItxTask &t = itx[i];
        const int sp = l->stride_px[t.plane], cs = l->inter->cell_stride[t.plane];
        if (sp <= 0) { l->dep[t.tx] = 0xffff; continue; }
        const int x = (int) (t.dst_off % (uint32_t) sp), y = (int) (t.dst_off / (uint32_t) sp);
        const std::vector<uint16_t> &wr = l->inter->writers[t.plane];
        uint16_t m = 0;
        for (int cy = y >> 2; cy <= (y + k_tx_h[t.tx] - 1) >> 2; cy++)
            for (int cx = x >> 2; cx <= (x + k_tx_w[t.tx] - 1) >> 2; cx++) {
                const size_t j = (size_t) cy * cs + cx;
                m |= (cx < cs && j < wr.size()) ? wr[j] : (uint16_t) 0xffff;      // off the map: wait for everything
            }
        l->dep[t.tx] |= m;
    }
    // the maps are only needed for the dependency masks
    for (int p = 0; p < 3; p++) std::vector<uint16_t>().swap(l->inter->writers[p]);
    *out = l;
    return 0;
}

void dav1d_hip_recon_list_destroy(Dav1dHipContext *c, Dav1dHipReconList *l) {
    if (!l) return;
    if (l->inter) dav1d_hip_inter_list_destroy(c, l->inter);
    if (l->itx) dav1d_hip_itx_list_destroy(c, l->itx);
    hipStreamSynchronize(c->stream);
    for (int k = 0; k < 5; k++) { if (l->f_tiles[k]) hipFree(l->f_tiles[k]); if (l->f_tasks[k]) hipFree(l->f_tasks[k]); }
    delete l;
}

static int recon_list_run_impl(Dav1dHipContext *c, const Dav1dHipReconList *l, const Dav1dHipPicture *dst, const Dav1dHipPicture *refs, int n_refs,
                               int16_t *prep, uint8_t *mask, void *coef, const bool wide, const DevPlanes *dst_twin) {
    if (!c || !l || !dst || !refs) return -EINVAL;
    const int bps = dst->bpc > 8 ? 2 : 1;
    for (int p = 0; p < 3; p++)
        if (l->stride_px[p] && dst->p[p].stride / bps != l->stride_px[p]) return -EINVAL;    // not the geometry the list was made for
    size_t n_paired = 0;
    bool paired_on_side = false;
    int n_ps = 0;                                        // side streams the paired launches went to
    for (int k = 0; k < 5; k++) n_paired += l->f_n[k];
    if (n_paired) {
        // the paired blocks: one launch per size, largest first; independent of each other and of everything below
        const DevPlanes dp = dev_planes(dst);
        DevPlanes rp[8];
        if (const int rv = checked_ref_planes(c, dst, refs, n_refs, l->f_max_ref, rp)) return rv;
        // one after the other on a side stream of their own, next to the pipeline of the unpaired rest below (main stream:
        // predictions, side stream 0: residuals).  Measured: the paired launches on one stream 0.317 ms per frame, on two
        // streams that run side by side 0.334-0.343 — three launches at a time share the memory system better than four.
        const bool side = c->concurrent && n_paired >= 16384;
        int rc = 0, lane = 0;
        // c->recon_pair_streams: 1 = the paired launches one after the other on ONE side stream, 2 / 3 = dealt over that many (side
        // streams 2 .. 4; their ends are ev_pair[]).  Measured, round 6 (profiles/r06/streams.txt): with ONE frame in flight the
        // extra streams change nothing — round 2 measured the same — but with two frame contexts they are worth 11 %: the launches of
        // two frames on five streams keep every SIMD supplied with waves through the heads and tails of the single launches.
        n_ps = side ? std::max(1, std::min(3, c->recon_pair_streams)) : 0;
        if (side) {
            (void) hipEventRecord(c->ev_fork, c->stream);
            for (int j = 0; j < n_ps; j++) (void) hipStreamWaitEvent(c->side[c->recon_pair_first + j], c->ev_fork, 0);
        }
        for (int k = 4; k >= 0 && !rc; k--)
            if (l->f_n[k]) {
                // the 4x4 pairs go to the main stream, in front of the unpaired predictions: the side streams' chains of long launches are
                // what the step waits for, and the short launches of the main stream end long before them
                const bool on_main = side && k == 0;
                rc = dav1d_hip_launch_recon_fused_out(&dp, rp, n_refs, dst->bpc, k, l->f_tiles[k], l->f_tasks[k], (int) l->f_n[k], prep, coef, c->recon_coop_below,
                                                      wide, dst_twin, side && !on_main ? c->side[c->recon_pair_first + lane] : c->stream);
                if (!on_main && n_ps) lane = (lane + 1) % n_ps;
            }
        for (int j = 0; j < n_ps; j++) (void) hipEventRecord(c->ev_pair[j], c->side[c->recon_pair_first + j]);
        if (rc) return rc;
        paired_on_side = side;
        if (!l->inter->mc->n && !l->inter->comp->n && !l->itx->n) {
            for (int j = 0; j < n_ps; j++) (void) hipStreamWaitEvent(c->stream, c->ev_pair[j], 0);
            return 0;
        }
    }
    const Dav1dHipMcList *ml = l->inter->mc;
    // c->recon_pipeline = smallest residual list worth two streams (0: always pipeline, -1: never)
    const long min_tasks = c->recon_pipeline;
    auto join_paired = [&]() {
        if (paired_on_side) for (int j = 0; j < n_ps; j++) (void) hipStreamWaitEvent(c->stream, c->ev_pair[j], 0);
    };
    if (!dst_twin && (min_tasks < 0 || !c->concurrent || mc_fused_min_bin() < MC_BINS || (long) l->itx->n < min_tasks)) {
        int rc = dav1d_hip_inter_list_run(c, l->inter, dst, refs, n_refs, prep, mask);
        if (!rc) rc = dav1d_hip_itx_list_run(c, l->itx, dst, coef);
        join_paired();
        return rc;
    }
    const DevPlanes dp = dev_planes(dst);
    DevPlanes rp[8];
    if (const int rv = checked_ref_planes(c, dst, refs, n_refs, ml->n ? ml->max_ref : 0, rp)) { join_paired(); return rv; }
    int rc = mc_regroup(c, const_cast<Dav1dHipMcList *>(ml), rp, n_refs);
    if (rc) { join_paired(); return rc; }
    // DAV1D_HIP_RECON_LANES: side streams the residual launches are dealt over.  Measured (8K 10-bit): 1 lane 0.379 ms,
    // 2 lanes 0.394, 3 lanes 0.407, 5 lanes 0.420 per frame — residual launches running next to each other take bandwidth from
    // the predictions they are waiting for; one in-order residual stream keeps the pipeline a pipeline.
    const int n_lanes = paired_on_side ? 1      // side streams 1 and 2 carry the paired launches
                      : std::max(1, std::min((int) Dav1dHipContext::N_SIDE, c->recon_lanes));
    hipStream_t sm = c->stream;
    (void) hipEventRecord(c->ev_fork, sm);
    for (int i = 0; i < n_lanes; i++) (void) hipStreamWaitEvent(c->side[i], c->ev_fork, 0);
    // The prediction launches run in order on one stream, so a residual launch only has to wait for the LAST launch it depends
    // on — and only those launches get an event (a cross-stream event is a cache release / acquire: not free).
    int seq[16], n_seq = 0;                              // launch order of the prediction side: bins descending, then the compound launch
    // largest tile shape first (measured: 16x16 first is as good, smallest first 8 % slower: its residuals are the shortest
    // and leave the long 64- and 32-point transforms for a tail that nothing overlaps)
    for (int b = MC_BINS - 1; b >= 0; b--) if (ml->off[b + 1] > ml->off[b]) seq[n_seq++] = b;
    if (l->inter->comp->n) seq[n_seq++] = 15;
    int last_dep[19];                                    // per transform size: position in seq[] of its last dependency, -1 none
    bool wanted[16] = { false };
    for (int b = 0; b < 19; b++) {
        last_dep[b] = -1;
        if (l->itx->off[b + 1] == l->itx->off[b]) continue;
        for (int k = 0; k < n_seq; k++) if (l->dep[b] >> seq[k] & 1) last_dep[b] = k;
        if (last_dep[b] >= 0) wanted[last_dep[b]] = true;
    }
    for (int k = 0; k < n_seq && !rc; k++) {
        const int b = seq[k];
        if (b == 15) rc = dav1d_hip_comp_list_run(c, l->inter->comp, dst, prep, mask);
        else if (dst_twin) rc = dav1d_hip_launch_mc_bin_twin(&dp, rp, n_refs, dst->bpc, b, ml->dev + ml->off[b], (int) (ml->off[b + 1] - ml->off[b]), prep, dst_twin, sm);
        else rc = dav1d_hip_launch_mc_bin(&dp, rp, n_refs, dst->bpc, b, ml->dev + ml->off[b], (int) (ml->off[b + 1] - ml->off[b]), prep, sm);
        if (wanted[k]) (void) hipEventRecord(c->ev_bin[k], sm);
    }
    int waited[Dav1dHipContext::N_SIDE];
    for (int i = 0; i < Dav1dHipContext::N_SIDE; i++) waited[i] = -1;
    int lane = 0;
    // residual launches in the order their predictions become ready (ties: largest transform first)
    int iorder[19];
    for (int k = 0; k < 19; k++) iorder[k] = k_itx_launch_order[k];
    std::stable_sort(iorder, iorder + 19, [&](int p, int q) { return last_dep[p] < last_dep[q]; });
    for (int k = 0; k < 19 && !rc; k++) {
        const int b = iorder[k];
        const size_t cnt = l->itx->off[b + 1] - l->itx->off[b];
        if (!cnt) continue;
        hipStream_t si = c->side[lane];
        if (last_dep[b] > waited[lane]) {                // a lane is in order too: an earlier wait covers everything before it
            (void) hipStreamWaitEvent(si, c->ev_bin[last_dep[b]], 0);
            waited[lane] = last_dep[b];
        }
        rc = dav1d_hip_launch_itx_bin_out(&dp, dst->bpc, b, l->itx->dev + l->itx->off[b], (int) cnt, coef, wide, dst_twin, si);
        lane = (lane + 1) % n_lanes;
    }
    for (int i = 0; i < n_lanes; i++) {
        (void) hipEventRecord(c->ev_join[i], c->side[i]);
        (void) hipStreamWaitEvent(sm, c->ev_join[i], 0);
    }
    join_paired();
    return rc;
}

int dav1d_hip_recon_list_run(Dav1dHipContext *c, const Dav1dHipReconList *l, const Dav1dHipPicture *dst,
                             const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask, void *coef) {
    if (!raster_dst_ok(dst)) return -EINVAL;
    return recon_list_run_impl(c, l, dst, refs, n_refs, prep, mask, coef, false, nullptr);
}

// dst's planes with the twin's storage behind them; tiled: DevPlanes.tiled of the launches that write through it (0: next to the raster planes, 2: the twin only)
static DevPlanes twin_planes(const Dav1dHipPicture *dst, int tiled) {
    DevPlanes tw = dev_planes(dst);
    for (int p = 0; p < 3; p++) tw.data[p] = dst->p[p].data ? dst->twin[p] : nullptr;
    tw.tiled = tiled;
    return tw;
}

// can every launch of the list write dst's twin itself?  (tiled references, blocks on the 8-pixel grid, no mask / blend tasks, aligned planes)
static bool recon_list_twin_direct(Dav1dHipContext *c, const Dav1dHipReconList *l, const Dav1dHipPicture *dst, const Dav1dHipPicture *refs, int n_refs) {
    bool direct = c->ref_twin != 0 && l->wide_ok && !l->inter->comp->n && mc_fused_min_bin() >= MC_BINS;
    const int bps = dst->bpc > 8 ? 2 : 1;
    for (int p = 0; p < 3 && direct; p++)
        if (dst->p[p].data) direct = dst->twin[p] && !((uintptr_t) dst->p[p].data & 15) && !((uintptr_t) dst->twin[p] & 15) && dst->p[p].stride % 16 == 0 &&
                                     (dst->p[p].stride / bps) % 8 == 0;
    for (int i = 0; i < n_refs && direct; i++) direct = picture_twin_usable(&refs[i]);
    static const bool debug_tiled = getenv("DAV1D_DEBUG_TILED") != nullptr;      // (asked once: this runs per frame)
    if (debug_tiled) fprintf(stderr, "twin_direct: ref_twin %d wide_ok %d comp %zu min_bin %d -> %d (refs ok: %d %d %d)\n", c->ref_twin, (int) l->wide_ok, (size_t) l->inter->comp->n, mc_fused_min_bin(), (int) direct, n_refs > 0 ? refs[0].twin_ok : -1, n_refs > 1 ? refs[1].twin_ok : -1, n_refs > 2 ? refs[2].twin_ok : -1);
    return direct;
}

// The same, and the picture's tiled twin (Dav1dHipPicture.twin) holds the frame's pixels afterwards: the step of a frame whose in-loop
// filters are off, as later frames will predict from it.  When every launch of the list can write the twin along with the raster
// planes — tiled references, blocks on the 8-pixel grid, no mask / blend tasks (those go through a kernel that only knows raster
// planes) — it is written by the launches themselves (the paired kernels and the residual kernels through tile_write_out, the
// prediction kernels strip by strip); otherwise the list runs as always and dav1d_hip_picture_retile follows.  Sets dst->twin_ok.
int dav1d_hip_recon_list_run_twin(Dav1dHipContext *c, const Dav1dHipReconList *l, Dav1dHipPicture *dst,
                                  const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask, void *coef) {
    if (!c || !l || !dst || !refs) return -EINVAL;
    if (const int rc = twin_on_demand(c, dst)) return rc;
    // (the launches write raster planes: a picture that lives in its twin gets them back first, so that what a partial list does not cover
    // is carried along, as in dav1d_hip_recon_list_run_tiled)
    if (const int ru = dav1d_hip_picture_untile(c, dst)) return ru;
    const bool direct = recon_list_twin_direct(c, l, dst, refs, n_refs);
    dst->twin_ok = 0;
    if (direct) {
        const DevPlanes tw = twin_planes(dst, 0);
        const int rc = recon_list_run_impl(c, l, dst, refs, n_refs, prep, mask, coef, true, &tw);
        if (!rc) dst->twin_ok = 1;
        return rc;
    }
    const int rc = recon_list_run_impl(c, l, dst, refs, n_refs, prep, mask, coef, false, nullptr);
    return rc ? rc : dav1d_hip_picture_retile(c, dst);
}

// The same with the picture living in its twin ONLY: nothing is written to the raster planes (dst->twin_ok = DAV1D_HIP_TWIN_ONLY
// afterwards) — an 8x8 block leaves as one 128-byte line instead of eight 16-byte row pieces, a 4x4 block as half a line instead of four
// 8-byte pieces, and the residual launches read the predicted pixels back the same way.  What reads such a picture: motion
// compensation of later frames (through the twin, as always), dav1d_hip_host_picture_fetch / dav1d_hip_plane_download (they un-tile
// on the way out: raster rows by the address rules of src/picture.c:46-63 exist at the output only) and dav1d_hip_picture_untile.
// `dst` on entry: any state; if it holds pixels the list does not overwrite (a partial list), they must be in the twin — a picture
// whose raster planes alone are valid is retiled first.  Lists that cannot run that way (recon_list_twin_direct) run on the raster
// planes and retile: twin_ok = 1 then.
int dav1d_hip_recon_list_run_tiled(Dav1dHipContext *c, const Dav1dHipReconList *l, Dav1dHipPicture *dst,
                                   const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask, void *coef) {
    if (!c || !l || !dst || !refs) return -EINVAL;
    if (const int rc = twin_on_demand(c, dst)) return rc;
    if (!recon_list_twin_direct(c, l, dst, refs, n_refs)) {
        int rc = dav1d_hip_picture_untile(c, dst);
        if (!rc) rc = recon_list_run_impl(c, l, dst, refs, n_refs, prep, mask, coef, false, nullptr);
        dst->twin_ok = 0;
        return rc ? rc : dav1d_hip_picture_retile(c, dst);
    }
    // (a picture whose raster planes alone are valid is retiled first — once per picture: it lives in its twin from then on.  The contract
    // keeps every pixel the list does not write, the allocator's padding included, so "the list covers the visible picture" is no licence
    // to skip it)
    if (!dst->twin_ok) { const int rc = dav1d_hip_picture_retile(c, dst); if (rc) return rc; }
    const DevPlanes tw = twin_planes(dst, 2);
    const int rc = recon_list_run_impl(c, l, dst, refs, n_refs, prep, mask, coef, true, &tw);
    dst->twin_ok = rc ? 0 : DAV1D_HIP_TWIN_ONLY;
    return rc;
}

// Measurement aid: the launches of a recon list one after the other on the context's stream, each bracketed by events.
// ms / counts: [0..4] the paired launches by size class (blocks), [5..19] the prediction launches by tile shape (tiles), [20] the
// compound / blend launch (tasks), [21..39] the residual launches by transform size (blocks).
static int recon_list_run_timed_impl(Dav1dHipContext *c, const Dav1dHipReconList *l, const Dav1dHipPicture *dst,
                                     const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask, void *coef,
                                     float *ms, size_t *counts, const DevPlanes *dst_twin) {
    if (!c || !l || !dst || !refs || !ms || !counts) return -EINVAL;
    const Dav1dHipMcList *ml = l->inter->mc;
    const DevPlanes dp = dev_planes(dst);
    DevPlanes rp[8];
    if (const int rv = checked_ref_planes(c, nullptr, refs, n_refs, std::max(ml->n ? ml->max_ref : 0, l->f_max_ref), rp)) return rv;
    if (const int rg = mc_regroup(c, const_cast<Dav1dHipMcList *>(ml), rp, n_refs)) return rg;
    return timed_launches<40>(c, ms, counts, [&](int k, size_t &cnt) {
        int rc = 0;
        if (k < 5) {
            cnt = l->f_n[k];
            if (cnt) rc = dav1d_hip_launch_recon_fused_out(&dp, rp, n_refs, dst->bpc, k, l->f_tiles[k], l->f_tasks[k], (int) cnt, prep, coef, c->recon_coop_below,
                                                           dst_twin != nullptr, dst_twin, c->stream);
        } else if (k < 20) {
            const int b = k - 5;
            cnt = ml->off[b + 1] - ml->off[b];
            if (cnt && dst_twin) rc = dav1d_hip_launch_mc_bin_twin(&dp, rp, n_refs, dst->bpc, b, ml->dev + ml->off[b], (int) cnt, prep, dst_twin, c->stream);
            else if (cnt) rc = dav1d_hip_launch_mc_bin(&dp, rp, n_refs, dst->bpc, b, ml->dev + ml->off[b], (int) cnt, prep, c->stream);
        } else if (k == 20) {
            cnt = l->inter->comp->n;
            if (cnt) rc = dav1d_hip_comp_list_run(c, l->inter->comp, dst, prep, mask);
        } else {
            const int b = k - 21;
            cnt = l->itx->off[b + 1] - l->itx->off[b];
            if (cnt) rc = dav1d_hip_launch_itx_bin_out(&dp, dst->bpc, b, l->itx->dev + l->itx->off[b], (int) cnt, coef, dst_twin != nullptr, dst_twin, c->stream);
        }
        return rc;
    });
}
int dav1d_hip_recon_list_run_timed(Dav1dHipContext *c, const Dav1dHipReconList *l, const Dav1dHipPicture *dst,
                                   const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask, void *coef,
                                   float *ms, size_t *counts) {
    if (!raster_dst_ok(dst)) return -EINVAL;
    return recon_list_run_timed_impl(c, l, dst, refs, n_refs, prep, mask, coef, ms, counts, nullptr);
}
// the launches of dav1d_hip_recon_list_run_tiled the same way (-ENOTSUP when the list cannot run with its picture in the twin only)
int dav1d_hip_recon_list_run_tiled_timed(Dav1dHipContext *c, const Dav1dHipReconList *l, Dav1dHipPicture *dst,
                                         const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask, void *coef,
                                         float *ms, size_t *counts) {
    if (!c || !l || !dst || !refs) return -EINVAL;
    if (const int rc = twin_on_demand(c, dst)) return rc;
    if (!recon_list_twin_direct(c, l, dst, refs, n_refs)) return -ENOTSUP;
    if (!dst->twin_ok) { const int rc = dav1d_hip_picture_retile(c, dst); if (rc) return rc; }
    const DevPlanes tw = twin_planes(dst, 2);
    const int rc = recon_list_run_timed_impl(c, l, dst, refs, n_refs, prep, mask, coef, ms, counts, &tw);
    dst->twin_ok = rc ? 0 : DAV1D_HIP_TWIN_ONLY;
    return rc;
}
} // extern "C"
