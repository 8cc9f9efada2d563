// Host side of the C ABI: the itx, mc, comp and inter task lists (binning, device copies, launches) and their *_batch calls.
#include "lists.h"
#include "av1_scan_prefix.h"
#include <stdlib.h>
#include <string.h>
#include <new>
#include <algorithm>
#include <unordered_set>

// ---------------------------------------------------------------------- itx

// legal (size, type) pairs, reference src/itx_tmpl.c:160-178 / 264-291
static bool itx_legal(int tx, int txtp) {
    if (tx < 0 || tx >= 19 || txtp < 0 || txtp > 16) return false;
    if (txtp == 16) return tx == 0;
    const int w = k_tx_w[tx], h = k_tx_h[tx];
    const int mx = w > h ? w : h;
    if (mx == 64) return txtp == 0;
    if (mx == 32) return txtp == 0 || txtp == 9;
    if (w == 16 && h == 16) return txtp <= 11;
    return true;
}

bool itx_task_ok(const Dav1dHipItxTask &t) {
    if (!itx_legal(t.tx, t.txtp) || t.plane > 2 || t.eob < 0 || t.flags > DAV1D_HIP_ITX_PACKED) return false;
    return t.eob < av1_scan_prefix_off[t.tx + 1] - av1_scan_prefix_off[t.tx];
}

// How much of the slab can be non-zero: coefficients past the eob in scan order are zero by contract (the entropy
// decoder only writes scan positions <= eob, src/recon_tmpl.c:458-520, and itx leaves slabs zeroed), so the kernel
// reads and re-zeroes only the prefix [0, end).  2-D classes: the zig-zag's reach; H classes: the scan is the
// slab order itself; V classes: every column can be touched.  The device copy carries `end` in the pad bytes.
void itx_fill_prefix(Dav1dHipItxTask &t) {
    const int ncoef = av1_scan_prefix_off[t.tx + 1] - av1_scan_prefix_off[t.tx];
    int end = ncoef;
    if (t.txtp <= 9 || t.txtp == 16) end = av1_scan_prefix_end[av1_scan_prefix_off[t.tx] + t.eob];
    else if (t.txtp == 11 || t.txtp == 13 || t.txtp == 15) end = t.eob + 1;
    t.rsv[0] = (uint8_t) (end & 255);
    t.rsv[1] = (uint8_t) (end >> 8);
}

// code path of a transform block: dc-only shortcut, else its two 1-D kinds (txtp_kinds() in itx_body.h); 16 = WHT
int itx_path_key(const Dav1dHipItxTask &t) {
    static const uint8_t kinds[17] = {
        0 | 0 << 2, 0 | 1 << 2, 1 | 0 << 2, 1 | 1 << 2, 0 | 3 << 2, 3 | 0 << 2, 3 | 3 << 2, 3 | 1 << 2,
        1 | 3 << 2, 2 | 2 << 2, 2 | 0 << 2, 0 | 2 << 2, 2 | 1 << 2, 1 | 2 << 2, 2 | 3 << 2, 3 | 2 << 2, 16 };
    return t.txtp == 0 && t.eob < 1 ? 0 : 1 + kinds[t.txtp];
}

extern "C" {

int dav1d_hip_itx_list_create(Dav1dHipContext *c, Dav1dHipItxList **out, const Dav1dHipItxTask *tasks, size_t n) {
    if (!out || (!tasks && n)) return -EINVAL;
    *out = nullptr;
    Dav1dHipItxList *l = new (std::nothrow) Dav1dHipItxList();
    if (!l) return -ENOMEM;
    memset(l, 0, sizeof(*l));
    l->n = n;
    size_t cnt[19] = { 0 };
    for (size_t i = 0; i < n; i++) {
        const Dav1dHipItxTask &t = tasks[i];
        if (!itx_task_ok(t)) { delete l; return -EINVAL; }
        cnt[t.tx]++;
    }
    for (int b = 0; b < 19; b++) l->off[b + 1] = l->off[b] + cnt[b];
    if (n) {
        std::vector<Dav1dHipItxTask> sorted(n);
        size_t pos[19];
        for (int b = 0; b < 19; b++) pos[b] = l->off[b];
        for (size_t i = 0; i < n; i++) {
            Dav1dHipItxTask &t = sorted[pos[tasks[i].tx]++] = tasks[i];          // stable: keeps decode order inside a bin
            itx_fill_prefix(t);
        }
        // Blocks that share a wave should share their code path: a wave runs every 1-D kernel (and the dc-only shortcut) that
        // any of its blocks needs, one after the other.  Inside windows of consecutive blocks (still close together in the
        // picture, so the destination lines stay in L2) the blocks are grouped by (dc-only, first kind, second kind).  The
        // blocks of one list write disjoint pixels, so their order is free.  Speed only.
        static const int win_waves = getenv("DAV1D_HIP_ITX_SORT_WINDOW") ? atoi(getenv("DAV1D_HIP_ITX_SORT_WINDOW")) : 128;
        if (win_waves > 0) {
            auto key = [](const Dav1dHipItxTask &t) -> int { return itx_path_key(t); };
            for (int b = 0; b < 19; b++) {
                const int w = k_tx_w[b], h = k_tx_h[b];
                const int lanes = std::max(std::min(h, 32), w);
                const size_t win = (size_t) win_waves * (size_t) std::max(1, 64 / lanes);
                for (size_t lo = l->off[b]; lo < l->off[b + 1]; lo += win) {
                    const size_t hi = std::min(lo + win, l->off[b + 1]);
                    std::stable_sort(sorted.begin() + lo, sorted.begin() + hi,
                                     [&](const Dav1dHipItxTask &p, const Dav1dHipItxTask &q) { return key(p) < key(q); });
                }
            }
        }
        if (hipMalloc((void **) &l->dev, n * sizeof(Dav1dHipItxTask)) != hipSuccess) { delete l; return -ENOMEM; }
        const int rc = dav1d_hip_upload(c, l->dev, sorted.data(), n * sizeof(Dav1dHipItxTask));
        if (rc) { hipFree(l->dev); delete l; return rc; }
    }
    *out = l;
    return 0;
}

void dav1d_hip_itx_list_destroy(Dav1dHipContext *c, Dav1dHipItxList *l) {
    if (!l) return;
    hipStreamSynchronize(c->stream);
    if (l->dev) hipFree(l->dev);
    delete l;
}

int dav1d_hip_itx_list_run(Dav1dHipContext *c, const Dav1dHipItxList *l, const Dav1dHipPicture *dst, void *coef) {
    if (!l || !raster_dst_ok(dst)) return -EINVAL;
    const DevPlanes dp = dev_planes(dst);
    // longest-running shapes first (k_itx_launch_order), each on its own side stream
    // short lists (the residuals of one intra wavefront step): every size in one launch
    static const size_t one_launch_below = getenv("DAV1D_HIP_ITX_ONE_LAUNCH") ? (size_t) atol(getenv("DAV1D_HIP_ITX_ONE_LAUNCH")) : 4096;
    if (l->n && l->n < one_launch_below) return dav1d_hip_launch_itx_all(&dp, dst->bpc, l->dev, l->off, coef, c->stream);
    StreamFan fan(c, l->n >= 16384);
    int rc = 0;
    for (int k = 0; k < 19 && !rc; k++) {
        const int b = k_itx_launch_order[k];
        const size_t cnt = l->off[b + 1] - l->off[b];
        if (!cnt) continue;
        rc = dav1d_hip_launch_itx_bin(&dp, dst->bpc, b, l->dev + l->off[b], (int) cnt, coef, fan.next());
    }
    fan.join();
    return rc;
}

// Same launches, each bracketed by HIP events on the context's stream; ms[b] receives the
// duration of bin b's kernel (0 for empty bins).  Measurement aid for bench.py.  The *_timed aids of the itx, mc and inter lists (not dav1d_hip_recon_list_run_timed,
// which is guarded like the run it times) take
// `dst` as somewhere to write: they run on the raster planes of a picture in any state and leave twin_ok alone (bench.py times them on
// the pictures of its tiled steps); what they leave in the raster planes of a DAV1D_HIP_TWIN_ONLY picture is not the picture.
int dav1d_hip_itx_list_run_timed(Dav1dHipContext *c, const Dav1dHipItxList *l, const Dav1dHipPicture *dst, void *coef,
                                 float *ms, size_t *counts) {
    if (!l || !dst || !ms) return -EINVAL;
    const DevPlanes dp = dev_planes(dst);
    return timed_launches<19>(c, ms, counts, [&](int b, size_t &cnt) {
        cnt = l->off[b + 1] - l->off[b];
        return cnt ? dav1d_hip_launch_itx_bin(&dp, dst->bpc, b, l->dev + l->off[b], (int) cnt, coef, c->stream) : 0;
    });
}

int dav1d_hip_itx_add_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipItxTask *tasks,
                            size_t n, void *coef) {
    if (!raster_dst_ok(dst)) return -EINVAL;
    Dav1dHipItxList *l = nullptr;
    int rc = dav1d_hip_itx_list_create(c, &l, tasks, n);
    if (rc) return rc;
    KernelTimer kt(c);
    rc = dav1d_hip_itx_list_run(c, l, dst, coef);
    kt.stop();
    dav1d_hip_itx_list_destroy(c, l);     // synchronises the stream
    return rc;
}

} // extern "C"

// ----------------------------------------------------------------------- mc


// DAV1D_HIP_MC_FUSED: which tile shapes share one launch over a source-ordered list instead of one launch per shape.
//   0  none;  2  the shapes that are at least 16 wide (bins 6 .. 14);  1  all of them.
// Measured on MI355X (8K 10-bit synthetic frame): mode 1 cuts the fetch traffic by a third (lines are shared across
// shapes while they sit in L2) but runs 10 % slower than per-shape launches, because every wave then pays the LDS / VGPR
// footprint of the hungriest (small-tile) shape.
int mc_fused_min_bin() {
    static const int mode = getenv("DAV1D_HIP_MC_FUSED") ? atoi(getenv("DAV1D_HIP_MC_FUSED")) : 0;
    return mode == 1 ? 0 : mode == 2 ? 6 : 15;
}

int tile_dim_class(int v) { return v <= 4 ? 0 : v <= 8 ? 1 : v <= 16 ? 2 : v <= 32 ? 3 : 4; }

int mc_task_valid(const Dav1dHipMcTask &t) {
    // widths are powers of two; heights too, except the 3/4-height `lap` predictions of obmc() (6, 12, 24 rows)
    return !(t.w < 2 || t.w > 128 || t.h < 2 || t.h > 128 || (t.w & (t.w - 1)) || (t.h & 1) ||
             t.mx > 15 || t.my > 15 || t.filter_2d > 9 || t.kind > 2 || t.plane > 2 || t.ref > 7);
}

McRef mc_ref_of(const Dav1dHipMcTask &t) {
    McRef r;
    memset(&r, 0, sizeof(r));
    r.src_x = t.src_x; r.src_y = t.src_y;
    r.mx = t.mx; r.my = t.my; r.ref = t.ref;
    if (t.filter_2d == 9) {
        r.fh = r.fv = 6;
    } else {
        // enum Filter2d -> (h type, v type) with REGULAR 0, SMOOTH 1, SHARP 2 (reference src/levels.h:184-196,
        // src/mc_tmpl.c:395-403); 4-tap rows for w <= 4 / h <= 4 (src/mc_tmpl.c:115-123)
        static const uint8_t ht[9] = { 0, 0, 0, 2, 2, 2, 1, 1, 1 };
        static const uint8_t vt[9] = { 0, 1, 2, 0, 1, 2, 0, 1, 2 };
        const int h_type = ht[t.filter_2d], v_type = vt[t.filter_2d];
        r.fh = t.w > 4 ? h_type : 3 + (h_type & 1);
        r.fv = t.h > 4 ? v_type : 3 + (v_type & 1);
    }
    r.vspan = av1_mc_tap_span_host[r.fv * 16 + r.my];
    r.hspan = av1_mc_tap_span_host[r.fh * 16 + r.mx];
    return r;
}

// cut one prediction block (or a fused pair) into <= 64x16 tiles and bin them by tile shape
void push_tiles(std::vector<McTile> *bins, const Dav1dHipMcTask &t, int kind, uint32_t dst_off,
                       const Dav1dHipMcTask *second, int weight, std::vector<McTile> *single) {
    McTile m;
    memset(&m, 0, sizeof(m));
    m.dst_off = dst_off;
    m.kind = kind; m.plane = t.plane; m.bw = t.w; m.weight = (int8_t) weight;
    const McRef r0 = mc_ref_of(t), r1 = second ? mc_ref_of(*second) : r0;
    const int tw = t.w < 64 ? t.w : 64, th = t.h < 16 ? t.h : 16;   // strips of one block, up to 64x16
    const int cls = tile_dim_class(tw) * 3 + tile_dim_class(th);
    for (int oy = 0; oy < t.h; oy += th)
        for (int ox = 0; ox < t.w; ox += tw) {
            m.w = tw; m.h = std::min(th, t.h - oy); m.ox = ox; m.oy = oy;
            m.r[0] = r0; m.r[0].src_x += ox; m.r[0].src_y += oy;
            m.r[1] = r1; m.r[1].src_x += ox; m.r[1].src_y += oy;
            if (single) single->push_back(m); else bins[cls].push_back(m);
        }
}

static int mc_list_from_bins(Dav1dHipContext *c, Dav1dHipMcList **out, std::vector<McTile> *bins) {
    Dav1dHipMcList *l = new (std::nothrow) Dav1dHipMcList();
    if (!l) return -ENOMEM;
    memset(l, 0, sizeof(*l));
    // Order the tiles of a bin by where they READ: (reference, plane, 64-row band, x).  The fetch of a tile is
    // row-granular (a 128-byte line per window row), so tiles that land on the same lines should run back to back on
    // one XCD while those lines sit in its L2; dst writes stay local because MVs are short.  Speed only.
    static const int sort_mode = getenv("DAV1D_HIP_MC_SORT") ? atoi(getenv("DAV1D_HIP_MC_SORT")) : 1;
    if (sort_mode) {
        auto key = [](const McTile &t) -> uint64_t {
            const McRef &r = t.r[0];
            const uint64_t y = (uint64_t) (r.src_y + 4096) & 0xffff, x = (uint64_t) (r.src_x + 4096) & 0xffff;
            if (sort_mode == 2) return ((uint64_t) r.ref << 56) | ((uint64_t) t.plane << 52) | ((x >> 9) << 40) | (y << 16) | x;
            if (sort_mode == 3) return ((uint64_t) t.plane << 52) | ((y >> 6) << 32) | (x << 8) | r.ref;
            return ((uint64_t) r.ref << 56) | ((uint64_t) t.plane << 52) | ((y >> 6) << 32) | x;
        };
        for (int b = 0; b < MC_BINS; b++)
            std::stable_sort(bins[b].begin(), bins[b].end(), [&](const McTile &p, const McTile &q) { return key(p) < key(q); });
    }
    std::vector<McTile> all;
    for (int b = 0; b < MC_BINS; b++) {
        l->off[b] = all.size();
        all.insert(all.end(), bins[b].begin(), bins[b].end());
    }
    l->off[MC_BINS] = all.size();
    l->n = all.size();
    for (const McTile &t : all) {
        const bool two = t.kind == MCT_AVG || t.kind == MCT_WAVG;
        l->max_ref = std::max(l->max_ref, std::max((int) t.r[0].ref, two ? (int) t.r[1].ref : 0));
    }
    if (l->n) {
        if (hipMalloc((void **) &l->dev, l->n * sizeof(McTile)) != hipSuccess) { delete l; return -ENOMEM; }
        int rc = dav1d_hip_upload(c, l->dev, all.data(), l->n * sizeof(McTile));
        if (!rc && !(l->host = (McTile *) malloc(l->n * sizeof(McTile)))) rc = -ENOMEM;
        if (rc) { hipFree(l->dev); delete l; return rc; }
        memcpy(l->host, all.data(), l->n * sizeof(McTile));
        // All shapes in one list: cells of (reference, plane, 64-row band, 512-pixel strip) of the SOURCE position, shapes
        // kept together inside a cell so that a wave gets a full group of one shape; a group never leaves its cell.
        struct Ent { uint64_t key; uint32_t idx; };
        const int fb = mc_fused_min_bin();
        l->n_fused = l->n - l->off[fb];
        std::vector<Ent> ord(l->n_fused);
        for (int b = fb; b < MC_BINS; b++)
            for (size_t i = l->off[b]; i < l->off[b + 1]; i++) {
                const McRef &r = all[i].r[0];
                const uint64_t y = (uint64_t) (r.src_y + 4096) & 0xffff, x = (uint64_t) (r.src_x + 4096) & 0xffff;
                Ent &e = ord[i - l->off[fb]];
                e.key = ((uint64_t) r.ref << 60) | ((uint64_t) all[i].plane << 58) | ((y >> 6) << 48) | ((x >> 9) << 42) |
                             ((uint64_t) b << 38) | (x << 16) | y;
                e.idx = (uint32_t) i;
            }
        std::sort(ord.begin(), ord.end(), [](const Ent &p, const Ent &q) { return p.key < q.key; });
        std::vector<McTile> fused(l->n_fused);
        std::vector<McGroup> groups;
        uint64_t cur = ~0ull;
        for (size_t i = 0; i < l->n_fused; i++) {
            fused[i] = all[ord[i].idx];
            const uint64_t cell_cls = ord[i].key >> 38;
            const int cls = (int) (cell_cls & 15);
            const int tw = 4 << (cls / 3), th = 4 << (cls % 3);
            const int per_wave = 64 / (tw * th / 4 < 64 ? tw * th / 4 : 64);
            if (cell_cls != cur || groups.back().n >= per_wave) {
                McGroup g = { (uint32_t) i, 0, (uint16_t) cls };
                groups.push_back(g);
                cur = cell_cls;
            }
            groups.back().n++;
        }
        l->n_groups = groups.size();
        if (l->n_fused) {
            if (hipMalloc((void **) &l->dev_all, l->n_fused * sizeof(McTile)) != hipSuccess ||
                hipMalloc((void **) &l->groups, groups.size() * sizeof(McGroup)) != hipSuccess) rc = -ENOMEM;
            if (!rc) rc = dav1d_hip_upload(c, l->dev_all, fused.data(), l->n_fused * sizeof(McTile));
            if (!rc) rc = dav1d_hip_upload(c, l->groups, groups.data(), groups.size() * sizeof(McGroup));
        }
        if (rc) { hipFree(l->dev); free(l->host); if (l->dev_all) hipFree(l->dev_all); if (l->groups) hipFree(l->groups); delete l; return rc; }
    }
    *out = l;
    return 0;
}

// Tiles that share a wave should share their code path: a wave runs the edge-emulating gather if ANY of its tiles leaves
// the reference plane, and the second prediction if ANY of them is a fused compound.  Inside windows of consecutive tiles
// (the source order, so the lines they read stay together) the tiles are grouped by (leaves the plane, kind).  Which tiles
// leave the plane depends on the reference geometry, known only at run time: done on the first run and again whenever the
// geometry changes.  The tiles of one list write disjoint rectangles (BLEND_V aside, which lives in the comp list), so
// their order is free.  Speed only.
uint64_t dav1d_hip_mc_geo_sig(const DevPlanes *rp, int n_refs) {
    uint64_t sig = 0xcbf29ce484222325ull;
    for (int r = 0; r < n_refs; r++)
        for (int p = 0; p < 3; p++) { sig = (sig ^ (uint32_t) rp[r].w[p]) * 0x100000001b3ull; sig = (sig ^ (uint32_t) rp[r].h[p]) * 0x100000001b3ull; }
    return sig | 1;
}

int mc_regroup(Dav1dHipContext *c, Dav1dHipMcList *l, const DevPlanes *rp, int n_refs) {
    static const int win_waves = getenv("DAV1D_HIP_MC_GROUP_WINDOW") ? atoi(getenv("DAV1D_HIP_MC_GROUP_WINDOW")) : 128;
    if (win_waves <= 0 || !l->n) return 0;
    const uint64_t sig = dav1d_hip_mc_geo_sig(rp, n_refs);
    if (l->geo_sig == sig) return 0;
    std::vector<McTile> g(l->host, l->host + l->n);
    std::vector<uint8_t> key(l->n);
    for (int b = 0; b < MC_BINS; b++) {
        const int tw = 4 << (b / 3), th = 4 << (b % 3);
        const int ws = tw == 4 ? 12 : (tw + 8 + 7) & ~7, ext_x = (ws + 7) / 8 * 8, ext_y = th + 7;   // mc.hip: NCH * 8, WR - 1
        const int lanes = tw * th / 4 < 64 ? tw * th / 4 : 64;
        const size_t win = (size_t) win_waves * (size_t) (64 / lanes);
        if (64 / lanes < 2) continue;                    // one tile per wave: nothing to share
        for (size_t i = l->off[b]; i < l->off[b + 1]; i++) {
            const McTile &t = g[i];
            const bool two = t.kind == MCT_AVG || t.kind == MCT_WAVG;
            bool edge = false;
            for (int k = 0; k < (two ? 2 : 1); k++) {
                const McRef &r = t.r[k];
                const int x0 = r.src_x - 4, y0 = r.src_y - 3;
                edge |= x0 < 0 || y0 < 0 || x0 + ext_x > rp[r.ref].w[t.plane] || y0 + ext_y > rp[r.ref].h[t.plane];
            }
            key[i] = (uint8_t) ((edge ? 16 : 0) | t.kind << 1 | (t.r[0].src_x & 1));       // the column parity: see the paired blocks of recon lists
        }
        std::vector<uint32_t> idx;
        for (size_t lo = l->off[b]; lo < l->off[b + 1]; lo += win) {
            const size_t hi = std::min(lo + win, l->off[b + 1]);
            idx.resize(hi - lo);
            for (size_t i = lo; i < hi; i++) idx[i - lo] = (uint32_t) i;
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t p, uint32_t q) { return key[p] < key[q]; });
            for (size_t i = lo; i < hi; i++) g[i] = l->host[idx[i - lo]];
        }
    }
    hipStreamSynchronize(c->stream);                     // an earlier run may still be reading the old order
    const int rc = dav1d_hip_upload(c, l->dev, g.data(), l->n * sizeof(McTile));
    if (!rc) l->geo_sig = sig;
    return rc;
}

extern "C" {

int dav1d_hip_mc_list_create(Dav1dHipContext *c, Dav1dHipMcList **out, const Dav1dHipMcTask *tasks, size_t n) {
    if (!out || (!tasks && n)) return -EINVAL;
    *out = nullptr;
    std::vector<McTile> bins[MC_BINS];
    for (size_t i = 0; i < n; i++) {
        if (!mc_task_valid(tasks[i])) return -EINVAL;
        push_tiles(bins, tasks[i], tasks[i].kind == DAV1D_HIP_MC_PUT ? MCT_PUT : tasks[i].kind == DAV1D_HIP_MC_PREP ? MCT_PREP : MCT_PUT_TMP,
                   tasks[i].dst_off, nullptr, 0);
    }
    return mc_list_from_bins(c, out, bins);
}

void dav1d_hip_mc_list_destroy(Dav1dHipContext *c, Dav1dHipMcList *l) {
    if (!l) return;
    hipStreamSynchronize(c->stream);
    if (l->dev) hipFree(l->dev);
    free(l->host);
    if (l->dev_all) hipFree(l->dev_all);
    if (l->groups) hipFree(l->groups);
    delete l;
}

int dav1d_hip_mc_list_run(Dav1dHipContext *c, const Dav1dHipMcList *l, const Dav1dHipPicture *dst,
                          const Dav1dHipPicture *refs, int n_refs, int16_t *prep) {
    if (!l || !raster_dst_ok(dst) || !refs) return -EINVAL;
    const DevPlanes dp = dev_planes(dst);
    DevPlanes rp[8];
    if (l->n_fused) {       // the all-shapes launch reads raster planes
        if (const int rv = refs_ok(dst, refs, n_refs, l->max_ref)) return rv;
        if (const int rv = raster_planes_valid(c, refs, n_refs)) return rv;
        for (int i = 0; i < n_refs; i++) rp[i] = dev_planes(&refs[i]);
    } else if (const int rv = checked_ref_planes(c, dst, refs, n_refs, l->n ? l->max_ref : 0, rp)) return rv;
    const int fb = mc_fused_min_bin();
    int rc = mc_regroup(c, const_cast<Dav1dHipMcList *>(l), rp, n_refs);
    if (rc) return rc;
    StreamFan fan(c);
    if (l->n_fused) rc = dav1d_hip_launch_mc_all(&dp, rp, n_refs, dst->bpc, l->dev_all, l->groups, (int) l->n_groups, fb == 0, prep, fan.next());
    for (int b = fb - 1; b >= 0 && !rc; b--) {
        const size_t cnt = l->off[b + 1] - l->off[b];
        if (!cnt) continue;
        rc = dav1d_hip_launch_mc_bin(&dp, rp, n_refs, dst->bpc, b, l->dev + l->off[b], (int) cnt, prep, fan.next());
    }
    fan.join();
    return rc;
}

int dav1d_hip_mc_list_run_timed(Dav1dHipContext *c, const Dav1dHipMcList *l, const Dav1dHipPicture *dst,
                                const Dav1dHipPicture *refs, int n_refs, int16_t *prep, float *ms, size_t *counts) {
    if (!l || !dst || !refs || !ms) return -EINVAL;
    const DevPlanes dp = dev_planes(dst);
    DevPlanes rp[8];
    if (const int rv = checked_ref_planes(c, nullptr, refs, n_refs, l->n ? l->max_ref : 0, rp)) return rv;
    if (int rg = mc_regroup(c, const_cast<Dav1dHipMcList *>(l), rp, n_refs)) return rg;
    return timed_launches<MC_BINS>(c, ms, counts, [&](int b, size_t &cnt) {
        cnt = l->off[b + 1] - l->off[b];
        return cnt ? dav1d_hip_launch_mc_bin(&dp, rp, n_refs, dst->bpc, b, l->dev + l->off[b], (int) cnt, prep, c->stream) : 0;
    });
}

int dav1d_hip_mc_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipPicture *refs, int n_refs,
                       const Dav1dHipMcTask *tasks, size_t n, int16_t *prep) {
    if (!raster_dst_ok(dst)) return -EINVAL;
    Dav1dHipMcList *l = nullptr;
    int rc = dav1d_hip_mc_list_create(c, &l, tasks, n);
    if (rc) return rc;
    rc = dav1d_hip_mc_list_run(c, l, dst, refs, n_refs, prep);
    dav1d_hip_mc_list_destroy(c, l);
    return rc;
}

} // extern "C"

// --------------------------------------------------------------------- comp

extern "C" {

int dav1d_hip_comp_list_create(Dav1dHipContext *c, Dav1dHipCompList **out, const Dav1dHipCompTask *tasks, size_t n) {
    if (!out || (!tasks && n)) return -EINVAL;
    *out = nullptr;
    for (size_t i = 0; i < n; i++) {
        const Dav1dHipCompTask &t = tasks[i];
        if (t.kind > 6 || t.plane > 2 || t.ss > 2 || t.w > 128 || t.h > 128 || t.w < 2 || t.h < 2 ||
            (t.kind <= 3 && (t.w < 4 || t.h < 4 || (t.w & 1) || (t.h & 1))))
            return -EINVAL;
    }
    Dav1dHipCompList *l = new (std::nothrow) Dav1dHipCompList();
    if (!l) return -ENOMEM;
    l->dev = nullptr;
    l->n = n;
    // obmc() blends the top neighbours' predictions (blend_h) before the left ones (blend_v) and the two overlap in the
    // block's top-left corner (reference src/recon_tmpl.c:1066-1111): keep that order with a second launch
    // The chroma planes of a COMP_INTER_SEG block are combined with the mask its luma W_MASK task wrote
    // (src/recon_tmpl.c:1812-1818, 1882-1889): those MASK tasks wait for the second launch as well.
    std::unordered_set<uint32_t> wmask_out;
    for (size_t i = 0; i < n; i++) if (tasks[i].kind == DAV1D_HIP_COMP_WMASK) wmask_out.insert(tasks[i].mask_off);
    auto second = [&](const Dav1dHipCompTask &t) {
        return t.kind == DAV1D_HIP_COMP_BLEND_V || (t.kind == DAV1D_HIP_COMP_MASK && wmask_out.count(t.mask_off));
    };
    std::vector<Dav1dHipCompTask> sorted;
    sorted.reserve(n);
    for (size_t i = 0; i < n; i++) if (!second(tasks[i])) sorted.push_back(tasks[i]);
    l->n_first = sorted.size();
    for (size_t i = 0; i < n; i++) if (second(tasks[i])) sorted.push_back(tasks[i]);
    if (n) {
        if (hipMalloc((void **) &l->dev, n * sizeof(Dav1dHipCompTask)) != hipSuccess) { delete l; return -ENOMEM; }
        const int rc = dav1d_hip_upload(c, l->dev, sorted.data(), n * sizeof(Dav1dHipCompTask));
        if (rc) { hipFree(l->dev); delete l; return rc; }
    }
    *out = l;
    return 0;
}

void dav1d_hip_comp_list_destroy(Dav1dHipContext *c, Dav1dHipCompList *l) {
    if (!l) return;
    hipStreamSynchronize(c->stream);
    if (l->dev) hipFree(l->dev);
    delete l;
}

static int comp_list_launch(Dav1dHipContext *c, const Dav1dHipCompList *l, const Dav1dHipPicture *dst, const int16_t *prep, uint8_t *mask) {
    const DevPlanes dp = dev_planes(dst);
    int rc = dav1d_hip_launch_comp(&dp, dst->bpc, l->dev, (int) l->n_first, prep, mask, c->stream);
    if (!rc) rc = dav1d_hip_launch_comp(&dp, dst->bpc, l->dev + l->n_first, (int) (l->n - l->n_first), prep, mask, c->stream);
    return rc;
}

int dav1d_hip_comp_list_run(Dav1dHipContext *c, const Dav1dHipCompList *l, const Dav1dHipPicture *dst,
                            const int16_t *prep, uint8_t *mask) {
    if (!l || !raster_dst_ok(dst)) return -EINVAL;
    return comp_list_launch(c, l, dst, prep, mask);
}

int dav1d_hip_comp_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipCompTask *tasks, size_t n,
                         const int16_t *prep, uint8_t *mask) {
    if (!raster_dst_ok(dst)) return -EINVAL;
    Dav1dHipCompList *l = nullptr;
    int rc = dav1d_hip_comp_list_create(c, &l, tasks, n);
    if (rc) return rc;
    rc = dav1d_hip_comp_list_run(c, l, dst, prep, mask);
    dav1d_hip_comp_list_destroy(c, l);
    return rc;
}

} // extern "C"

// ------------------------------------------------------- inter list (mc + comp, fused)

// All inter prediction of a frame / tile-sbrow: the PUT / PREP tasks plus the compound
// tasks that consume the PREP outputs, exactly as the reference driver issues them
// (src/recon_tmpl.c:1784-1826).  Where an AVG / W_AVG task reads two PREP blocks that no
// other task reads, the three are fused into one tile kind (both predictions + combine in
// registers, nothing written to the prep arena).  MASK / W_MASK compounds keep the
// two-step form.

// marks the 4x4 cells of a w x h rectangle at pixel offset `off` of a plane
static void mark_cells(Dav1dHipInterList *l, int plane, uint32_t off, int w, int h, uint16_t bit) {
    const int sp = l->stride_px[plane], cs = l->cell_stride[plane];
    if (sp <= 0) return;
    const int x = (int) (off % (uint32_t) sp), y = (int) (off / (uint32_t) sp);
    for (int cy = y >> 2; cy <= (y + h - 1) >> 2; cy++)
        for (int cx = x >> 2; cx <= (x + w - 1) >> 2; cx++) {
            const size_t i = (size_t) cy * cs + cx;
            if (cx < cs && i < l->writers[plane].size()) l->writers[plane][i] |= bit;
        }
}

extern "C" {

int dav1d_hip_inter_list_create(Dav1dHipContext *c, Dav1dHipInterList **out, const Dav1dHipMcTask *mc, size_t n_mc,
                                const Dav1dHipCompTask *comp, size_t n_comp) {
    return inter_list_create_geo(c, out, mc, n_mc, comp, n_comp, nullptr);
}

} // extern "C"

int inter_list_create_geo(Dav1dHipContext *c, Dav1dHipInterList **out, const Dav1dHipMcTask *mc, size_t n_mc,
                                 const Dav1dHipCompTask *comp, size_t n_comp, const Dav1dHipPicture *geom, ReconPairing *pair) {
    if (!out || (!mc && n_mc) || (!comp && n_comp)) return -EINVAL;
    *out = nullptr;
    // prep offset -> producing PREP task, and how many compound inputs read that offset
    std::unordered_map<uint32_t, size_t> producer;
    std::unordered_map<uint32_t, int> readers;
    for (size_t i = 0; i < n_mc; i++) {
        if (!mc_task_valid(mc[i])) return -EINVAL;
        if (mc[i].kind == DAV1D_HIP_MC_PREP) producer[mc[i].dst_off] = i;
    }
    for (size_t i = 0; i < n_comp; i++) { readers[comp[i].tmp1_off]++; readers[comp[i].tmp2_off]++; }
    // A block some BLEND / BLEND_H / BLEND_V task writes on top of (OBMC, src/recon_tmpl.c:1052-1112) must not be paired:
    // the reference's order is prediction, blends, residual, and a paired wave would add the residual before the blends.
    if (pair)
        for (size_t i = 0; i < n_comp; i++)
            if (comp[i].kind >= DAV1D_HIP_COMP_BLEND) pair->block_blend(comp[i]);
    std::vector<char> fused_prep(n_mc, 0);
    std::vector<Dav1dHipCompTask> rest;
    std::vector<McTile> bins[MC_BINS];
    size_t n_fused = 0;
    for (size_t i = 0; i < n_comp; i++) {
        const Dav1dHipCompTask &k = comp[i];
        bool fuse = k.kind == DAV1D_HIP_COMP_AVG || k.kind == DAV1D_HIP_COMP_WAVG;
        size_t a = 0, b = 0;
        if (fuse) {
            auto pa = producer.find(k.tmp1_off), pb = producer.find(k.tmp2_off);
            fuse = pa != producer.end() && pb != producer.end() && k.tmp1_off != k.tmp2_off &&
                   readers[k.tmp1_off] == 1 && readers[k.tmp2_off] == 1;
            if (fuse) {
                a = pa->second; b = pb->second;
                fuse = mc[a].w == k.w && mc[a].h == k.h && mc[b].w == k.w && mc[b].h == k.h &&
                       mc[a].plane == k.plane && mc[b].plane == k.plane;
            }
        }
        if (fuse) {
            const long j = pair ? pair->find(k.plane, k.dst_off, k.w, k.h) : -1;
            if (j >= 0) { pair->taken[j] = 1; pair->itx_idx[pair->itx[j].tx].push_back((uint32_t) j); }
            push_tiles(bins, mc[a], k.kind == DAV1D_HIP_COMP_AVG ? MCT_AVG : MCT_WAVG, k.dst_off, &mc[b], k.arg,
                       j >= 0 ? &pair->tiles[pair->itx[j].tx] : nullptr);
            fused_prep[a] = fused_prep[b] = 1;
            n_fused++;
        } else {
            rest.push_back(k);
        }
    }
    for (size_t i = 0; i < n_mc; i++)
        if (!fused_prep[i]) {
            const long j = (pair && mc[i].kind == DAV1D_HIP_MC_PUT) ? pair->find(mc[i].plane, mc[i].dst_off, mc[i].w, mc[i].h) : -1;
            if (j >= 0) { pair->taken[j] = 1; pair->itx_idx[pair->itx[j].tx].push_back((uint32_t) j); }
            push_tiles(bins, mc[i], mc[i].kind == DAV1D_HIP_MC_PUT ? MCT_PUT : mc[i].kind == DAV1D_HIP_MC_PREP ? MCT_PREP : MCT_PUT_TMP,
                       mc[i].dst_off, nullptr, 0, j >= 0 ? &pair->tiles[pair->itx[j].tx] : nullptr);
        }
    Dav1dHipInterList *l = new (std::nothrow) Dav1dHipInterList();
    if (!l) return -ENOMEM;
    l->mc = nullptr; l->comp = nullptr; l->n_fused = n_fused;
    for (int p = 0; p < 3; p++) l->cell_stride[p] = l->stride_px[p] = 0;
    if (geom) {
        const int bps = geom->bpc > 8 ? 2 : 1;
        for (int p = 0; p < 3; p++) {
            if (!geom->p[p].data) continue;
            l->stride_px[p] = (int) (geom->p[p].stride / bps);
            l->cell_stride[p] = (l->stride_px[p] + 3) >> 2;
            l->writers[p].assign((size_t) l->cell_stride[p] * (size_t) ((geom->p[p].h + 127 + 3) >> 2), 0);
        }
        for (int b = 0; b < MC_BINS; b++)
            for (const McTile &t : bins[b])
                if (t.kind == MCT_PUT || t.kind == MCT_AVG || t.kind == MCT_WAVG)
                    mark_cells(l, t.plane, t.dst_off + (uint32_t) t.oy * (uint32_t) l->stride_px[t.plane] + t.ox, t.w, t.h, (uint16_t) (1u << b));
        for (const Dav1dHipCompTask &k : rest) mark_cells(l, k.plane, k.dst_off, k.w, k.h, 1u << 15);
    }
    int rc = mc_list_from_bins(c, &l->mc, bins);
    if (!rc) rc = dav1d_hip_comp_list_create(c, &l->comp, rest.data(), rest.size());
    if (rc) { dav1d_hip_mc_list_destroy(c, l->mc); delete l; return rc; }
    *out = l;
    return 0;
}

extern "C" {

void dav1d_hip_inter_list_destroy(Dav1dHipContext *c, Dav1dHipInterList *l) {
    if (!l) return;
    dav1d_hip_mc_list_destroy(c, l->mc);
    dav1d_hip_comp_list_destroy(c, l->comp);
    delete l;
}

int dav1d_hip_inter_list_run(Dav1dHipContext *c, const Dav1dHipInterList *l, const Dav1dHipPicture *dst,
                             const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask) {
    if (!l || !raster_dst_ok(dst)) return -EINVAL;
    int rc = dav1d_hip_mc_list_run(c, l->mc, dst, refs, n_refs, prep);
    if (!rc && l->comp->n) rc = dav1d_hip_comp_list_run(c, l->comp, dst, prep, mask);
    return rc;
}

int dav1d_hip_inter_list_run_timed(Dav1dHipContext *c, const Dav1dHipInterList *l, const Dav1dHipPicture *dst,
                                   const Dav1dHipPicture *refs, int n_refs, int16_t *prep, uint8_t *mask,
                                   float *ms, size_t *counts) {
    if (!l || !ms) return -EINVAL;
    int rc = dav1d_hip_mc_list_run_timed(c, l->mc, dst, refs, n_refs, prep, ms, counts);
    ms[MC_BINS] = 0.f;
    if (counts) counts[MC_BINS] = l->comp->n;
    if (!rc && l->comp->n)
        rc = timed_launches<1>(c, &ms[MC_BINS], nullptr, [&](int, size_t &cnt) {
            cnt = l->comp->n;
            return comp_list_launch(c, l->comp, dst, prep, mask);
        });
    return rc;
}

size_t dav1d_hip_inter_list_fused(const Dav1dHipInterList *l) { return l ? l->n_fused : 0; }

} // extern "C"
