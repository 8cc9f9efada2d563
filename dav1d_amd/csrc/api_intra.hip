// Host side of the C ABI: intra prediction batches and lists, the intra wavefront list, the dataflow launch and the superblock route.
#include "lists.h"
#include <stdlib.h>
#include <string.h>
#include <new>
#include <algorithm>

// -------------------------------------------------------------------- ipred

static int ipred_tasks_valid(const Dav1dHipIpredTask *tasks, size_t n, const uint8_t *aux) {
    for (size_t i = 0; i < n; i++) {
        const Dav1dHipIpredTask &t = tasks[i];
        if (t.plane > 2 || t.kind > DAV1D_HIP_IPRED_COPY || t.mode > 13 || !t.tw || !t.th || t.tw > 16 || t.th > 16) return -EINVAL;
        if (t.kind == DAV1D_HIP_IPRED_COPY) { if ((t.pal[2] & 0xf0f0) != 0) return -EINVAL; continue; }
        if (t.kind >= DAV1D_HIP_IPRED_PAL && t.kind != DAV1D_HIP_IPRED_PRED_TMP && !aux) return -EINVAL;
        if (t.kind == DAV1D_HIP_IPRED_PRED_TMP && (t.tw > 8 || t.th > 8 || t.mode > 12)) return -EINVAL;
        const bool cfl = t.kind == DAV1D_HIP_IPRED_CFL || t.kind >= DAV1D_HIP_IPRED_DSP_CFL_AC;
        if ((cfl || (t.kind != DAV1D_HIP_IPRED_PAL && t.mode == 13)) && (t.tw > 8 || t.th > 8)) return -EINVAL;   // both are limited to 32x32
        if (t.kind == DAV1D_HIP_IPRED_DSP_CFL_PRED && t.mode != 0 && (t.mode < 3 || t.mode > 5)) return -EINVAL;
    }
    return 0;
}

// Blocks of 1024 pixels or more whose predictor has no serial dependency are predicted by four workgroups each
// (ipred.hip: IPRED_PARTS); they go first in a batch so that the grid holds exactly 4 * n_big + n_small workgroups.
// The tasks of one batch are independent of each other, so their order is free.
static bool ipred_task_big(const Dav1dHipIpredTask &t) {
    if ((int) t.tw * t.th * 16 < 1024) return false;
    if (t.kind == DAV1D_HIP_IPRED_PAL) return true;
    return (t.kind == DAV1D_HIP_IPRED_PRED || t.kind == DAV1D_HIP_IPRED_DSP) && t.mode != 13;      // 13 = filter intra: serial
}
static size_t ipred_big_first(Dav1dHipIpredTask *t, size_t n) {
    return (size_t) (std::stable_partition(t, t + n, ipred_task_big) - t);
}

extern "C" int dav1d_hip_ipred_batch(Dav1dHipContext *c, const Dav1dHipPicture *dst, const Dav1dHipIpredTask *tasks, size_t n,
                                     uint8_t *pal_idx) {
    if (!raster_dst_ok(dst) || (!tasks && n)) return -EINVAL;
    if (!n) return 0;
    if (ipred_tasks_valid(tasks, n, pal_idx)) return -EINVAL;
    std::vector<Dav1dHipIpredTask> ordered(tasks, tasks + n);
    const size_t n_big = ipred_big_first(ordered.data(), n);
    TaskBuf dev_buf(c, n * sizeof(Dav1dHipIpredTask));
    Dav1dHipIpredTask *const dev = reinterpret_cast<Dav1dHipIpredTask *>(dev_buf.p);
    if (!dev) return -ENOMEM;
    int rc = dav1d_hip_upload(c, dev, ordered.data(), n * sizeof(*dev));
    const DevPlanes dp = dev_planes(dst);
    KernelTimer kt(c);
    if (!rc) rc = dav1d_hip_launch_ipred(&dp, dst->bpc, dst->layout, dev, (int) n, (int) n_big, pal_idx, nullptr, c->stream);
    kt.stop();
    hipStreamSynchronize(c->stream);
    return rc;
}

// Device-resident wavefront: the batches of an intra frame (or of the intra blocks of an inter frame) uploaded once; batch k
// = tasks [start[k], start[k + 1]).  run_batch() only enqueues the launch, so a caller can interleave the residual lists of
// every wave on the same stream without a host round trip per wave.
struct Dav1dHipIpredList {
    Dav1dHipIpredTask *dev;
    std::vector<size_t> start, n_big;     // batch k = tasks [start[k], start[k + 1]), its first n_big[k] are split four ways
    bool needs_aux, needs_tmp;
};

extern "C" int dav1d_hip_ipred_list_create(Dav1dHipContext *c, Dav1dHipIpredList **out, const Dav1dHipIpredTask *tasks,
                                           const size_t *batch_sizes, size_t n_batches) {
    if (!out || !batch_sizes) return -EINVAL;
    *out = nullptr;
    size_t n = 0;
    for (size_t k = 0; k < n_batches; k++) n += batch_sizes[k];
    if (n && !tasks) return -EINVAL;
    uint8_t dummy = 0;
    if (ipred_tasks_valid(tasks, n, &dummy)) return -EINVAL;
    Dav1dHipIpredList *l = new (std::nothrow) Dav1dHipIpredList();
    if (!l) return -ENOMEM;
    l->dev = nullptr;
    l->needs_aux = l->needs_tmp = false;
    for (size_t i = 0; i < n; i++) {
        if (tasks[i].kind >= DAV1D_HIP_IPRED_PAL && tasks[i].kind < DAV1D_HIP_IPRED_PRED_TMP) l->needs_aux = true;
        if (tasks[i].kind == DAV1D_HIP_IPRED_PRED_TMP) l->needs_tmp = true;
    }
    l->start.push_back(0);
    for (size_t k = 0; k < n_batches; k++) l->start.push_back(l->start.back() + batch_sizes[k]);
    if (n) {
        std::vector<Dav1dHipIpredTask> ordered(tasks, tasks + n);
        for (size_t k = 0; k < n_batches; k++) l->n_big.push_back(ipred_big_first(ordered.data() + l->start[k], batch_sizes[k]));
        if (hipMalloc((void **) &l->dev, n * sizeof(Dav1dHipIpredTask)) != hipSuccess) { delete l; return -ENOMEM; }
        const int rc = dav1d_hip_upload(c, l->dev, ordered.data(), n * sizeof(Dav1dHipIpredTask));
        if (rc) { hipFree(l->dev); delete l; return rc; }
    }
    *out = l;
    return 0;
}

// tmp: the scratch (prep) arena PRED_TMP tasks write to; NULL when the list holds none
static int ipred_list_run_batch_tmp(Dav1dHipContext *c, const Dav1dHipIpredList *l, size_t batch, const Dav1dHipPicture *dst, uint8_t *aux,
                                    void *tmp) {
    if (!l || !raster_dst_ok(dst) || batch + 1 >= l->start.size() || (l->needs_aux && !aux) || (l->needs_tmp && !tmp)) return -EINVAL;
    const size_t n = l->start[batch + 1] - l->start[batch];
    if (!n) return 0;
    const DevPlanes dp = dev_planes(dst);
    return dav1d_hip_launch_ipred(&dp, dst->bpc, dst->layout, l->dev + l->start[batch], (int) n, (int) l->n_big[batch], aux, tmp, c->stream);
}

extern "C" int dav1d_hip_ipred_list_run_batch(Dav1dHipContext *c, const Dav1dHipIpredList *l, size_t batch, const Dav1dHipPicture *dst,
                                              uint8_t *aux) {
    return ipred_list_run_batch_tmp(c, l, batch, dst, aux, nullptr);
}

extern "C" void dav1d_hip_ipred_list_destroy(Dav1dHipContext *c, Dav1dHipIpredList *l) {
    if (!l) return;
    hipStreamSynchronize(c->stream);
    if (l->dev) hipFree(l->dev);
    delete l;
}

extern "C" {

// ------------------------------------------------------------------ intra wavefront list
//
// The batches (wavefront steps) of an intra frame with both halves of every block: predictions and residuals.  A 4x4 or 8x8
// block whose residual covers exactly its prediction runs as a pair in one wave (intra_pair.hip); the other blocks of the
// step keep the prediction launch + residual launch route.  run_batch() only enqueues: at most three launches per step, one
// for the steps that hold nothing but small blocks (the second half of every superblock's wavefront).
struct Dav1dHipIntraList {
    Dav1dHipIpredList *preds;                 // unpaired predictions, batch by batch
    std::vector<Dav1dHipItxList *> itx;       // unpaired residuals, one list per batch
    Dav1dHipIpredTask *p_dev;                 // paired blocks of all batches: predictions ...
    Dav1dHipItxTask *t_dev;                   // ... and their residuals, same order
    std::vector<size_t> pair_start;           // batch k = pairs [pair_start[k], pair_start[k + 1])
    Dav1dHipCompTask *b_dev;                  // inter-intra blends of all batches (run between a batch's predictions and residuals)
    std::vector<size_t> blend_start;          // batch k = blends [blend_start[k], blend_start[k + 1])
    bool needs_aux;
};

void dav1d_hip_intra_list_destroy(Dav1dHipContext *c, Dav1dHipIntraList *l) {
    if (!l) return;
    if (l->preds) dav1d_hip_ipred_list_destroy(c, l->preds);
    for (Dav1dHipItxList *t : l->itx) if (t) dav1d_hip_itx_list_destroy(c, t);
    hipStreamSynchronize(c->stream);
    if (l->p_dev) hipFree(l->p_dev);
    if (l->t_dev) hipFree(l->t_dev);
    if (l->b_dev) hipFree(l->b_dev);
    delete l;
}

int dav1d_hip_intra_list_create(Dav1dHipContext *c, Dav1dHipIntraList **out, const Dav1dHipIpredTask *preds, const size_t *pred_sizes,
                                const Dav1dHipItxTask *txs, const size_t *tx_sizes, size_t n_batches) {
    return dav1d_hip_intra_list_create_blend(c, out, preds, pred_sizes, txs, tx_sizes, nullptr, nullptr, n_batches);
}

int dav1d_hip_intra_list_create_blend(Dav1dHipContext *c, Dav1dHipIntraList **out, const Dav1dHipIpredTask *preds, const size_t *pred_sizes,
                                      const Dav1dHipItxTask *txs, const size_t *tx_sizes, const Dav1dHipCompTask *blends,
                                      const size_t *blend_sizes, size_t n_batches) {
    if (!c || !out || !pred_sizes || !tx_sizes) return -EINVAL;
    *out = nullptr;
    size_t np = 0, nt = 0;
    for (size_t k = 0; k < n_batches; k++) { np += pred_sizes[k]; nt += tx_sizes[k]; }
    if ((np && !preds) || (nt && !txs)) return -EINVAL;
    uint8_t dummy = 0;
    if (ipred_tasks_valid(preds, np, &dummy)) return -EINVAL;
    for (size_t i = 0; i < nt; i++) if (!itx_task_ok(txs[i])) return -EINVAL;
    Dav1dHipIntraList *l = new (std::nothrow) Dav1dHipIntraList();
    if (!l) return -ENOMEM;
    l->preds = nullptr; l->p_dev = nullptr; l->t_dev = nullptr; l->b_dev = nullptr; l->needs_aux = false;
    for (size_t i = 0; i < np; i++) if (preds[i].kind >= DAV1D_HIP_IPRED_PAL && preds[i].kind < DAV1D_HIP_IPRED_PRED_TMP) l->needs_aux = true;
    l->blend_start.push_back(0);
    for (size_t k = 0; k < n_batches; k++) l->blend_start.push_back(l->blend_start.back() + (blend_sizes ? blend_sizes[k] : 0));
    if (l->blend_start.back()) {
        const size_t nb = l->blend_start.back();
        for (size_t i = 0; i < nb; i++)
            if (!blends || blends[i].kind != DAV1D_HIP_COMP_BLEND || blends[i].plane > 2 || blends[i].w < 4 || blends[i].h < 4) { delete l; return -EINVAL; }
        if (hipMalloc((void **) &l->b_dev, nb * sizeof(Dav1dHipCompTask)) != hipSuccess) { delete l; return -ENOMEM; }
        const int brc = dav1d_hip_upload(c, l->b_dev, blends, nb * sizeof(Dav1dHipCompTask));
        if (brc) { hipFree(l->b_dev); delete l; return brc; }
    }
    static const bool pairing = !(getenv("DAV1D_HIP_INTRA_PAIR") && !atoi(getenv("DAV1D_HIP_INTRA_PAIR")));
    std::vector<Dav1dHipIpredTask> rest_p, pair_p;
    std::vector<Dav1dHipItxTask> pair_t;
    std::vector<size_t> rest_p_sizes;
    int rc = 0;
    size_t p0 = 0, t0 = 0;
    l->pair_start.push_back(0);
    for (size_t k = 0; k < n_batches && !rc; k++) {
        std::unordered_map<uint64_t, size_t> tx_at;
        for (size_t i = 0; i < tx_sizes[k]; i++) {
            const Dav1dHipItxTask &t = txs[t0 + i];
            if (pairing && t.tx <= 1) tx_at[(uint64_t) t.plane << 32 | t.dst_off] = i;
        }
        std::vector<char> taken(tx_sizes[k], 0);
        size_t n_rest = 0;
        for (size_t i = 0; i < pred_sizes[k]; i++) {
            const Dav1dHipIpredTask &p = preds[p0 + i];
            long j = -1;
            if (p.tw == p.th && p.tw <= 2 && p.kind <= DAV1D_HIP_IPRED_PAL) {
                auto it = tx_at.find((uint64_t) p.plane << 32 | p.dst_off);
                if (it != tx_at.end() && !taken[it->second] && txs[t0 + it->second].tx == p.tw - 1) j = (long) it->second;
            }
            if (j >= 0) {
                taken[j] = 1;
                pair_p.push_back(p);
                pair_t.push_back(txs[t0 + j]);
                itx_fill_prefix(pair_t.back());
            } else {
                rest_p.push_back(p);
                n_rest++;
            }
        }
        rest_p_sizes.push_back(n_rest);
        l->pair_start.push_back(pair_p.size());
        std::vector<Dav1dHipItxTask> rest_t;
        for (size_t i = 0; i < tx_sizes[k]; i++) if (!taken[i]) rest_t.push_back(txs[t0 + i]);
        Dav1dHipItxList *tl = nullptr;
        rc = dav1d_hip_itx_list_create(c, &tl, rest_t.data(), rest_t.size());
        l->itx.push_back(tl);
        p0 += pred_sizes[k]; t0 += tx_sizes[k];
    }
    if (!rc) rc = dav1d_hip_ipred_list_create(c, &l->preds, rest_p.data(), rest_p_sizes.data(), n_batches);
    if (!rc && !pair_p.empty()) {
        if (hipMalloc((void **) &l->p_dev, pair_p.size() * sizeof(Dav1dHipIpredTask)) != hipSuccess ||
            hipMalloc((void **) &l->t_dev, pair_t.size() * sizeof(Dav1dHipItxTask)) != hipSuccess) rc = -ENOMEM;
        if (!rc) rc = dav1d_hip_upload(c, l->p_dev, pair_p.data(), pair_p.size() * sizeof(Dav1dHipIpredTask));
        if (!rc) rc = dav1d_hip_upload(c, l->t_dev, pair_t.data(), pair_t.size() * sizeof(Dav1dHipItxTask));
    }
    if (rc) { dav1d_hip_intra_list_destroy(c, l); return rc; }
    *out = l;
    return 0;
}

// ------------------------------------------------------------------ intra dataflow launch (intra_flow.hip)
struct Dav1dHipIntraFlow {
    IntraUnit *units;
    uint32_t *ctr;              // [0 .. 31]: error word; then FLOW_SUB counters of FLOW_SUB_STRIDE words per group
    size_t ctr_bytes;
    size_t n_units, n_steps, n_groups;
    bool needs_aux;
};

void dav1d_hip_intra_flow_destroy(Dav1dHipContext *c, Dav1dHipIntraFlow *l) {
    if (!l) return;
    hipStreamSynchronize(c->stream);
    if (l->units) hipFree(l->units);
    if (l->ctr) hipFree(l->ctr);
    delete l;
}
size_t dav1d_hip_intra_flow_units(const Dav1dHipIntraFlow *l) { return l ? l->n_units : 0; }
// after a run: tickets drawn, units finished, waves that gave up waiting (0 unless something is broken); synchronizes
int dav1d_hip_intra_flow_status(Dav1dHipContext *c, const Dav1dHipIntraFlow *l, uint32_t out[3]) {
    if (!c || !l || !out) return -EINVAL;
    // out[0]: unused (tickets are static), out[1]: units finished (sum of every group's counters), out[2]: waves that gave up
    std::vector<uint32_t> w(l->ctr_bytes / 4);
    const int rc = dav1d_hip_download(c, w.data(), l->ctr, l->ctr_bytes);
    uint64_t done = 0;
    for (size_t g = 0; g < l->n_groups; g++)
        for (int k = 0; k < FLOW_SUB; k++) done += w[32 + (g * FLOW_SUB + k) * FLOW_SUB_STRIDE];
    out[0] = 0; out[1] = (uint32_t) done; out[2] = w[0];
    return rc;
}

// Units of one set of tasks sorted by step (*_end[s] = end of step s): per step first the predictions, each with the residual
// of the same rectangle when there is one (that is how the reference walks an intra block: predict a transform block, add
// its residual, next one), then the residuals without a prediction of their own — those wait for every prediction of their
// step (a palette block: one prediction, many residuals).  need is left 0.  -ENOTSUP: a task kind the dataflow launch
// does not run (PRED_TMP of inter-intra blocks, the DSP-level kinds).
int dav1d_hip_intra_units_build(const Dav1dHipIpredTask *preds, const uint32_t *pred_end, const Dav1dHipItxTask *txs, const uint32_t *tx_end,
                                size_t n_steps, std::vector<IntraUnit> &units, std::vector<uint32_t> &ua_end, std::vector<uint32_t> &ub_end,
                                const Dav1dHipCompTask *blends, const uint32_t *blend_end) {
    const size_t np = n_steps ? pred_end[n_steps - 1] : 0, nt = n_steps ? tx_end[n_steps - 1] : 0;
    uint8_t dummy = 0;
    if (ipred_tasks_valid(preds, np, &dummy)) return -EINVAL;
    for (size_t i = 0; i < nt; i++) if (!itx_task_ok(txs[i])) return -EINVAL;
    // inter-intra blocks (kind PRED_TMP + a BLEND of the same rectangle in the same step) only where the caller brings the blends: the
    // unit then carries the blend — its mask offset in the place of the scratch offset nobody needs when the prediction stays in LDS
    for (size_t i = 0; i < np; i++) {
        const int k = preds[i].kind;
        if (k == DAV1D_HIP_IPRED_PRED_TMP && blends) continue;
        if (k != DAV1D_HIP_IPRED_PRED && k != DAV1D_HIP_IPRED_CFL && k != DAV1D_HIP_IPRED_PAL && k != DAV1D_HIP_IPRED_COPY) return -ENOTSUP;
    }
    if (blends) {
        const size_t nb = n_steps ? blend_end[n_steps - 1] : 0;
        for (size_t i = 0; i < nb; i++) if (blends[i].kind != DAV1D_HIP_COMP_BLEND || blends[i].plane > 2) return -ENOTSUP;
    }
    units.clear();
    units.reserve(np + nt / 4);
    ua_end.assign(n_steps, 0); ub_end.assign(n_steps, 0);
    auto unit = [&](const Dav1dHipIpredTask *p, const Dav1dHipItxTask *t) {
        IntraUnit u;
        memset(&u, 0, sizeof(u));
        if (p) { u.p = *p; u.has |= 1; }
        if (t) { u.t = *t; itx_fill_prefix(u.t); u.has |= 2; }
        units.push_back(u);
    };
    std::vector<uint32_t> slot;        // open-addressed map (plane, dst_off) -> transform task of the step
    std::vector<char> taken;
    for (size_t k = 0; k < n_steps; k++) {
        const size_t p0 = k ? pred_end[k - 1] : 0, t0 = k ? tx_end[k - 1] : 0;
        const size_t npk = pred_end[k] - p0, ntk = tx_end[k] - t0;
        if (npk || ntk) {
            size_t cap = 16;
            while (cap < 2 * ntk + 2) cap <<= 1;
            slot.assign(cap, 0xffffffffu);
            taken.assign(ntk, 0);
            auto hash = [&](uint32_t plane, uint32_t off) { return (size_t) ((off * 2654435761u) ^ (plane * 0x9e3779b9u)) & (cap - 1); };
            for (size_t i = 0; i < ntk; i++) {
                const Dav1dHipItxTask &t = txs[t0 + i];
                size_t h = hash(t.plane, t.dst_off);
                while (slot[h] != 0xffffffffu) h = (h + 1) & (cap - 1);
                slot[h] = (uint32_t) i;
            }
            for (size_t i = 0; i < npk; i++) {
                const Dav1dHipIpredTask &p = preds[p0 + i];
                uint32_t j = 0xffffffffu;
                for (size_t h = hash(p.plane, p.dst_off); slot[h] != 0xffffffffu; h = (h + 1) & (cap - 1)) {
                    const Dav1dHipItxTask &t = txs[t0 + slot[h]];
                    if (t.plane == p.plane && t.dst_off == p.dst_off && !taken[slot[h]] && k_tx_w[t.tx] == p.tw * 4 && k_tx_h[t.tx] == p.th * 4) {
                        j = slot[h];
                        break;
                    }
                }
                if (j != 0xffffffffu) taken[j] = 1;
                unit(&p, j == 0xffffffffu ? nullptr : &txs[t0 + j]);
                if (p.kind == DAV1D_HIP_IPRED_PRED_TMP) {
                    // its blend: the one of the step with the same rectangle
                    const size_t b0 = k ? blend_end[k - 1] : 0, b1 = blend_end[k];
                    const Dav1dHipCompTask *bl = nullptr;
                    for (size_t q = b0; q < b1 && !bl; q++)
                        if (blends[q].plane == p.plane && blends[q].dst_off == p.dst_off && blends[q].w == p.tw * 4 && blends[q].h == p.th * 4) bl = &blends[q];
                    if (!bl) return -EINVAL;
                    units.back().has |= 4;
                    units.back().p.aux_off = bl->mask_off;
                }
            }
            // units of a group are independent: put those that run the same code (transform size, then predictor) next to each
            // other, so that the waves of a CU — which are dealt consecutive units — share instruction cache lines.  The launch's
            // code is several hundred KB; with mixed sizes every wave misses on its own path.  Speed only.
            std::stable_sort(units.begin() + (k ? ub_end[k - 1] : 0), units.end(), [](const IntraUnit &a, const IntraUnit &b) {
                const int ka = ((a.has & 2) ? a.t.tx : 31) << 8 | a.p.mode, kb = ((b.has & 2) ? b.t.tx : 31) << 8 | b.p.mode;
                return ka < kb;
            });
            ua_end[k] = (uint32_t) units.size();
            for (size_t i = 0; i < ntk; i++) if (!taken[i]) unit(nullptr, &txs[t0 + i]);
        } else {
            ua_end[k] = (uint32_t) units.size();
        }
        ub_end[k] = (uint32_t) units.size();
    }
    return 0;
}

// units (host, need set, sorted) -> device-resident list; grp / prev_n are filled in here (the array is the caller's scratch)
int dav1d_hip_intra_flow_from_units(Dav1dHipContext *c, Dav1dHipIntraFlow **out, IntraUnit *units, size_t n) {
    if (!c || !out || (!units && n)) return -EINVAL;
    *out = nullptr;
    Dav1dHipIntraFlow *l = new (std::nothrow) Dav1dHipIntraFlow();
    if (!l) return -ENOMEM;
    memset(l, 0, sizeof(*l));
    l->n_units = n;
    for (size_t i = 0; i < n && !l->needs_aux; i++) if ((units[i].has & 1) && units[i].p.kind == DAV1D_HIP_IPRED_PAL) l->needs_aux = true;
    // groups: runs of equal `need`; the device copy gets the group index and the size of the group before
    size_t groups = 0, prev_n = 0, cur_start = 0;
    for (size_t i = 0; i < n; i++) {
        if (i && units[i].need != units[i - 1].need) { prev_n = i - cur_start; cur_start = i; groups++; }
        units[i].grp = (uint32_t) groups;
        units[i].prev_n = (uint32_t) prev_n;
    }
    l->n_groups = n ? groups + 1 : 0;
    l->ctr_bytes = (32 + l->n_groups * FLOW_SUB * FLOW_SUB_STRIDE) * sizeof(uint32_t);
    int rc = 0;
    if (hipMalloc((void **) &l->ctr, l->ctr_bytes) != hipSuccess) rc = -ENOMEM;
    if (!rc && n) {
        // one record past the end: the waves fetch a unit ahead
        if (hipMalloc((void **) &l->units, (n + 1) * sizeof(IntraUnit)) != hipSuccess) rc = -ENOMEM;
        if (!rc) rc = dav1d_hip_upload(c, l->units, units, n * sizeof(IntraUnit));
    }
    if (rc) { dav1d_hip_intra_flow_destroy(c, l); return rc; }
    *out = l;
    return 0;
}

int dav1d_hip_intra_flow_create(Dav1dHipContext *c, Dav1dHipIntraFlow **out, const Dav1dHipIpredTask *preds, const size_t *pred_sizes,
                                const Dav1dHipItxTask *txs, const size_t *tx_sizes, size_t n_batches) {
    if (!c || !out || !pred_sizes || !tx_sizes) return -EINVAL;
    *out = nullptr;
    std::vector<uint32_t> pe(n_batches), te(n_batches), ua, ub;
    size_t np = 0, nt = 0;
    for (size_t k = 0; k < n_batches; k++) {
        np += pred_sizes[k]; nt += tx_sizes[k];
        if (np >= 0xffffffffu || nt >= 0xffffffffu) return -ENOTSUP;
        pe[k] = (uint32_t) np; te[k] = (uint32_t) nt;
    }
    if ((np && !preds) || (nt && !txs)) return -EINVAL;
    std::vector<IntraUnit> units;
    const int rc = dav1d_hip_intra_units_build(preds, pe.data(), txs, te.data(), n_batches, units, ua, ub, nullptr, nullptr);
    if (rc) return rc;
    for (size_t k = 0, i = 0; k < n_batches; k++) {
        const uint32_t need_a = (uint32_t) i, need_b = ua[k];
        for (; i < ua[k]; i++) units[i].need = need_a;
        for (; i < ub[k]; i++) units[i].need = need_b;
    }
    return dav1d_hip_intra_flow_from_units(c, out, units.data(), units.size());
}

// enqueues: counters to zero, then the launch
int dav1d_hip_intra_flow_run(Dav1dHipContext *c, const Dav1dHipIntraFlow *l, const Dav1dHipPicture *dst, void *coef, uint8_t *aux) {
    if (!c || !l || !raster_dst_ok(dst) || (l->needs_aux && !aux)) return -EINVAL;
    if (!l->n_units) return 0;
    if (hipMemsetAsync(l->ctr, 0, l->ctr_bytes, c->stream) != hipSuccess) return -EIO;
    const DevPlanes dp = dev_planes(dst);
    // 8 one-wave workgroups per CU: more waves only poll
    return dav1d_hip_launch_intra_flow(&dp, dst->bpc, dst->layout, l->units, (int) l->n_units, aux, coef, l->ctr, c->flow_groups, c->flow_mode,
                                       c->stream);
}

// ------------------------------------------------------------------ intra wavefront superblock by superblock (intra_sb.hip)
struct Dav1dHipIntraSb {
    IntraUnit *units;
    SbRegion *regions;
    uint32_t *flags;            // n_regions + 1 words for the one-launch form
    std::vector<uint32_t> level_start;
    size_t n_units, n_regions;
    int sb_log2, sbw;
    bool needs_aux;
    bool has_copies;            // intra block copies among the units: the L2 hand-off kernel only, and (one launch) the `where` table
    uint32_t *where;            // superblock (raster) -> its region, for the copies' waits in the one-launch form
};

void dav1d_hip_intra_sb_destroy(Dav1dHipContext *c, Dav1dHipIntraSb *l) {
    if (!l) return;
    hipStreamSynchronize(c->stream);
    if (l->units) hipFree(l->units);
    if (l->regions) hipFree(l->regions);
    if (l->flags) hipFree(l->flags);
    if (l->where) hipFree(l->where);
    delete l;
}
size_t dav1d_hip_intra_sb_levels(const Dav1dHipIntraSb *l) { return l && !l->level_start.empty() ? l->level_start.size() - 1 : 0; }
size_t dav1d_hip_intra_sb_superblocks(const Dav1dHipIntraSb *l) { return l ? l->n_regions : 0; }

int dav1d_hip_intra_sb_create(Dav1dHipContext *c, Dav1dHipIntraSb **out, const Dav1dHipIpredTask *preds, const size_t *pred_sizes,
                              const Dav1dHipItxTask *txs, const size_t *tx_sizes, size_t n_batches, const Dav1dHipPicture *geometry,
                              int sb128, int n_tile_cols, const uint16_t *col_start_sb, int n_tile_rows, const uint16_t *row_start_sb) {
    if (!c || !out || !pred_sizes || !tx_sizes || !geometry) return -EINVAL;
    *out = nullptr;
    SbTiling tl;
    int rc = dav1d_hip_sb_tiling_make(&tl, geometry->p[0].w, geometry->p[0].h, sb128, n_tile_cols, col_start_sb, n_tile_rows, row_start_sb);
    if (rc) return rc;
    std::vector<uint32_t> pe(n_batches), te(n_batches), ua, ub;
    size_t np = 0, nt = 0;
    for (size_t k = 0; k < n_batches; k++) {
        np += pred_sizes[k]; nt += tx_sizes[k];
        if (np >= 0xffffffffu || nt >= 0xffffffffu) return -ENOTSUP;
        pe[k] = (uint32_t) np; te[k] = (uint32_t) nt;
    }
    if ((np && !preds) || (nt && !txs)) return -EINVAL;
    std::vector<IntraUnit> units;
    rc = dav1d_hip_intra_units_build(preds, pe.data(), txs, te.data(), n_batches, units, ua, ub, nullptr, nullptr);
    if (rc) return rc;
    const DevPlanes dp = dev_planes(geometry);
    SbSort st;
    rc = dav1d_hip_sbw_prepare(units, ua, ub, tl, dp.stride, geometry->layout != DAV1D_HIP_LAYOUT_I444, geometry->layout == DAV1D_HIP_LAYOUT_I420, st);
    if (rc) return rc;
    std::vector<IntraUnit> sorted(st.n_records);
    dav1d_hip_sbw_emit(units, st, sorted.data());
    bool has_pal = false;
    for (const IntraUnit &u : units) if ((u.has & 1) && u.p.kind == DAV1D_HIP_IPRED_PAL) { has_pal = true; break; }
    units.swap(sorted);
    const std::vector<SbPart> &parts = st.parts;
    SbPlan plan;
    std::sort(st.copy_deps.begin(), st.copy_deps.end());
    st.copy_deps.erase(std::unique(st.copy_deps.begin(), st.copy_deps.end()), st.copy_deps.end());
    rc = dav1d_hip_sbw_plan(tl, { &parts }, { 0 }, nullptr, plan, st.copy_deps.empty() ? nullptr : &st.copy_deps);
    if (rc) return rc;
    Dav1dHipIntraSb *l = new (std::nothrow) Dav1dHipIntraSb();
    if (!l) return -ENOMEM;
    l->units = nullptr; l->regions = nullptr; l->flags = nullptr; l->where = nullptr;
    l->has_copies = !st.copy_deps.empty(); l->sbw = tl.sbw;
    l->n_units = units.size(); l->n_regions = plan.regions.size();
    l->level_start = plan.level_start;
    l->sb_log2 = tl.sb_log2;
    l->needs_aux = has_pal;
    if (l->n_units) {
        if (hipMalloc((void **) &l->units, (l->n_units + 1) * sizeof(IntraUnit)) != hipSuccess) rc = -ENOMEM;
        if (!rc && hipMalloc((void **) &l->regions, l->n_regions * sizeof(SbRegion)) != hipSuccess) rc = -ENOMEM;
        if (!rc && hipMalloc((void **) &l->flags, (l->n_regions + 1) * sizeof(uint32_t)) != hipSuccess) rc = -ENOMEM;
        if (!rc) rc = dav1d_hip_upload(c, l->units, units.data(), l->n_units * sizeof(IntraUnit));
        if (!rc) rc = dav1d_hip_upload(c, l->regions, plan.regions.data(), l->n_regions * sizeof(SbRegion));
        if (!rc && l->has_copies) {
            if (hipMalloc((void **) &l->where, plan.where.size() * sizeof(uint32_t)) != hipSuccess) rc = -ENOMEM;
            if (!rc) rc = dav1d_hip_upload(c, l->where, plan.where.data(), plan.where.size() * sizeof(uint32_t));
        }
    }
    if (rc) { dav1d_hip_intra_sb_destroy(c, l); return rc; }
    *out = l;
    return 0;
}

// enqueues the launches on the context's stream: one per level, or (option intra_sb_flow, L2 hand-off form, more than one level) ONE
// for all of them with the superblocks waiting for their neighbours' flags
int dav1d_hip_intra_sb_run(Dav1dHipContext *c, const Dav1dHipIntraSb *l, const Dav1dHipPicture *dst, void *coef, uint8_t *aux) {
    if (!c || !l || !raster_dst_ok(dst) || (l->needs_aux && !aux)) return -EINVAL;
    const DevPlanes dp = dev_planes(dst);
    int rc = 0;
    const int lds = c->intra_sb_lds && !l->has_copies;          // (the LDS-resident form does not copy)
    if (c->intra_sb_flow && !lds && l->level_start.size() > 2) {
        if (hipMemsetAsync(l->flags, 0, (l->n_regions + 1) * sizeof(uint32_t), c->stream) != hipSuccess) return -EIO;
        // (four waves per workgroup where the levels are wide and nothing is copied, unless asked otherwise: see frame.hip)
        const bool wide_levels = l->n_regions >= 128 * (l->level_start.size() - 1);
        return dav1d_hip_launch_intra_sb(&dp, dst->bpc, dst->layout, l->units, l->regions, (int) l->n_regions, aux, nullptr, coef,
                                         c->intra_sb_waves ? c->intra_sb_waves : !l->has_copies && wide_levels ? 4 : 8, l->sb_log2, 0, l->flags, c->stream, l->where, l->sbw);
    }
    for (size_t k = 0; k + 1 < l->level_start.size() && !rc; k++)
        rc = dav1d_hip_launch_intra_sb(&dp, dst->bpc, dst->layout, l->units, l->regions + l->level_start[k],
                                       (int) (l->level_start[k + 1] - l->level_start[k]), aux, nullptr, coef, c->intra_sb_waves, l->sb_log2, lds, nullptr, c->stream);
    return rc;
}

// after dav1d_hip_intra_sb_run: waits for the stream; workgroups of the one-launch form that gave up waiting for a neighbour (none in
// a sound run, see include/dav1d_hip.h) left their superblocks unreconstructed -> -EIO
int dav1d_hip_intra_sb_status(Dav1dHipContext *c, const Dav1dHipIntraSb *l, uint32_t *gave_up) {
    if (!c || !l) return -EINVAL;
    uint32_t n = 0;
    if (gave_up) *gave_up = 0;
    if (!l->flags || !l->n_units) return dav1d_hip_sync(c);
    const int rc = dav1d_hip_download(c, &n, l->flags + l->n_regions, sizeof(n));
    if (rc) return rc;
    if (!(c->intra_sb_flow && !(c->intra_sb_lds && !l->has_copies) && l->level_start.size() > 2)) n = 0;      // the flags are only written by the one-launch form
    if (gave_up) *gave_up = n;
    return n ? -EIO : 0;
}

int dav1d_hip_intra_list_run_batch(Dav1dHipContext *c, const Dav1dHipIntraList *l, size_t batch, const Dav1dHipPicture *dst, void *coef,
                                   uint8_t *aux) {
    return dav1d_hip_intra_list_run_batch_blend(c, l, batch, dst, coef, aux, nullptr, nullptr);
}

// every batch of the list, in order, back to back on the context's stream (what a frame does; one call instead of one per step)
int dav1d_hip_intra_list_run_all(Dav1dHipContext *c, const Dav1dHipIntraList *l, const Dav1dHipPicture *dst, void *coef, uint8_t *aux) {
    if (!c || !l) return -EINVAL;
    int rc = 0;
    for (size_t k = 0; k + 1 < l->pair_start.size() && !rc; k++) rc = dav1d_hip_intra_list_run_batch_blend(c, l, k, dst, coef, aux, nullptr, nullptr);
    return rc;
}

// prep / mask: the scratch arena the PRED_TMP predictions of the batch go to and the blends read, and the mask arena
int dav1d_hip_intra_list_run_batch_blend(Dav1dHipContext *c, const Dav1dHipIntraList *l, size_t batch, const Dav1dHipPicture *dst, void *coef,
                                         uint8_t *aux, int16_t *prep, uint8_t *mask) {
    if (!c || !l || !raster_dst_ok(dst) || batch + 1 >= l->pair_start.size() || (l->needs_aux && !aux)) return -EINVAL;
    const size_t n_blend = l->blend_start[batch + 1] - l->blend_start[batch];
    if (n_blend && (!prep || !mask)) return -EINVAL;
    const DevPlanes dp = dev_planes(dst);
    int rc = 0;
    const size_t n_pairs = l->pair_start[batch + 1] - l->pair_start[batch];
    const Dav1dHipIpredList *pl = l->preds;
    const size_t n_rest = pl ? pl->start[batch + 1] - pl->start[batch] : 0;
    if (n_pairs && n_rest) {
        // the pairs and the other predictions of the step are independent: one launch, side by side (intra_pair.hip)
        if ((pl->needs_aux && !aux) || (pl->needs_tmp && !prep)) return -EINVAL;
        rc = dav1d_hip_launch_intra_step(&dp, dst->bpc, dst->layout, pl->dev + pl->start[batch], (int) n_rest, (int) pl->n_big[batch],
                                         l->p_dev + l->pair_start[batch], l->t_dev + l->pair_start[batch], (int) n_pairs, aux, prep, coef, c->stream);
    } else {
        if (n_pairs)
            rc = dav1d_hip_launch_intra_pairs(&dp, dst->bpc, dst->layout, l->p_dev + l->pair_start[batch], l->t_dev + l->pair_start[batch],
                                              (int) n_pairs, aux, coef, c->stream);
        if (!rc) rc = ipred_list_run_batch_tmp(c, l->preds, batch, dst, aux, prep);
    }
    if (!rc && n_blend) rc = dav1d_hip_launch_comp(&dp, dst->bpc, l->b_dev + l->blend_start[batch], (int) n_blend, prep, mask, c->stream);
    if (!rc && l->itx[batch]->n) rc = dav1d_hip_itx_list_run(c, l->itx[batch], dst, coef);
    return rc;
}

} // extern "C"
