/* The backend inside dav1d's own task loop.  TEST INFRASTRUCTURE ONLY: linked into oracle/_ref_hooked/libdav1d_hooked.so, the
 * reference build with src/thread_task.c patched at the hook points of INTEGRATION.md 2 (patches/dav1d-1.5.4-hip.patch).
 *
 * What runs here is dav1d: dav1d_open() creates the context, its frame contexts (n_fc >= 3) and its worker threads
 * (dav1d_worker_task); every frame goes through the reference's dav1d_submit_frame(), dav1d_decode_frame_init(), the task
 * queues of src/thread_task.c with their inter-frame dependencies (check_tile), dav1d_decode_frame_exit() and the output queue
 * drained by dav1d_get_picture().  There are no AV1 streams in either box, so the ONE thing that is replaced in both modes is the
 * entropy decoder: the frame headers are built here instead of parsed, and pass 1's output (Av1Block / cbi / cf, the deblocking
 * masks built by the reference's own dav1d_create_lf_mask_*, cdef indices, restoration units) is injected when a frame's
 * arrays exist (Dav1dHooks.after_init), the pass-1 tile tasks return at once.
 *   mode 0: pass 2 and the in-loop filters are the reference's own code on its worker threads — the peer.
 *   mode 1: the PRODUCT's binding (dav1d_amd/host/dav1d_glue.c, linked in: Dav1dPicAllocator on dav1d_hip_host_picture_*, the frame /
 *           filter descriptors, dav1d_hip_lister_tile_sbrow from the pass-2 tile task, dav1d_hip_lister_filter_sbrow from the filter
 *           tasks, dav1d_hip_frame_end on its own threads, dav1d_hip_frame_done) behind the harness's own after_init / entropy hooks.
 * Frames form a chain: a key frame, then inter frames that each predict from the three frames before them. */
#include "config.h"
#include <dlfcn.h>
#include <errno.h>
#include <limits.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "dav1d/dav1d.h"
#include "common/frame.h"
#include "src/internal.h"
#include "src/tables.h"
#include "src/decode.h"
#include "src/lf_mask.h"
#include "src/ref.h"
#include "src/picture.h"
#include "src/warpmv.h"
#include "src/thread_task.h"
#include "dav1d_hooks.h"
#include "dav1d_glue.h"
#include "dav1d_hip.h"
#include "dav1d_synth.h"

typedef struct HookedParams {
    int w, h, layout, bpc, sb128;
    int n_tile_cols, n_tile_rows;
    uint16_t col_start_sb[65], row_start_sb[65];
    int n_threads, frame_delay, n_frames;
    int lf_level_y[2], lf_level_u, lf_level_v, lf_sharpness;
    int cdef_enabled, cdef_damping, cdef_n_bits;
    int cdef_y_strength[8], cdef_uv_strength[8];
    int lr_type[3], lr_unit_size[2];
    int mode;                  /* 0 the reference's pass 2 + filters, 1 the HIP backend */
    int free_listing;          /* mode 1: 1 = a frame is listed without waiting for its references (their pixels are only needed when
                                  the frame ends, and the frames end in order); 0 = dav1d's own rule with every reference fully needed */
    int device;
    int keep_output;           /* copy every output picture (for comparisons) */
    int inject;                /* 0: pass 1's output is generated when a frame's arrays exist (inside the run); 1: ... and a copy is kept in the
                                  store; 2: taken from the store of an earlier run (the generator and the mask-building walk — one thread
                                  per frame here, where dav1d spreads entropy decoding over all of them — stay out of the timed chain) */
    int pack;                  /* mode 1: the lister packs (Dav1dHipFrameDesc.cf = f->frame_thread.cf): the coefficients that exist travel with
                                  the frame's lists, cf is left zero as the reference's inverse transforms leave it, no dense arena goes to
                                  the device.  With inject = 2 the arrays of the STORE are what gets consumed: replay such a store last. */
    Dav1dSynthParams synth; /* block decisions of the generated frames; seed + frame number per frame */
    int stream;                /* 1: NOTHING is injected.  The harness is handed an AV1 bitstream (tests/av1_obu.py: real headers, tile payloads of
                                  seeded random bytes) and drives dav1d's public API with it — dav1d_send_data / dav1d_get_picture, dav1d_parse_obus,
                                  dav1d_submit_frame, and the reference's own pass 1 (dav1d_msac_*, decode_b, decode_coefs, read_restoration_info,
                                  dav1d_create_lf_mask_*) on its worker threads.  mode 0 is then dav1d itself, no hook installed but an error
                                  recorder around the pass-1 tile call; mode 1 the glue of INTEGRATION.md behind dav1d's real pass 1 */
    int row_progress;          /* mode 1: rows are published as the frame's last stage completes them (dav1d_hip_frame_set_progress_callback ->
                                  dav1d_hooked_rows_done: the store of src/thread_task.c:888-896), not only when the frame has ended.  With
                                  free_listing = 0 the tile tasks of the next frames then really wait in check_tile() for the rows of their
                                  references (decode_b's lowest_pixel bookkeeping) and start while this frame's filters still run */
    int apply_grain;           /* stream mode: film grain on the output pictures — mode 0: Dav1dSettings.apply_grain (dav1d_apply_grain on the
                                  host); mode 1: apply_grain = 0 and the "application" applies it on the device (dav1d_hip_fg_apply on the picture
                                  dav1d returns, frame_hdr->film_grain.data), as GPU video outputs do.
                                  chain mode: every frame header carries a grain set with luma scaling points and none for chroma (the chroma
                                  planes of the output are copies), and the pictures kept are the ones with grain — mode 0: dav1d_apply_grain
                                  (src/lib.c:485-524) on the picture dav1d hands out, mode 1: dav1d_hip_glue_output_with_grain */
    int filters_off;           /* in-loop filters the "application" switches off, both modes: Dav1dSettings.inloop_filters = ALL & ~filters_off
                                  (bit 0 deblock, 1 CDEF, 2 restoration; include/dav1d/dav1d.h:61-69) */
    int n_devices;             /* mode 1: Dav1dHipGlueOptions.n_devices — frames end on devices device .. device + n_devices - 1 in turn */
} HookedParams;

/* pass 1's output of one frame, as dav1d_decode_frame_init() sizes the arrays */
typedef struct StoredFrame {
    void *b, *cbi, *cf, *pal, *pal_idx;
    size_t b_bytes, cbi_bytes, cf_bytes, pal_bytes, pal_idx_bytes;
    void *lf_mask, *lf_level, *lr_mask, *re0, *re1, *a;
    size_t lf_mask_bytes, lf_level_bytes, lr_mask_bytes, re_bytes, a_bytes;
} StoredFrame;
typedef struct Store { int n; StoredFrame *fr; } Store;

/* the entry points of include/dav1d_hip.h, resolved from the library the caller names (libdav1d_hip.so, or the SIMT-emulated
 * build of the same sources on a machine without a GPU) */
typedef struct Hip {
    void *synth_dl;
    /* chain mode: the generator of synthetic pass-1 output (tests/synth/libdav1d_synth.so, test infrastructure like this file) */
    int (*synth_frame)(const Dav1dHipFrameDesc *, const Dav1dSynthParams *, void *, size_t, size_t, uint8_t *, size_t);
} Hip;

/* The binding itself — Dav1dPicAllocator on dav1d_hip_host_picture_*, the descriptors, the tile / filter / frame-complete hooks, the three
 * stage threads, progress and error handling — is PRODUCT code: dav1d_amd/host/dav1d_glue.c, linked in here.  This file keeps what a
 * test needs around it: injection of pass-1 output, the stream runner, output comparison, statistics. */

/* per frame context: what the harness keeps (the glue has its own state) */
typedef struct FcState {
    /* inject == 2, mode 1: the frame context's own arrays while the stored ones stand in for them */
    void *own_b, *own_cbi, *own_cf;
    int swapped;
} FcState;

typedef struct OutPic { int w, h, layout, bpc, frame_offset, grain; uint8_t *plane[3]; uint64_t hash[3]; double t; } OutPic;

/* which tools pass 1's output of a stream really holds (blocks counted by the reference's own decode_sb walk, count_walk below) */
enum { HIST_FRAMES_KEY, HIST_FRAMES_INTER, HIST_FRAMES_INTRA_ONLY, HIST_FRAMES_SUPER_RES, HIST_FRAMES_SCALED_REFS, HIST_FRAMES_INTRABC,
       HIST_FRAMES_FILM_GRAIN, HIST_FRAMES_DELTA_LF, HIST_FRAMES_SEGMENTED, HIST_FRAMES_LOSSLESS,
       HIST_B_INTRA, HIST_B_INTER, HIST_B_INTRABC, HIST_B_SKIP, HIST_B_SKIP_MODE, HIST_B_SEG_NONZERO,
       HIST_B_PALETTE_Y, HIST_B_PALETTE_UV, HIST_B_CFL, HIST_B_FILTER_INTRA, HIST_B_DIRECTIONAL, HIST_B_ANGLE_DELTA, HIST_B_SMOOTH, HIST_B_PAETH,
       HIST_B_COMP_AVG, HIST_B_COMP_WAVG, HIST_B_COMP_SEG, HIST_B_COMP_WEDGE, HIST_B_INTERINTRA, HIST_B_INTERINTRA_WEDGE, HIST_B_OBMC,
       HIST_B_LOCAL_WARP, HIST_B_GLOBALMV, HIST_B_GLOBAL_WARP, HIST_B_SCALED_REF, HIST_B_FILTER_NOT_REGULAR, HIST_B_DUAL_FILTER,
       HIST_B_TX_SPLIT, HIST_B_TX64, HIST_B_LOSSLESS, HIST_B_SUB8X8_CHROMA, HIST_B_128, HIST_B_4XN,
       HIST_TX_BLOCKS, HIST_TX_NON_DCT, HIST_TX_EOB0, HIST_TX_NO_COEFS,
       HIST_LR_WIENER, HIST_LR_SGR, HIST_CDEF_NONZERO_IDX, HIST_N };

typedef struct Hooked {
    HookedParams p;
    Hip hip;
    Dav1dHipGlue *glue;                   /* mode 1: the binding (dav1d_amd/host/dav1d_glue.c) */
    Dav1dContext *c;
    unsigned n_fc;
    Dav1dRef *seq_ref;
    FcState *fcs;
    Store *store;
    double *q_done_t;                     /* chain mode, [frame number]: when dav1d_hip_frame_done returned */
    double *out_t;                        /* chain mode, [frame number]: when the picture came out of dav1d */
    uint64_t *out_hash;                   /* chain mode, keep_output == 2: [frame * 3 + plane] digests of the pictures */
    /* stream mode */
    struct OutPic *out_pics;              /* what dav1d_get_picture handed out, in that order */
    int n_out_pics, cap_out_pics;
    const uint8_t *const *tu;             /* the temporal units of the run (tile data points into them) */
    const size_t *tu_size;
    int n_tu;
    int n_errors;                         /* pictures dav1d reported an error for */
    struct TileError { int tu; size_t off; int overread; } tile_err[64];
    int n_tile_err;
    uint64_t hist[HIST_N];
    /* outputs */
    uint8_t **out_plane;                  /* [frame * 3 + plane]: tight rows */
    int n_out;
    double seconds;
    int failed;
    /* where the time goes (seconds, summed over frames): [0] picture allocation, [1] after_init, [2] listing (tile tasks), [3] filter
     * listing, [4] waiting for a frame's turn, [5] uploads, [6] dav1d_hip_frame_end, [7] fetch to the host planes, [8] picture release */
    double stat[16];
    double frame_end_s[64];               /* dav1d_hip_frame_end of frame k */
    pthread_mutex_t stat_mtx;
} Hooked;

static Hooked *g_h;                       /* one harness at a time: the hooks carry no user pointer */

/* DAV1D_HOOKED_BACKTRACE=1: a crash inside the harness, dav1d or the backend prints where (there is no debugger on the boxes) */
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
static void crash_handler(const int sig) {
    void *bt[64];
    const int n = backtrace(bt, 64);
    backtrace_symbols_fd(bt, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
static void crash_handler_install(void) {
    const char *const e = getenv("DAV1D_HOOKED_BACKTRACE");
    if (e && *e == '1') { signal(SIGSEGV, crash_handler); signal(SIGABRT, crash_handler); signal(SIGBUS, crash_handler); }
}

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + ts.tv_nsec * 1e-9; }
static void stat_add(Hooked *const h, const int i, const double t0) {
    const double dt = now_s() - t0;
    pthread_mutex_lock(&h->stat_mtx); h->stat[i] += dt; pthread_mutex_unlock(&h->stat_mtx);
}

/* ------------------------------------------------------------------------------------------------ pass-1 stand-in: filter inputs
 * The reference's own block walk (decode_sb with pass == 2) visits every block with the two reconstruction hooks pointed at the
 * functions below, which make the calls of dav1d_create_lf_mask_intra / _inter that pass 1 makes (src/decode.c:1216-1226,
 * 1882-1900) and the cdef_idx / noskip_mask updates (:938-956, 1945-1956) — as oracle/ref_frame.c does for single frames. */
typedef struct WalkState { BlockContext lf_l; int cur_tile_row; uint32_t rng; } WalkState;
static __thread WalkState *g_walk;

static uint32_t walk_rnd(WalkState *const r) { r->rng = r->rng * 1664525u + 1013904223u; return r->rng >> 8; }

static void walk_common(Dav1dTaskContext *const t, const enum BlockSize bs, const Av1Block *const b) {
    WalkState *const r = g_walk;
    const Dav1dFrameContext *const f = t->f;
    Av1Filter *const lf_mask = f->lf.mask + (t->by >> 5) * f->sb128w + (t->bx >> 5);
    const uint8_t *const b_dim = dav1d_block_dimensions[bs];
    const int bx4 = t->bx & 31, by4 = t->by & 31, bw4 = b_dim[0], bh4 = b_dim[1];
    if (!b->skip) {
        const int idx = ((t->bx & 16) >> 4) + ((t->by & 16) >> 3);
        if (lf_mask->cdef_idx[idx] == -1) {
            const int v = walk_rnd(r) & ((1 << f->frame_hdr->cdef.n_bits) - 1);
            lf_mask->cdef_idx[idx] = v;
            if (bw4 > 16) lf_mask->cdef_idx[idx + 1] = v;
            if (bh4 > 16) lf_mask->cdef_idx[idx + 2] = v;
            if (bw4 == 32 && bh4 == 32) lf_mask->cdef_idx[idx + 3] = v;
        }
        uint16_t (*noskip_mask)[2] = &lf_mask->noskip_mask[by4 >> 1];
        const unsigned mask = (~0U >> (32 - bw4)) << (bx4 & 15);
        const int bx_idx = (bx4 & 16) >> 4;
        for (int y = 0; y < bh4; y += 2, noskip_mask++) {
            (*noskip_mask)[bx_idx] |= mask;
            if (bw4 == 32) (*noskip_mask)[1] |= mask;
        }
    }
}

static void walk_intra(Dav1dTaskContext *const t, const enum BlockSize bs, const enum EdgeFlags flags, const Av1Block *const b) {
    (void) flags;
    WalkState *const r = g_walk;
    const Dav1dFrameContext *const f = t->f;
    const int ss_ver = f->cur.p.layout == DAV1D_PIXEL_LAYOUT_I420, ss_hor = f->cur.p.layout != DAV1D_PIXEL_LAYOUT_I444;
    const uint8_t *const b_dim = dav1d_block_dimensions[bs];
    const int bx4 = t->bx & 31, by4 = t->by & 31, cbx4 = bx4 >> ss_hor, cby4 = by4 >> ss_ver;
    const int has_chroma = f->cur.p.layout != DAV1D_PIXEL_LAYOUT_I400 && (b_dim[0] > ss_hor || t->bx & 1) && (b_dim[1] > ss_ver || t->by & 1);
    BlockContext *const a = &f->a[r->cur_tile_row * f->sb128w + (t->bx >> 5)];
    if (f->frame_hdr->loopfilter.level_y[0] || f->frame_hdr->loopfilter.level_y[1])
        dav1d_create_lf_mask_intra(f->lf.mask + (t->by >> 5) * f->sb128w + (t->bx >> 5), f->lf.level, f->b4_stride,
                                   (const uint8_t (*)[8][2]) &t->ts->lflvl[b->seg_id][0][0][0], t->bx, t->by, f->w4, f->h4, bs,
                                   b->tx, b->uvtx, f->cur.p.layout, &a->tx_lpf_y[bx4], &r->lf_l.tx_lpf_y[by4],
                                   has_chroma ? &a->tx_lpf_uv[cbx4] : NULL, has_chroma ? &r->lf_l.tx_lpf_uv[cby4] : NULL);
    walk_common(t, bs, b);
}

static int walk_inter(Dav1dTaskContext *const t, const enum BlockSize bs, const Av1Block *const b) {
    WalkState *const r = g_walk;
    const Dav1dFrameContext *const f = t->f;
    const int ss_ver = f->cur.p.layout == DAV1D_PIXEL_LAYOUT_I420, ss_hor = f->cur.p.layout != DAV1D_PIXEL_LAYOUT_I444;
    const uint8_t *const b_dim = dav1d_block_dimensions[bs];
    const int bx4 = t->bx & 31, by4 = t->by & 31, cbx4 = bx4 >> ss_hor, cby4 = by4 >> ss_ver;
    const int has_chroma = f->cur.p.layout != DAV1D_PIXEL_LAYOUT_I400 && (b_dim[0] > ss_hor || t->bx & 1) && (b_dim[1] > ss_ver || t->by & 1);
    BlockContext *const a = &f->a[r->cur_tile_row * f->sb128w + (t->bx >> 5)];
    if (f->frame_hdr->loopfilter.level_y[0] || f->frame_hdr->loopfilter.level_y[1]) {
        const int is_comp = b->comp_type != COMP_INTER_NONE;
        const int is_globalmv = b->inter_mode == (is_comp ? GLOBALMV_GLOBALMV : GLOBALMV);
        const uint8_t (*const lf_lvls)[8][2] = (const uint8_t (*)[8][2]) &t->ts->lflvl[b->seg_id][0][b->ref[0] + 1][!is_globalmv];
        const uint16_t tx_split[2] = { b->tx_split0, b->tx_split1 };
        enum RectTxfmSize ytx = b->max_ytx, uvtx = b->uvtx;
        if (f->frame_hdr->segmentation.lossless[b->seg_id]) { ytx = (enum RectTxfmSize) TX_4X4; uvtx = (enum RectTxfmSize) TX_4X4; }
        dav1d_create_lf_mask_inter(f->lf.mask + (t->by >> 5) * f->sb128w + (t->bx >> 5), f->lf.level, f->b4_stride, lf_lvls,
                                   t->bx, t->by, f->w4, f->h4, b->skip, bs, ytx, tx_split, uvtx, f->cur.p.layout,
                                   &a->tx_lpf_y[bx4], &r->lf_l.tx_lpf_y[by4],
                                   has_chroma ? &a->tx_lpf_uv[cbx4] : NULL, has_chroma ? &r->lf_l.tx_lpf_uv[cby4] : NULL);
    }
    walk_common(t, bs, b);
    return 0;
}

static int build_filter_inputs(Dav1dFrameContext *const f, const unsigned seed) {
    const Dav1dFrameHeader *const fh = f->frame_hdr;
    const int num_sb128 = f->sb128w * f->sb128h;
    WalkState ws;
    memset(&ws, 0, sizeof(ws));
    ws.rng = seed * 2654435761u + 12345u;
    Dav1dTaskContext *t = NULL;
    if (posix_memalign((void **) &t, 64, sizeof(*t))) return -1;
    memset(t, 0, sizeof(*t));
    memset(f->lf.mask, 0, sizeof(*f->lf.mask) * num_sb128);
    for (int i = 0; i < num_sb128; i++) memset(f->lf.mask[i].cdef_idx, -1, 4);
    memset(f->lf.level, 0, sizeof(*f->lf.level) * num_sb128 * 32 * 32);
    /* reset_context() of the pass-1 half of f->a: tx_lpf_y = 2, tx_lpf_uv = 1 (src/decode.c:2401-2402) */
    for (int n = 0; n < f->sb128w * fh->tiling.rows; n++) {
        memset(f->a[n].tx_lpf_y, 2, sizeof(f->a[n].tx_lpf_y));
        memset(f->a[n].tx_lpf_uv, 1, sizeof(f->a[n].tx_lpf_uv));
    }
    const recon_b_intra_fn keep_intra = f->bd_fn.recon_b_intra;
    const recon_b_inter_fn keep_inter = f->bd_fn.recon_b_inter;
    f->bd_fn.recon_b_intra = walk_intra;
    f->bd_fn.recon_b_inter = walk_inter;
    g_walk = &ws;
    t->c = f->c; t->f = f;
    t->frame_thread.pass = 2;
    int rc = 0;
    const int ss_ver = f->cur.p.layout == DAV1D_PIXEL_LAYOUT_I420;
    for (int tile_row = 0; tile_row < fh->tiling.rows && !rc; tile_row++)
        for (int sby = fh->tiling.row_start_sb[tile_row]; sby < fh->tiling.row_start_sb[tile_row + 1] && !rc; sby++) {
            t->by = sby << f->sb_shift;
            for (int tile_col = 0; tile_col < fh->tiling.cols && !rc; tile_col++) {
                t->ts = &f->ts[tile_row * fh->tiling.cols + tile_col];
                ws.cur_tile_row = tile_row;
                memset(ws.lf_l.tx_lpf_y, 2, sizeof(ws.lf_l.tx_lpf_y));
                memset(ws.lf_l.tx_lpf_uv, 1, sizeof(ws.lf_l.tx_lpf_uv));
                rc = dav1d_decode_tile_sbrow(t);
                /* src/decode.c:2730-2740: the left context at the tile's right edge, for the mask fix-ups across tile columns */
                int align_h = (f->bh + 31) & ~31;
                memcpy(&f->lf.tx_lpf_right_edge[0][align_h * tile_col + t->by], &ws.lf_l.tx_lpf_y[t->by & 16], f->sb_step);
                align_h >>= ss_ver;
                memcpy(&f->lf.tx_lpf_right_edge[1][align_h * tile_col + (t->by >> ss_ver)], &ws.lf_l.tx_lpf_uv[(t->by & 16) >> ss_ver],
                       f->sb_step >> ss_ver);
            }
        }
    f->bd_fn.recon_b_intra = keep_intra;
    f->bd_fn.recon_b_inter = keep_inter;
    g_walk = NULL;
    /* the walk moved the pass-2 tile cursors and contexts: back to the start of the frame (setup_tile, src/decode.c:2438-2452;
     * reset_context of the pass-2 half, :3182-3188) */
    {
        static const uint8_t ss_size_mul[4][2] = { { 4, 4 }, { 6, 5 }, { 8, 6 }, { 12, 8 } };
        const uint8_t *const size_mul = ss_size_mul[f->cur.p.layout];
        const int hbd = f->cur.p.bpc > 8;
        for (int j = 0; j < fh->tiling.cols * fh->tiling.rows; j++) {
            const unsigned off = f->frame_thread.tile_start_off[j];
            Dav1dTileState *const ts = &f->ts[j];
            for (int q = 0; q < 2; q++) {
                ts->frame_thread[q].pal_idx = f->frame_thread.pal_idx ? &f->frame_thread.pal_idx[(size_t) off * size_mul[1] / 8] : NULL;
                ts->frame_thread[q].cbi = &f->frame_thread.cbi[(size_t) off * size_mul[0] / 64];
                ts->frame_thread[q].cf = (uint8_t *) f->frame_thread.cf + (((size_t) off * size_mul[0]) >> !hbd);
            }
        }
        const int keyframe = IS_KEY_OR_INTRA(fh);
        for (int n = f->sb128w * fh->tiling.rows; n < f->sb128w * fh->tiling.rows * 2; n++) {
            memset(&f->a[n], 0, sizeof(f->a[n]));
            memset(f->a[n].intra, keyframe, sizeof(f->a[n].intra));
            memset(f->a[n].uvmode, DC_PRED, sizeof(f->a[n].uvmode));
            if (keyframe) memset(f->a[n].mode, DC_PRED, sizeof(f->a[n].mode));
        }
    }
    /* restoration units: what read_restoration_info() parses (src/decode.c:2511-2592), drawn in its ranges */
    if (f->lf.lr_mask && f->lf.restore_planes) {
        static const uint8_t sgr_s[16][2] = { { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 }, { 1, 1 },
                                              { 0, 1 }, { 0, 1 }, { 0, 1 }, { 0, 1 }, { 1, 0 }, { 1, 0 } };
        for (int i = 0; i < f->lf.lr_mask_sz; i++)
            for (int pl = 0; pl < 3; pl++) {
                const int ft = fh->restoration.type[pl];
                for (int u = 0; u < 4; u++) {
                    Av1RestorationUnit *const lr = &f->lf.lr_mask[i].lr[pl][u];
                    memset(lr, 0, sizeof(*lr));
                    int kind = 0;                                        /* 0 none, 1 Wiener, 2 self-guided */
                    if (ft == DAV1D_RESTORATION_SWITCHABLE) kind = walk_rnd(&ws) % 3;
                    else if (ft == DAV1D_RESTORATION_WIENER) kind = walk_rnd(&ws) % 5 ? 1 : 0;
                    else if (ft == DAV1D_RESTORATION_SGRPROJ) kind = walk_rnd(&ws) % 5 ? 2 : 0;
                    const int idx = walk_rnd(&ws) & 15;
                    lr->type = kind == 0 ? DAV1D_RESTORATION_NONE : kind == 1 ? DAV1D_RESTORATION_WIENER : DAV1D_RESTORATION_SGRPROJ + idx;
                    lr->filter_h[0] = lr->filter_v[0] = 0;
                    if (!pl) { lr->filter_h[0] = (int) (walk_rnd(&ws) % 16) - 5; lr->filter_v[0] = (int) (walk_rnd(&ws) % 16) - 5; }
                    lr->filter_h[1] = (int) (walk_rnd(&ws) % 32) - 23; lr->filter_v[1] = (int) (walk_rnd(&ws) % 32) - 23;
                    lr->filter_h[2] = (int) (walk_rnd(&ws) % 64) - 17; lr->filter_v[2] = (int) (walk_rnd(&ws) % 64) - 17;
                    lr->sgr_weights[0] = sgr_s[idx][0] ? (int) (walk_rnd(&ws) % 128) - 96 : 0;
                    lr->sgr_weights[1] = sgr_s[idx][1] ? (int) (walk_rnd(&ws) % 128) - 32 : 95;
                }
            }
    }
    free(t);
    return rc;
}

/* ------------------------------------------------------------------------------------------------ the hooks */
static FcState *state_of(const Dav1dFrameContext *const f) { return &g_h->fcs[f - f->c->fc]; }

static int hk_after_init_(Dav1dFrameContext *const f);
static int hk_after_init(Dav1dFrameContext *const f) {
    const double t0 = now_s();
    const int rc = hk_after_init_(f);
    stat_add(g_h, 1, t0);
    return rc;
}
static int hk_after_init_(Dav1dFrameContext *const f) {
    Hooked *const h = g_h;
    FcState *const s = state_of(f);
    const Dav1dFrameHeader *const fh = f->frame_hdr;
    const int n_tiles = fh->tiling.cols * fh->tiling.rows;
    const size_t cf_bytes = (size_t) f->frame_thread.cf_sz * 128 * 128 / 2;
    const size_t cbi_entries = (size_t) f->frame_thread.cbi_sz * 32 * 32 / 4;
    const size_t pal_idx_bytes = (size_t) f->frame_thread.pal_idx_sz * 128 * 128 / 8;
    const size_t b_bytes = sizeof(*f->frame_thread.b) * (size_t) f->sb128w * f->sb128h * 32 * 32;
    const size_t pal_bytes = (size_t) f->frame_thread.pal_sz * 16 * 16 * 24;
    const int num_sb128 = f->sb128w * f->sb128h;
    const size_t re_bytes = (size_t) f->lf.re_sz * 32;
    const size_t a_bytes = sizeof(*f->a) * (size_t) f->sb128w * fh->tiling.rows;           /* the pass-1 half */
    int rc = 0;
    Dav1dHipFrameDesc desc;             /* what the generator below is told about the frame (the glue makes its own for the lister) */
    StoredFrame *const sf = !h->p.stream && h->store && fh->frame_offset < h->store->n ? &h->store->fr[fh->frame_offset] : NULL;
    if (h->p.stream) {
        /* ---- nothing to inject: dav1d's own pass 1 fills the arrays from the tile data (dav1d_decode_tile_sbrow in hk_entropy) */
        return h->p.mode == 1 ? dav1d_hip_glue_frame_init(f) : 0;
    } else if (h->p.inject == 2) {
        for (int j = 0; j < n_tiles; j++) f->ts[j].lflvl = f->lf.lvl;       /* no delta_lf here: the frame's level table, src/decode.c:1018-1021 */
        /* ---- pass 1's output from the store: the three large arrays stand in for the frame context's own where nothing writes them
         * (mode 1; the reference's pass 2 consumes cf, so mode 0 takes copies), the small ones are copied */
        if (!sf || !sf->b || sf->b_bytes != b_bytes || sf->cf_bytes != cf_bytes || sf->cbi_bytes != cbi_entries * 2) return DAV1D_ERR(EINVAL);
        if (h->p.mode == 1) {
            s->own_b = f->frame_thread.b; s->own_cbi = f->frame_thread.cbi; s->own_cf = f->frame_thread.cf;
            f->frame_thread.b = sf->b; f->frame_thread.cbi = sf->cbi; f->frame_thread.cf = sf->cf;
            s->swapped = 1;
        } else {
            memcpy(f->frame_thread.b, sf->b, b_bytes); memcpy(f->frame_thread.cbi, sf->cbi, sf->cbi_bytes); memcpy(f->frame_thread.cf, sf->cf, cf_bytes);
        }
        if (sf->pal_bytes) memcpy(f->frame_thread.pal, sf->pal, sf->pal_bytes);
        if (sf->pal_idx_bytes) memcpy(f->frame_thread.pal_idx, sf->pal_idx, sf->pal_idx_bytes);
        memcpy(f->lf.mask, sf->lf_mask, sf->lf_mask_bytes);
        memcpy(f->lf.level, sf->lf_level, sf->lf_level_bytes);
        if (sf->lr_mask_bytes) memcpy(f->lf.lr_mask, sf->lr_mask, sf->lr_mask_bytes);
        memcpy(f->lf.tx_lpf_right_edge[0], sf->re0, sf->re_bytes); memcpy(f->lf.tx_lpf_right_edge[1], sf->re1, sf->re_bytes);
        memcpy(f->a, sf->a, sf->a_bytes);
    } else {
        for (int j = 0; j < n_tiles; j++) f->ts[j].lflvl = f->lf.lvl;
        /* ---- pass 1's output, generated: block records, cbi, coefficients, palettes */
        dav1d_hip_glue_frame_desc(&desc, f);
        memset(f->frame_thread.cf, 0, cf_bytes);
        memset(f->frame_thread.b, 0, b_bytes);
        Dav1dSynthParams sp = h->p.synth;
        sp.seed += 7919u * (uint64_t) fh->frame_offset;
        sp.cf_align64 = ARCH_X86_64;
        rc = h->hip.synth_frame(&desc, &sp, f->frame_thread.cf, cf_bytes, cbi_entries, f->frame_thread.pal_idx, pal_idx_bytes);
        if (rc) return DAV1D_ERR(EINVAL);
        /* ---- ... and what pass 1 builds for the in-loop filters */
        if (build_filter_inputs(f, (unsigned) (sp.seed & 0xffffff) + 3)) return DAV1D_ERR(EINVAL);
        if (h->p.inject == 1 && sf) {
#define KEEP(dst, n_dst, src, n) do { free(dst); dst = NULL; n_dst = 0; if ((n) && (src)) { dst = malloc(n); if (!dst) return DAV1D_ERR(ENOMEM); memcpy(dst, src, n); n_dst = n; } } while (0)
            KEEP(sf->b, sf->b_bytes, f->frame_thread.b, b_bytes);
            KEEP(sf->cbi, sf->cbi_bytes, f->frame_thread.cbi, cbi_entries * 2);
            KEEP(sf->cf, sf->cf_bytes, f->frame_thread.cf, cf_bytes);
            KEEP(sf->pal, sf->pal_bytes, f->frame_thread.pal, pal_bytes);
            KEEP(sf->pal_idx, sf->pal_idx_bytes, f->frame_thread.pal_idx, pal_idx_bytes);
            KEEP(sf->lf_mask, sf->lf_mask_bytes, f->lf.mask, sizeof(*f->lf.mask) * (size_t) num_sb128);
            KEEP(sf->lf_level, sf->lf_level_bytes, f->lf.level, sizeof(*f->lf.level) * (size_t) num_sb128 * 32 * 32);
            KEEP(sf->lr_mask, sf->lr_mask_bytes, f->lf.lr_mask, sizeof(*f->lf.lr_mask) * (size_t) f->lf.lr_mask_sz);
            size_t dummy;
            KEEP(sf->re0, sf->re_bytes, f->lf.tx_lpf_right_edge[0], re_bytes);
            KEEP(sf->re1, dummy, f->lf.tx_lpf_right_edge[1], re_bytes);
            KEEP(sf->a, sf->a_bytes, f->a, a_bytes);
            (void) dummy;
#undef KEEP
        }
    }
    /* ---- the rows of its references a tile-sbrow needs (decode_b's lowest_pixel bookkeeping, src/decode.c:1957-1990): all of them,
     * or none when the listing may run ahead (the pixels are read when the frame ends, and frames end in order) */
    if (IS_INTER_OR_SWITCH(fh) && !h->p.stream)
        for (int j = 0; j < n_tiles; j++) {
            Dav1dTileState *const ts = &f->ts[j];
            const int rows = (ts->tiling.row_end - ts->tiling.row_start + f->sb_step - 1) >> f->sb_shift;
            for (int r = 0; r < rows; r++)
                for (int n = 0; n < 7; n++) {
                    const int need = h->p.mode == 1 && h->p.free_listing ? INT_MIN : f->refp[n].p.p.h;
                    ts->lowest_pixel[r][n][0] = need;
                    ts->lowest_pixel[r][n][1] = need == INT_MIN ? INT_MIN : need >> (f->cur.p.layout == DAV1D_PIXEL_LAYOUT_I420);
                }
        }
    /* ---- mode 1: the binding takes it from here (frame + lister, the filter stages pointed at the filter lister) */
    return h->p.mode == 1 ? dav1d_hip_glue_frame_init(f) : 0;
}

/* Pass 1.  Chain mode: the hand-off arrays were injected, nothing to do.  Stream mode: dav1d's own entropy decoding of the tile's
 * superblock row, src/decode.c:2594-2748 (this wrapper only records WHERE a tile failed, for the writer of the random payloads,
 * and — mode 1, listing ahead of the references — forgets the reference rows decode_b noted, src/decode.c:1957-1990). */
static int hk_entropy(Dav1dTaskContext *const t) {
    Hooked *const h = g_h;
    if (!h->p.stream) return 0;
    const int rc = dav1d_decode_tile_sbrow(t);
    const Dav1dFrameContext *const f = t->f;
    Dav1dTileState *const ts = t->ts;
    if (rc) {
        const uint8_t *pos = ts->msac.buf_pos < ts->msac.buf_end ? ts->msac.buf_pos : ts->msac.buf_end;
        pthread_mutex_lock(&h->stat_mtx);
        for (int i = 0; i < h->n_tu && h->n_tile_err < 64; i++)
            if (pos >= h->tu[i] && pos <= h->tu[i] + h->tu_size[i]) {
                h->tile_err[h->n_tile_err].tu = i;
                h->tile_err[h->n_tile_err].off = (size_t) (pos - h->tu[i]);
                h->tile_err[h->n_tile_err++].overread = ts->msac.cnt <= -15;
                break;
            }
        pthread_mutex_unlock(&h->stat_mtx);
    } else if (h->p.mode == 1) {
        dav1d_hip_glue_after_entropy(t);
    }
    (void) f;
    return rc;
}

/* ---- which tools the frame's blocks use: the reference's own block walk (decode_sb with pass == 2) over pass 1's output with the two
 * reconstruction hooks pointed at counters.  Stream mode, mode 1, after the frame's listing: nothing else uses the pass-2 cursors. */
static __thread uint64_t *g_hist;
static void count_common(const Dav1dTaskContext *const t, const enum BlockSize bs, const Av1Block *const b) {
    const Dav1dFrameContext *const f = t->f;
    const uint8_t *const b_dim = dav1d_block_dimensions[bs];
    uint64_t *const hs = g_hist;
    hs[HIST_B_SKIP] += b->skip;
    hs[HIST_B_SEG_NONZERO] += !!b->seg_id;
    hs[HIST_B_LOSSLESS] += f->frame_hdr->segmentation.lossless[b->seg_id];
    hs[HIST_B_128] += b_dim[0] == 32 || b_dim[1] == 32;
    hs[HIST_B_4XN] += b_dim[0] == 1 || b_dim[1] == 1;
    const int ss_ver = f->cur.p.layout == DAV1D_PIXEL_LAYOUT_I420, ss_hor = f->cur.p.layout != DAV1D_PIXEL_LAYOUT_I444;
    hs[HIST_B_SUB8X8_CHROMA] += f->cur.p.layout != DAV1D_PIXEL_LAYOUT_I400 && ((b_dim[0] == 1 && ss_hor) || (b_dim[1] == 1 && ss_ver));
}
static void count_intra(Dav1dTaskContext *const t, const enum BlockSize bs, const enum EdgeFlags flags, const Av1Block *const b) {
    (void) flags;
    uint64_t *const hs = g_hist;
    hs[HIST_B_INTRA]++;
    hs[HIST_B_PALETTE_Y] += !!b->pal_sz[0];
    hs[HIST_B_PALETTE_UV] += !!b->pal_sz[1];
    hs[HIST_B_CFL] += b->uv_mode == CFL_PRED;
    hs[HIST_B_FILTER_INTRA] += b->y_mode == FILTER_PRED;
    hs[HIST_B_DIRECTIONAL] += b->y_mode >= VERT_PRED && b->y_mode <= VERT_LEFT_PRED;
    hs[HIST_B_ANGLE_DELTA] += b->y_mode >= VERT_PRED && b->y_mode <= VERT_LEFT_PRED && b->y_angle;
    hs[HIST_B_SMOOTH] += b->y_mode >= SMOOTH_PRED && b->y_mode <= SMOOTH_H_PRED;
    hs[HIST_B_PAETH] += b->y_mode == PAETH_PRED;
    hs[HIST_B_TX64] += b->tx == TX_64X64 || b->tx == RTX_64X32 || b->tx == RTX_32X64 || b->tx == RTX_64X16 || b->tx == RTX_16X64;
    count_common(t, bs, b);
}
static int count_inter(Dav1dTaskContext *const t, const enum BlockSize bs, const Av1Block *const b) {
    const Dav1dFrameContext *const f = t->f;
    uint64_t *const hs = g_hist;
    if (!IS_INTER_OR_SWITCH(f->frame_hdr)) { hs[HIST_B_INTRABC]++; count_common(t, bs, b); return 0; }
    hs[HIST_B_INTER]++;
    hs[HIST_B_SKIP_MODE] += b->skip_mode;
    const int is_comp = b->comp_type != COMP_INTER_NONE;
    hs[HIST_B_COMP_AVG] += b->comp_type == COMP_INTER_AVG;
    hs[HIST_B_COMP_WAVG] += b->comp_type == COMP_INTER_WEIGHTED_AVG;
    hs[HIST_B_COMP_SEG] += b->comp_type == COMP_INTER_SEG;
    hs[HIST_B_COMP_WEDGE] += b->comp_type == COMP_INTER_WEDGE;
    if (!is_comp) {
        hs[HIST_B_INTERINTRA] += !!b->interintra_type;
        hs[HIST_B_INTERINTRA_WEDGE] += b->interintra_type == INTER_INTRA_WEDGE;
        hs[HIST_B_OBMC] += b->motion_mode == MM_OBMC;
        hs[HIST_B_LOCAL_WARP] += b->motion_mode == MM_WARP;
    }
    const int is_gmv = b->inter_mode == (is_comp ? GLOBALMV_GLOBALMV : GLOBALMV);
    hs[HIST_B_GLOBALMV] += is_gmv;
    hs[HIST_B_GLOBAL_WARP] += is_gmv && f->gmv_warp_allowed[b->ref[0]] && imin(dav1d_block_dimensions[bs][0], dav1d_block_dimensions[bs][1]) > 1;
    hs[HIST_B_SCALED_REF] += !!f->svc[b->ref[0]][0].scale || (is_comp && f->svc[b->ref[1]][0].scale);
    hs[HIST_B_FILTER_NOT_REGULAR] += b->filter2d != FILTER_2D_8TAP_REGULAR;
    hs[HIST_B_DUAL_FILTER] += dav1d_filter_dir[b->filter2d][0] != dav1d_filter_dir[b->filter2d][1];
    hs[HIST_B_TX_SPLIT] += b->tx_split0 || b->tx_split1;
    hs[HIST_B_TX64] += b->max_ytx == TX_64X64 || b->max_ytx == RTX_64X32 || b->max_ytx == RTX_32X64 || b->max_ytx == RTX_64X16 || b->max_ytx == RTX_16X64;
    count_common(t, bs, b);
    return 0;
}
static void restore_pass2_cursors(Dav1dFrameContext *const f) {
    /* back to the start of the frame (setup_tile, src/decode.c:2438-2452; reset_context of the pass-2 half, :3182-3188) */
    static const uint8_t ss_size_mul[4][2] = { { 4, 4 }, { 6, 5 }, { 8, 6 }, { 12, 8 } };
    const Dav1dFrameHeader *const fh = f->frame_hdr;
    const uint8_t *const size_mul = ss_size_mul[f->cur.p.layout];
    const int hbd = f->cur.p.bpc > 8;
    for (int j = 0; j < fh->tiling.cols * fh->tiling.rows; j++) {
        const unsigned off = f->frame_thread.tile_start_off[j];
        Dav1dTileState *const ts = &f->ts[j];
        /* (the cursors of pass 2 are [0], those of pass 1 [1]: ts->frame_thread[pass & 1]) */
        ts->frame_thread[0].pal_idx = f->frame_thread.pal_idx ? &f->frame_thread.pal_idx[(size_t) off * size_mul[1] / 8] : NULL;
        ts->frame_thread[0].cbi = &f->frame_thread.cbi[(size_t) off * size_mul[0] / 64];
        ts->frame_thread[0].cf = (uint8_t *) f->frame_thread.cf + (((size_t) off * size_mul[0]) >> !hbd);
    }
}
static void count_frame(Hooked *const h, Dav1dFrameContext *const f) {
    const Dav1dFrameHeader *const fh = f->frame_hdr;
    uint64_t hs[HIST_N];
    memset(hs, 0, sizeof(hs));
    hs[fh->frame_type == DAV1D_FRAME_TYPE_KEY ? HIST_FRAMES_KEY : fh->frame_type == DAV1D_FRAME_TYPE_INTRA ? HIST_FRAMES_INTRA_ONLY : HIST_FRAMES_INTER]++;
    hs[HIST_FRAMES_SUPER_RES] += fh->width[0] != fh->width[1];
    int scaled = 0;
    if (IS_INTER_OR_SWITCH(fh)) for (int i = 0; i < 7; i++) scaled |= !!f->svc[i][0].scale;
    hs[HIST_FRAMES_SCALED_REFS] += scaled;
    hs[HIST_FRAMES_INTRABC] += fh->allow_intrabc;
    hs[HIST_FRAMES_FILM_GRAIN] += fh->film_grain.present;
    hs[HIST_FRAMES_DELTA_LF] += fh->delta.lf.present;
    hs[HIST_FRAMES_SEGMENTED] += fh->segmentation.enabled;
    hs[HIST_FRAMES_LOSSLESS] += fh->all_lossless;
    /* transform blocks: the cbi entries pass 1 wrote, tile by tile (its cursor stands behind the last one) */
    {
        static const uint8_t ss_size_mul[4][2] = { { 4, 4 }, { 6, 5 }, { 8, 6 }, { 12, 8 } };
        for (int j = 0; j < fh->tiling.cols * fh->tiling.rows; j++) {
            const int16_t *c0 = &f->frame_thread.cbi[(size_t) f->frame_thread.tile_start_off[j] * ss_size_mul[f->cur.p.layout][0] / 64];
            const int16_t *const c1 = f->ts[j].frame_thread[1].cbi;
            for (; c0 < c1; c0++) {
                const int eob = *c0 >> 5, txtp = *c0 & 31;
                hs[HIST_TX_BLOCKS]++;
                hs[HIST_TX_NO_COEFS] += eob < 0;
                hs[HIST_TX_EOB0] += eob == 0;
                hs[HIST_TX_NON_DCT] += eob >= 0 && txtp != DCT_DCT;
            }
        }
    }
    if (f->lf.lr_mask && f->lf.restore_planes)
        for (int i = 0; i < f->lf.lr_mask_sz; i++)
            for (int pl = 0; pl < 3; pl++)
                for (int u = 0; u < 4; u++) {
                    const int ty = f->lf.lr_mask[i].lr[pl][u].type;
                    hs[HIST_LR_WIENER] += ty == DAV1D_RESTORATION_WIENER;
                    hs[HIST_LR_SGR] += ty >= DAV1D_RESTORATION_SGRPROJ;
                }
    for (int i = 0; i < f->sb128w * f->sb128h; i++)
        for (int q = 0; q < 4; q++) hs[HIST_CDEF_NONZERO_IDX] += f->lf.mask[i].cdef_idx[q] > 0;
    Dav1dTaskContext *t = NULL;
    if (!posix_memalign((void **) &t, 64, sizeof(*t))) {
        memset(t, 0, sizeof(*t));
        const recon_b_intra_fn keep_intra = f->bd_fn.recon_b_intra;
        const recon_b_inter_fn keep_inter = f->bd_fn.recon_b_inter;
        f->bd_fn.recon_b_intra = count_intra;
        f->bd_fn.recon_b_inter = count_inter;
        g_hist = hs;
        t->c = f->c; t->f = f;
        t->frame_thread.pass = 2;
        int rc = 0;
        for (int tile_row = 0; tile_row < fh->tiling.rows && !rc; tile_row++)
            for (int sby = fh->tiling.row_start_sb[tile_row]; sby < fh->tiling.row_start_sb[tile_row + 1] && !rc; sby++) {
                t->by = sby << f->sb_shift;
                for (int tile_col = 0; tile_col < fh->tiling.cols && !rc; tile_col++) {
                    t->ts = &f->ts[tile_row * fh->tiling.cols + tile_col];
                    rc = dav1d_decode_tile_sbrow(t);
                }
            }
        g_hist = NULL;
        f->bd_fn.recon_b_intra = keep_intra;
        f->bd_fn.recon_b_inter = keep_inter;
        restore_pass2_cursors(f);
        free(t);
    }
    pthread_mutex_lock(&h->stat_mtx);
    for (int i = 0; i < HIST_N; i++) h->hist[i] += hs[i];
    pthread_mutex_unlock(&h->stat_mtx);
}

/* ---- what the harness wants to know while the binding works (Dav1dHipGlueOptions observers) */
static void ob_stat(void *const cookie, const int what, const double t0) { stat_add(cookie, what, t0); }
static void ob_frame_listed(void *const cookie, Dav1dFrameContext *const f) { Hooked *const h = cookie; if (h->p.stream) count_frame(h, f); }
static void ob_frame_end_seconds(void *const cookie, Dav1dFrameContext *const f, const double sec) {
    Hooked *const h = cookie;
    if (!h->p.stream && f->frame_hdr->frame_offset < 64) h->frame_end_s[f->frame_hdr->frame_offset] = sec;
}
static void ob_before_frame_done(void *const cookie, Dav1dFrameContext *const f, const int rc) {
    (void) cookie; (void) rc;
    FcState *const s = state_of(f);
    if (s->swapped) {          /* the frame context gets its own arrays back before dav1d sees the frame again */
        f->frame_thread.b = s->own_b; f->frame_thread.cbi = s->own_cbi; f->frame_thread.cf = s->own_cf;
        s->swapped = 0;
    }
}
static void ob_after_frame_done(void *const cookie, const int k) {
    Hooked *const h = cookie;
    if (!h->p.stream && k >= 0 && k < h->p.n_frames) h->q_done_t[k] = now_s();
}

static const Dav1dHooks hooks_cpu = { NULL, hk_after_init, hk_entropy, NULL, NULL };
static const Dav1dHooks hooks_hip = { dav1d_hip_glue_before_init, hk_after_init, hk_entropy, dav1d_hip_glue_recon_tile_sbrow, dav1d_hip_glue_frame_complete };

/* ------------------------------------------------------------------------------------------------ headers */
static void fill_seq(Dav1dSequenceHeader *const seq, const HookedParams *const p) {
    memset(seq, 0, sizeof(*seq));
    seq->profile = p->layout == DAV1D_PIXEL_LAYOUT_I444 ? 1 : p->layout == DAV1D_PIXEL_LAYOUT_I422 || p->bpc == 12 ? 2 : 0;
    seq->max_width = p->w; seq->max_height = p->h;
    seq->layout = p->layout;
    seq->hbd = p->bpc == 8 ? 0 : p->bpc == 10 ? 1 : 2;
    seq->monochrome = p->layout == DAV1D_PIXEL_LAYOUT_I400;
    seq->ss_hor = p->layout != DAV1D_PIXEL_LAYOUT_I444; seq->ss_ver = p->layout == DAV1D_PIXEL_LAYOUT_I420;
    seq->sb128 = p->sb128;
    seq->intra_edge_filter = 1;
    seq->inter_intra = seq->masked_compound = seq->warped_motion = seq->dual_filter = seq->filter_intra = 1;
    seq->order_hint = 1; seq->order_hint_n_bits = 7;
    seq->jnt_comp = 1;
    seq->cdef = p->cdef_enabled;
    seq->restoration = p->lr_type[0] || p->lr_type[1] || p->lr_type[2];
    seq->num_operating_points = 1;
}

static void fill_frame(Dav1dFrameHeader *const fh, const HookedParams *const p, const int k) {
    memset(fh, 0, sizeof(*fh));
    fh->frame_type = k ? DAV1D_FRAME_TYPE_INTER : DAV1D_FRAME_TYPE_KEY;
    fh->show_frame = fh->showable_frame = 1;
    fh->error_resilient_mode = !k;
    fh->width[0] = fh->width[1] = fh->render_width = p->w;
    fh->height = fh->render_height = p->h;
    fh->super_res.width_scale_denominator = 8;
    fh->frame_offset = k;
    fh->primary_ref_frame = DAV1D_PRIMARY_REF_NONE;
    fh->refresh_frame_flags = k ? 1 << (k & 7) : 0xff;
    /* the three frames before this one, round and round: frame j >= 1 sits in slot j & 7 (until frame j + 8 takes the slot), the key
     * frame in every slot it has not been pushed out of — slot 0 as long as it is referenced (k <= 3) */
    for (int i = 0; i < 7; i++) {
        int j = k - 1 - i % 3;
        if (j < 0) j = 0;
        fh->refidx[i] = j & 7;
    }
    fh->hp = 1;
    fh->subpel_filter_mode = DAV1D_FILTER_SWITCHABLE;
    fh->switchable_motion_mode = 1;
    fh->warp_motion = 1;
    fh->switchable_comp_refs = !!k;
    fh->txfm_mode = DAV1D_TX_SWITCHABLE;
    fh->tiling.uniform = 1;
    fh->tiling.cols = p->n_tile_cols; fh->tiling.rows = p->n_tile_rows;
    for (int i = 0; i <= p->n_tile_cols; i++) fh->tiling.col_start_sb[i] = p->col_start_sb[i];
    for (int i = 0; i <= p->n_tile_rows; i++) fh->tiling.row_start_sb[i] = p->row_start_sb[i];
    fh->quant.yac = 100;
    fh->loopfilter.level_y[0] = p->lf_level_y[0]; fh->loopfilter.level_y[1] = p->lf_level_y[1];
    fh->loopfilter.level_u = p->lf_level_u; fh->loopfilter.level_v = p->lf_level_v;
    fh->loopfilter.sharpness = p->lf_sharpness;
    fh->cdef.damping = p->cdef_damping; fh->cdef.n_bits = p->cdef_n_bits;
    for (int i = 0; i < 8; i++) { fh->cdef.y_strength[i] = p->cdef_y_strength[i]; fh->cdef.uv_strength[i] = p->cdef_uv_strength[i]; }
    for (int i = 0; i < 3; i++) fh->restoration.type[i] = p->lr_type[i];
    fh->restoration.unit_size[0] = p->lr_unit_size[0]; fh->restoration.unit_size[1] = p->lr_unit_size[1];
    for (int i = 0; i < 7; i++) fh->gmv[i] = dav1d_default_wm_params;
    if (p->apply_grain && !p->stream) {
        /* luma scaling points only: dav1d_apply_grain copies both chroma planes from the source picture (src/fg_apply_tmpl.c:127-163) */
        Dav1dFilmGrainData *const fg = &fh->film_grain.data;
        fh->film_grain.present = 1; fh->film_grain.update = 1;
        fg->seed = (unsigned) (1234 + 977 * k) & 0xffff;
        fg->num_y_points = 3;
        fg->y_points[0][0] = 0;   fg->y_points[0][1] = 48;
        fg->y_points[1][0] = 128; fg->y_points[1][1] = 96 + 8 * (k & 3);
        fg->y_points[2][0] = 255; fg->y_points[2][1] = 32;
        fg->scaling_shift = 10; fg->ar_coeff_lag = 2; fg->ar_coeff_shift = 7;
        for (int i = 0; i < 12; i++) fg->ar_coeffs_y[i] = (int8_t) ((i * 7 + k) % 17 - 8);
        fg->overlap_flag = 1;
    }
}

/* ------------------------------------------------------------------------------------------------ outputs */
static uint64_t hash_bytes(uint64_t x, const uint8_t *p, size_t n);
static int pic_has_grain(const Dav1dPicture *pic);
/* chain mode with HookedParams.apply_grain: frame k's picture with its film grain, as tight planes (or their digests) */
static void keep_picture_with_grain(Hooked *const h, const Dav1dPicture *const pic, const int k) {
    const int bps = pic->p.bpc > 8 ? 2 : 1, n_pl = pic->p.layout == DAV1D_PIXEL_LAYOUT_I400 ? 1 : 3;
    const int ss_hor = pic->p.layout != DAV1D_PIXEL_LAYOUT_I444, ss_ver = pic->p.layout == DAV1D_PIXEL_LAYOUT_I420;
    uint8_t *planes[3] = { NULL, NULL, NULL };
    int rc = 0;
    for (int pl = 0; pl < n_pl; pl++) {
        const int w = pl ? (pic->p.w + ss_hor) >> ss_hor : pic->p.w, hh = pl ? (pic->p.h + ss_ver) >> ss_ver : pic->p.h;
        planes[pl] = malloc((size_t) w * hh * bps);
        if (!planes[pl]) rc = -ENOMEM;
    }
    if (!rc && h->p.mode == 1) rc = dav1d_hip_glue_output_with_grain(h->glue, pic, planes);
    else if (!rc) {
        Dav1dPicture grained;
        memset(&grained, 0, sizeof(grained));
        rc = dav1d_apply_grain(h->c, &grained, pic);
        for (int pl = 0; pl < n_pl && !rc; pl++) {
            const int w = pl ? (pic->p.w + ss_hor) >> ss_hor : pic->p.w, hh = pl ? (pic->p.h + ss_ver) >> ss_ver : pic->p.h;
            for (int y = 0; y < hh; y++) memcpy(planes[pl] + (size_t) y * w * bps, (const uint8_t *) grained.data[pl] + (ptrdiff_t) y * grained.stride[!!pl], (size_t) w * bps);
        }
        if (grained.data[0]) dav1d_picture_unref(&grained);
    }
    for (int pl = 0; pl < n_pl; pl++) {
        const int w = pl ? (pic->p.w + ss_hor) >> ss_hor : pic->p.w, hh = pl ? (pic->p.h + ss_ver) >> ss_ver : pic->p.h;
        if (rc) { free(planes[pl]); continue; }
        if (h->p.keep_output == 2) {
            uint64_t x = 0xDA71Dull + (uint64_t) pl;
            for (int y = 0; y < hh; y++) x = hash_bytes(x, planes[pl] + (size_t) y * w * bps, (size_t) w * bps);
            h->out_hash[k * 3 + pl] = x;
            free(planes[pl]);
        } else {
            free(h->out_plane[k * 3 + pl]);
            h->out_plane[k * 3 + pl] = planes[pl];
        }
    }
    if (rc) h->failed = 1;
}

static void keep_picture(Hooked *const h, const Dav1dPicture *const pic) {
    const int k = pic->frame_hdr->frame_offset;
    if (k < 0 || k >= h->p.n_frames) return;
    h->n_out++;
    h->out_t[k] = now_s();                /* when dav1d_get_picture / dav1d_submit_frame handed frame k out (either mode) */
    if (h->p.keep_output && h->p.apply_grain && pic_has_grain(pic)) { keep_picture_with_grain(h, pic, k); return; }
    if (h->p.keep_output == 2) {          /* digests of the visible rows only (long chains of large pictures) */
        const int bps2 = pic->p.bpc > 8 ? 2 : 1;
        const int ssh = pic->p.layout != DAV1D_PIXEL_LAYOUT_I444, ssv = pic->p.layout == DAV1D_PIXEL_LAYOUT_I420;
        for (int pl = 0; pl < (pic->p.layout == DAV1D_PIXEL_LAYOUT_I400 ? 1 : 3); pl++) {
            const int w = pl ? (pic->p.w + ssh) >> ssh : pic->p.w, hh = pl ? (pic->p.h + ssv) >> ssv : pic->p.h;
            uint64_t x = 0xDA71Dull + (uint64_t) pl;
            for (int y = 0; y < hh; y++) x = hash_bytes(x, (const uint8_t *) pic->data[pl] + (ptrdiff_t) y * pic->stride[!!pl], (size_t) w * bps2);
            h->out_hash[k * 3 + pl] = x;
        }
        return;
    }
    if (!h->p.keep_output) return;
    const int bps = pic->p.bpc > 8 ? 2 : 1;
    const int ss_hor = pic->p.layout != DAV1D_PIXEL_LAYOUT_I444, ss_ver = pic->p.layout == DAV1D_PIXEL_LAYOUT_I420;
    for (int pl = 0; pl < (pic->p.layout == DAV1D_PIXEL_LAYOUT_I400 ? 1 : 3); pl++) {
        const int w = pl ? (pic->p.w + ss_hor) >> ss_hor : pic->p.w, hh = pl ? (pic->p.h + ss_ver) >> ss_ver : pic->p.h;
        uint8_t *const dst = malloc((size_t) w * hh * bps);
        if (!dst) { h->failed = 1; return; }
        for (int y = 0; y < hh; y++) memcpy(dst + (size_t) y * w * bps, (const uint8_t *) pic->data[pl] + (ptrdiff_t) y * pic->stride[!!pl], (size_t) w * bps);
        free(h->out_plane[k * 3 + pl]);
        h->out_plane[k * 3 + pl] = dst;
    }
}

/* stream mode: every picture dav1d_get_picture hands out, in that order, as tight planes.  Film grain (HookedParams.apply_grain): mode 0
 * gets it from dav1d (dav1d_apply_grain behind output_image, src/lib.c:311-329); in mode 1 dav1d was opened with apply_grain = 0 and the
 * grain goes on here, on the device, from the picture's own header — what an application with a GPU output path does. */
static int pic_has_grain(const Dav1dPicture *const pic) {          /* has_grain(), src/lib.c:303-309 */
    const Dav1dFilmGrainData *const fg = &pic->frame_hdr->film_grain.data;
    return fg->num_y_points || fg->num_uv_points[0] || fg->num_uv_points[1] || (fg->clip_to_restricted_range && fg->chroma_scaling_from_luma);
}
static uint64_t hash_bytes(uint64_t x, const uint8_t *p, size_t n) {
    for (; n >= 8; n -= 8, p += 8) { uint64_t v; memcpy(&v, p, 8); x = (x ^ v) * 0x9E3779B97F4A7C15ull; x ^= x >> 29; }
    for (; n; n--, p++) { x = (x ^ *p) * 0x100000001B3ull; }
    return x;
}
static void keep_stream_picture(Hooked *const h, const Dav1dPicture *const pic) {
    if (h->n_out_pics == h->cap_out_pics) {
        const int cap = h->cap_out_pics ? 2 * h->cap_out_pics : 64;
        OutPic *const np = realloc(h->out_pics, (size_t) cap * sizeof(*np));
        if (!np) { h->failed = 1; return; }
        h->out_pics = np; h->cap_out_pics = cap;
    }
    OutPic *const o = &h->out_pics[h->n_out_pics];
    memset(o, 0, sizeof(*o));
    o->w = pic->p.w; o->h = pic->p.h; o->layout = pic->p.layout; o->bpc = pic->p.bpc; o->frame_offset = pic->frame_hdr->frame_offset;
    const int bps = pic->p.bpc > 8 ? 2 : 1, n_pl = pic->p.layout == DAV1D_PIXEL_LAYOUT_I400 ? 1 : 3;
    const int ss_hor = pic->p.layout != DAV1D_PIXEL_LAYOUT_I444, ss_ver = pic->p.layout == DAV1D_PIXEL_LAYOUT_I420;
    const int grain_here = h->p.mode == 1 && h->p.apply_grain && pic_has_grain(pic);
    o->grain = h->p.apply_grain && pic_has_grain(pic);
    int rc = 0;
    uint8_t *planes[3] = { NULL, NULL, NULL };
    for (int pl = 0; pl < n_pl; pl++) {
        const int w = pl ? (pic->p.w + ss_hor) >> ss_hor : pic->p.w, hh = pl ? (pic->p.h + ss_ver) >> ss_ver : pic->p.h;
        planes[pl] = malloc((size_t) w * hh * bps);
        if (!planes[pl]) rc = -ENOMEM;
    }
    if (!rc && grain_here) rc = dav1d_hip_glue_output_with_grain(h->glue, pic, planes);
    for (int pl = 0; pl < n_pl; pl++) {
        const int w = pl ? (pic->p.w + ss_hor) >> ss_hor : pic->p.w, hh = pl ? (pic->p.h + ss_ver) >> ss_ver : pic->p.h;
        uint8_t *const dst = planes[pl];
        if (rc || !dst) { free(dst); continue; }
        if (!grain_here) for (int y = 0; y < hh; y++) memcpy(dst + (size_t) y * w * bps, (const uint8_t *) pic->data[pl] + (ptrdiff_t) y * pic->stride[!!pl], (size_t) w * bps);
        o->hash[pl] = hash_bytes(0xDA71Dull + (uint64_t) pl, dst, (size_t) w * hh * bps);
        if (h->p.keep_output == 2) free(dst);           /* digests only (long chains of large pictures) */
        else o->plane[pl] = dst;
    }
    o->t = now_s();
    if (rc) h->failed = 1;
    h->n_out_pics++;
}

/* ------------------------------------------------------------------------------------------------ entry points */
void dav1d_hooked_close(void *handle);

void *dav1d_hooked_store_create(const int n_frames) {
    Store *const st = calloc(1, sizeof(*st));
    if (!st) return NULL;
    st->fr = calloc((size_t) n_frames, sizeof(*st->fr));
    if (!st->fr) { free(st); return NULL; }
    st->n = n_frames;
    return st;
}
void dav1d_hooked_store_destroy(void *const store) {
    Store *const st = store;
    if (!st) return;
    for (int i = 0; i < st->n; i++) {
        StoredFrame *const f = &st->fr[i];
        free(f->b); free(f->cbi); free(f->cf); free(f->pal); free(f->pal_idx); free(f->lf_mask); free(f->lf_level); free(f->lr_mask);
        free(f->re0); free(f->re1); free(f->a);
    }
    free(st->fr);
    free(st);
}

void *dav1d_hooked_open(const HookedParams *const p, const char *const hip_lib, void *const store) {
    Hooked *const h = calloc(1, sizeof(*h));
    if (!h) return NULL;
    crash_handler_install();
    h->p = *p;
    h->store = store;
    if (p->inject && !store) { free(h); return NULL; }
    pthread_mutex_init(&h->stat_mtx, NULL);
    if (!p->stream) {
        /* ../../tests/synth/libdav1d_synth.so, seen from where this library lies (oracle/_ref_hooked/) */
        Dl_info me;
        char path[4096];
        if (!dladdr((void *) dav1d_hooked_close, &me) || !me.dli_fname || strlen(me.dli_fname) > sizeof(path) - 64) goto fail;
        strcpy(path, me.dli_fname);
        char *slash = strrchr(path, '/');
        if (!slash) goto fail;
        strcpy(slash, "/../../tests/synth/libdav1d_synth.so");
        h->hip.synth_dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!h->hip.synth_dl) goto fail;
        *(void **) &h->hip.synth_frame = dlsym(h->hip.synth_dl, "dav1d_synth_frame");
        if (!h->hip.synth_frame) goto fail;
    }
    Dav1dSettings s;
    dav1d_default_settings(&s);
    s.n_threads = p->n_threads;
    s.max_frame_delay = p->frame_delay;
    s.apply_grain = p->stream && p->mode == 0 && p->apply_grain;
    s.inloop_filters = DAV1D_INLOOPFILTER_ALL & ~p->filters_off;
    if (p->mode == 1) {
        Dav1dHipGlueOptions o;
        memset(&o, 0, sizeof(o));
        o.hip_lib = hip_lib; o.device = p->device; o.n_devices = p->n_devices; o.pack = p->pack; o.free_listing = p->free_listing; o.row_progress = p->row_progress;
        o.keep_cf = !p->stream;                      /* chain mode: the generator / the store owns the arena */
        o.cookie = h; o.stat = ob_stat; o.frame_listed = ob_frame_listed; o.frame_end_seconds = ob_frame_end_seconds;
        o.before_frame_done = ob_before_frame_done; o.after_frame_done = ob_after_frame_done;
        if (dav1d_hip_glue_create(&h->glue, &o)) goto fail;
        dav1d_hip_glue_settings(h->glue, &s);        /* the allocator; apply_grain off: the grain goes on on the device */
    }
    if (dav1d_open(&h->c, &s)) goto fail;
    if (h->c->n_fc < 2) goto fail;                       /* the two-pass hand-off only exists with frame threading */
    h->n_fc = h->c->n_fc;
    h->fcs = calloc(h->n_fc, sizeof(*h->fcs));
    h->q_done_t = calloc((size_t) p->n_frames + 1, sizeof(*h->q_done_t));
    h->out_t = calloc((size_t) p->n_frames + 1, sizeof(*h->out_t));
    h->out_hash = calloc((size_t) p->n_frames * 3 + 3, sizeof(*h->out_hash));
    h->out_plane = calloc((size_t) p->n_frames * 3 + 3, sizeof(*h->out_plane));
    if (!h->fcs || !h->out_plane || !h->q_done_t || !h->out_t || !h->out_hash) goto fail;
    h->seq_ref = dav1d_ref_create(ALLOC_OBU_HDR, sizeof(Dav1dSequenceHeader));
    if (!h->seq_ref) goto fail;
    fill_seq(h->seq_ref->data, p);
    return h;
fail:
    dav1d_hooked_close(h);
    return NULL;
}

void dav1d_hooked_stats(void *const handle, double *const out) { memcpy(out, ((Hooked *) handle)->stat, sizeof(((Hooked *) handle)->stat)); }
void dav1d_hooked_frame_end_seconds(void *const handle, double *const out) { memcpy(out, ((Hooked *) handle)->frame_end_s, sizeof(((Hooked *) handle)->frame_end_s)); }
/* seconds between the completion of frame `from` and of the last frame (mode 1): the chain without its key frame and warm-up */
double dav1d_hooked_tail_seconds(void *const handle, const int from) {
    Hooked *const h = handle;
    if (from < 0 || from >= h->p.n_frames - 1 || !h->q_done_t[from] || !h->q_done_t[h->p.n_frames - 1]) return 0.;
    return h->q_done_t[h->p.n_frames - 1] - h->q_done_t[from];
}
/* chain mode: seconds between the output of frame `from` and of the last frame (either mode: the steady state of the peer too) */
double dav1d_hooked_output_tail_seconds(void *const handle, const int from) {
    const Hooked *const h = handle;
    if (from < 0 || from >= h->p.n_frames - 1) return 0.;
    return h->out_t[h->p.n_frames - 1] - h->out_t[from];
}
/* chain mode, keep_output == 2: the digests of frame k's planes */
int dav1d_hooked_picture_digest(void *const handle, const int k, uint64_t out[3]) {
    const Hooked *const h = handle;
    if (k < 0 || k >= h->p.n_frames) return -1;
    for (int pl = 0; pl < 3; pl++) out[pl] = h->out_hash[k * 3 + pl];
    return 0;
}
/* device d of the binding: frames that ended on it (out[0]) and reference pictures copied to it from another device (out[1]); returns the number of devices */
int dav1d_hooked_device_stats(void *const handle, const int d, int out[2]) {
    if (!handle || !((Hooked *) handle)->glue) return 0;
    out[0] = out[1] = 0;
    (void) dav1d_hip_glue_device_stats(((Hooked *) handle)->glue, d, &out[0], &out[1]);
    return dav1d_hip_glue_devices(((Hooked *) handle)->glue);
}
int dav1d_hooked_band_copies(void *const handle, const int d) { return handle && ((Hooked *) handle)->glue ? dav1d_hip_glue_band_copies(((Hooked *) handle)->glue, d) : 0; }
int dav1d_hooked_twin_only_frames(void *const handle, const int d) { return handle && ((Hooked *) handle)->glue ? dav1d_hip_glue_twin_only_frames(((Hooked *) handle)->glue, d) : 0; }
int dav1d_hooked_row_publications(void *const handle) { return handle ? dav1d_hip_glue_row_publications(((Hooked *) handle)->glue) : 0; }
int dav1d_hooked_n_fc(void *const handle) { return handle ? (int) ((Hooked *) handle)->n_fc : 0; }

/* the whole chain: returns 0 and the wall-clock seconds from the first dav1d_submit_frame to the last picture out */
int dav1d_hooked_run(void *const handle, double *const seconds) {
    Hooked *const h = handle;
    Dav1dContext *const c = h->c;
    const HookedParams *const p = &h->p;
    const int n_tiles = p->n_tile_cols * p->n_tile_rows;
    g_h = h;
    dav1d_hooks = &hooks_cpu;
    if (p->stream) return -1;
    h->n_out = 0; h->failed = 0;
    memset(h->stat, 0, sizeof(h->stat));
    if (p->mode == 1) {
        if (dav1d_hip_glue_attach(h->glue, c)) return -1;           /* per-frame-context state, the three stage threads */
        dav1d_hooks = &hooks_hip;                                    /* (the harness's after_init / entropy hooks in front of the glue's) */
    }
    int rc = 0;
    const double t0 = now_s();
    for (int k = 0; k < p->n_frames && !rc; k++) {
        /* what dav1d_parse_obus leaves behind for dav1d_submit_frame (src/obu.c:1220 ff.): sequence and frame header, tile groups */
        c->seq_hdr_ref = h->seq_ref; c->seq_hdr = h->seq_ref->data;
        if (!k) dav1d_ref_inc(h->seq_ref);
        c->frame_hdr_ref = dav1d_ref_create(ALLOC_OBU_HDR, sizeof(Dav1dFrameHeader));
        if (!c->frame_hdr_ref) { rc = -1; break; }
        c->frame_hdr = c->frame_hdr_ref->data;
        fill_frame(c->frame_hdr, p, k);
        if (c->n_tile_data_alloc < n_tiles) {
            c->tile = dav1d_realloc(ALLOC_TILE, c->tile, sizeof(*c->tile) * n_tiles);
            if (!c->tile) { rc = -1; break; }
            c->n_tile_data_alloc = n_tiles;
        }
        memset(c->tile, 0, sizeof(*c->tile) * n_tiles);
        for (int j = 0; j < n_tiles; j++) c->tile[j].start = c->tile[j].end = j;     /* one empty tile group per tile: no bytes to parse */
        c->n_tile_data = n_tiles;
        c->n_tiles = n_tiles;
        rc = dav1d_submit_frame(c);
        if (rc) break;
        if (c->out.p.data[0]) { keep_picture(h, &c->out.p); dav1d_thread_picture_unref(&c->out); }
    }
    /* drain */
    c->drain = 1;
    for (;;) {
        Dav1dPicture pic;
        memset(&pic, 0, sizeof(pic));
        const int r = dav1d_get_picture(c, &pic);
        if (r) { if (r != DAV1D_ERR(EAGAIN) && !rc) rc = r; break; }
        keep_picture(h, &pic);
        dav1d_picture_unref(&pic);
    }
    h->seconds = now_s() - t0;
    if (p->mode == 1) dav1d_hip_glue_detach(h->glue);
    dav1d_hooks = NULL;
    if (p->mode == 1 && dav1d_hip_glue_backend_failures(h->glue)) h->failed = 1;
    if (seconds) *seconds = h->seconds;
    if (!rc && (h->failed || h->n_out != p->n_frames)) rc = -2;
    return rc;
}

/* ---- stream mode: an AV1 bitstream through dav1d's public API (the loop of tools/dav1d.c:  dav1d_send_data / dav1d_get_picture until the
 * input is used up, then draining).  tu[i] / tu_size[i]: the temporal units, which must stay alive and unchanged during the call (the
 * tile data is referenced in place, dav1d_data_wrap).  Returns 0 when dav1d accepted every unit; the pictures it produced, the
 * pictures it reported an error for and the tiles whose entropy decoding failed are read with the functions below. */
static void no_free(const uint8_t *const data, void *const cookie) { (void) data; (void) cookie; }

int dav1d_hooked_stream_run(void *const handle, const uint8_t *const *const tu, const size_t *const tu_size, const int n_tu, double *const seconds) {
    Hooked *const h = handle;
    Dav1dContext *const c = h->c;
    const HookedParams *const p = &h->p;
    if (!p->stream) return -1;
    g_h = h;
    dav1d_hooks = &hooks_cpu;
    h->failed = 0; h->n_errors = 0; h->n_tile_err = 0;
    h->tu = tu; h->tu_size = tu_size; h->n_tu = n_tu;
    memset(h->stat, 0, sizeof(h->stat));
    memset(h->hist, 0, sizeof(h->hist));
    for (int i = 0; i < h->n_out_pics; i++) for (int pl = 0; pl < 3; pl++) free(h->out_pics[i].plane[pl]);
    h->n_out_pics = 0;
    if (p->mode == 1) {
        if (dav1d_hip_glue_attach(h->glue, c)) return -1;           /* per-frame-context state, the three stage threads */
        dav1d_hooks = &hooks_hip;                                    /* (the harness's after_init / entropy hooks in front of the glue's) */
    }
    int rc = 0;
    const double t0 = now_s();
    for (int k = 0; k < n_tu && !rc; k++) {
        Dav1dData data;
        memset(&data, 0, sizeof(data));
        if (dav1d_data_wrap(&data, tu[k], tu_size[k], no_free, NULL)) { rc = -1; break; }
        do {
            int r = dav1d_send_data(c, &data);
            if (r < 0 && r != DAV1D_ERR(EAGAIN)) { h->n_errors++; dav1d_data_unref(&data); break; }      /* a unit the parser rejects */
            Dav1dPicture pic;
            memset(&pic, 0, sizeof(pic));
            r = dav1d_get_picture(c, &pic);
            if (!r) { keep_stream_picture(h, &pic); dav1d_picture_unref(&pic); }
            else if (r != DAV1D_ERR(EAGAIN)) h->n_errors++;                                              /* a frame that failed to decode */
        } while (data.sz > 0);
    }
    for (;;) {          /* drain */
        Dav1dPicture pic;
        memset(&pic, 0, sizeof(pic));
        const int r = dav1d_get_picture(c, &pic);
        if (r == DAV1D_ERR(EAGAIN)) break;
        if (r) { h->n_errors++; continue; }
        keep_stream_picture(h, &pic);
        dav1d_picture_unref(&pic);
    }
    h->seconds = now_s() - t0;
    if (p->mode == 1) dav1d_hip_glue_detach(h->glue);
    dav1d_hooks = NULL;
    if (p->mode == 1 && dav1d_hip_glue_backend_failures(h->glue)) h->failed = 1;
    h->tu = NULL; h->tu_size = NULL; h->n_tu = 0;
    if (seconds) *seconds = h->seconds;
    if (!rc && h->failed) rc = -2;           /* the BACKEND failed (a frame dav1d itself rejects is not that: n_errors) */
    return rc;
}
int dav1d_hooked_stream_pictures(void *const handle) { return ((Hooked *) handle)->n_out_pics; }
int dav1d_hooked_stream_errors(void *const handle) { return ((Hooked *) handle)->n_errors; }
/* info: w, h, layout, bpc, frame_offset (the order hint), film grain applied */
const void *dav1d_hooked_stream_picture(void *const handle, const int i, const int plane, int info[6]) {
    Hooked *const h = handle;
    if (i < 0 || i >= h->n_out_pics || plane < 0 || plane > 2) return NULL;
    const OutPic *const o = &h->out_pics[i];
    if (info) { info[0] = o->w; info[1] = o->h; info[2] = o->layout; info[3] = o->bpc; info[4] = o->frame_offset; info[5] = o->grain; }
    return o->plane[plane];
}
/* out[0..2] = digests of the planes (keep_output = 2 keeps nothing else), returns the time the picture came out of dav1d_get_picture */
double dav1d_hooked_stream_picture_digest(void *const handle, const int i, uint64_t out[3]) {
    Hooked *const h = handle;
    if (i < 0 || i >= h->n_out_pics) return 0.;
    for (int pl = 0; pl < 3; pl++) out[pl] = h->out_pics[i].hash[pl];
    return h->out_pics[i].t;
}
/* tiles whose pass 1 failed: out[3 * i] = temporal unit, [3 * i + 1] = byte offset in it the symbol decoder had reached, [3 * i + 2] = 1 if it
 * ran out of data (src/decode.c:2743) */
int dav1d_hooked_stream_tile_errors(void *const handle, long *const out, const int cap) {
    Hooked *const h = handle;
    const int n = h->n_tile_err < cap ? h->n_tile_err : cap;
    for (int i = 0; i < n; i++) { out[3 * i] = h->tile_err[i].tu; out[3 * i + 1] = (long) h->tile_err[i].off; out[3 * i + 2] = h->tile_err[i].overread; }
    return h->n_tile_err;
}
int dav1d_hooked_stream_histogram(void *const handle, uint64_t *const out, const int cap) {
    Hooked *const h = handle;
    for (int i = 0; i < HIST_N && i < cap; i++) out[i] = h->hist[i];
    return HIST_N;
}

const void *dav1d_hooked_plane(void *const handle, const int frame, const int plane) {
    Hooked *const h = handle;
    return frame >= 0 && frame < h->p.n_frames && plane >= 0 && plane < 3 ? h->out_plane[frame * 3 + plane] : NULL;
}

void dav1d_hooked_close(void *const handle) {
    Hooked *const h = handle;
    if (!h) return;
    if (h->c) {
        /* the references of the last frames still hold pictures: dav1d_close releases them through the allocator */
        dav1d_close(&h->c);
    }
    free(h->fcs);
    if (h->seq_ref) dav1d_ref_dec(&h->seq_ref);
    dav1d_hip_glue_destroy(h->glue);
    if (h->out_plane) { for (int i = 0; i < h->p.n_frames * 3; i++) free(h->out_plane[i]); free(h->out_plane); }
    for (int i = 0; i < h->n_out_pics; i++) for (int pl = 0; pl < 3; pl++) free(h->out_pics[i].plane[pl]);
    free(h->out_pics);
    free(h->q_done_t);
    free(h->out_t);
    free(h->out_hash);
    if (h->hip.synth_dl) dlclose(h->hip.synth_dl);
    free(h);
}
