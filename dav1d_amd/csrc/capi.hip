// Host side of the C ABI declared in include/dav1d_hip.h: context, recorded launch sequences, options, device memory, devices (the rest: api_*.hip).
#include "capi.h"

#ifndef RECON_FUSE_DEFAULT
#define RECON_FUSE_DEFAULT 15       // which square block sizes run paired by default: see recon_fuse_mask(), api_recon.hip
#endif
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <new>
#include <algorithm>
extern "C" void dav1d_hip_note_context_device(int device);

extern "C" {

// ------------------------------------------------------------------ context

// Objects alive right now, by kind (0 contexts, 1 frames, 2 listers, 3 host pictures): what a caller that must not leak — dav1d's frame
// contexts under error recovery, src/decode.c:3242-3251 — checks after it has closed everything (tests/test_stream_errors.py).
long long dav1d_hip_live[8];
int dav1d_hip_live_objects(long long out[4]) {
    if (!out) return -EINVAL;
    for (int i = 0; i < 4; i++) out[i] = __atomic_load_n(&dav1d_hip_live[i], __ATOMIC_RELAXED);
    return 0;
}

int dav1d_hip_open(Dav1dHipContext **out, int device, void *stream) {
    if (!out) return -EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return -ENODEV;
    if (hipSetDevice(device) != hipSuccess) return -ENODEV;
    Dav1dHipContext *c = new (std::nothrow) Dav1dHipContext();
    if (!c) return -ENOMEM;
    c->device = device;
    c->own_stream = stream == nullptr;
    dav1d_hip_note_context_device(device);
    c->scratch = nullptr;
    c->scratch_size = 0;
    if (stream) c->stream = (hipStream_t) stream;
    else if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return -ENODEV; }
    // the library holds gfx950 code only: any other device cannot run it
#ifndef DAV1D_HIP_EMU
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6)) { delete c; return -ENODEV; }
    }
#endif
    // tuning knobs: context state, the environment only supplies the defaults at open (dav1d_hip_set_option changes them later)
    auto env_int = [](const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; };
    c->recon_fuse = (int) env_int("DAV1D_HIP_RECON_FUSE", RECON_FUSE_DEFAULT);
    c->recon_pipeline = env_int("DAV1D_HIP_RECON_PIPELINE", 16384);
    c->recon_lanes = (int) env_int("DAV1D_HIP_RECON_LANES", 1);
    c->chunk_upload = (int) env_int("DAV1D_HIP_CHUNK_UPLOAD", 0);
    c->recon_coop_below = (int) env_int("DAV1D_HIP_RECON_COOP_BELOW", 4096);
    c->post_bands = (int) env_int("DAV1D_HIP_POST_BANDS", 0);
    c->colour_cells = (int) env_int("DAV1D_HIP_COLOUR_CELLS", 0);
    c->ref_twin = (int) env_int("DAV1D_HIP_REF_TWIN", 1);
    c->recon_pair_streams = (int) env_int("DAV1D_HIP_RECON_PAIR_STREAMS", 2);
    // (per-context lists "a,b,...": the i-th context opened in the process takes element i mod length)
    static std::atomic<int> n_opened{0};
    const int ctx_index = n_opened.fetch_add(1);
    auto env_list = [&](const char *name, long dflt) {
        const char *e = getenv(name);
        if (!e || !*e) return dflt;
        int n = 1;
        for (const char *q = e; *q; q++) n += *q == ',';
        int want = ctx_index % n;
        const char *q = e;
        while (want-- > 0) q = strchr(q, ',') + 1;
        return atol(q);
    };
    c->recon_pair_first = (int) std::max(1L, std::min(3L, env_list("DAV1D_HIP_RECON_PAIR_FIRST", 2)));
    // Which streams share a HARDWARE queue.  The runtime deals a process's streams over GPU_MAX_HW_QUEUES (4) hardware queues in the order they are
    // made, and a hardware queue runs its packets in order: a stream that waits for an event holds up every stream behind it in the same queue.  A
    // step's launches run on four streams of the context — main (4x4 pairs, 64-wide predictions, the join), side 0 (64x64 residuals), side 2 and 3 (the
    // paired launches).  With the side streams made straight behind the main stream, side 2 and 3 of the first context share ONE queue, and a second
    // context's side 2 joins them there while its side 3 sits behind its own main stream: three of the four streams that carry the long launches in one
    // queue (rocprofv3's Queue_Id per dispatch, profiles/r06/queue_map.txt).  One unused stream in front of the side streams shifts the dealing so that
    // each of those four has a queue to itself or shares it with a short stream: measured on the 8K step 0.274 -> 0.260 ms with one frame in flight,
    // 0.239 -> 0.229 with two, 4K 0.099 -> 0.088 with one (0.0735 -> 0.0765 with two; three 8K contexts 0.243 -> 0.259); more hardware queues (5 .. 16)
    // or fewer are all slower (profiles/r06/hw_queues.txt).
    c->n_pad_streams = (int) std::max(0L, std::min(8L, env_list("DAV1D_HIP_STREAM_PAD", 1)));
    for (int i = 0; i < c->n_pad_streams; i++)
        if (hipStreamCreateWithFlags(&c->pad_streams[i], hipStreamNonBlocking) != hipSuccess) { c->n_pad_streams = i; break; }
    const char *ser = getenv("DAV1D_HIP_SERIAL");
    c->concurrent = !(ser && atoi(ser));
    const char *cu = getenv("DAV1D_HIP_CDEF_UNIT");
    c->cdef_unit_kernel = cu && atoi(cu);
    c->cdef_full_copy = env_int("DAV1D_HIP_FILTER_FULL_COPY", 0) != 0;
    c->cdef_rows = env_int("DAV1D_HIP_CDEF_ROWS", 1) != 0;
    const char *fg = getenv("DAV1D_HIP_FLOW_GROUPS");
    c->flow_groups = fg && atoi(fg) > 0 ? atoi(fg) : 512;
    const char *fm = getenv("DAV1D_HIP_FLOW_MODE");
    c->flow_mode = fm ? atoi(fm) : 0;
    const char *fs = getenv("DAV1D_HIP_FLOW_MIN_STEPS");
    c->flow_min_steps = fs ? atoi(fs) : 200;
    const char *isb = getenv("DAV1D_HIP_INTRA_SB");
    c->intra_sb = isb ? atoi(isb) : 2;
    c->intra_sb_waves = (int) env_int("DAV1D_HIP_INTRA_SB_WAVES", 0);
    c->intra_sb_one_below = (int) env_int("DAV1D_HIP_INTRA_SB_ONE_BELOW", 0);
    c->intra_sb_fallbacks = 0;
    c->prep_async = (int) env_int("DAV1D_HIP_PREP_ASYNC", 1);
    c->intra_sb_lds = (int) env_int("DAV1D_HIP_INTRA_SB_LDS", 0);
    c->intra_sb_flow = (int) env_int("DAV1D_HIP_INTRA_SB_FLOW", 1);
    // (DAV1D_HIP_PAIR_PRIORITY=1, an experiment's knob: the streams of the paired launches are made with the device's highest stream priority — the
    // runtime keeps a pool of hardware queues per priority, so they are dealt over queues no other stream of the process is in.  Measured: 0.27 -
    // 0.49 ms per 8K step against 0.22 - 0.24, highest or lowest priority alike, profiles/r06/queue_search.txt — off)
    const long pair_prio = env_list("DAV1D_HIP_PAIR_PRIORITY", 0);
    int prio_least = 0, prio_greatest = 0;
#ifndef DAV1D_HIP_EMU
    if (pair_prio) (void) hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
#endif
    auto make_side = [&](const int i) {
#ifndef DAV1D_HIP_EMU
        if (pair_prio && i >= c->recon_pair_first && i < c->recon_pair_first + 3)
            return hipStreamCreateWithPriority(&c->side[i], hipStreamNonBlocking, pair_prio > 0 ? prio_greatest : prio_least);
#endif
        return hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking);
    };
    (void) prio_least; (void) prio_greatest;
    for (int i = 0; i < Dav1dHipContext::N_SIDE; i++) {
        if (make_side(i) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming) != hipSuccess) { delete c; return -ENODEV; }
        if (i < 3 && hipEventCreateWithFlags(&c->ev_pair[i], hipEventDisableTiming) != hipSuccess) { delete c; return -ENODEV; }
    }
    if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess) { delete c; return -ENODEV; }
    for (int i = 0; i < 16; i++)
        if (hipEventCreateWithFlags(&c->ev_bin[i], hipEventDisableTiming) != hipSuccess) { delete c; return -ENODEV; }
    if (hipEventCreate(&c->ev_t0) != hipSuccess || hipEventCreate(&c->ev_t1) != hipSuccess) { delete c; return -ENODEV; }
    if (hipEventCreateWithFlags(&c->ev_retile, hipEventDisableTiming) != hipSuccess) { delete c; return -ENODEV; }
    c->retile_pending = false;
    c->last_ms = 0.f;
    c->last_ms_pending = false;
    c->gather_dev = c->segtab_dev = c->pending_slab = nullptr;
    c->gather_cap = c->segtab_cap = c->pending_slab_cap = 0;
    c->arena_hint = 0;
    c->arena_min = (size_t) 1 << 24;
    c->chunk_order = (int) env_int("DAV1D_HIP_CHUNK_ORDER", 0);
    c->chunk_hints = (int) env_int("DAV1D_HIP_CHUNK_HINTS", 1);
    c->carena_hint = 0;
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_untile, hipEventDisableTiming) != hipSuccess) { delete c; return -ENODEV; }
    *out = c;
    __atomic_fetch_add(&dav1d_hip_live[0], 1, __ATOMIC_RELAXED);
    return 0;
}

void dav1d_hip_close(Dav1dHipContext *c) {
    if (!c) return;
    __atomic_fetch_sub(&dav1d_hip_live[0], 1, __ATOMIC_RELAXED);
    (void) hipSetDevice(c->device);
    // everything this context (or a frame, a grain handle, a peer of it) still has in flight on ANY of its streams is through before the
    // streams, events and pools go: the per-stream waits below do not cover streams that belong to objects the caller destroyed without
    // waiting (a GPU test run died once in here, at the session's end, after 249 green tests)
    (void) hipDeviceSynchronize();
    hipStreamSynchronize(c->stream);
    if (c->scratch) hipFree(c->scratch);
    for (int i = 0; i < c->n_pad_streams; i++) hipStreamDestroy(c->pad_streams[i]);
    for (int i = 0; i < Dav1dHipContext::N_SIDE; i++) { hipStreamSynchronize(c->side[i]); hipStreamDestroy(c->side[i]); hipEventDestroy(c->ev_join[i]); if (i < 3) hipEventDestroy(c->ev_pair[i]); }
    hipEventDestroy(c->ev_fork);
    for (int i = 0; i < 16; i++) hipEventDestroy(c->ev_bin[i]);
    hipEventDestroy(c->ev_t0); hipEventDestroy(c->ev_t1); hipEventDestroy(c->ev_retile);
    hipStreamSynchronize(c->copy_stream); hipStreamDestroy(c->copy_stream); hipEventDestroy(c->ev_copy); hipEventDestroy(c->ev_untile);
    if (c->band_cnt) (void) hipFree(c->band_cnt);
    if (c->band_flags) (void) hipHostFree(c->band_flags);
    for (const Dav1dHipContext::Arena &ar : c->free_arenas) hipFree(ar.dev);
    for (const Dav1dHipContext::Arena &ar : c->free_task_bufs) hipFree(ar.dev);
    for (Dav1dHipPicture &q : c->free_pictures) { if (q.alloc) hipFree(q.alloc); if (q.twin_alloc) hipFree(q.twin_alloc); }
    for (Dav1dHipContext::BatchStage &bs : c->batch_stage) {
        if (bs.made) hipEventDestroy(bs.done);
        if (bs.host) hipHostFree(bs.host);
        if (bs.dev) hipFree(bs.dev);
    }
    for (void *q : c->batch_retired_host) hipHostFree(q);
    for (void *q : c->batch_retired_dev) hipFree(q);
    if (c->reduce_scratch) hipFree(c->reduce_scratch);
    if (c->gather_dev) hipFree(c->gather_dev);
    if (c->segtab_dev) hipFree(c->segtab_dev);
    if (c->pending_slab) hipHostFree(c->pending_slab);
    for (const std::vector<Dav1dHipContext::Slab> &cls : c->free_slabs) for (const Dav1dHipContext::Slab &sl : cls) hipHostFree(sl.host);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
}

int dav1d_hip_sync(Dav1dHipContext *c) {
    if (c->retile_pending) { (void) hipEventSynchronize(c->ev_retile); c->retile_pending = false; }
    return hip_rc(hipStreamSynchronize(c->stream));
}
void *dav1d_hip_stream(Dav1dHipContext *c) { return (void *) c->stream; }

// ---- recorded launch sequences (hipGraph)
struct Dav1dHipGraph {
    hipGraph_t graph;
    hipGraphExec_t exec;
    size_t nodes;
};

int dav1d_hip_graph_begin(Dav1dHipContext *c) {
    if (!c) return -EINVAL;
    return hip_rc(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
}

int dav1d_hip_graph_end(Dav1dHipContext *c, Dav1dHipGraph **out) {
    if (!c || !out) return -EINVAL;
    *out = nullptr;
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamEndCapture(c->stream, &graph));
    if (!graph) return -EIO;
    Dav1dHipGraph *g = new (std::nothrow) Dav1dHipGraph();
    if (!g) { hipGraphDestroy(graph); return -ENOMEM; }
    g->graph = graph;
    g->nodes = 0;
    (void) hipGraphGetNodes(graph, nullptr, &g->nodes);
    const hipError_t e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { hipGraphDestroy(graph); delete g; return hip_rc(e); }
    *out = g;
    return 0;
}

int dav1d_hip_graph_launch(Dav1dHipContext *c, const Dav1dHipGraph *g) {
    if (!c || !g) return -EINVAL;
    return hip_rc(hipGraphLaunch(g->exec, c->stream));
}

size_t dav1d_hip_graph_nodes(const Dav1dHipGraph *g) { return g ? g->nodes : 0; }

void dav1d_hip_graph_destroy(Dav1dHipContext *c, Dav1dHipGraph *g) {
    if (!g) return;
    if (c) hipStreamSynchronize(c->stream);
    hipGraphExecDestroy(g->exec);
    hipGraphDestroy(g->graph);
    delete g;
}
int dav1d_hip_get_option(Dav1dHipContext *c, const char *name, long *value) {
    if (!c || !name || !value) return -EINVAL;
    if (!strcmp(name, "intra_sb_fallbacks")) *value = c->intra_sb_fallbacks;
    else if (!strcmp(name, "intra_sb_waves")) *value = c->intra_sb_waves;
    else if (!strcmp(name, "intra_sb_one_below")) *value = c->intra_sb_one_below;
    else if (!strcmp(name, "recon_fuse")) *value = c->recon_fuse;
    else if (!strcmp(name, "recon_pair_streams")) *value = c->recon_pair_streams;
    else if (!strcmp(name, "recon_pair_first")) *value = c->recon_pair_first;
    else if (!strcmp(name, "ref_twin")) *value = c->ref_twin;
    else return -EINVAL;
    return 0;
}
// knobs by name (the environment variables of DESIGN.md without the DAV1D_HIP_ prefix, lower case); -EINVAL for an unknown name
int dav1d_hip_set_option(Dav1dHipContext *c, const char *name, long value) {
    if (!c || !name) return -EINVAL;
    if (!strcmp(name, "recon_fuse")) c->recon_fuse = (int) value;
    else if (!strcmp(name, "recon_pipeline")) c->recon_pipeline = value;
    else if (!strcmp(name, "recon_lanes")) c->recon_lanes = (int) value;
    else if (!strcmp(name, "chunk_upload")) c->chunk_upload = (int) value;
    else if (!strcmp(name, "recon_coop_below")) c->recon_coop_below = (int) value;
    else if (!strcmp(name, "post_bands")) c->post_bands = (int) value;
    else if (!strcmp(name, "colour_cells")) c->colour_cells = value < 0 ? 0 : value > 64 ? 64 : (int) value;
    else if (!strcmp(name, "ref_twin")) c->ref_twin = (int) value;
    else if (!strcmp(name, "recon_pair_streams")) c->recon_pair_streams = (int) value;
    else if (!strcmp(name, "recon_pair_first")) c->recon_pair_first = (int) std::max(1L, std::min(3L, (long) value));
    else if (!strcmp(name, "serial")) c->concurrent = !value;
    else if (!strcmp(name, "cdef_unit")) c->cdef_unit_kernel = value != 0;
    else if (!strcmp(name, "filter_full_copy")) c->cdef_full_copy = value != 0;
    else if (!strcmp(name, "cdef_rows")) c->cdef_rows = value != 0;
    else if (!strcmp(name, "flow_groups")) c->flow_groups = value > 0 ? (int) value : c->flow_groups;
    else if (!strcmp(name, "flow_mode")) c->flow_mode = (int) value;
    else if (!strcmp(name, "flow_min_steps")) c->flow_min_steps = (int) value;
    else if (!strcmp(name, "intra_sb")) c->intra_sb = (int) value;
    else if (!strcmp(name, "intra_sb_waves")) c->intra_sb_waves = value >= 8 ? 8 : value >= 4 ? 4 : value == 1 ? 1 : 0;
    else if (!strcmp(name, "intra_sb_one_below")) c->intra_sb_one_below = value > 0 ? (int) value : 0;
    else if (!strcmp(name, "intra_sb_lds")) c->intra_sb_lds = value != 0;
    else if (!strcmp(name, "intra_sb_flow")) c->intra_sb_flow = value != 0;
    else if (!strcmp(name, "intra_sb_fine")) dav1d_hip_sbw_set_fine(value != 0);
    else if (!strcmp(name, "intra_sb_fail_at")) dav1d_hip_sbw_set_fail_at((int) value);
    else if (!strcmp(name, "prep_async")) c->prep_async = value < 0 ? 0 : value > 2 ? 2 : (int) value;
    else if (!strcmp(name, "chunk_order")) c->chunk_order = value != 0;
    else if (!strcmp(name, "chunk_hints")) c->chunk_hints = value != 0;
    else if (!strcmp(name, "chunk_arena_min")) { if (value < 4096) return -EINVAL; c->arena_min = (size_t) 1 << 12; while (c->arena_min < (size_t) value) c->arena_min <<= 1; c->arena_hint = 0; }
    else return -EINVAL;
    return 0;
}

const char *dav1d_hip_version(void) { return "dav1d_hip 0.1 (gfx950)"; }
float dav1d_hip_last_kernel_ms(Dav1dHipContext *c) {
    if (!c) return 0.f;
    if (c->last_ms_pending) {           // the call that recorded the events did not wait for them (dav1d_hip_surface_export)
        c->last_ms_pending = false;
        c->last_ms = 0.f;
        if (hipEventSynchronize(c->ev_t1) == hipSuccess) (void) hipEventElapsedTime(&c->last_ms, c->ev_t0, c->ev_t1);
    }
    return c->last_ms;
}

int dav1d_hip_malloc(Dav1dHipContext *c, void **dev, size_t bytes) {
    (void) c;
    return hip_rc(hipMalloc(dev, bytes ? bytes : 1));
}
int dav1d_hip_free(Dav1dHipContext *c, void *dev) {
    hipStreamSynchronize(c->stream);
    return hip_rc(hipFree(dev));
}
int dav1d_hip_memset(Dav1dHipContext *c, void *dev, int v, size_t bytes) {
    return hip_rc(hipMemsetAsync(dev, v, bytes, c->stream));
}
thread_local int dav1d_hip_tls_last_error = 0;
const char *dav1d_hip_last_hip_error(int *code) {
    const int e = dav1d_hip_tls_last_error;
    if (code) *code = e;
    return e ? hipGetErrorString((hipError_t) e) : "no error";
}

int dav1d_hip_upload(Dav1dHipContext *c, void *dev, const void *host, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return hip_rc(hipStreamSynchronize(c->stream));
}
int dav1d_hip_download(Dav1dHipContext *c, void *host, const void *dev, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    return hip_rc(hipStreamSynchronize(c->stream));
}

// ---- more than one device in a process (dav1d is ONE process with n_fc frame contexts: the binding ends frame context k's frames on device
// k mod N, dav1d_amd/host/dav1d_glue.c).  The current device is a property of the calling THREAD in HIP: a thread that serves contexts of
// several devices says which one it means before it calls in.
int dav1d_hip_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : -ENODEV;
}
int dav1d_hip_context_device(const Dav1dHipContext *c) { return c ? c->device : -EINVAL; }
int dav1d_hip_context_use(Dav1dHipContext *c) {
    if (!c) return -EINVAL;
    return hipSetDevice(c->device) == hipSuccess ? 0 : -ENODEV;
}
// direct copies between the devices of two contexts (xGMI): without it hipMemcpyPeerAsync goes through host memory.  Both directions; a pair
// that is enabled already or cannot be peers is not an error (the copy still works, staged).  Leaves the caller's device current.
int dav1d_hip_enable_peer_access(Dav1dHipContext *a, Dav1dHipContext *b) {
    if (!a || !b) return -EINVAL;
    if (a->device == b->device) return 0;
    int prev = 0, enabled = 0;
    (void) hipGetDevice(&prev);
    const int dev[2] = { a->device, b->device };
    for (int k = 0; k < 2; k++) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dev[k], dev[k ^ 1]) != hipSuccess || !can) continue;
        if (hipSetDevice(dev[k]) != hipSuccess) continue;
        const hipError_t e = hipDeviceEnablePeerAccess(dev[k ^ 1], 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) enabled++;
    }
    (void) hipGetLastError();
    (void) hipSetDevice(prev);
    return enabled;         // 0, 1 or 2 directions
}
// for callers that borrow a thread (an allocator callback on the application's thread): what the thread had, and back to it
int dav1d_hip_current_device(void) {
    int d = 0;
    return hipGetDevice(&d) == hipSuccess ? d : -ENODEV;
}
int dav1d_hip_set_device(int device) { return hipSetDevice(device) == hipSuccess ? 0 : -ENODEV; }
// the device a picture's planes live on (-EINVAL: not device memory the runtime knows)
int dav1d_hip_picture_device(const Dav1dHipPicture *pic) {
    if (!pic) return -EINVAL;
    const void *p = pic->twin_ok == DAV1D_HIP_TWIN_ONLY && pic->twin[0] ? pic->twin[0] : pic->p[0].data;
    hipPointerAttribute_t a;
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice) { (void) hipGetLastError(); return -EINVAL; }
    return a.device;
}
// with more than one device: are these pictures where context c can launch on them?  (-EXDEV names the first that is not)
// (asked only when this process has opened contexts on more than one device: the question is a trip to the driver per picture, on the
// frame's critical path, and a process that uses one of a node's eight GPUs cannot have got a picture from another)
static std::atomic<uint64_t> g_ctx_devices{0};
void dav1d_hip_note_context_device(int device) { if (device >= 0 && device < 64) g_ctx_devices.fetch_or(1ull << device); }
int pictures_on_device(const Dav1dHipContext *c, const Dav1dHipPicture *pics, int n) {
    const uint64_t m = g_ctx_devices.load(std::memory_order_relaxed);
    if (!(m & (m - 1))) return 0;
    for (int i = 0; i < n; i++) {
        if (!pics[i].p[0].data) continue;
        const int d = dav1d_hip_picture_device(&pics[i]);
        if (d >= 0 && d != c->device) return -EXDEV;
    }
    return 0;
}

} // extern "C"

int dav1d_hip_scratch(Dav1dHipContext *c, size_t bytes, void **out) {
    if (c->scratch_size < bytes) {
        hipStreamSynchronize(c->stream);
        if (c->scratch) hipFree(c->scratch);
        c->scratch = nullptr;
        c->scratch_size = 0;
        size_t sz = bytes < (1u << 20) ? (1u << 20) : bytes;
        HIP_TRY(hipMalloc(&c->scratch, sz));
        c->scratch_size = sz;
    }
    *out = c->scratch;
    return 0;
}

Dav1dHipContext *dav1d_hip_default_context(void) {
    static std::mutex mtx;
    static Dav1dHipContext *g = nullptr;
    std::lock_guard<std::mutex> lk(mtx);
    if (!g) {
        const char *e = getenv("DAV1D_HIP_DEVICE");
        if (dav1d_hip_open(&g, e ? atoi(e) : 0, nullptr)) g = nullptr;
    }
    return g;
}
