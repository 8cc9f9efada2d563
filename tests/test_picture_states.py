"""Every entry point that reads or writes a picture, with the picture in each of the three states it can be in.

Dav1dHipPicture.twin_ok (include/dav1d_hip.h): 0 = the raster planes are the picture, 1 = raster planes and the 8x8-tiled twin agree,
DAV1D_HIP_TWIN_ONLY = the picture lives in its twin and the raster planes are stale — what dav1d_hip_recon_list_run_tiled and a frame under
context option ref_twin = 3 leave.  A reader of raster planes that forgets to un-tile such a picture fails no call: it returns plausible
pixels.  So the "twin-only" state here has 0x5A in every byte of the raster allocation (util.forget_raster), and every expectation comes
from the oracle through the family tests' own case builders: the family test runs as it is, on a context whose reader calls put their
source pictures into the state under test first (StateCtx).  All comparisons are exact.

  1. readers: cdef_batch (strip and unit kernels), lr_batch (src and lpf apart), resize, mc_scaled_batch, warp_batch, fg_apply /
     fg_apply_prepared (the four grain sets of test_filmgrain), motion compensation through mc / inter / recon lists with all references
     twin-only, a twin-only next to a raster-only one (ref_planes falls back to raster and un-tiles), and all twin-only under ref_twin = 0
  2. the re-tile and un-tile passes: 8 / 10 / 12 bits x four layouts x six sizes, library-allocated and caller-wrapped pictures; the banded
     un-tile behind dav1d_hip_host_picture_fetch
  3. copies between devices (the emulator's two)
  4. writers handed a twin-only `dst`: -EINVAL, nothing touched (WRITERS is the table to extend)

Not covered: the broadcast and all-gather paths of dav1d_amd/csrc/peer.hip, which un-tile first — they need the launcher of
tests/test_dist.py."""
import ctypes as C
import errno

import numpy as np
import pytest

import util
import synth_frames as synth
import test_cdef
import test_filmgrain
import test_frame
import test_lr
import test_mcx
from dav1d_amd import api
from util import STATES, forget_raster, make_source, put_in_state, twin_bytes

FLAG = {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}
LAYOUTS = [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444]
LAYOUT_IDS = ["i400", "i420", "i422", "i444"]
SIZES = [(190, 102), (64, 64), (333, 77), (7, 5), (8, 8), (129, 130)]


# ------------------------------------------------------------------------------------------------ 1. readers

class StateCtx:
    """A context as the family tests take it.  Each call that reads pictures first puts them into the states under test (`single`: state of
    a picture handed over by pointer, by argument name; `refs`: state of reference i), calls the library, and checks what the call may
    not change: the twin's bytes, and twin_ok — 1 after a guarded reader was given a twin-only record by pointer, the value it had
    otherwise (reference arrays are copies made by dav1d_amd/api.py: the pictures' own records keep their value)."""

    def __init__(self, ctx, single=None, refs=None):
        self._ctx, self._single, self._refs = ctx, single or {}, refs or (lambda i: "raster")
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def _read(self, call, single=(), refs=()):
        ctx = self._ctx
        watched = []
        for name, pic in single:
            put_in_state(ctx, pic, self._single.get(name, "raster"))
            watched.append((pic, FLAG[self._single.get(name, "raster")] and 1))
        for i, pic in enumerate(refs):
            put_in_state(ctx, pic, self._refs(i))
            watched.append((pic, FLAG[self._refs(i)]))
        before = [twin_bytes(ctx, pic) if pic.pic.twin_alloc else None for pic, _ in watched]
        call()
        self.calls += 1
        for (pic, flag), b in zip(watched, before):
            assert pic.pic.twin_ok == flag, "twin_ok is %d after the call, expected %d" % (pic.pic.twin_ok, flag)
            if b is not None:
                assert np.array_equal(twin_bytes(ctx, pic), b), "the call changed the tiled twin of a picture it reads"

    def cdef_batch(self, dst, src, *a):
        self._read(lambda: self._ctx.cdef_batch(dst, src, *a), single=[("src", src)])

    def lr_batch(self, dst, src, lpf, tasks):
        self._read(lambda: self._ctx.lr_batch(dst, src, lpf, tasks), single=[("src", src), ("lpf", lpf)])

    def resize(self, dst, src, *a):
        self._read(lambda: self._ctx.resize(dst, src, *a), single=[("src", src)])

    def fg_apply(self, dst, src, *a):
        self._read(lambda: self._ctx.fg_apply(dst, src, *a), single=[("src", src)])

    def fg_apply_prepared(self, dst, src, *a):
        self._read(lambda: self._ctx.fg_apply_prepared(dst, src, *a), single=[("src", src)])

    def warp_batch(self, dst, refs, *a):
        self._read(lambda: self._ctx.warp_batch(dst, refs, *a), refs=refs)

    def mc_scaled_batch(self, dst, refs, *a):
        self._read(lambda: self._ctx.mc_scaled_batch(dst, refs, *a), refs=refs)

    def mc_batch(self, dst, refs, *a):
        self._read(lambda: self._ctx.mc_batch(dst, refs, *a), refs=refs)

    def run_inter_list(self, lst, dst, refs, *a):
        self._read(lambda: self._ctx.run_inter_list(lst, dst, refs, *a), refs=refs)

    def recon_list(self, *a):
        outer, rl = self, self._ctx.recon_list(*a)

        class Run:
            def run(self, dst, refs, *b):
                outer._read(lambda: rl.run(dst, refs, *b), refs=refs)

            def destroy(self):
                rl.destroy()
        return Run()


def need_ref():
    if util.ref_lib() is None:
        pytest.skip("needs the reference build")


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kernel", ["strips", "units"])
@pytest.mark.parametrize("bpc,layout", [(8, api.LAYOUT_I420), (10, api.LAYOUT_I444), (10, api.LAYOUT_I422)], ids=["8bit-420", "10bit-444", "10bit-422"])
def test_cdef_reads_its_source_in_every_state(ctx, bpc, layout, kernel, state):
    sc = StateCtx(ctx, single={"src": state})
    ctx.set_option("cdef_unit", kernel == "units")
    try:
        test_cdef.test_cdef_units_match_reference(sc, bpc, layout)
    finally:
        ctx.set_option("cdef_unit", 0)
    assert sc.calls == 1


LR_STATES = [("raster", "raster"), ("retiled", "raster"), ("twin-only", "raster"), ("raster", "retiled"), ("raster", "twin-only"),
             ("twin-only", "twin-only")]


@pytest.mark.parametrize("src_state,lpf_state", LR_STATES, ids=["src-%s-lpf-%s" % s for s in LR_STATES])
@pytest.mark.parametrize("filt", ["wiener-10bit", "sgr-8bit"])
def test_restoration_reads_its_source_and_its_row_store_in_every_state(ctx, filt, src_state, lpf_state):
    sc = StateCtx(ctx, single={"src": src_state, "lpf": lpf_state})
    if filt.startswith("wiener"):
        test_lr.test_wiener_matches_reference(sc, 10)
    else:
        test_lr.test_sgr_matches_reference(sc, 8)
    assert sc.calls == 1


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("bpc", [8, 10])
def test_resize_reads_its_source_in_every_state(ctx, bpc, state):
    need_ref()
    sc = StateCtx(ctx, single={"src": state})
    test_mcx.test_resize_matches_reference(sc, bpc)
    assert sc.calls == 4


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("bpc,kind", [(8, 0), (10, 1)], ids=["8bit-put", "10bit-prep"])
def test_scaled_prediction_reads_its_reference_in_every_state(ctx, bpc, kind, state):
    need_ref()
    sc = StateCtx(ctx, refs=lambda i: state)
    test_mcx.test_mc_scaled_matches_reference(sc, bpc, kind)
    assert sc.calls == 1


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("bpc", [8, 10])
def test_warped_prediction_reads_its_reference_in_every_state(ctx, bpc, state):
    need_ref()
    sc = StateCtx(ctx, refs=lambda i: state)
    test_mcx.test_warp_matches_reference(sc, bpc)
    assert sc.calls == 1


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["all-planes", "chroma-from-luma", "v-copied", "luma-copied"])
@pytest.mark.parametrize("bpc", [8, 10])
def test_film_grain_reads_its_source_in_every_state(ctx, bpc, variant, state):
    """dav1d_hip_fg_apply and dav1d_hip_fg_apply_prepared (the family test runs both): the planes that get no grain are copies of the
    source's, taken from where the picture lives.
    (Before the un-tile moved above the plane copies in fg_apply_core, the twin-only cases of "v-copied" and "luma-copied" returned
    0x5A5A / 0x5A in the copied plane.)"""
    sc = StateCtx(ctx, single={"src": state})
    test_filmgrain.test_film_grain_matches_reference(sc, bpc, variant)
    assert sc.calls == 2


REF_CONFIGS = {
    "all-raster": (lambda i: "raster", 1),
    "all-retiled": (lambda i: "retiled", 1),
    "all-twin-only": (lambda i: "twin-only", 1),
    "twin-only-next-to-raster": (lambda i: "raster" if i == 1 else "twin-only", 1),
    "all-twin-only-ref_twin-0": (lambda i: "twin-only", 0),
}


@pytest.mark.parametrize("config", list(REF_CONFIGS))
@pytest.mark.parametrize("route", ["mc-batch", "inter-list", "recon-list"])
def test_motion_compensation_reads_its_references_in_every_state(ctx, route, config):
    """mc_batch + comp_batch, the fused inter list and the recon list of test_frame.hip_frame against the oracle's replay; with one
    raster-only reference among twin-only ones, and with ref_twin = 0, ref_planes() takes the raster kernels and has to un-tile."""
    states, ref_twin = REF_CONFIGS[config]
    w, h, bpc = 256, 128, 10
    frame = synth.make_frame(w, h, bpc, seed=2024, edge_frac=0.1)
    assert frame.n_refs >= 2
    rng = np.random.default_rng(2025)
    refs = [synth.make_planes(rng, w, h, bpc) for _ in range(frame.n_refs)]
    dst0 = synth.make_planes(rng, w, h, bpc, smooth=False)
    want, want_prep, want_coef = test_frame.oracle_frame(util.default_oracle(), frame, dst0, refs)
    sc = StateCtx(ctx, refs=states)
    ctx.set_option("ref_twin", ref_twin)
    try:
        got, got_prep, got_coef = test_frame.hip_frame(sc, frame, dst0, refs, fused=route == "inter-list", recon=route == "recon-list")
    finally:
        ctx.set_option("ref_twin", 1)
    assert sc.calls == 1
    for pl in range(3):
        bad = np.argwhere(got[pl] != want[pl])
        assert not len(bad), "plane %d differs at %s (%d px)" % (pl, bad[0], len(bad))
    if route == "mc-batch":
        assert np.array_equal(got_prep, want_prep)
    assert np.array_equal(got_coef, want_coef)


@pytest.mark.parametrize("state", STATES)
def test_the_ways_out_leave_the_record_as_it_was(ctx, state):
    """export, plane download and host fetch take a const picture: twin_ok keeps its value in all three states (include/dav1d_hip.h)"""
    w, h, bpc, layout = 190, 102, 10, api.LAYOUT_I420
    pic, vis = make_source(ctx, np.random.default_rng(8100), w, h, layout, bpc, state)
    host = api.HostPictureBuf(ctx, w, h, layout, bpc)
    s = ctx.surface(w, h, layout, bpc, api.SURFACE_PLANAR, api.SAMPLE_NATIVE)
    try:
        twin = twin_bytes(ctx, pic) if state != "raster" else None
        pic.export(s)
        assert pic.pic.twin_ok == FLAG[state]
        got = s.download()
        host.fetch(pic.pic, 0, h)
        host.wait()
        assert pic.pic.twin_ok == FLAG[state]
        for pl in range(3):
            assert np.array_equal(got[pl], vis[pl]), ("export", pl)
            assert np.array_equal(host.plane(pl)[:vis[pl].shape[0], :vis[pl].shape[1]], vis[pl]), ("fetch", pl)
            assert np.array_equal(pic.download(pl)[:vis[pl].shape[0], :vis[pl].shape[1]], vis[pl]), ("download", pl)
            assert pic.pic.twin_ok == FLAG[state]
        if twin is not None:
            assert np.array_equal(twin_bytes(ctx, pic), twin)
    finally:
        host.release()
        s.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 2. the re-tile and un-tile passes

def raw_planes(ctx, pic, rows):
    """every byte of every plane as the device holds it: rows[pl] x stride"""
    ctx.sync()
    out = []
    for pl in range(3):
        if not pic.p[pl].data:
            continue
        a = np.zeros(rows[pl] * pic.p[pl].stride, np.uint8)
        assert ctx.lib.dav1d_hip_download(ctx.h, a.ctypes.data, pic.p[pl].data, a.nbytes) == 0
        out.append(a)
    return out


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_retile_then_untile_gives_every_byte_back_library_pictures(ctx, bpc, layout):
    """pictures of dav1d_hip_picture_alloc: the allocator's padding rows and the stride's padding columns travel with the picture"""
    for w, h in SIZES:
        rng = np.random.default_rng(8200 + 100 * bpc + 10 * layout + w)
        pic = ctx.picture(w, h, layout, bpc)
        try:
            for pl, p in enumerate(util.random_planes(rng, pic)):
                pic.upload(pl, p)
            rows = [pic.padded_shape(pl)[0] for pl in range(pic.n_planes)]
            want = raw_planes(ctx, pic.pic, rows)
            pic.retile()
            assert pic.pic.twin_ok == 1
            twin = twin_bytes(ctx, pic)
            forget_raster(ctx, pic)
            assert all((a == 0x5A).all() for a in raw_planes(ctx, pic.pic, rows))
            pic.untile()
            assert pic.pic.twin_ok == 1
            got = raw_planes(ctx, pic.pic, rows)
            for pl in range(pic.n_planes):
                bad = np.flatnonzero(got[pl] != want[pl])
                assert not len(bad), "%dx%d plane %d: %d bytes did not come back, first at %d" % (w, h, pl, len(bad), bad[0])
            assert np.array_equal(twin_bytes(ctx, pic), twin), "un-tiling changed the twin"
        finally:
            pic.free()


def wrapped_picture(ctx, rng, w, h, layout, bpc, stride_px_extra=0):
    """a picture in memory of the caller's: the visible rows and nothing below them, 0xA5 behind the last row of each plane"""
    bps = 1 if bpc == 8 else 2
    dt = np.uint8 if bpc == 8 else np.uint16
    pic = api.Picture()
    pic.bpc, pic.layout = bpc, layout
    bufs, planes = [], []
    for pl in range(1 if layout == api.LAYOUT_I400 else 3):
        ss_h = 1 if pl and layout != api.LAYOUT_I444 else 0
        ss_v = 1 if pl and layout == api.LAYOUT_I420 else 0
        pw, ph = (w + ss_h) >> ss_h, (h + ss_v) >> ss_v
        align = 16 // bps          # a stride the tiles fit: a multiple of 8 pixels and of 16 bytes
        stride_px = ((pw + align - 1) & ~(align - 1)) + stride_px_extra
        a = rng.integers(0, 1 << bpc, size=(ph, stride_px)).astype(dt)
        b = ctx.buffer(a.nbytes + 256)
        assert ctx.lib.dav1d_hip_memset(ctx.h, b.ptr, 0xA5, b.nbytes) == 0
        b.upload(a)
        pic.p[pl].data, pic.p[pl].stride, pic.p[pl].w, pic.p[pl].h = b.ptr, stride_px * bps, pw, ph
        bufs.append(b)
        planes.append(a)
    return pic, bufs, planes


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_retile_then_untile_gives_every_byte_back_wrapped_pictures(ctx, bpc, layout):
    """a caller-wrapped picture promises its visible rows only: the passes neither read nor write below them"""
    for w, h in SIZES:
        rng = np.random.default_rng(8300 + 100 * bpc + 10 * layout + w)
        pic, bufs, planes = wrapped_picture(ctx, rng, w, h, layout, bpc, stride_px_extra=16 if bpc != 10 else 0)
        try:
            assert ctx.lib.dav1d_hip_picture_retile(ctx.h, C.byref(pic)) == 0
            assert pic.twin_ok == 1 and pic.twin_alloc and not pic.alloc
            for b in bufs:
                assert ctx.lib.dav1d_hip_memset(ctx.h, b.ptr, 0x5A, b.nbytes - 256) == 0
            pic.twin_ok = api.TWIN_ONLY
            assert ctx.lib.dav1d_hip_picture_untile(ctx.h, C.byref(pic)) == 0
            assert pic.twin_ok == 1
            ctx.sync()
            for pl, (b, a) in enumerate(zip(bufs, planes)):
                got = b.download(np.uint8)
                want = np.concatenate([a.view(np.uint8).ravel(), np.full(256, 0xA5, np.uint8)])
                bad = np.flatnonzero(got != want)
                assert not len(bad), "%dx%d plane %d: %d bytes differ, first at %d of %d" % (w, h, pl, len(bad), bad[0], a.nbytes)
        finally:
            ctx.lib.dav1d_hip_picture_free(ctx.h, C.byref(pic))
            for b in bufs:
                b.free()


@pytest.mark.parametrize("bpc,extra", [(8, 4), (8, 8), (10, 4), (10, 12)], ids=["8bit-4px", "8bit-8px", "10bit-4px", "10bit-12px"])
def test_twin_storage_is_refused_for_a_stride_the_tiles_do_not_fit(ctx, bpc, extra):
    """dav1d_hip_picture_twin_alloc: a stride has to be a multiple of 8 pixels and of 16 bytes"""
    pic, bufs, _ = wrapped_picture(ctx, np.random.default_rng(8400), 64, 16, api.LAYOUT_I400, bpc, stride_px_extra=extra)
    try:
        assert ctx.lib.dav1d_hip_picture_twin_alloc(ctx.h, C.byref(pic)) == -errno.EINVAL
        assert not pic.twin_alloc and not pic.twin[0]
        assert ctx.lib.dav1d_hip_picture_retile(ctx.h, C.byref(pic)) == -errno.EINVAL
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("layout", [api.LAYOUT_I420, api.LAYOUT_I444, api.LAYOUT_I400], ids=["i420", "i444", "i400"])
@pytest.mark.parametrize("bpc", [8, 10])
def test_a_banded_fetch_untiles_its_own_rows_and_no_others(ctx, bpc, layout):
    """dav1d_hip_host_picture_fetch of a twin-only picture in bands whose edges are no multiples of 8 (even, as a 4:2:0 band has to be): the
    host gets the uploaded rows, and the raster planes — the staging — hold the rows of the bands fetched so far and 0x5A everywhere else"""
    w, h = 190, 102
    pic, vis = make_source(ctx, np.random.default_rng(8500 + bpc + layout), w, h, layout, bpc, "twin-only")
    host = api.HostPictureBuf(ctx, w, h, layout, bpc)
    bps = 1 if bpc == 8 else 2
    try:
        rows = [pic.padded_shape(pl)[0] for pl in range(pic.n_planes)]
        ss_v = 1 if layout == api.LAYOUT_I420 else 0
        done = [np.zeros(r, bool) for r in rows]
        for r0, r1 in ((2, 56), (0, 2), (56, h)):
            host.fetch(pic.pic, r0, r1)
            host.wait()
            assert pic.pic.twin_ok == api.TWIN_ONLY
            raw = raw_planes(ctx, pic.pic, rows)
            for pl in range(pic.n_planes):
                sv = ss_v if pl else 0
                c0, c1 = r0 >> sv, (vis[pl].shape[0] if r1 >= h else r1 >> sv)
                done[pl][c0:c1] = True
                stride = pic.pic.p[pl].stride
                body = raw[pl].reshape(rows[pl], stride)
                vw = vis[pl].shape[1] * bps
                assert np.array_equal(body[c0:c1, :vw], np.ascontiguousarray(vis[pl][c0:c1]).view(np.uint8).reshape(c1 - c0, vw)), ("staged rows", pl, r0, r1)
                stale = body[~done[pl]]
                assert (stale == 0x5A).all(), "band [%d, %d) plane %d: %d raster bytes outside the bands fetched so far were written" % (
                    r0, r1, pl, int((stale != 0x5A).sum()))
        for pl in range(pic.n_planes):
            assert np.array_equal(host.plane(pl)[:vis[pl].shape[0], :vis[pl].shape[1]], vis[pl]), ("fetched", pl)
    finally:
        host.release()
        pic.free()


# ------------------------------------------------------------------------------------------------ 3. copies between devices

def test_copies_between_devices_of_a_picture_that_lives_in_its_twin():
    """dav1d_hip_picture_copy_peer: twin-only source -> a picture with twin storage becomes twin-only with the same pixels, its raster planes
    untouched; -> a picture without twin storage is refused; dav1d_hip_picture_copy_peer_rows (raster rows) refuses such a source."""
    ctx = util.make_context("emu")
    lib = ctx.lib
    assert lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    w, h, bpc, layout = 200, 120, 10, api.LAYOUT_I420
    try:
        assert lib.dav1d_hip_context_use(ctx.h) == 0
        a, vis = make_source(ctx, np.random.default_rng(8600), w, h, layout, bpc, "twin-only")
        assert lib.dav1d_hip_context_use(other.h) == 0
        b, bare = other.picture(w, h, layout, bpc), other.picture(w, h, layout, bpc)
        assert lib.dav1d_hip_picture_twin_alloc(other.h, C.byref(b.pic)) == 0
        for p in (b, bare):
            assert lib.dav1d_hip_memset(other.h, p.pic.alloc, 0x3C, p.pic.alloc_size) == 0
        other.sync()

        def raster(p):
            out = np.zeros(p.pic.alloc_size, np.uint8)
            other.sync()
            assert lib.dav1d_hip_download(other.h, out.ctypes.data, p.pic.alloc, out.nbytes) == 0
            return out
        # no twin storage at the destination: refused, nothing copied
        assert lib.dav1d_hip_picture_copy_peer(other.h, C.byref(bare.pic), ctx.h, C.byref(a.pic)) == -errno.EINVAL
        assert bare.pic.twin_ok == 0 and (raster(bare) == 0x3C).all()
        # rows of raster planes: a twin-only source has none
        for dst in (b, bare):
            assert lib.dav1d_hip_picture_copy_peer_rows(other.h, C.byref(dst.pic), ctx.h, C.byref(a.pic), 0, h) == -errno.EINVAL
            assert (raster(dst) == 0x3C).all() and dst.pic.twin_ok == 0
        assert lib.dav1d_hip_picture_copy_peer(other.h, C.byref(b.pic), ctx.h, C.byref(a.pic)) == 0
        other.sync()
        assert b.pic.twin_ok == api.TWIN_ONLY and a.pic.twin_ok == api.TWIN_ONLY
        assert (raster(b) == 0x3C).all(), "the raster planes of the destination were written"
        assert lib.dav1d_hip_context_use(ctx.h) == 0
        ta = twin_bytes(ctx, a)
        assert lib.dav1d_hip_context_use(other.h) == 0
        assert np.array_equal(twin_bytes(other, b), ta)
        for pl in range(3):
            assert np.array_equal(b.download(pl)[:vis[pl].shape[0], :vis[pl].shape[1]], vis[pl]), pl
        b.free(); bare.free()
        assert lib.dav1d_hip_context_use(ctx.h) == 0
        a.free()
    finally:
        lib.dav1d_hip_context_use(ctx.h)
        other.close()
        lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 4. writers handed a twin-only dst

class Writers:
    """What the entries of WRITERS call with: the lists of a small inter frame, its in-loop filter tasks and an intra pass over it
    (tests/synth_frames.py), one warped and one scaled block, a set of grain parameters, sources and scratch.  Every entry has real tasks
    that write inside the picture, so that a call which is not refused shows in dst."""

    def __init__(self, ctx, w, h, bpc):
        self.ctx, self.w, self.h, self.bpc = ctx, w, h, bpc
        self.frame = synth.make_frame(w, h, bpc, seed=8700, edge_frac=0.1)
        rng = np.random.default_rng(8701)
        self.src, _ = make_source(ctx, rng, w, h, api.LAYOUT_I420, bpc, "raster")
        self.refs = [make_source(ctx, rng, w, h, api.LAYOUT_I420, bpc, "raster")[0] for _ in range(self.frame.n_refs)]
        self.ref_arr = (api.Picture * len(self.refs))(*[r.pic for r in self.refs])
        self.prep = ctx.buffer(max(self.frame.prep_elems, 64) * 2)
        self.coef = ctx.buffer_from(self.frame.coef)
        self.post = synth.make_post_filters(self.frame, seed=8702)
        self.lvl = ctx.buffer_from(self.post.lvl)
        self.lut_e, self.lut_i = (np.ascontiguousarray(a, dtype=np.uint8) for a in (self.post.lut_e, self.post.lut_i))
        self.lf, self.cdef, self.lr = (np.ascontiguousarray(a) for a in (self.post.lf, self.post.cdef, self.post.lr))
        assert len(self.lf) and len(self.cdef) and len(self.lr)
        self.ip = synth.make_intra_pass(self.frame, seed=8703)
        self.first_wave = np.ascontiguousarray(self.ip.batches[0][0], dtype=api.IPRED_TASK)
        assert len(self.first_wave) and sum(len(b[1]) for b in self.ip.batches)
        self.icoef = ctx.buffer_from(self.ip.coef)
        self.warp = np.zeros(1, api.WARP_TASK)
        self.warp[0] = (0, 16, 16, 0, 0, (0, 0, 0, 0), 64, 0, 0, 0, (0, 0, 0))          # one 8x8 block, PUT, at the picture's origin
        self.scaled = np.zeros(1, api.MC_SCALED_TASK)
        self.scaled[0] = (0, 16, 16, 0, 0, 1024, 1024, 8, 8, 0, 0, 0, 0, (0, 0))        # one 8x8 block, PUT, step 1:1
        self.ms, self.counts = (C.c_float * 40)(), (C.c_size_t * 40)()
        self.grain = test_filmgrain.random_fg(rng, bpc, 0)
        self.prepared = ctx.fg_prepare(self.grain, bpc, api.LAYOUT_I420)
        f = self.frame
        self.itx, self.mc, self.comp = ctx.itx_list(f.itx), ctx.mc_list(f.mc), ctx.comp_list(f.comp)
        self.inter = ctx.inter_list(f.mc, f.comp)
        self.recon = ctx.recon_list(self.src, f.mc, f.comp, f.itx)
        self.ipred = ctx.ipred_list([b[0] for b in self.ip.batches])
        self.intra = ctx.intra_list(self.ip.batches)
        self.flow = ctx.intra_flow(self.ip.batches)
        self.sb = ctx.intra_sb(self.ip.batches, self.src)

    def fresh_coefficients(self):
        """(the residual launches zero what they consume)"""
        self.coef.upload(self.frame.coef)
        self.icoef.upload(self.ip.coef)

    def free(self):
        self.ctx.fg_grain_destroy(self.prepared)
        for o in (self.itx, self.mc, self.comp, self.inter, self.recon, self.ipred, self.intra, self.flow, self.sb):
            o.destroy()
        for o in [self.src, self.prep, self.coef, self.icoef, self.lvl] + self.refs:
            o.free()


def _ptr(a):
    return a.ctypes.data


# name -> call(lib, ctx handle, byref(dst), Writers) -> the entry point's return value.  A new entry point that takes
# `const Dav1dHipPicture *dst` and reads or writes its raster planes gets a line here.
# (dav1d_hip_intra_list_run_batch and _run_all go through dav1d_hip_intra_list_run_batch_blend, which holds their check.  Not in the table, and
# not guarded: dav1d_hip_itx_list_run_timed, dav1d_hip_mc_list_run_timed and dav1d_hip_inter_list_run_timed.  bench.py times them on the
# pictures of its tiled steps and uses nothing of what they write; they take a picture in any state and leave twin_ok alone, as
# dav1d_amd/csrc/api_lists.hip says (tests/test_timed_runs.py runs them).  dav1d_hip_recon_list_run_timed IS guarded, like the run it times.)
WRITERS = {
    "lf_batch": lambda l, h, d, s: l.dav1d_hip_lf_batch(h, d, _ptr(s.lf), len(s.lf), s.lvl.ptr, s.post.b4_stride, _ptr(s.lut_e), _ptr(s.lut_i)),
    "ipred_batch": lambda l, h, d, s: l.dav1d_hip_ipred_batch(h, d, _ptr(s.first_wave), len(s.first_wave), None),
    "ipred_list_run_batch": lambda l, h, d, s: l.dav1d_hip_ipred_list_run_batch(h, s.ipred.h, 0, d, None),
    "intra_list_run_batch": lambda l, h, d, s: l.dav1d_hip_intra_list_run_batch(h, s.intra.h, 0, d, s.icoef.ptr, None),
    "intra_list_run_all": lambda l, h, d, s: l.dav1d_hip_intra_list_run_all(h, s.intra.h, d, s.icoef.ptr, None),
    "intra_flow_run": lambda l, h, d, s: l.dav1d_hip_intra_flow_run(h, s.flow.h, d, s.icoef.ptr, None),
    "intra_sb_run": lambda l, h, d, s: l.dav1d_hip_intra_sb_run(h, s.sb.h, d, s.icoef.ptr, None),
    "itx_list_run": lambda l, h, d, s: l.dav1d_hip_itx_list_run(h, s.itx.h, d, s.coef.ptr),
    "itx_add_batch": lambda l, h, d, s: l.dav1d_hip_itx_add_batch(h, d, _ptr(s.frame.itx), len(s.frame.itx), s.coef.ptr),
    "mc_list_run": lambda l, h, d, s: l.dav1d_hip_mc_list_run(h, s.mc.h, d, s.ref_arr, len(s.refs), s.prep.ptr),
    "mc_batch": lambda l, h, d, s: l.dav1d_hip_mc_batch(h, d, s.ref_arr, len(s.refs), _ptr(s.frame.mc), len(s.frame.mc), s.prep.ptr),
    "comp_list_run": lambda l, h, d, s: l.dav1d_hip_comp_list_run(h, s.comp.h, d, s.prep.ptr, None),
    "comp_batch": lambda l, h, d, s: l.dav1d_hip_comp_batch(h, d, _ptr(s.frame.comp), len(s.frame.comp), s.prep.ptr, None),
    "inter_list_run": lambda l, h, d, s: l.dav1d_hip_inter_list_run(h, s.inter.h, d, s.ref_arr, len(s.refs), s.prep.ptr, None),
    "recon_list_run": lambda l, h, d, s: l.dav1d_hip_recon_list_run(h, s.recon.h, d, s.ref_arr, len(s.refs), s.prep.ptr, None, s.coef.ptr),
    "recon_list_run_timed": lambda l, h, d, s: l.dav1d_hip_recon_list_run_timed(h, s.recon.h, d, s.ref_arr, len(s.refs), s.prep.ptr, None, s.coef.ptr,
                                                                                s.ms, s.counts),
    "warp_batch": lambda l, h, d, s: l.dav1d_hip_warp_batch(h, d, s.ref_arr, len(s.refs), _ptr(s.warp), 1, None),
    "mc_scaled_batch": lambda l, h, d, s: l.dav1d_hip_mc_scaled_batch(h, d, s.ref_arr, len(s.refs), _ptr(s.scaled), 1, None),
    "cdef_batch": lambda l, h, d, s: l.dav1d_hip_cdef_batch(h, d, C.byref(s.src.pic), _ptr(s.cdef), len(s.cdef), s.post.cdef_damping, None),
    "lr_batch": lambda l, h, d, s: l.dav1d_hip_lr_batch(h, d, C.byref(s.src.pic), C.byref(s.src.pic), _ptr(s.lr), len(s.lr)),
    "resize": lambda l, h, d, s: l.dav1d_hip_resize(h, d, C.byref(s.src.pic), 0, s.w, 0, 8, s.w, 1 << 14, 0),
    "fg_apply": lambda l, h, d, s: l.dav1d_hip_fg_apply(h, d, C.byref(s.src.pic), C.byref(s.grain), 0),
    "fg_apply_prepared": lambda l, h, d, s: l.dav1d_hip_fg_apply_prepared(h, d, C.byref(s.src.pic), s.prepared, 0),
}


@pytest.fixture(scope="module")
def writers(ctx):
    s = Writers(ctx, 256, 128, 10)
    yield s
    s.free()


@pytest.mark.parametrize("name", list(WRITERS))
def test_a_writer_refuses_a_destination_that_lives_in_its_twin(ctx, writers, name):
    """-EINVAL before anything is enqueued: raster planes (0x5A throughout), twin and flag of `dst` are what they were.  The same call is
    accepted for the same picture once its raster planes are valid, so it is the state that is refused and nothing else."""
    s = writers
    dst, _ = make_source(ctx, np.random.default_rng(8800), s.w, s.h, api.LAYOUT_I420, s.bpc, "twin-only")
    try:
        twin = twin_bytes(ctx, dst)
        s.fresh_coefficients()
        rc = WRITERS[name](ctx.lib, ctx.h, C.byref(dst.pic), s)
        ctx.sync()
        assert rc == -errno.EINVAL, "%s returned %d for a twin-only dst" % (name, rc)
        assert dst.pic.twin_ok == api.TWIN_ONLY
        raw = np.zeros(dst.pic.alloc_size, np.uint8)
        assert ctx.lib.dav1d_hip_download(ctx.h, raw.ctypes.data, dst.pic.alloc, raw.nbytes) == 0
        assert (raw == 0x5A).all(), "%s wrote %d bytes of the raster planes" % (name, int((raw != 0x5A).sum()))
        assert np.array_equal(twin_bytes(ctx, dst), twin), "%s wrote the twin" % name
        dst.untile()
        assert dst.pic.twin_ok == 1
        before = np.zeros(dst.pic.alloc_size, np.uint8)
        assert ctx.lib.dav1d_hip_download(ctx.h, before.ctypes.data, dst.pic.alloc, before.nbytes) == 0
        rc = WRITERS[name](ctx.lib, ctx.h, C.byref(dst.pic), s)
        ctx.sync()
        assert rc == 0, "%s returned %d for the same picture with valid raster planes" % (name, rc)
        # ... and that call is one whose work shows in dst: had the refused one enqueued anything, the 0x5A check above would have seen it
        assert ctx.lib.dav1d_hip_download(ctx.h, raw.ctypes.data, dst.pic.alloc, raw.nbytes) == 0
        assert not np.array_equal(raw, before), "%s: the accepted call wrote nothing, so the refusal above proves nothing" % name
    finally:
        dst.free()


@pytest.mark.parametrize("refs_tiled", [True, False], ids=["launches-write-the-twin", "retile-after"])
def test_recon_list_run_twin_carries_a_twin_only_picture_along(ctx, refs_tiled):
    """dav1d_hip_recon_list_run_twin takes a picture it may change (no const): handed one that lives in its twin, with a list that
    covers half of it, it has to leave raster planes and twin that both hold the oracle's picture — the half the list does not write
    comes from the twin, not from the stale raster planes."""
    import copy
    w, h, bpc = 256, 128, 10
    frame = synth.make_frame(w, h, bpc, seed=8900, edge_frac=0.1)
    geo = synth.plane_geometry(w, h, bpc, 1)

    def upper_half(t):          # tasks whose block starts in the upper half of its plane
        stride = np.array([geo[0][0], geo[1][0], geo[2][0]])[t["plane"]]
        return t["dst_off"] // stride < np.where(t["plane"] == 0, h // 2, h // 4)
    half = copy.copy(frame)
    put = frame.mc[frame.mc["kind"] == 0]          # plain predictions only: no compound pairs, whose PREP halves live in the scratch arena
    half.mc, half.comp, half.itx = put[upper_half(put)], frame.comp[:0], frame.itx[upper_half(frame.itx)]
    assert 0 < len(half.itx) < len(frame.itx) and len(half.mc)
    rng = np.random.default_rng(8901)
    refs_h = [synth.make_planes(rng, w, h, bpc) for _ in range(frame.n_refs)]
    dst0 = synth.make_planes(rng, w, h, bpc, smooth=False)
    want, _, _ = test_frame.oracle_frame(util.default_oracle(), half, dst0, refs_h)
    refs = []
    for rp in refs_h:
        r = ctx.picture(w, h, api.LAYOUT_I420, bpc)
        for pl in range(3):
            r.upload(pl, rp[pl])
        if refs_tiled:
            r.retile()
        refs.append(r)
    dst = ctx.picture(w, h, api.LAYOUT_I420, bpc)
    for pl in range(3):
        dst.upload(pl, dst0[pl])
    put_in_state(ctx, dst, "twin-only")
    prep = ctx.buffer(frame.prep_elems * 2)
    prep.zero()
    coef = ctx.buffer_from(half.coef)
    rl = ctx.recon_list(dst, half.mc, half.comp, half.itx)
    try:
        rl.run_twin(dst, refs, prep, coef)
        assert dst.pic.twin_ok == 1
        for pl in range(3):
            vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
            got = dst.download(pl)
            assert np.array_equal(got[:vh, :vw], want[pl][:vh, :vw]), "raster plane %d" % pl
            assert np.array_equal(test_frame.read_twin(ctx, dst, pl)[:vh, :vw], want[pl][:vh, :vw]), "twin of plane %d" % pl
    finally:
        rl.destroy()
        for o in [dst, prep, coef] + refs:
            o.free()
