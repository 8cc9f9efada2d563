"""The timed measurement aids of the itx, mc and inter lists (dav1d_hip_itx_list_run_timed, dav1d_hip_mc_list_run_timed,
dav1d_hip_inter_list_run_timed): the same launches as the untimed runs, one after the other on the context's stream, each between two
events.  bench.py reads its per-kernel table from them; here they are held to what include/dav1d_hip.h promises:

  * rc == 0, counts[] sum to the list's size and are non-zero in exactly the slots the tasks' shapes fall into,
  * ms[k] == 0 where counts[k] == 0, finite and >= 0 elsewhere (the emulated runtime has no clock: all 0 there),
  * the destination planes (and the prep arena, the coefficient arena) are byte for byte what the untimed *_run leaves from the same
    inputs in a fresh picture — the untimed itx run of a list this short is the all-sizes launch, the timed one a launch per size,
  * ms = NULL is -EINVAL, counts = NULL is accepted,
  * nothing is left alive (dav1d_hip_live_objects).

A 64x64 4:2:0 10-bit picture with one reference; the task lists are written out by hand: two luma blocks (8x8, 16x16) with their chroma,
and — in the case with a compound — two 16x16 PREP predictions combined by a MASK task (a MASK compound keeps the two-step form, an AVG of
two PREP blocks nobody else reads would be folded into the mc tiles and leave the compound launch empty)."""
import ctypes as C
import errno
import math

import numpy as np
import pytest

from dav1d_amd import _lib, api

W = H = 64
BPC = 10
MC_BINS = 15


def _cls(v):
    return 0 if v <= 4 else 1 if v <= 8 else 2 if v <= 16 else 3 if v <= 32 else 4


def _bin(w, h):
    """tile-shape bin of a block of at most 64x16 (include/dav1d_hip.h: 3 * class(w) + class(h))"""
    return 3 * _cls(w) + _cls(h)


@pytest.fixture(scope="module")
def host():
    """dst / reference planes (padded shapes), the compound's mask: made once, never changed"""
    rng = np.random.default_rng(20)
    shapes = [(128, 128), (64, 64), (64, 64)]
    return {"dst": [rng.integers(0, 1 << BPC, s, dtype=np.uint16) for s in shapes],
            "ref": [rng.integers(0, 1 << BPC, s, dtype=np.uint16) for s in shapes],
            "mask": rng.integers(0, 65, 256, dtype=np.uint8)}


def _mc_tasks(sp, with_comp):
    """(dst x, dst y, w, plane, src x, src y, mx, my, filter_2d) -> PUT tasks; with_comp: + two 16x16 PREP tasks and the MASK task over them"""
    blocks = [(0, 0, 8, 0, 5, 3, 4, 9, 0), (0, 0, 4, 1, 2, 1, 2, 12, 0), (0, 0, 4, 2, 2, 1, 2, 12, 0),
              (16, 16, 16, 0, 13, 20, 11, 0, 4), (8, 8, 8, 1, 6, 10, 13, 8, 4), (8, 8, 8, 2, 6, 10, 13, 8, 4)]
    mc = np.zeros(len(blocks) + (2 if with_comp else 0), _lib.MC_TASK)
    for t, (x, y, w, pl, sx, sy, mx, my, f) in zip(mc, blocks):
        t["dst_off"], t["src_x"], t["src_y"], t["w"], t["h"] = y * sp[pl] + x, sx, sy, w, w
        t["mx"], t["my"], t["filter_2d"], t["kind"], t["plane"], t["ref"] = mx, my, f, 0, pl, 0
    comp = np.zeros(1 if with_comp else 0, _lib.COMP_TASK)
    if with_comp:
        for k, (sx, sy, mx, my) in enumerate([(30, 33, 7, 5), (36, 29, 0, 14)]):
            t = mc[len(blocks) + k]
            t["dst_off"], t["src_x"], t["src_y"], t["w"], t["h"] = 256 * k, sx, sy, 16, 16
            t["mx"], t["my"], t["filter_2d"], t["kind"], t["plane"], t["ref"] = mx, my, 1, 1, 0, 0
        k = comp[0]
        k["dst_off"], k["tmp1_off"], k["tmp2_off"], k["mask_off"] = 32 * sp[0] + 32, 0, 256, 0
        k["w"], k["h"], k["kind"], k["plane"] = 16, 16, 2, 0
    return mc, comp


def _itx_tasks(sp):
    """three 4x4 blocks (one of them chroma) and two 8x8 blocks, DCT_DCT, three small coefficients each at scan positions 0 .. 2"""
    blocks = [(0, 32, 0, 0), (4, 32, 0, 0), (12, 4, 0, 1), (16, 40, 1, 0), (40, 8, 1, 0)]       # x, y, tx, plane
    itx = np.zeros(len(blocks), _lib.ITX_TASK)
    coef = np.zeros(3 * 16 + 2 * 64, np.int32)
    off = 0
    for i, (t, (x, y, tx, pl)) in enumerate(zip(itx, blocks)):
        side = 4 << tx
        t["dst_off"], t["cf_off"], t["eob"], t["tx"], t["txtp"], t["plane"] = y * sp[pl] + x, off, 2, tx, 0, pl
        coef[off], coef[off + 1], coef[off + side] = 96 + 16 * i, -40 + 8 * i, 24 - 8 * i
        off += side * side
    return itx, coef


class _Scene:
    """fresh device copies of the inputs: a destination, the reference, the arenas"""

    def __init__(self, ctx, host, coef=None):
        self.ctx = ctx
        self.dst = ctx.picture(W, H, api.LAYOUT_I420, BPC)
        self.ref = ctx.picture(W, H, api.LAYOUT_I420, BPC)
        for pl in range(3):
            self.dst.upload(pl, host["dst"][pl])
            self.ref.upload(pl, host["ref"][pl])
        self.prep = ctx.buffer(2 * 512)
        self.prep.zero()
        self.mask = ctx.buffer_from(host["mask"])
        self.coef = ctx.buffer_from(coef) if coef is not None else None
        self.sp = [self.dst.stride_px(pl) for pl in range(3)]
        self.refs = (api.Picture * 1)(self.ref.pic)

    def state(self):
        out = [self.dst.download(pl).copy() for pl in range(3)] + [self.prep.download(np.int16)]
        if self.coef is not None:
            out.append(self.coef.download(np.int32))
        return out

    def free(self):
        for o in (self.dst, self.ref, self.prep, self.mask, self.coef):
            if o is not None:
                o.free()


def _live(ctx):
    out = (C.c_longlong * 4)()
    assert ctx.lib.dav1d_hip_live_objects(out) == 0
    return list(out)


def _check_slots(ms, counts, expect):
    """expect: {slot: count}; every other slot is empty"""
    counts, ms = [int(v) for v in counts], [float(v) for v in ms]
    print("counts", counts, "ms", ms)
    assert {k: n for k, n in enumerate(counts) if n} == expect
    for k, n in enumerate(counts):
        if n:
            assert math.isfinite(ms[k]) and ms[k] >= 0, (k, ms[k])
        else:
            assert ms[k] == 0, (k, ms[k])


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "%s: %s differs from the untimed run" % (what, ("plane 0", "plane 1", "plane 2", "prep arena", "coefficient arena")[k])


def test_itx_list_run_timed(ctx, host):
    live = _live(ctx)
    probe = ctx.picture(W, H, api.LAYOUT_I420, BPC)
    itx, coef = _itx_tasks([probe.stride_px(pl) for pl in range(3)])
    probe.free()
    lst = ctx.itx_list(itx)
    a, b, c = _Scene(ctx, host, coef), _Scene(ctx, host, coef), _Scene(ctx, host, coef)
    ctx.run_itx_list(lst, a.dst, a.coef)
    ctx.sync()
    ms, counts = (C.c_float * 19)(*([-1.0] * 19)), (C.c_size_t * 19)(*([99] * 19))
    fn = ctx.lib.dav1d_hip_itx_list_run_timed
    assert fn(ctx.h, lst.h, C.byref(b.dst.pic), b.coef.ptr, ms, counts) == 0
    _check_slots(ms, counts, {0: 3, 1: 2})
    assert sum(counts) == len(itx)
    _same(b.state(), a.state(), "timed")
    assert fn(ctx.h, lst.h, C.byref(c.dst.pic), c.coef.ptr, None, counts) == -errno.EINVAL
    ms2 = (C.c_float * 19)(*([-1.0] * 19))
    assert fn(ctx.h, lst.h, C.byref(c.dst.pic), c.coef.ptr, ms2, None) == 0
    _same(c.state(), a.state(), "timed, counts = NULL")
    assert all(v == 0 for k, v in enumerate(ms2) if k > 1) and all(math.isfinite(v) and v >= 0 for v in ms2)
    lst.destroy()
    for s in (a, b, c):
        s.free()
    assert _live(ctx) == live


@pytest.mark.parametrize("with_comp", [True, False], ids=["compound", "no-compound"])
def test_mc_list_run_timed(ctx, host, with_comp):
    live = _live(ctx)
    a, b, c = _Scene(ctx, host), _Scene(ctx, host), _Scene(ctx, host)
    mc, _ = _mc_tasks(a.sp, with_comp)
    lst = ctx.mc_list(mc)
    ctx.run_mc_list(lst, a.dst, [a.ref], a.prep)
    ctx.sync()
    expect = {}
    for t in mc:
        expect[_bin(t["w"], t["h"])] = expect.get(_bin(t["w"], t["h"]), 0) + 1
    assert set(expect) == {0, 4, 8} and sum(expect.values()) == len(mc)        # every block is one tile
    ms, counts = (C.c_float * MC_BINS)(*([-1.0] * MC_BINS)), (C.c_size_t * MC_BINS)(*([99] * MC_BINS))
    fn = ctx.lib.dav1d_hip_mc_list_run_timed
    assert fn(ctx.h, lst.h, C.byref(b.dst.pic), b.refs, 1, b.prep.ptr, ms, counts) == 0
    _check_slots(ms, counts, expect)
    assert sum(counts) == len(mc)
    _same(b.state(), a.state(), "timed")
    assert fn(ctx.h, lst.h, C.byref(c.dst.pic), c.refs, 1, c.prep.ptr, None, counts) == -errno.EINVAL
    ms2 = (C.c_float * MC_BINS)(*([-1.0] * MC_BINS))
    assert fn(ctx.h, lst.h, C.byref(c.dst.pic), c.refs, 1, c.prep.ptr, ms2, None) == 0
    _same(c.state(), a.state(), "timed, counts = NULL")
    lst.destroy()
    for s in (a, b, c):
        s.free()
    assert _live(ctx) == live


@pytest.mark.parametrize("with_comp", [True, False], ids=["compound", "no-compound"])
def test_inter_list_run_timed(ctx, host, with_comp):
    live = _live(ctx)
    a, b, c = _Scene(ctx, host), _Scene(ctx, host), _Scene(ctx, host)
    mc, comp = _mc_tasks(a.sp, with_comp)
    lst = ctx.inter_list(mc, comp)
    assert lst.n_fused == 0                 # the MASK compound stays a launch of its own
    ctx.run_inter_list(lst, a.dst, [a.ref], a.prep, a.mask)
    ctx.sync()
    expect = {}
    for t in mc:
        expect[_bin(t["w"], t["h"])] = expect.get(_bin(t["w"], t["h"]), 0) + 1
    if with_comp:
        expect[MC_BINS] = 1                 # ms[MC_BINS] / counts[MC_BINS]: the compound launch
    n = MC_BINS + 1
    ms, counts = (C.c_float * n)(*([-1.0] * n)), (C.c_size_t * n)(*([99] * n))
    fn = ctx.lib.dav1d_hip_inter_list_run_timed
    assert fn(ctx.h, lst.h, C.byref(b.dst.pic), b.refs, 1, b.prep.ptr, b.mask.ptr, ms, counts) == 0
    _check_slots(ms, counts, expect)
    assert sum(counts) == len(mc) + len(comp)
    _same(b.state(), a.state(), "timed")
    assert fn(ctx.h, lst.h, C.byref(c.dst.pic), c.refs, 1, c.prep.ptr, c.mask.ptr, None, counts) == -errno.EINVAL
    ms2 = (C.c_float * n)(*([-1.0] * n))
    assert fn(ctx.h, lst.h, C.byref(c.dst.pic), c.refs, 1, c.prep.ptr, c.mask.ptr, ms2, None) == 0
    _same(c.state(), a.state(), "timed, counts = NULL")
    lst.destroy()
    for s in (a, b, c):
        s.free()
    assert _live(ctx) == live
