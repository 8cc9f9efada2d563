"""Film grain fused into the device surface export: dav1d_hip_surface_export_grain (dav1d_amd/csrc/surface_grain.hip).

The call must write byte for byte what dav1d_hip_surface_export writes from the picture dav1d_hip_fg_apply_prepared produces.  Expected bytes
never come from the library: the grained planes are the ORACLE's dav1d_apply_grain (test_filmgrain.fg_driver) on the planes the test uploaded,
the surface is the numpy restatement of tests/test_surface.py (expect_yuv / expect_rgb) of those planes.  Every comparison is exact; every
destination is filled with 0xA5 first and compared byte by byte, padding included (test_surface.Dest).  Before a grain set is used the test
asserts that the oracle's grain changed every plane that is supposed to get grain, so a set that changes nothing cannot pass vacuously.

Sizes: (157, 83), (190, 102), (333, 77), (64, 64): more than one 32-row block row, a block boundary inside a 64-sample cell, a partial last
unit in all but the last; two of them odd in both directions with a height that is no multiple of 32.

Thinned on the emulator (the device runs the full product):
  * test_every_geometry: one of the four sizes per (bpc, layout, state), rotating so that every size meets every layout and every state; the
    device runs all four per case;
  * test_sample_types: planar + float, semi-planar + MSB16 and RGB + float per case instead of {planar, semi-planar, RGB} x {MSB16, float}."""
import ctypes as C

import numpy as np
import pytest

import test_filmgrain
import util
from dav1d_amd import api
from test_surface import Dest, expect_rgb, expect_yuv
from util import STATES, make_source

EINVAL = 22
LAYOUTS = [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444]
LAYOUT_IDS = ["i400", "i420", "i422", "i444"]
SIZES = [(157, 83), (190, 102), (333, 77), (64, 64)]
P, S, R = api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, api.SURFACE_RGB_PLANAR
N, M, F = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32


# ------------------------------------------------------------------------------------------------ grain sets

def grain_set(key, bpc, layout, seed):
    """(Dav1dFilmGrainData, is_id, the planes that must change).  Keys: all (every plane, overlap on), csfl (chroma scaled from luma), id444
    (4:4:4 with is_id = 1), noluma (no luma grain), none (no grain at all), clip0 / clip1 (clip_to_restricted_range forced)."""
    rng = np.random.default_rng(seed)
    variant = {"all": 0, "csfl": 1, "id444": 2, "noluma": 3, "none": 0, "clip0": 0, "clip1": 0}[key]
    d = test_filmgrain.random_fg(rng, bpc, variant)
    if key in ("clip0", "clip1"):
        d.clip_to_restricted_range = int(key == "clip1")
    if key == "none":
        d.num_y_points = d.num_uv_points[0] = d.num_uv_points[1] = d.chroma_scaling_from_luma = 0
    mono = layout == api.LAYOUT_I400
    if mono:          # a monochrome stream carries no chroma scaling (the frame header parser leaves it 0)
        d.num_uv_points[0] = d.num_uv_points[1] = d.chroma_scaling_from_luma = 0
    changed = [bool(d.num_y_points)] + ([] if mono else [bool(d.num_uv_points[i] or d.chroma_scaling_from_luma) for i in range(2)])
    return d, int(key == "id444"), changed


def oracle_grain(padded, w, h, layout, bpc, data, is_id):
    """the oracle's dav1d_apply_grain on copies of the padded planes; returns the visible grained planes"""
    lib = test_filmgrain.fg_driver()
    n = len(padded)
    inp = [np.ascontiguousarray(p).copy() for p in padded]
    out = [np.zeros_like(p) for p in inp]
    outp = (C.c_void_p * 3)(*([p.ctypes.data for p in out] + [None] * (3 - n)))
    inpp = (C.c_void_p * 3)(*([p.ctypes.data for p in inp] + [None] * (3 - n)))
    lib.apply_grain(bpc, C.byref(data), w, h, layout, is_id, outp, inpp, out[0].strides[0], out[1].strides[0] if n == 3 else 0)
    ss_h, ss_v = int(layout in (api.LAYOUT_I420, api.LAYOUT_I422)), int(layout == api.LAYOUT_I420)
    return [out[pl][:h, :w] if pl == 0 else out[pl][:(h + ss_v) >> ss_v, :(w + ss_h) >> ss_h] for pl in range(n)]


_MEMO = {}          # the oracle's grained planes per case: computed once, shared, read-only


class Case:
    """A source picture in `state` with a grain handle, the oracle's grained planes (computed once, left unchanged) and the check of one export."""

    def __init__(self, ctx, w, h, layout, bpc, state, gkey="all", seed=0):
        self.ctx, self.w, self.h, self.layout, self.bpc, self.state = ctx, w, h, layout, bpc, state
        seed = 9000 + 1000 * seed + 100 * bpc + 10 * layout + w
        self.pic, self.vis = make_source(ctx, np.random.default_rng(seed), w, h, layout, bpc, state)
        memo = _MEMO.setdefault((w, h, layout, bpc, gkey, seed), {})
        if "g" not in memo:
            # a random set can be void for a plane (one scaling point of value 0, ...): the first of a few seeds whose ORACLE output changes every
            # plane that is supposed to get grain and no other; the library under test has no say in the choice
            for attempt in range(8):
                data, is_id, changed = grain_set(gkey, bpc, layout, seed + 1 + attempt)
                g = oracle_grain([v.base for v in self.vis], w, h, layout, bpc, data, is_id)
                if all(np.array_equal(g[pl], self.vis[pl]) != ch for pl, ch in enumerate(changed)):
                    break
            for pl, ch in enumerate(changed):
                assert np.array_equal(g[pl], self.vis[pl]) != ch, "plane %d: the grain set %s it" % (pl, "leaves" if ch else "changes")
            for a in g:
                a.setflags(write=False)
            memo["g"], memo["data"], memo["is_id"] = g, data, is_id
        self.grained, self.data, self.is_id = memo["g"], memo["data"], memo["is_id"]
        self.handle = ctx.fg_prepare(self.data, bpc, layout)

    def want(self, fmt, sample, matrix=1, full_range=0):
        if fmt == R:
            return expect_rgb(self.grained, self.layout, self.bpc, matrix, full_range, sample)
        return expect_yuv(self.grained, self.bpc, fmt, sample)

    def dest(self, fmt, sample, **kw):
        return Dest(self.ctx, self.w, self.h, self.layout, self.bpc, fmt, sample, **kw)

    def check(self, fmt, sample, matrix=1, full_range=0, **kw):
        d = self.dest(fmt, sample, matrix=matrix, full_range=full_range, **kw)
        try:
            self.pic.export(d.surface, grain=self.handle, is_id=self.is_id)
            d.check(self.want(fmt, sample, matrix, full_range),
                    what="%dx%d %d bpc layout %d %s format %d sample %d matrix %d" % (self.w, self.h, self.bpc, self.layout, self.state, fmt, sample, matrix))
        finally:
            d.free()

    def close(self):
        self.ctx.fg_grain_destroy(self.handle)
        self.pic.free()


# ------------------------------------------------------------------------------------------------ 1. formats and samples

@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_geometry(ctx, bpc, layout, state):
    """every layout x depth x picture state, planar / semi-planar / RGB (BT.709 limited), native samples; a twin-only source has 0x5A in every
    raster byte (util.forget_raster) and must stay twin-only"""
    k = bpc // 2 + layout + STATES.index(state)
    for w, h in SIZES if ctx.backend != "emu" else [SIZES[k % 4]]:
        c = Case(ctx, w, h, layout, bpc, state)
        try:
            before = c.pic.pic.twin_ok
            assert before == {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}[state]
            for fmt in (P, S, R):
                c.check(fmt, N)
            assert c.pic.pic.twin_ok == before
        finally:
            c.close()


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I444], ids=["i400", "i420", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_sample_types(ctx, bpc, layout, state):
    """MSB16 (P010 family) and float behind every format; MSB16 at 8 bpc is refused with -EINVAL and writes nothing"""
    w, h = 190, 102
    c = Case(ctx, w, h, layout, bpc, state, seed=1)
    try:
        combos = [(P, F), (S, M), (R, F)] if ctx.backend == "emu" else [(f, s) for f in (P, S, R) for s in (M, F)]
        for fmt, sample in combos:
            if sample == M and bpc == 8:
                d = c.dest(fmt, N)
                d.surface.desc.sample = M
                rc = ctx.lib.dav1d_hip_surface_export_grain(ctx.h, C.byref(d.surface.desc), C.byref(c.pic.pic), c.handle, 0, 0, h)
                assert rc == -EINVAL
                d.check(None, what="MSB16 at 8 bpc")
                d.free()
                continue
            c.check(fmt, sample)
    finally:
        c.close()


@pytest.mark.parametrize("matrix,full_range,layout,bpc,gkey", [(1, 1, api.LAYOUT_I420, 10, "all"), (9, 0, api.LAYOUT_I422, 12, "all"),
                                                              (0, 0, api.LAYOUT_I444, 8, "id444")], ids=["bt709-full", "bt2020-limited", "identity"])
def test_rgb_matrices(ctx, matrix, full_range, layout, bpc, gkey):
    c = Case(ctx, 157, 83, layout, bpc, "twin-only", gkey, seed=2)
    try:
        c.check(R, N, matrix=matrix, full_range=full_range)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 2. grain variants

VARIANTS = {
    "all-planes-overlap": ("all", api.LAYOUT_I420, 10, (157, 83)),
    "chroma-from-luma": ("csfl", api.LAYOUT_I420, 10, (190, 102)),
    "444-identity": ("id444", api.LAYOUT_I444, 8, (64, 64)),
    "no-luma-odd-width": ("noluma", api.LAYOUT_I420, 12, (333, 77)),
    "monochrome": ("all", api.LAYOUT_I400, 10, (157, 83)),
    "no-grain": ("none", api.LAYOUT_I420, 10, (190, 102)),
    "clip-0": ("clip0", api.LAYOUT_I422, 10, (157, 83)),
    "clip-1": ("clip1", api.LAYOUT_I422, 8, (333, 77)),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_grain_variants(ctx, name):
    gkey, layout, bpc, (w, h) = VARIANTS[name]
    for state in ("twin-only", "raster"):
        c = Case(ctx, w, h, layout, bpc, state, gkey, seed=3)
        try:
            if gkey == "none":          # must equal the plain export: the grained planes are the planes
                assert all(np.array_equal(a, b) for a, b in zip(c.grained, c.vis))
            if gkey in ("clip0", "clip1"):
                assert c.data.clip_to_restricted_range == int(gkey == "clip1")
            for fmt in (P, S, R):
                c.check(fmt, N)
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------ 3. bands

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("fmt", [P, S, R], ids=["planar", "semiplanar", "rgb"])
def test_bands(ctx, fmt, state):
    """[0, 34), [34, 70), [70, h): not aligned with the 32-row grain blocks.  Each band alone leaves every other row at the sentinel; the three
    into one destination equal the single call (whose bytes test_every_geometry holds to the oracle: the same expectation here)"""
    w, h, bpc, layout = 190, 102, 10, api.LAYOUT_I420
    c = Case(ctx, w, h, layout, bpc, state, seed=4)
    want = c.want(fmt, N)
    ch = (h + 1) >> 1

    def plane_rows(r0, r1):
        if fmt == R:
            return [(r0, r1)] * 3
        return [(r0, r1)] + [(r0 >> 1, ch if r1 >= h else r1 >> 1)] * (len(want) - 1)
    bands = ((0, 34), (34, 70), (70, h))
    try:
        for r0, r1 in bands:
            d = c.dest(fmt, N)
            c.pic.export(d.surface, r0, r1, grain=c.handle)
            d.check(want, rows=plane_rows(r0, r1), what="band [%d, %d)" % (r0, r1))
            d.free()
        d = c.dest(fmt, N)
        for r0, r1 in bands:
            c.pic.export(d.surface, r0, r1 if r1 < h else 1 << 30, grain=c.handle)
        d.check(want, what="three bands")
        d.free()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 4. unaligned destinations

@pytest.mark.parametrize("fmt,sample", [(P, N), (S, N), (S, F), (R, N)], ids=["planar", "semiplanar", "semiplanar-float", "rgb"])
def test_unaligned_destinations(ctx, fmt, sample):
    """a base one sample past a 256-byte boundary and rows padded by one sample / by 14 bytes: the narrow store path, whole units and the last
    partial one"""
    for w, h, layout, bpc in ((333, 77, api.LAYOUT_I422, 10), (157, 83, api.LAYOUT_I420, 8)):
        c = Case(ctx, w, h, layout, bpc, "twin-only", seed=5)
        es = 4 if sample == F else 2 if bpc > 8 else 1
        try:
            c.check(fmt, sample, pad=es, offset=es)
            if 14 % es == 0:
                c.check(fmt, sample, pad=14, offset=0)
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------ 5. the source is left alone

def _live(ctx):
    out = (C.c_longlong * 4)()
    assert ctx.lib.dav1d_hip_live_objects(out) == 0
    return list(out)


def _raster_bytes(ctx, pic):
    out = np.zeros(pic.pic.alloc_size, np.uint8)
    ctx.sync()
    assert ctx.lib.dav1d_hip_download(ctx.h, out.ctypes.data, pic.pic.alloc, pic.pic.alloc_size) == 0
    return out


@pytest.mark.parametrize("fmt", [S, R], ids=["semiplanar", "rgb"])
def test_source_untouched(ctx, fmt):
    w, h, bpc, layout = 157, 83, 10, api.LAYOUT_I420
    c = Case(ctx, w, h, layout, bpc, "twin-only", seed=6)
    try:
        twin = util.twin_bytes(ctx, c.pic)
        ptrs = [c.pic.pic.twin[pl] for pl in range(3)]
        live = _live(ctx)
        d = c.dest(fmt, N)
        c.pic.export(d.surface, grain=c.handle)
        assert _live(ctx) == live, "the call allocated a picture"
        d.check(c.want(fmt, N), what="twin-only")
        d.free()
        assert c.pic.pic.twin_ok == api.TWIN_ONLY and [c.pic.pic.twin[pl] for pl in range(3)] == ptrs
        assert (_raster_bytes(ctx, c.pic) == 0x5A).all(), "the raster planes of a twin-only source were written"
        assert np.array_equal(util.twin_bytes(ctx, c.pic), twin)
    finally:
        c.close()
    c = Case(ctx, w, h, layout, bpc, "raster", seed=6)
    try:
        before = _raster_bytes(ctx, c.pic)
        live = _live(ctx)
        d = c.dest(fmt, N)
        c.pic.export(d.surface, grain=c.handle)
        assert _live(ctx) == live
        d.check(c.want(fmt, N), what="raster")
        d.free()
        assert c.pic.pic.twin_ok == 0 and np.array_equal(_raster_bytes(ctx, c.pic), before)
        for pl in range(3):
            assert np.array_equal(c.pic.download(pl)[:c.vis[pl].shape[0], :c.vis[pl].shape[1]], c.vis[pl])
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 6. errors

def test_errors(ctx):
    w, h, bpc, layout = 190, 102, 10, api.LAYOUT_I420
    c = Case(ctx, w, h, layout, bpc, "raster", seed=7)
    other_bpc = ctx.fg_prepare(c.data, 8, layout)
    other_layout = ctx.fg_prepare(c.data, bpc, api.LAYOUT_I444)
    try:
        for fmt in (P, R):
            for handle, rows in ((None, (0, h)), (other_bpc, (0, h)), (other_layout, (0, h)), (c.handle, (1, 32)), (c.handle, (0, 33))):
                d = c.dest(fmt, N)
                rc = ctx.lib.dav1d_hip_surface_export_grain(ctx.h, C.byref(d.surface.desc), C.byref(c.pic.pic), handle, 0, rows[0], rows[1])
                assert rc == -EINVAL, (rc, rows)
                d.check(None, what="a refused export")
                d.free()
        # an argument error of the plain export comes back as it does there
        d = c.dest(P, N)
        d.surface.desc.w = w + 1
        assert ctx.lib.dav1d_hip_surface_export_grain(ctx.h, C.byref(d.surface.desc), C.byref(c.pic.pic), c.handle, 0, 0, h) == -EINVAL
        d.check(None, what="a refused export")
        d.free()
        d = c.dest(R, N, matrix=4)
        assert ctx.lib.dav1d_hip_surface_export_grain(ctx.h, C.byref(d.surface.desc), C.byref(c.pic.pic), c.handle, 0, 0, h) == -95
        d.check(None, what="a refused export")
        d.free()
        c.check(P, N)          # ... and the same handle and picture are accepted when nothing is wrong
    finally:
        ctx.fg_grain_destroy(other_bpc)
        ctx.fg_grain_destroy(other_layout)
        c.close()


# ------------------------------------------------------------------------------------------------ 7. Python

def test_export_is_asynchronous_and_timed(ctx):
    """Context.surface + DevicePicture.export(grain=): the bytes, a device time from the two events, nothing left behind"""
    before = _live(ctx)
    c = Case(ctx, 64, 64, api.LAYOUT_I420, 10, "retiled", seed=8)
    s = ctx.surface(64, 64, api.LAYOUT_I420, 10, S, M)
    c.pic.export(s, grain=c.handle)
    got = s.download()
    assert ctx.last_kernel_ms() >= 0.0
    assert all(np.array_equal(a, b) for a, b in zip(got, c.want(S, M)))
    s.free()
    c.close()
    assert _live(ctx) == before


def _torch_child():
    """(a process of its own: torch brings its own HIP runtime, see tests/test_surface.py)"""
    import torch
    w, h, bpc, layout = 190, 102, 10, api.LAYOUT_I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    c = Case(tctx, w, h, layout, bpc, "twin-only", seed=9)
    t = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    api.export_to_tensor(c.pic, t, matrix=1, full_range=0, grain=c.handle)
    tctx.sync()
    got, want = t.cpu().numpy(), c.want(R, F)
    for k in range(3):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), "RGB float tensor, plane %d" % k
    d = c.dest(R, F)
    c.pic.export(d.surface, grain=c.handle)          # DevicePicture.export gives the same bytes
    d.check(want, what="export next to export_to_tensor")
    d.free()
    y = torch.empty((h, w), dtype=torch.int16, device="cuda")
    uv = torch.empty(((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=torch.int16, device="cuda")
    api.export_to_tensor(c.pic, y, chroma=uv, sample=M, grain=c.handle)
    tctx.sync()
    p010 = c.want(S, M)
    assert np.array_equal(y.cpu().numpy().view(np.uint16), p010[0]) and np.array_equal(uv.cpu().numpy().view(np.uint16), p010[1]), "P010 tensors"
    assert c.pic.pic.twin_ok == api.TWIN_ONLY
    c.close()
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_to_tensor_with_grain():
    """export_to_tensor(..., grain=) into torch tensors equals the oracle's grain rearranged by numpy, and DevicePicture.export(..., grain=)"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
