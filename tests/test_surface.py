"""Device output surfaces: dav1d_hip_surface_export (dav1d_amd/csrc/surface.hip) against numpy.

A picture is exported where it lives — raster planes, or the tiled twin of a DAV1D_HIP_TWIN_ONLY picture, which must stay one — into
planar, semi-planar (NV12 / P010 family) and planar RGB surfaces of the caller.  Every expected value comes from numpy on the planes
the test uploaded (or from the oracle where a frame is reconstructed / grain is applied); every comparison is exact.  Every destination
is filled with 0xA5 first and compared byte by byte, padding included, so a store outside the visible samples shows in any case."""
import ctypes as C
import math

import numpy as np
import pytest

import util
import synth_frames as synth
import test_frame
import test_filmgrain
from dav1d_amd import api
from util import STATES, forget_raster, make_source          # the three picture states: shared with tests/test_picture_states.py

EINVAL, ENOTSUP = 22, 95
SENTINEL = 0xA5
LAYOUTS = [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444]
SIZES = [(190, 102), (64, 64), (333, 77)]
MATRICES = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}


# ------------------------------------------------------------------------------------------------ expectations (numpy)

def convert(a, bpc, sample):
    if sample == api.SAMPLE_MSB16:
        return (a.astype(np.uint16) << (16 - bpc)).astype(np.uint16)
    if sample == api.SAMPLE_F32:
        return a.astype(np.float32) * np.float32(1.0 / ((1 << bpc) - 1))
    return a


def expect_yuv(vis, bpc, fmt, sample):
    if fmt == api.SURFACE_SEMIPLANAR and len(vis) == 3:
        uv = np.empty((vis[1].shape[0], 2 * vis[1].shape[1]), vis[1].dtype)
        uv[:, 0::2], uv[:, 1::2] = vis[1], vis[2]
        vis = [vis[0], uv]
    return [convert(p, bpc, sample) for p in vis]


def rgb_coefficients(matrix, full_range, d):
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    mx = (1 << d) - 1
    sy = 1.0 if full_range else mx / (219 << (d - 8))
    sc = 1.0 if full_range else mx / (224 << (d - 8))
    q = lambda x: int(math.floor(x * 16384 + 0.5))      # noqa: E731
    return q(sy), q(2 * (1 - kr) * sc), q(2 * (1 - kb) * sc), q(2 * (1 - kb) * kb / kg * sc), q(2 * (1 - kr) * kr / kg * sc)


def expect_rgb(vis, layout, bpc, matrix, full_range, sample=api.SAMPLE_NATIVE):
    """the formula of include/dav1d_hip.h / DESIGN.md 10, restated"""
    d, mx = bpc, (1 << bpc) - 1
    Y = vis[0].astype(np.int32)
    h, w = Y.shape
    if layout == api.LAYOUT_I400:
        U = V = np.full((h, w), 1 << (d - 1), np.int32)
    else:
        ss_h = 1 if layout != api.LAYOUT_I444 else 0
        ss_v = 1 if layout == api.LAYOUT_I420 else 0
        yy, xx = np.arange(h)[:, None] >> ss_v, np.arange(w)[None, :] >> ss_h
        U, V = vis[1].astype(np.int32)[yy, xx], vis[2].astype(np.int32)[yy, xx]
    if matrix == 0:
        R, G, B = V, Y, U
    else:
        cy, crv, cbu, cgu, cgv = rgb_coefficients(matrix, full_range, d)
        y = Y - (0 if full_range else 16 << (d - 8))
        cb, cr = U - (1 << (d - 1)), V - (1 << (d - 1))
        R = np.clip((cy * y + crv * cr + 8192) >> 14, 0, mx)
        G = np.clip((cy * y - cgu * cb - cgv * cr + 8192) >> 14, 0, mx)
        B = np.clip((cy * y + cbu * cb + 8192) >> 14, 0, mx)
    dt = np.uint8 if bpc == 8 else np.uint16
    return [convert(p.astype(dt), bpc, sample) for p in (R, G, B)]


# ------------------------------------------------------------------------------------------------ destinations

class Dest:
    """Caller-owned destination planes with a byte offset and a row padding of choice, described to the library by Surface.wrap; check()
    compares every byte of every buffer: the expected samples where they belong, the sentinel everywhere else."""

    def __init__(self, ctx, w, h, layout, bpc, fmt, sample, matrix=1, full_range=0, pad=0, offset=0, sentinel=SENTINEL):
        self.ctx, self.sentinel = ctx, sentinel
        self.shapes, self.dtype = api.surface_planes(w, h, layout, bpc, fmt, sample)
        es = self.dtype.itemsize
        self.offset = offset
        self.strides = [cols * es + pad for _, cols in self.shapes]
        self.bufs = [ctx.buffer(256 + offset + rows * st + 64) for (rows, _), st in zip(self.shapes, self.strides)]
        self.lead = [-b.ptr % 256 for b in self.bufs]          # up to the next 256-byte boundary: `offset` counts from there
        for b in self.bufs:
            assert ctx.lib.dav1d_hip_memset(ctx.h, b.ptr, sentinel, b.nbytes) == 0
        self.surface = api.Surface.wrap(ctx, [b.ptr + ld + offset for b, ld in zip(self.bufs, self.lead)], self.strides, w, h, layout, bpc, fmt, sample,
                                        matrix, full_range)

    def image(self, k, expected=None, rows=None):
        """what buffer k must hold, byte for byte"""
        b = self.bufs[k]
        want = np.full(b.nbytes, self.sentinel, np.uint8)
        if expected is not None:
            n_rows, cols = self.shapes[k]
            start = self.lead[k] + self.offset
            body = want[start:start + n_rows * self.strides[k]].reshape(n_rows, self.strides[k])
            e = np.ascontiguousarray(expected).view(np.uint8).reshape(n_rows, cols * self.dtype.itemsize)
            r0, r1 = rows[k] if rows is not None else (0, n_rows)
            body[r0:r1, :e.shape[1]] = e[r0:r1]
        return want

    def check(self, expected, rows=None, what=""):
        self.ctx.sync()
        for k, b in enumerate(self.bufs):
            got = b.download(np.uint8)
            want = self.image(k, expected[k] if expected is not None else None, rows)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError("%s plane %d: %d bytes differ, first at byte %d (offset %d, stride %d): got %d, want %d"
                                     % (what, k, len(bad), bad[0], self.offset, self.strides[k], got[bad[0]], want[bad[0]]))

    def free(self):
        for b in self.bufs:
            b.free()


def export_and_check(ctx, pic, expected, fmt, sample, what, **kw):
    d = Dest(ctx, pic.w, pic.h, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export(d.surface)
        d.check(expected, what=what)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 1. planar and semi-planar, every geometry

@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_planar_and_semiplanar_every_geometry(ctx, bpc, layout, state):
    for w, h in SIZES:
        rng = np.random.default_rng(7000 + 100 * bpc + 10 * layout + w)
        pic, vis = make_source(ctx, rng, w, h, layout, bpc, state)
        try:
            before = pic.pic.twin_ok
            assert before == {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}[state]
            for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR):
                export_and_check(ctx, pic, expect_yuv(vis, bpc, fmt, api.SAMPLE_NATIVE), fmt, api.SAMPLE_NATIVE,
                                 "%dx%d %d bpc layout %d %s format %d" % (w, h, bpc, layout, state, fmt))
            assert pic.pic.twin_ok == before
        finally:
            pic.free()


class _KeepPictures:
    """A context as test_frame.hip_frame takes it whose pictures outlive the helper: hip_frame frees what it made, this test wants the
    reconstructed picture itself (hip_frame is used as it is)."""

    def __init__(self, ctx):
        self._ctx, self.made = ctx, []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def picture(self, *a):
        p = self._ctx.picture(*a)
        p.really_free, p.free = p.free, lambda: None
        self.made.append(p)
        return p


def test_reconstructed_frame_is_exported_from_its_twin(ctx):
    """a 512x320 10-bit frame reconstructed with the picture living in its twin only (ref_twin = 3, dav1d_hip_recon_list_run_tiled), the way
    the suite makes them; expected planes from the oracle's replay"""
    w, h, bpc = 512, 320, 10
    frame = synth.make_frame(w, h, bpc, seed=7, edge_frac=0.1)
    rng = np.random.default_rng(11)
    refs = [synth.make_planes(rng, w, h, bpc) for _ in range(frame.n_refs)]
    dst0 = synth.make_planes(rng, w, h, bpc, smooth=False)
    want, _, _ = test_frame.oracle_frame(util.default_oracle(), frame, dst0, refs)
    keep = _KeepPictures(ctx)
    ctx.auto_retile, ctx.tiled_native = True, True
    ctx.set_option("ref_twin", 3)
    try:
        got, _, _ = test_frame.hip_frame(keep, frame, dst0, refs, recon=True)
        pic = keep.made[0]
        assert pic.pic.twin_ok == api.TWIN_ONLY
        forget_raster(ctx, pic)          # (hip_frame's download staged raster rows there)
        vis = [want[pl][:pic.pic.p[pl].h, :pic.pic.p[pl].w] for pl in range(3)]
        for pl in range(3):
            assert np.array_equal(got[pl][:vis[pl].shape[0], :vis[pl].shape[1]], vis[pl])
        for fmt, sample in ((api.SURFACE_PLANAR, api.SAMPLE_NATIVE), (api.SURFACE_SEMIPLANAR, api.SAMPLE_MSB16)):
            export_and_check(ctx, pic, expect_yuv(vis, bpc, fmt, sample), fmt, sample, "frame, format %d" % fmt)
        export_and_check(ctx, pic, expect_rgb(vis, api.LAYOUT_I420, bpc, 1, 0), api.SURFACE_RGB_PLANAR, api.SAMPLE_NATIVE, "frame, RGB")
        assert pic.pic.twin_ok == api.TWIN_ONLY
    finally:
        ctx.auto_retile, ctx.tiled_native = False, False
        ctx.set_option("ref_twin", 1)
        for p in keep.made:
            p.really_free()


# ------------------------------------------------------------------------------------------------ 2. sample types

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I444], ids=["i400", "i420", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_sample_types(ctx, bpc, layout, state):
    w, h = 190, 102
    rng = np.random.default_rng(7100 + bpc + layout)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, state)
    try:
        for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR):
            for sample in (api.SAMPLE_MSB16, api.SAMPLE_F32):
                if sample == api.SAMPLE_MSB16 and bpc == 8:
                    continue          # refused: test_refusals
                want = expect_yuv(vis, bpc, fmt, sample)
                native = expect_yuv(vis, bpc, fmt, api.SAMPLE_NATIVE)
                if sample == api.SAMPLE_MSB16:
                    assert all(np.array_equal(a, n.astype(np.uint16) << (16 - bpc)) for a, n in zip(want, native))
                else:
                    assert all(np.array_equal(a.view(np.uint32), (n.astype(np.float32) * np.float32(1.0 / ((1 << bpc) - 1))).view(np.uint32))
                               for a, n in zip(want, native))
                export_and_check(ctx, pic, want, fmt, sample, "%d bpc layout %d format %d sample %d" % (bpc, layout, fmt, sample))
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 3. RGB

def test_rgb_table_restated():
    """the invariants of the formula, on the numpy side (the device is held to the same numpy below)"""
    for bpc in (8, 10, 12):
        mx, mid = (1 << bpc) - 1, 1 << (bpc - 1)
        for matrix in (1, 5, 6, 9):
            g = np.arange(0, mx + 1, dtype=np.uint16)[None, :]
            grey = expect_rgb([g, np.full_like(g, mid), np.full_like(g, mid)], api.LAYOUT_I444, bpc, matrix, 0)
            assert np.array_equal(grey[0], grey[1]) and np.array_equal(grey[1], grey[2])
            assert grey[0][0, 16 << (bpc - 8)] == 0 and grey[0][0, 235 << (bpc - 8)] == mx
            full = expect_rgb([g, np.full_like(g, mid), np.full_like(g, mid)], api.LAYOUT_I444, bpc, matrix, 1)
            assert np.array_equal(full[0][0], g[0].astype(full[0].dtype))


@pytest.mark.parametrize("layout", LAYOUTS, ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("full_range", [0, 1], ids=["limited", "full"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_rgb_matches_the_integer_formula(ctx, bpc, full_range, layout):
    w, h = 190, 102
    mx, mid = (1 << bpc) - 1, 1 << (bpc - 1)
    rng = np.random.default_rng(7200 + bpc + 3 * layout + full_range)
    for extremes, state in ((False, "raster"), (True, "twin-only")):
        pic, vis = make_source(ctx, rng, w, h, layout, bpc, state, extremes=extremes)
        try:
            for matrix in (1, 5, 6, 9) + ((0,) if layout == api.LAYOUT_I444 else ()):
                want = expect_rgb(vis, layout, bpc, matrix, full_range)
                if matrix == 0:
                    assert all(np.array_equal(a, b) for a, b in zip(want, (vis[2], vis[0], vis[1]))), "identity returns the planes"
                export_and_check(ctx, pic, want, api.SURFACE_RGB_PLANAR, api.SAMPLE_NATIVE,
                                 "RGB %d bpc layout %d matrix %d full %d %s" % (bpc, layout, matrix, full_range, state), matrix=matrix, full_range=full_range)
            assert pic.pic.twin_ok == (api.TWIN_ONLY if state == "twin-only" else 0)
        finally:
            pic.free()
    # invariants, on the device: grey stays grey; limited-range black / white reach 0 / max
    pic = ctx.picture(w, h, layout, bpc)
    try:
        ramp = (np.arange(pic.padded_shape(0)[0] * pic.padded_shape(0)[1]) % (mx + 1)).reshape(pic.padded_shape(0)).astype(pic.dtype)
        ramp[0, :8], ramp[1, :8] = 16 << (bpc - 8), 235 << (bpc - 8)
        pic.upload(0, ramp)
        for pl in range(1, pic.n_planes):
            pic.upload(pl, np.full(pic.padded_shape(pl), mid, pic.dtype))
        s = ctx.surface(w, h, layout, bpc, api.SURFACE_RGB_PLANAR, api.SAMPLE_NATIVE, matrix=9, full_range=full_range)
        pic.export(s)
        R, G, B = s.download()
        s.free()
        assert np.array_equal(R, G) and np.array_equal(G, B)
        if not full_range:
            assert (R[0, :8] == 0).all() and (R[1, :8] == mx).all()
        else:
            assert np.array_equal(R, ramp[:h, :w])
    finally:
        pic.free()


def test_rgb_sample_types(ctx):
    """the output functor is the same one behind RGB: P010-style and float RGB planes"""
    w, h, bpc = 190, 102, 10
    rng = np.random.default_rng(7250)
    pic, vis = make_source(ctx, rng, w, h, api.LAYOUT_I420, bpc, "twin-only", extremes=True)
    try:
        for sample in (api.SAMPLE_MSB16, api.SAMPLE_F32):
            export_and_check(ctx, pic, expect_rgb(vis, api.LAYOUT_I420, bpc, 1, 0, sample), api.SURFACE_RGB_PLANAR, sample, "RGB sample %d" % sample)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 4. bands

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("fmt", [api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, api.SURFACE_RGB_PLANAR], ids=["planar", "semiplanar", "rgb"])
def test_bands(ctx, fmt, state):
    w, h, bpc, layout = 190, 77, 10, api.LAYOUT_I420
    rng = np.random.default_rng(7300 + fmt)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, state)
    want = expect_rgb(vis, layout, bpc, 1, 0) if fmt == api.SURFACE_RGB_PLANAR else expect_yuv(vis, bpc, fmt, api.SAMPLE_NATIVE)
    ch = (h + 1) >> 1

    def plane_rows(r0, r1):
        if fmt == api.SURFACE_RGB_PLANAR:
            return [(r0, r1)] * 3
        return [(r0, r1)] + [(r0 >> 1, ch if r1 >= h else r1 >> 1)] * (len(want) - 1)
    try:
        # a band export leaves every row outside it at the sentinel
        for r0, r1 in ((32, 34), (0, 32), (34, 1 << 30), (40, 56)):
            d = Dest(ctx, w, h, layout, bpc, fmt, api.SAMPLE_NATIVE)
            pic.export(d.surface, r0, r1)
            d.check(want, rows=plane_rows(r0, min(r1, h)), what="band [%d, %d)" % (r0, r1))
            d.free()
        # three bands into one surface equal one whole export
        d = Dest(ctx, w, h, layout, bpc, fmt, api.SAMPLE_NATIVE)
        for r0, r1 in ((0, 32), (32, 34), (34, h)):
            pic.export(d.surface, r0, r1)
        d.check(want, what="three bands")
        d.free()
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. strides and overwrite detection

@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-sample-off"])
@pytest.mark.parametrize("pad", [0, 2, 14, 64])
@pytest.mark.parametrize("bpc", [8, 10])
def test_strides_and_overwrites(ctx, bpc, pad, offset):
    """tight rows, rows padded by 2, 14 and 64 bytes, a base one sample past a 256-byte boundary: the 16-byte store path and the narrow one,
    whole groups and the last partial group of a row; every byte outside the visible samples keeps the sentinel"""
    rng = np.random.default_rng(7400 + bpc + pad)
    for w, h, layout in ((190, 102, api.LAYOUT_I420), (64, 64, api.LAYOUT_I444), (333, 77, api.LAYOUT_I422)):
        pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
        try:
            for fmt, sample in ((api.SURFACE_PLANAR, api.SAMPLE_NATIVE), (api.SURFACE_SEMIPLANAR, api.SAMPLE_NATIVE),
                                (api.SURFACE_SEMIPLANAR, api.SAMPLE_F32), (api.SURFACE_RGB_PLANAR, api.SAMPLE_NATIVE)):
                es = 4 if sample == api.SAMPLE_F32 else 2 if bpc > 8 else 1
                if pad % es:
                    continue          # not a stride of this sample type: test_refusals
                want = expect_rgb(vis, layout, bpc, 1, 0) if fmt == api.SURFACE_RGB_PLANAR else expect_yuv(vis, bpc, fmt, sample)
                export_and_check(ctx, pic, want, fmt, sample, "%dx%d %d bpc format %d sample %d pad %d offset %d" % (w, h, bpc, fmt, sample, pad, offset),
                                 pad=pad, offset=offset * es)
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refusals(ctx):
    w, h = 190, 102
    rng = np.random.default_rng(7500)
    pics = {}
    for bpc, layout in ((10, api.LAYOUT_I420), (8, api.LAYOUT_I420), (10, api.LAYOUT_I444), (10, api.LAYOUT_I400)):
        pics[bpc, layout] = make_source(ctx, rng, w, h, layout, bpc, "raster")[0]

    def refused(code, bpc, layout, fmt, sample, change=None, rows=(0, 1 << 30), **kw):
        pic = pics[bpc, layout]
        d = Dest(ctx, w, h, layout, bpc, fmt, sample if not (sample == api.SAMPLE_MSB16 and bpc == 8) else api.SAMPLE_NATIVE, **kw)
        d.surface.desc.sample = sample
        if change:
            change(d.surface.desc)
        rc = ctx.lib.dav1d_hip_surface_export(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), rows[0], rows[1])
        assert rc == -code, (rc, code)
        d.check(None, what="a refused export")
        d.free()

    P, S, R = api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, api.SURFACE_RGB_PLANAR
    N, M, F = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32
    try:
        def null_plane(k):
            def f(desc):
                desc.data[k] = None
            return f
        for fmt, k in ((P, 0), (P, 1), (P, 2), (S, 0), (S, 1), (R, 0), (R, 2)):
            refused(EINVAL, 10, api.LAYOUT_I420, fmt, N, null_plane(k))
        refused(EINVAL, 10, api.LAYOUT_I400, P, N, null_plane(0))
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, lambda d: setattr(d, "w", w + 1))
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, lambda d: setattr(d, "h", h - 1))

        def stride(k, delta=None, value=None):
            def f(desc):
                desc.stride[k] = value if value is not None else desc.stride[k] + delta
            return f
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, stride(0, -2))            # below the row's bytes
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, stride(2, -2))
        refused(EINVAL, 10, api.LAYOUT_I420, S, N, stride(1, -2))            # interleaved row: 2 * 95 samples
        refused(EINVAL, 10, api.LAYOUT_I420, R, F, stride(1, -4))
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, stride(0, +1), pad=2)      # not a multiple of the sample size
        refused(EINVAL, 10, api.LAYOUT_I420, R, F, stride(2, +2), pad=4)
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, stride(0, value=-380))
        refused(EINVAL, 8, api.LAYOUT_I420, P, M)                             # MSB16 at 8 bpc
        refused(EINVAL, 8, api.LAYOUT_I420, S, M)
        refused(EINVAL, 10, api.LAYOUT_I420, R, N, matrix=0)                  # identity needs 4:4:4
        refused(EINVAL, 10, api.LAYOUT_I400, R, N, matrix=0)
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, rows=(1, 32))              # odd row0
        refused(EINVAL, 10, api.LAYOUT_I420, R, N, rows=(33, 64))
        refused(EINVAL, 10, api.LAYOUT_I420, P, N, rows=(0, 33))              # odd row1 that is not the picture's end
        for m in (2, 3, 4, 7, 8, 10, 12, 14, -1):
            refused(ENOTSUP, 10, api.LAYOUT_I420, R, N, matrix=m)
        refused(ENOTSUP, 10, api.LAYOUT_I444, R, N, matrix=4)
        # ... and the same surfaces are accepted when nothing is wrong with them
        for (bpc, layout), pic in pics.items():
            d = Dest(ctx, w, h, layout, bpc, R, N, matrix=0 if layout == api.LAYOUT_I444 else 6)
            pic.export(d.surface, 0, h)
            ctx.sync()
            d.free()
    finally:
        for p in pics.values():
            p.free()


def test_a_picture_of_another_device_is_refused():
    """-EXDEV by the check the frame calls use, on the emulator's two devices (tests/conftest.py)"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        pic = other.picture(64, 64, api.LAYOUT_I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        d = Dest(ctx, 64, 64, api.LAYOUT_I420, 10, api.SURFACE_PLANAR, api.SAMPLE_NATIVE)
        assert ctx.lib.dav1d_hip_surface_export(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), 0, 64) == -18
        d.check(None, what="a refused export")
        d.free()
        ctx.lib.dav1d_hip_context_use(other.h)
        pic.free()
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. grain, then export

@pytest.mark.parametrize("bpc,layout", [(10, api.LAYOUT_I420), (8, api.LAYOUT_I444)], ids=["10bit-420", "8bit-444"])
def test_grain_then_export(ctx, bpc, layout):
    """The two library calls of dav1d_hip_glue_output_surface in its order (the function itself needs a decoder around it: it is compiled and
    linked by the hooked build): dav1d_hip_fg_apply into a temporary picture, dav1d_hip_surface_export from that.  Equals the oracle's grain
    output rearranged by numpy.  Semi-planar; MSB16 (P010) at 10 bits, native samples at 8 bits, where MSB16 is refused by definition."""
    lib = test_filmgrain.fg_driver()
    rng = np.random.default_rng(7600 + bpc)
    w, h = 160, 96
    is_id = int(layout == api.LAYOUT_I444)
    data = test_filmgrain.random_fg(rng, bpc, 2 if is_id else 0)
    src, tmp = ctx.picture(w, h, layout, bpc), ctx.picture(w, h, layout, bpc)
    try:
        planes = []
        for pl in range(3):
            ph, pw = src.padded_shape(pl)
            base = np.zeros((ph, src.stride_px(pl)), src.dtype)
            base[:, :pw] = rng.integers(0, 1 << bpc, size=(ph, pw))
            planes.append(base[:, :pw])
            src.upload(pl, planes[pl])
            tmp.upload(pl, np.zeros_like(planes[pl]))
        want = [np.zeros_like(p.base)[:, :p.shape[1]] for p in planes]
        inp = synth.copy_planes(planes)
        outp = (C.c_void_p * 3)(*[p.ctypes.data for p in want])
        inpp = (C.c_void_p * 3)(*[p.ctypes.data for p in inp])
        lib.apply_grain(bpc, C.byref(data), w, h, layout, is_id, outp, inpp, want[0].strides[0], want[1].strides[0])
        vis = [want[pl][:tmp.pic.p[pl].h, :tmp.pic.p[pl].w] for pl in range(3)]
        assert any(not np.array_equal(vis[pl], planes[pl][:vis[pl].shape[0], :vis[pl].shape[1]]) for pl in range(3)), "the grain set changes nothing"
        ctx.fg_apply(tmp, src, data, is_id)
        sample = api.SAMPLE_MSB16 if bpc > 8 else api.SAMPLE_NATIVE
        export_and_check(ctx, tmp, expect_yuv(vis, bpc, api.SURFACE_SEMIPLANAR, sample), api.SURFACE_SEMIPLANAR, sample, "grain %d bpc" % bpc)
    finally:
        src.free()
        tmp.free()


# ------------------------------------------------------------------------------------------------ 8. the size users run (GPU only)

@pytest.fixture
def gpu_ctx():
    c = util.make_context("hip")
    c.backend = "hip"
    yield c
    c.close()


@pytest.mark.gpu
def test_8k_picture_from_its_twin(gpu_ctx):
    ctx = gpu_ctx
    w, h, bpc, layout = 7680, 4320, 10, api.LAYOUT_I420
    rng = np.random.default_rng(7700)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        export_and_check(ctx, pic, expect_yuv(vis, bpc, api.SURFACE_SEMIPLANAR, api.SAMPLE_MSB16), api.SURFACE_SEMIPLANAR, api.SAMPLE_MSB16, "8K P010")
        export_and_check(ctx, pic, expect_rgb(vis, layout, bpc, 1, 0), api.SURFACE_RGB_PLANAR, api.SAMPLE_NATIVE, "8K RGB")
        assert pic.pic.twin_ok == api.TWIN_ONLY
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 9. torch (GPU only)

def _torch_child():
    """(runs in a process of its own: torch brings its own HIP runtime, which has to come up before the library's in a process, the order
    bench.py uses; the pytest process has long opened the device through the library)"""
    import torch
    w, h, bpc, layout = 190, 102, 10, api.LAYOUT_I420
    stream = torch.cuda.current_stream().cuda_stream
    tctx = api.Context(0, stream=stream)
    rng = np.random.default_rng(7200 + bpc + 3 * layout)
    pic, vis = make_source(tctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    t = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    api.export_to_tensor(pic, t, matrix=1, full_range=0)
    tctx.sync()
    got = t.cpu().numpy()
    want = expect_rgb(vis, layout, bpc, 1, 0, api.SAMPLE_F32)
    for k in range(3):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), "RGB float tensor, plane %d" % k
    y = torch.empty((h, w), dtype=torch.int16, device="cuda")
    uv = torch.empty(((h + 1) // 2, 2 * ((w + 1) // 2)), dtype=torch.int16, device="cuda")
    api.export_to_tensor(pic, y, chroma=uv, sample=api.SAMPLE_MSB16)
    tctx.sync()
    p010 = expect_yuv(vis, bpc, api.SURFACE_SEMIPLANAR, api.SAMPLE_MSB16)
    assert np.array_equal(y.cpu().numpy().view(np.uint16), p010[0]) and np.array_equal(uv.cpu().numpy().view(np.uint16), p010[1]), "P010 tensors"
    assert pic.pic.twin_ok == api.TWIN_ONLY
    pic.free()
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_to_tensor():
    """export_to_tensor into torch.empty((3, h, w), float32, "cuda") with the context opened on torch's current stream equals the RGB
    expectation of test_rgb_matches_the_integer_formula for the same planes; a P010 pair of int16 tensors likewise"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 10. hygiene

def test_no_object_is_left_behind(ctx):
    def live():
        out = (C.c_longlong * 4)()
        assert ctx.lib.dav1d_hip_live_objects(out) == 0
        return list(out)
    before = live()
    pic, vis = make_source(ctx, np.random.default_rng(7900), 64, 64, api.LAYOUT_I420, 10, "retiled")
    s = ctx.surface(64, 64, api.LAYOUT_I420, 10, api.SURFACE_SEMIPLANAR, api.SAMPLE_MSB16)
    pic.export(s)
    got = s.download()
    assert ctx.last_kernel_ms() >= 0.0
    want = expect_yuv(vis, 10, api.SURFACE_SEMIPLANAR, api.SAMPLE_MSB16)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    s.free()
    pic.free()
    assert live() == before


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
