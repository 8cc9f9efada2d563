"""Scaled tensor-ready RGB: dav1d_hip_surface_export_rgb_scaled / dav1d_hip_surface_rgb_scaled_rows_needed (dav1d_amd/csrc/surface_rgb_scale.hip).

The call must write byte for byte what dav1d_hip_surface_export_rgb writes from the picture Q whose planes are the scaled planes of
dav1d_hip_surface_export_scaled.  The expectation is numpy only and a composition of the two restatements the suite has already:
test_surface_scaled.scaled_planes (the scaler of include/dav1d_hip.h with Python integers) fed into test_surface_rgb.expect (sited chroma, packed
layouts, binary16, normalisation).  Every comparison is exact; every destination is filled with 0xA5 first and compared byte by byte, padding
included (test_surface.Dest).  Every case runs on the emulated build and, under -m gpu, on the device.

The owned chroma cell of a workgroup is cell_of() below: smaller than the scaler's where the axis is filtered, because a ring of
one scaled chroma sample per side is scaled with it; test_worst_case_windows asserts from those sizes that its cases span two cells per axis.

Nothing is thinned on the emulator.  The emulator has no clock: a positive device time is asked for on the device only."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import util
import test_surface_rgb as tr
import test_surface_scaled as tsc
from dav1d_amd import api
from dav1d_amd._lib import RgbParams
from test_surface import Dest, expect_rgb
from test_surface_scaled import CROPS, GEOMS, scaled_planes, source_from, ss_of
from util import make_source

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16


def cell_of(sw, sh, dw, dh, ss_h, ss_v, pos):
    """the owned cell of the scaled chroma planes: the scaler's 128 / 64 / 32 x 8 / 4 by ratio class, less 4 across where
    there is a ring column, and less the ring rows down: one below, at chroma_pos 1 one above as well"""
    csw, csh, cdw, cdh = (sw + ss_h) >> ss_h, (sh + ss_v) >> ss_v, (dw + ss_h) >> ss_h, (dh + ss_v) >> ss_v
    ow = 128 if csw <= 2 * cdw else 64 if csw <= 4 * cdw else 32
    oh = 8 if csh <= 4 * cdh else 4
    return ow - (4 if ss_h and pos else 0), oh - ((2 if pos == 1 else 1) if ss_v and pos else 0)


def want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, planes=None, **kw):
    planes = planes if planes is not None else scaled_planes(vis, layout, dw, dh, crop)
    return tr.expect(planes, layout, bpc, fmt, sample, pos, **kw)


def check(ctx, pic, want, dw, dh, fmt, sample, crop=None, pos=0, scale=None, bias=None, rows=(0, 1 << 30), what="", **kw):
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export_rgb_scaled(d.surface, crop, pos, scale, bias, rows[0], rows[1])
        d.check(want, what="%s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d chroma_pos %d" % (what, pic.w, pic.h, dw, dh, crop, pic.bpc, pic.layout,
                                                                                                       fmt, sample, pos))
    finally:
        d.free()


def same_bytes(a, b):
    """two destinations of one shape hold the same bytes from their 256-byte boundary on, and something was written"""
    a.ctx.sync()
    for k, (x, y) in enumerate(zip(a.bufs, b.bufs)):
        gx, gy = x.download(np.uint8), y.download(np.uint8)
        n = min(len(gx) - a.lead[k], len(gy) - b.lead[k])
        assert (gx != 0xA5).any() and np.array_equal(gx[a.lead[k]:a.lead[k] + n], gy[b.lead[k]:b.lead[k] + n]), k
        assert (gy[:b.lead[k]] == 0xA5).all() and (gy[b.lead[k] + n:] == 0xA5).all()


def even_crop(crop, layout):
    ssh, ssv = ss_of(layout)
    return (crop[0] - (crop[0] & ssh), crop[1] - (crop[1] & ssv), crop[2], crop[3])


# ------------------------------------------------------------------------------------------------ 1. the windows a ring can break

WORST = [((544, 96), (14, 14, 528, 80), (264, 20)),          # exactly 2:1 across, 4:1 down; the chroma window starts at offset 7 in both axes
         ((592, 112), (14, 14, 576, 96), (144, 24)),         # 4:1, 4:1
         ((592, 112), (14, 14, 576, 96), (72, 12))]          # 8:1, 8:1


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("case", range(3), ids=["2to1", "4to1", "8to1"])
def test_worst_case_windows(ctx, case, bpc, state):
    """cell + ring at the ratios where today's cells fill the LDS window exactly: a cell the scaler skips keeps the sentinel"""
    (w, h), crop, (dw, dh) = WORST[case]
    layout = I420
    assert (crop[0] >> 1) & 7 == 7 and (crop[1] >> 1) & 7 == 7
    pic, vis = make_source(ctx, np.random.default_rng(13000 + case + bpc), w, h, layout, bpc, state)
    try:
        planes = scaled_planes(vis, layout, dw, dh, crop)
        for pos in (1, 2):
            cw, ch = cell_of(crop[2], crop[3], dw, dh, 1, 1, pos)
            assert (cw, ch) == {1: [(124, 6), (60, 6), (28, 2)], 2: [(124, 7), (60, 7), (28, 3)]}[pos][case]
            assert planes[1].shape[1] > cw and planes[1].shape[0] > ch, "two chroma cells across and two down"
            check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, P, N, pos, planes), dw, dh, P, N, crop, pos, what="worst window " + state)
        check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 1, planes), dw, dh, K4, F16, crop, 1, what="worst window " + state)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 2. every geometry class

ALL_GEOMS = [(size, None, out) for size, out in GEOMS] + [((190, 102), crop, out) for crop, out in CROPS]


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [I400, I420, I422, I444], ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_geometry(ctx, bpc, layout, state):
    """planar native at chroma_pos 0 / 1 / 2; chroma_pos 0 is also what dav1d_hip_surface_export_scaled writes, and a sited position differs from it"""
    geoms = ALL_GEOMS
    pics = {}
    try:
        for (w, h), crop, (dw, dh) in geoms:
            if (w, h) not in pics:
                pics[w, h] = make_source(ctx, np.random.default_rng(13100 + 100 * bpc + 10 * layout + w), w, h, layout, bpc, state)
            pic, vis = pics[w, h]
            crop = even_crop(crop, layout) if crop else None
            planes = scaled_planes(vis, layout, dw, dh, crop)
            replicated = expect_rgb(planes, layout, bpc, 1, 0)
            for pos in (0, 1, 2):
                want = want_of(vis, layout, bpc, dw, dh, crop, P, N, pos, planes)
                if pos == 0:
                    assert all(np.array_equal(a, b) for a, b in zip(want, replicated))
                    a, b = Dest(ctx, dw, dh, layout, bpc, P, N), Dest(ctx, dw, dh, layout, bpc, P, N)
                    pic.export_scaled(a.surface, crop)
                    pic.export_rgb_scaled(b.surface, crop, 0)
                    same_bytes(a, b)          # chroma_pos 0 is export_scaled
                    a.free()
                    b.free()
                elif layout in (I420, I422) and dw > 8 and dh > 8:
                    assert any(not np.array_equal(a, b) for a, b in zip(want, replicated)), "the sited result is not the replicated one"
                check(ctx, pic, want, dw, dh, P, N, crop, pos, what=state)
            assert pic.pic.twin_ok == (api.TWIN_ONLY if state == "twin-only" else 0)
    finally:
        for pic, _ in pics.values():
            pic.free()


def test_same_size_is_export_rgb(ctx):
    """dst of the picture's size, NULL crop: the bytes of dav1d_hip_surface_export_rgb, library against library"""
    w, h, bpc, layout = 190, 102, 10, I420
    pic, _ = make_source(ctx, np.random.default_rng(13150), w, h, layout, bpc, "twin-only", extremes=True)
    try:
        for fmt, sample, pos in ((P, N, 1), (K3, F16, 2), (K4, F32, 1)):
            a, b = Dest(ctx, w, h, layout, bpc, fmt, sample), Dest(ctx, w, h, layout, bpc, fmt, sample)
            pic.export_rgb(a.surface, pos)
            pic.export_rgb_scaled(b.surface, None, pos)
            same_bytes(a, b)
            a.free()
            b.free()
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 3. composition on the device

CELL_CLASSES = [((190, 102), None, (95, 51)),               # up to 2:1 across, up to 4:1 down
                ((333, 77), None, (100, 12)),               # up to 4:1 across, up to 8:1 down
                ((190, 102), (10, 6, 133, 71), (24, 13))]   # up to 8:1 across


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("case", range(3), ids=["2to1", "4to1", "8to1"])
def test_composition_on_the_device(ctx, case, state):
    """export_scaled to planar native, those planes uploaded as a picture of the output size, export_rgb from it: the bytes of the one call.
    No numpy model takes part."""
    (w, h), crop, (dw, dh) = CELL_CLASSES[case]
    bpc, layout = 10, I420
    mx = (1 << bpc) - 1
    scale, bias = [1.0 / (mx * s) for s in tr.IMAGENET_STD], [-m / s for m, s in zip(tr.IMAGENET_MEAN, tr.IMAGENET_STD)]
    pic, _ = make_source(ctx, np.random.default_rng(13200 + case), w, h, layout, bpc, state, extremes=True)
    s = ctx.surface(dw, dh, layout, bpc, api.SURFACE_PLANAR, N)
    q = ctx.picture(dw, dh, layout, bpc)
    a, b = Dest(ctx, dw, dh, layout, bpc, K4, F16), Dest(ctx, dw, dh, layout, bpc, K4, F16)
    try:
        pic.export_scaled(s, crop)
        for pl, plane in enumerate(s.download()):
            padded = np.zeros(q.padded_shape(pl), q.dtype)
            padded[:plane.shape[0], :plane.shape[1]] = plane
            q.upload(pl, padded)
        q.export_rgb(a.surface, 1, scale, bias)
        pic.export_rgb_scaled(b.surface, crop, 1, scale, bias)
        same_bytes(a, b)
    finally:
        for d in (a, b, s, q, pic):
            d.free()


# ------------------------------------------------------------------------------------------------ 4. formats and samples

@pytest.mark.parametrize("fmt", [P, K3, K4], ids=["planar", "rgb", "rgba"])
@pytest.mark.parametrize("bpc", [8, 10])
def test_formats_and_samples(ctx, bpc, fmt):
    (w, h), (dw, dh), layout = (190, 102), (47, 13), I420
    mx = (1 << bpc) - 1
    imagenet = ([np.float32(1.0 / (mx * s)) for s in tr.IMAGENET_STD], [np.float32(-m / s) for m, s in zip(tr.IMAGENET_MEAN, tr.IMAGENET_STD)])
    pic, vis = make_source(ctx, np.random.default_rng(13300 + bpc), w, h, layout, bpc, "twin-only", extremes=True)
    try:
        planes = scaled_planes(vis, layout, dw, dh)
        for sample in (N, M, F32, F16):
            if sample == M and bpc == 8:
                continue
            want = want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 1, planes)
            if fmt == K4:
                alpha = {N: mx, M: mx << (16 - bpc), F32: 1.0, F16: 1.0}[sample]
                assert (want[0][:, 3::4] == alpha).all()
            check(ctx, pic, want, dw, dh, fmt, sample, None, 1, what="sample")
            if sample in (F32, F16):
                scale, bias = imagenet
                assert min(bias) < 0
                check(ctx, pic, want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 1, planes, scale=scale, bias=bias), dw, dh, fmt, sample, None, 1, scale, bias,
                      what="normalised")
    finally:
        pic.free()


@pytest.mark.parametrize("full_range", [0, 1], ids=["limited", "full"])
@pytest.mark.parametrize("matrix", [1, 5, 6, 9])
def test_matrices(ctx, matrix, full_range):
    (w, h), (dw, dh), bpc, layout = (190, 102), (60, 33), 10, I422
    crop = (10, 6, 133, 71)
    pic, vis = make_source(ctx, np.random.default_rng(13400 + matrix), w, h, layout, bpc, "raster", extremes=True)
    try:
        want = want_of(vis, layout, bpc, dw, dh, crop, K3, N, 2, matrix=matrix, full_range=full_range)
        check(ctx, pic, want, dw, dh, K3, N, crop, 2, what="matrix %d" % matrix, matrix=matrix, full_range=full_range)
    finally:
        pic.free()


@pytest.mark.parametrize("bpc", [8, 12])
def test_identity_matrix_at_444(ctx, bpc):
    (w, h), (dw, dh), layout = (190, 102), (47, 13), I444
    pic, vis = make_source(ctx, np.random.default_rng(13450 + bpc), w, h, layout, bpc, "twin-only", extremes=True)
    try:
        planes = scaled_planes(vis, layout, dw, dh)
        for fmt, sample in ((P, N), (K4, F16)):
            want = want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 1, planes, matrix=0)
            if fmt == P:
                assert np.array_equal(want[0], planes[2]) and np.array_equal(want[1], planes[0]) and np.array_equal(want[2], planes[1])      # G, B, R = Y, U, V
            check(ctx, pic, want, dw, dh, fmt, sample, None, 1, what="identity", matrix=0)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. extremal content

@pytest.mark.parametrize("size", [(95, 51), (47, 13)], ids=["half", "odd-ratio"])
@pytest.mark.parametrize("content", ["zero", "max", "columns", "rows"])
def test_extremal_content(ctx, content, size):
    """the upsampling sum and the 24-bit multiplies at their limits, 12 bits (the emulated build traps on overflow)"""
    (w, h), (dw, dh), bpc, layout = (190, 102), size, 12, I420
    mx = (1 << bpc) - 1
    fill = {"zero": lambda pl, s: np.zeros(s, np.int64), "max": lambda pl, s: np.full(s, mx, np.int64),
            "columns": lambda pl, s: np.broadcast_to((np.arange(s[1])[None, :] & 1) * mx, s),
            "rows": lambda pl, s: np.broadcast_to((np.arange(s[0])[:, None] & 1) * mx, s)}[content]
    pic, vis = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", fill)
    try:
        planes = scaled_planes(vis, layout, dw, dh)
        for pos in (1, 2):
            for full in (0, 1):
                check(ctx, pic, want_of(vis, layout, bpc, dw, dh, None, P, N, pos, planes, matrix=9, full_range=full), dw, dh, P, N, None, pos,
                      what="%s full %d" % (content, full), matrix=9, full_range=full)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 6. bands

@pytest.mark.parametrize("band", [2, 6, 16])
@pytest.mark.parametrize("fmt,sample", [(P, N), (K4, F16)], ids=["planar", "rgba-f16"])
def test_bands(ctx, fmt, sample, band):
    """destination bands at chroma_pos 1: each alone leaves every other row at the sentinel, their union equals the one call"""
    (w, h), (dw, dh), bpc, layout = (190, 102), (47, 33), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(13500), w, h, layout, bpc, "twin-only")
    want = want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 1)
    try:
        whole = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
        for r0 in range(0, dh, band):
            r1 = min(r0 + band, dh)
            d = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            pic.export_rgb_scaled(d.surface, None, 1, row0=r0, row1=r1)
            d.check(want, rows=[(r0, r1)] * len(want), what="band [%d, %d)" % (r0, r1))
            d.free()
            pic.export_rgb_scaled(whole.surface, None, 1, row0=r0, row1=r1 if r1 < dh else 1 << 30)
        whole.check(want, what="the union of the bands")
        whole.free()
    finally:
        pic.free()


@pytest.mark.parametrize("crop,size", [(None, (47, 33)), ((10, 6, 133, 71), (60, 33)), (None, (95, 51))], ids=["odd-ratio", "crop", "half"])
def test_rows_needed_is_safe_and_tight(ctx, crop, size):
    """For every band end r1: a copy of the source whose luma rows at and below rgb_scaled_rows_needed(r1), and the chroma rows under them, hold other
    values gives the same rows [0, r1); with one row fewer than the helper says at least one band of the sweep changes.  The answer is
    scaled_rows_needed of r1 + 2 rows: the chroma row below the band is scaled as well."""
    (w, h), (dw, dh), bpc, layout, pos = (190, 102), size, 10, I420, 1
    pic, vis = make_source(ctx, np.random.default_rng(13600), w, h, layout, bpc, "raster")
    padded = [v.base for v in vis]
    want = want_of(vis, layout, bpc, dw, dh, crop, K3, N, pos)
    surface = Dest(ctx, dw, dh, layout, bpc, K3, N)
    planar = Dest(ctx, dw, dh, layout, bpc, P, N)
    tight = False
    try:
        last = 0
        for r1 in list(range(6, dh, 6)) + [dh]:
            need = pic.rgb_scaled_rows_needed(surface.surface, crop, pos, r1)
            assert last <= need <= h
            last = need
            assert need == pic.scaled_rows_needed(planar.surface, crop, min(dh, r1 + 2))
            assert pic.rgb_scaled_rows_needed(surface.surface, crop, 0, r1) == pic.scaled_rows_needed(planar.surface, crop, r1)
            for rows, same in ((need, True), (need - 1, False)):
                other = [p.copy() for p in padded]
                other[0][rows:] ^= 0x155
                for pl in (1, 2):          # safe: the chroma rows wholly below; tight: from the chroma row that luma row `rows` belongs to (the answer can be chroma's)
                    other[pl][(rows + 1) >> 1 if same else rows >> 1:] ^= 0x155
                pic2, _ = source_from(ctx, other, w, h, layout, bpc, "twin-only")
                d = Dest(ctx, dw, dh, layout, bpc, K3, N)
                pic2.export_rgb_scaled(d.surface, crop, pos, row0=0, row1=r1)
                if same:
                    d.check(want, rows=[(0, r1)], what="rows below %d changed, band [0, %d)" % (rows, r1))
                else:
                    try:
                        d.check(want, rows=[(0, r1)])
                    except AssertionError:
                        tight = True
                d.free()
                pic2.free()
        assert tight, "one source row fewer never changed a band: the helper is not tight"
        assert pic.rgb_scaled_rows_needed(surface.surface, crop, pos, 0) == 0
    finally:
        surface.free()
        planar.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 7. unaligned destinations

@pytest.mark.parametrize("pad", [0, 2, 10])
@pytest.mark.parametrize("offset", [0, 2, 6])
def test_unaligned_destinations(ctx, offset, pad):
    """the sample-by-sample store path, whole units and the partial last unit (47 = 5 * 8 + 7 samples)"""
    (w, h), (dw, dh), layout = (190, 102), (47, 13), I420
    for bpc, fmt, sample in ((8, K3, N), (10, K4, F16)):
        pic, vis = make_source(ctx, np.random.default_rng(13700 + bpc), w, h, layout, bpc, "twin-only")
        try:
            check(ctx, pic, want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 2), dw, dh, fmt, sample, None, 2, pad=pad, offset=offset,
                  what="offset %d pad %d" % (offset, pad))
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 8. the source is left alone; asynchronous, timed

@pytest.mark.parametrize("state", ["twin-only", "raster"])
def test_source_untouched_and_timed(ctx, state):
    (w, h), (dw, dh), bpc, layout = (190, 102), (47, 13), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(13800), w, h, layout, bpc, state)
    try:
        raster = tsc._raster_bytes(ctx, pic)
        twin = util.twin_bytes(ctx, pic) if state == "twin-only" else None
        ptrs, ok, live = [pic.pic.twin[pl] for pl in range(3)], pic.pic.twin_ok, tsc._live(ctx)
        if state == "twin-only":
            assert (raster == 0x5A).all()
        crop = (10, 6, 133, 71)
        check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 1), dw, dh, K4, F16, crop, 1, what=state)
        ms = ctx.last_kernel_ms()
        assert ms > 0.0 if ctx.backend == "hip" else ms >= 0.0
        assert tsc._live(ctx) == live, "the call allocated an object"
        assert pic.pic.twin_ok == ok and [pic.pic.twin[pl] for pl in range(3)] == ptrs
        assert np.array_equal(tsc._raster_bytes(ctx, pic), raster)
        if twin is not None:
            assert np.array_equal(util.twin_bytes(ctx, pic), twin)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 9. errors

def test_errors(ctx):
    w, h = 190, 102
    rng = np.random.default_rng(13900)
    pics = {key: make_source(ctx, rng, w, h, key[1], key[0], "raster")[0] for key in ((10, I420), (8, I420), (10, I422), (10, I444))}

    def refused(code, fmt=K3, sample=N, size=(95, 51), crop=None, rows=(0, 1 << 30), change=None, key=(10, I420), params=None, helper=True, shape_as=None, **kw):
        pic = pics[key]
        d = Dest(ctx, size[0], size[1], key[1], key[0], shape_as[0] if shape_as else fmt, shape_as[1] if shape_as else sample, **kw)
        d.surface.desc.format, d.surface.desc.sample = fmt, sample
        if change:
            change(d.surface.desc)
        rect = C.byref(api.SurfaceRect(*crop)) if crop is not None else None
        p = C.byref(params) if params is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_rgb_scaled(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), rect, p, rows[0], rows[1])
        assert rc == -code, (rc, code, fmt, sample, crop, size, rows)
        d.check(None, what="a refused export")
        if helper:
            assert ctx.lib.dav1d_hip_surface_rgb_scaled_rows_needed(C.byref(d.surface.desc), C.byref(pic.pic), rect, p, rows[1]) == -code
        d.free()

    def setter(name, value):
        return lambda desc: setattr(desc, name, value)

    def stride(k, delta):
        def f(desc):
            desc.stride[k] = desc.stride[k] + delta
        return f

    def null_plane(k):
        def f(desc):
            desc.data[k] = None
        return f
    try:
        # what dav1d_hip_surface_export_rgb refuses
        for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, 5, -1):
            refused(EINVAL, fmt, N, shape_as=(P, N))
        for sample in (4, -1):
            refused(EINVAL, K3, sample, shape_as=(K3, N))
        for fmt in (P, K3, K4):
            refused(EINVAL, fmt, M, key=(8, I420), shape_as=(fmt, F16))             # MSB16 at 8 bpc
            for sample in (N, M):                                                  # normalisation is for float samples
                refused(EINVAL, fmt, sample, params=RgbParams(1, 1, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)))
            for pos in (-1, 3):
                refused(EINVAL, fmt, F16, params=RgbParams(pos, 0))
            refused(EINVAL, fmt, N, change=setter("w", 0))
            refused(EINVAL, fmt, N, change=null_plane(0))
            refused(EINVAL, fmt, F16, change=stride(0, -2))
            refused(EINVAL, fmt, F32, change=stride(0, +2), pad=4)
            refused(EINVAL, fmt, N, matrix=0)                                       # identity needs 4:4:4
            refused(EINVAL, fmt, N, rows=(1, 32), helper=False)                     # odd band rows
            refused(EINVAL, fmt, N, rows=(0, 33))
            for m in (2, 4, 8, 14, -1):
                refused(ENOTSUP, fmt, N, matrix=m)
        refused(EINVAL, P, N, change=null_plane(2))
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled(None, None, None, None, None, 0, 2) == -EINVAL
        # what dav1d_hip_surface_export_scaled refuses: the crop
        refused(EINVAL, crop=(100, 0, 100, 51), size=(50, 51))
        refused(EINVAL, crop=(0, 60, 95, 51))
        refused(EINVAL, crop=(-2, 0, 95, 51))
        refused(EINVAL, crop=(0, -2, 95, 51))
        refused(EINVAL, crop=(0, 0, 0, 51))
        refused(EINVAL, crop=(0, 0, 95, 0))
        refused(EINVAL, crop=(1, 0, 95, 51))
        refused(EINVAL, crop=(0, 1, 95, 51))
        refused(EINVAL, crop=(1, 0, 95, 51), key=(10, I422))
        # ... and the ratios that are not built
        refused(ENOTSUP, size=(191, 102))
        refused(ENOTSUP, size=(190, 103))
        refused(ENOTSUP, size=(23, 51))
        refused(ENOTSUP, size=(95, 12))
        refused(ENOTSUP, crop=(0, 0, 94, 51), size=(95, 51))
        # what is accepted: the same surfaces with nothing wrong, odd origins where the layout does not subsample the axis
        for key, crop, size in (((10, I420), None, (95, 51)), ((10, I422), (0, 1, 95, 51), (95, 51)), ((10, I444), (1, 1, 95, 51), (24, 13)),
                                ((8, I420), (0, 0, 184, 96), (23, 12))):
            for fmt in (P, K3, K4):
                d = Dest(ctx, size[0], size[1], key[1], key[0], fmt, F16, matrix=0 if key[1] == I444 else 6)
                pics[key].export_rgb_scaled(d.surface, crop, 2)
                assert pics[key].rgb_scaled_rows_needed(d.surface, crop, 2, 1 << 30) == (crop[1] + crop[3] if crop else h)
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
        pic = other.picture(64, 64, I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        d = Dest(ctx, 32, 32, I420, 10, K3, F16)
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, None, 0, 32) == -EXDEV
        d.check(None, what="a refused export")
        d.free()
        ctx.lib.dav1d_hip_context_use(other.h)
        pic.free()
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


def test_the_older_calls_are_what_they_were(ctx):
    """the three older export calls still refuse formats 3, 4 and sample 3, and export_scaled still writes the oracle's bytes (the scaler moved into
    the shared header)"""
    w, h, bpc, layout = 190, 102, 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(13950), w, h, layout, bpc, "twin-only")
    try:
        for fmt, sample in ((K3, N), (K4, N), (P, F16), (K4, F16)):
            for size in ((w, h), (47, 13)):
                d = Dest(ctx, size[0], size[1], layout, bpc, fmt, sample)
                desc, p = C.byref(d.surface.desc), C.byref(pic.pic)
                assert ctx.lib.dav1d_hip_surface_export(ctx.h, desc, p, 0, h) == -EINVAL
                assert ctx.lib.dav1d_hip_surface_export_grain(ctx.h, desc, p, None, 0, 0, h) == -EINVAL
                assert ctx.lib.dav1d_hip_surface_export_scaled(ctx.h, desc, p, None, 0, h) == -EINVAL
                assert ctx.lib.dav1d_hip_surface_scaled_rows_needed(desc, p, None, h) == -EINVAL
                d.check(None, what="a refused export")
                d.free()
        for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, P):
            tsc.check_scaled(ctx, pic, vis, 47, 13, fmt, N, crop=(10, 6, 133, 71), what="export_scaled")
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 10. Python

def test_python_methods(ctx):
    (w, h), (dw, dh), bpc, layout = (190, 102), (96, 54), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(14000), w, h, layout, bpc, "retiled")
    s = ctx.surface(dw, dh, layout, bpc, K4, F16)
    try:
        s.fill(0xA5)
        crop = (10, 6, 133, 71)
        pic.export_rgb_scaled(s, crop=crop, chroma_pos=api.CHROMA_COLOCATED, scale=[2.0, 1.0, 0.5], bias=[-1.0, 0.0, 1.0])
        got = s.download()[0]
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 2, scale=[np.float32(v) for v in (2.0, 1.0, 0.5)], bias=[np.float32(v) for v in (-1.0, 0.0, 1.0)])[0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        planar = ctx.surface(dw, dh, layout, bpc, P, N)
        assert pic.rgb_scaled_rows_needed(s, crop, 1, 1 << 30) == pic.scaled_rows_needed(planar, crop, 1 << 30) == 78      # (the odd crop's last chroma row)
        assert pic.rgb_scaled_rows_needed(s, crop, 0, 10) == pic.scaled_rows_needed(planar, crop, 10)
        assert pic.rgb_scaled_rows_needed(s, crop, 1, 10) == pic.scaled_rows_needed(planar, crop, 12)
        planar.free()
        assert pic.rgb_scaled_rows_needed(s, crop, 1, 10) > pic.rgb_scaled_rows_needed(s, crop, 0, 10)
        with pytest.raises(api.HipError):
            pic.rgb_scaled_rows_needed(s, (1, 0, 95, 51), 1, 10)
    finally:
        s.free()
        pic.free()


def _torch_child():
    """(a process of its own, for the reason tests/test_surface.py gives)"""
    import torch
    w, h, bpc, layout = 190, 102, 10, I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    pic, vis = make_source(tctx, np.random.default_rng(14100), w, h, layout, bpc, "twin-only", extremes=True)
    mx = (1 << bpc) - 1
    scale, bias = [1.0 / (mx * s) for s in tr.IMAGENET_STD], [-m / s for m, s in zip(tr.IMAGENET_MEAN, tr.IMAGENET_STD)]
    f32 = dict(scale=[np.float32(v) for v in scale], bias=[np.float32(v) for v in bias])
    for crop in (None, (10, 6, 133, 71)):
        t = torch.full((54, 96, 4), 7.0, dtype=torch.float16, device="cuda")
        api.export_to_tensor(pic, t, matrix=1, full_range=0, crop=crop, resize=True, chroma_pos=api.CHROMA_VERTICAL, scale=scale, bias=bias)
        tctx.sync()
        want = want_of(vis, layout, bpc, 96, 54, crop, K4, F16, 1, **f32)[0]
        assert np.array_equal(t.cpu().numpy().reshape(54, 96 * 4).view(np.uint16), want.view(np.uint16)), "HWC float16 tensor, crop %s" % (crop,)
        t = torch.empty((3, 54, 96), dtype=torch.float16, device="cuda")
        api.export_to_tensor(pic, t, crop=crop, resize=True, scale=scale, bias=bias)
        tctx.sync()
        want = want_of(vis, layout, bpc, 96, 54, crop, P, F16, 0, **f32)
        assert all(np.array_equal(t[k].cpu().numpy().view(np.uint16), want[k].view(np.uint16)) for k in range(3)), "CHW float16 tensor, crop %s" % (crop,)
    grain = tctx.fg_prepare(__import__("test_filmgrain").random_fg(np.random.default_rng(1), bpc, 0), bpc, layout)
    try:
        api.export_to_tensor(pic, torch.empty((54, 96, 4), dtype=torch.float16, device="cuda"), resize=True, grain=grain)
    except ValueError:
        pass
    else:
        raise AssertionError("grain with resize was accepted")
    tctx.fg_grain_destroy(grain)
    assert pic.pic.twin_ok == api.TWIN_ONLY
    pic.free()
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_to_tensor_resized_rgbx():
    """export_to_tensor(resize=True) into a (54, 96, 4) and a (3, 54, 96) float16 tensor from a 190x102 picture, with crop= and scale / bias; grain
    with resize still raises"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 11. the binding

def test_the_glue_call_sequence_leaves_no_object(ctx):
    """The library calls of dav1d_hip_glue_output_rgb_scaled, in its order (the function itself needs a decoder around it): NULL params with an
    unknown chroma site mean chroma_pos 1, dav1d_hip_surface_export_rgb_scaled over rows [0, dst->h), dav1d_hip_sync.  No grain, nothing allocated."""
    (w, h), (dw, dh), bpc, layout = (190, 102), (47, 13), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(14200), w, h, layout, bpc, "twin-only")
    d = Dest(ctx, dw, dh, layout, bpc, K4, F16)
    before = tsc._live(ctx)
    try:
        crop = api.SurfaceRect(10, 6, 133, 71)
        p = RgbParams(1, 0)
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), C.byref(crop), C.byref(p), 0, dh) == 0
        ctx.sync()
        assert tsc._live(ctx) == before
        d.check(want_of(vis, layout, bpc, dw, dh, (10, 6, 133, 71), K4, F16, 1), what="the glue's calls")
    finally:
        d.free()
        pic.free()


REF = "/root/reference"
INC = os.path.join(util.ROOT, "oracle", "_ref", "inc")


@pytest.mark.skipif(not os.path.isdir(REF) or not os.path.isdir(INC), reason="needs the reference tree and oracle/_ref (built by __graft_entry__.build())")
def test_glue_compiles_against_the_reference_headers(tmp_path):
    """tests/test_integration_glue.py's method on the binding itself: syntax and types against the reference's own headers, and a caller of the
    new function"""
    host = os.path.join(util.ROOT, "dav1d_amd", "host")
    f = tmp_path / "use.c"
    f.write_text('#include "%s"\n' % os.path.join(host, "dav1d_glue.c") +
                 "int use(Dav1dHipGlue *g, const Dav1dPicture *pic, const Dav1dHipSurface *dst) {\n"
                 "    const Dav1dHipSurfaceRect crop = { 0, 0, pic->p.w & ~1, pic->p.h & ~1 };\n"
                 "    return dav1d_hip_glue_output_rgb_scaled(g, pic, dst, &crop, NULL);\n}\n")
    # ... and the "Output on the device" snippet of INTEGRATION.md, which shows the call, as the body of a function
    text = open(os.path.join(util.ROOT, "INTEGRATION.md")).read()
    snippet = next(b for b in re.findall(r"```c\n(.*?)```", text, re.S) if "dav1d_hip_glue_output_rgb_scaled" in b)
    assert "dav1d_hip_surface_export_rgb_scaled(ctx, &tin, filtered, &crop, &np, drow0, drow1);" in snippet
    with open(f, "a") as out:
        out.write("void snippet(Dav1dHipGlue *g, Dav1dPicture pic, Dav1dHipContext *ctx, const Dav1dHipPicture *filtered, const Dav1dHipGrain *grain, int is_id,\n"
                  "             void *dev_y, void *dev_uv, void *dev_r, void *dev_g, void *dev_b, void *dev_rgba, void *dev_in, Dav1dHipSurface small,\n"
                  "             int row0, int row1, int drow0, int drow1, float sr, float sg, float sb, float br, float bg, float bb) {\n" + snippet + "}\n")
    cmd = ["gcc", "-std=gnu11", "-D_GNU_SOURCE", "-fsyntax-only", "-Wall", "-Werror", "-I" + INC, "-I" + REF, "-I" + os.path.join(REF, "include"),
           "-I" + os.path.join(REF, "include", "dav1d"), "-I" + os.path.join(REF, "src"), "-I" + host, "-I" + os.path.join(util.ROOT, "include"), str(f)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


if __name__ == "__main__":
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
