"""Batched linear-light tensor export: dav1d_hip_surface_export_rgb_linear_reduced_batch (dav1d_amd/csrc/surface_linear.hip).

For every item the call must write the bytes, at the addresses, that dav1d_hip_surface_export_rgb_linear_reduced writes for it over the whole surface,
and no other byte.  The expectation is test_surface_linear.want_of; every comparison is exact, every destination is filled with 0xA5 first and compared
byte by byte, padding and the gaps between the items of a shared buffer included.  Every case with `ctx` runs on the emulated build and, under -m gpu,
on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_surface_colour as tc
import test_surface_linear as ln
from dav1d_amd import api
from dav1d_amd._lib import Picture, RgbParams, SURFACE_BATCH_MAX
from dav1d_amd._lib import Surface as SurfaceDesc
from test_surface import Dest
from test_surface_batch import Shared
from test_surface_rgb_scaled import even_crop, same_bytes
from util import make_source

EINVAL, ENOTSUP = 22, 95
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16
f32 = np.float32
N_BATCH_STAGE = 4          # the staging slots of a context (dav1d_amd/csrc/capi.h)


class Item:
    def __init__(self, pic, vis, crop, size):
        self.pic, self.vis, self.size = pic, vis, size
        self.crop = even_crop(crop, pic.layout) if crop is not None else None

    @property
    def rect(self):
        return self.crop if self.crop is not None else (0, 0, self.pic.w, self.pic.h)

    def kind(self):
        """per axis: 2 down past 8:1, else -1 / 0 / 1: down / nowhere / up"""
        r = self.rect
        return tuple(2 if s > 8 * d else (d > s) - (d < s) for s, d in ((r[2], self.size[0]), (r[3], self.size[1])))

    def want(self, fmt, sample, pos, tables, **kw):
        return ln.want_of(self.vis, self.pic.layout, self.pic.bpc, self.size[0], self.size[1], self.crop, fmt, sample, pos, tables, **kw)

    def dest(self, ctx, fmt, sample, **kw):
        return Dest(ctx, self.size[0], self.size[1], self.pic.layout, self.pic.bpc, fmt, sample, **kw)


def run_and_check(ctx, items, colour, tables, fmt, sample, pos, scale=None, bias=None, what="", single=False):
    """one batch into a Dest per item; every Dest is checked against the expectation and (`single`) against the single call's bytes"""
    dests = [it.dest(ctx, fmt, sample) for it in items]
    try:
        ctx.export_rgb_linear_reduced_batch([d.surface for d in dests], [it.pic for it in items], colour, [it.rect for it in items], pos, scale, bias)
        kw = {} if scale is None else dict(scale=scale, bias=bias)
        for k, (it, d) in enumerate(zip(items, dests)):
            d.check(it.want(fmt, sample, pos, tables, **kw), what="%s item %d of %d: %dx%d crop %s -> %s, %d bpc layout %d format %d sample %d chroma_pos %d"
                    % (what, k, len(items), it.pic.w, it.pic.h, it.crop, it.size, it.pic.bpc, it.pic.layout, fmt, sample, pos))
            if single:
                one = it.dest(ctx, fmt, sample)
                it.pic.export_rgb_linear_reduced(one.surface, colour, it.crop, pos, scale, bias)
                same_bytes(one, d)
                one.free()
    finally:
        for d in dests:
            d.free()


def mixed_items(a, b, c):
    """items over 8:1, under it, at d == s and going up in one table; a 1 x 1 target; repeated sources; another layout of the same depth"""
    return [Item(*a, None, (30, 11)),                           # over 8:1 on both axes
            Item(*a, None, (95, 51)),                           # under it
            Item(*a, (20, 10, 64, 90), (112, 9)),               # up across, 10:1 down
            Item(*b, None, (264, 40)),                          # exactly 8x up, another picture
            Item(*a, (14, 14, 300, 12), (7, 40)),               # 42.9:1 across, up down
            Item(*c, None, (64, 64)),                           # the picture's own size; another layout: another instance of the kernel
            Item(*c, None, (3, 5)),                             # ... reduced
            Item(*a, (10, 6, 133, 71), (133, 71)),              # d == s from a crop of odd size
            Item(*a, (0, 0, 256, 102), (1, 1)),                 # 256:1 across to 1 x 1
            Item(*a, (0, 0, 80, 3), (4, 4)),                    # 20:1 across, up down
            Item(*b, None, (33, 12))]                           # up down only


# ------------------------------------------------------------------------------------------------ 1. a mixed batch is its single calls

@pytest.mark.parametrize("layout", [I400, I420, I422, I444], ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_a_mixed_batch_is_its_single_calls(ctx, bpc, layout):
    rng = np.random.default_rng(32100 + 10 * bpc + layout)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    other_layout = I420 if layout == I444 else I444
    a = make_source(ctx, rng, 330, 102, layout, bpc, "raster", extremes=True)
    b = make_source(ctx, rng, 33, 5, layout, bpc, "raster")
    c = make_source(ctx, rng, 64, 64, other_layout, bpc, "raster")
    try:
        items = mixed_items(a, b, c)
        assert {it.kind() for it in items} >= {(2, 2), (-1, -1), (1, 2), (1, 1), (2, 1), (0, 0), (0, 1)}
        for k, (fmt, sample, pos, norm) in enumerate([(P, F32, 0, False), (K3, F16, 2, True), (K4, F16, 1, True)]):
            scale, bias = ([f32(2), f32(0.5), f32(1)], [f32(-1), f32(0.25), f32(0)]) if norm else (None, None)
            run_and_check(ctx, items, colour, tables, fmt, sample, pos, scale, bias, what="mixed batch", single=k == 2)
    finally:
        ctx.sync()
        for pic, _ in (a, b, c):
            pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("bpc", [8, 10])
def test_mixed_picture_states_and_layouts(ctx, bpc):
    """raster, twin-only and retiled pictures of two layouts interleaved in one batch (a launch per state and subsampling present); no picture changes
    its state"""
    rng = np.random.default_rng(32200 + bpc)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    states = ["raster", "twin-only", "retiled", "twin-only", "raster", "retiled", "twin-only", "raster"]
    srcs = {(s, l): make_source(ctx, rng, 330, 102, l, bpc, s) for s in set(states) for l in (I420, I422)}
    geoms = [(None, (30, 11)), (None, (21, 9)), ((14, 14, 300, 12), (7, 40)), ((20, 10, 64, 90), (112, 56)), (None, (165, 51)),
             (None, (330, 102)), ((0, 0, 80, 3), (4, 4)), ((0, 0, 256, 102), (1, 1))]
    try:
        items = [Item(*srcs[s, I422 if k % 3 == 1 else I420], crop, size) for k, (s, (crop, size)) in enumerate(zip(states, geoms))]
        before = {k: (v[0].pic.twin_ok, [v[0].pic.twin[pl] for pl in range(3)]) for k, v in srcs.items()}
        run_and_check(ctx, [it for it in items if it.pic.pic.twin_ok == api.TWIN_ONLY], colour, tables, P, F32, 1, what="twin-only alone")
        run_and_check(ctx, items, colour, tables, K4, F16, 1, [f32(2), f32(0.5), f32(1)], [f32(-1), f32(0.25), f32(0)], what="mixed states")
        ms = ctx.last_kernel_ms()          # (the emulator has no clock)
        assert ms > 0.0 if ctx.backend == "hip" else ms >= 0.0
        assert {k: (v[0].pic.twin_ok, [v[0].pic.twin[pl] for pl in range(3)]) for k, v in srcs.items()} == before
    finally:
        ctx.sync()
        for pic, _ in srcs.values():
            pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 2. one source, many crops, one buffer

@pytest.mark.parametrize("fmt,sample", [(P, F32), (K4, F16)], ids=["n3hw", "nhw4"])
def test_one_source_many_crops_one_buffer(ctx, fmt, sample):
    """7 crops of one picture into slices of one buffer laid out as (7, 3, h, w) / (7, h, w, 4) with a batch stride larger than an image: the bytes
    between and around the items stay sentinel"""
    (w, h), (dw, dh), bpc, layout = (330, 102), (13, 9), 10, I420
    crops = [(0, 0, 330, 102), (10, 6, 133, 91), (64, 8, 20, 94), (2, 2, 13, 9), (0, 0, 300, 12), (100, 50, 2, 2), (30, 0, 118, 100)]
    rng = np.random.default_rng(32300)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    sh = Shared(ctx, len(crops), dw, dh, layout, bpc, fmt, sample, gap=40)
    try:
        ctx.export_rgb_linear_reduced_batch(sh.surfaces, [pic] * len(crops), colour, crops, 1)
        sh.check([ln.want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, 1, tables) for crop in crops], what="seven crops, one buffer")
        assert pic.pic.twin_ok == api.TWIN_ONLY
    finally:
        sh.free()
        pic.free()
        ctx.colour_destroy(colour)


def test_one_item_and_null_arguments(ctx):
    (w, h), crop, (dw, dh), bpc, layout = (330, 102), (14, 14, 300, 80), (21, 7), 10, I420
    rng = np.random.default_rng(32400)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    a, b, c = (Dest(ctx, dw, dh, layout, bpc, K4, F16) for _ in range(3))
    whole_a, whole_b = Dest(ctx, 33, 10, layout, bpc, K4, F16), Dest(ctx, 33, 10, layout, bpc, K4, F16)
    try:
        pic.export_rgb_linear_reduced(a.surface, colour, crop, 2)
        ctx.export_rgb_linear_reduced_batch([b.surface], [pic], colour, [crop], 2)
        same_bytes(a, b)
        pic.export_rgb_linear_reduced(whole_a.surface, colour, None, 2)
        ctx.export_rgb_linear_reduced_batch([whole_b.surface], [pic], colour, None, 2)          # crop == NULL: every item whole
        same_bytes(whole_a, whole_b)
        src = (C.POINTER(Picture) * 1)(C.pointer(pic.pic))
        rect = api.SurfaceRect(*crop)
        assert ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced_batch(ctx.h, 1, C.byref(c.surface.desc), src, C.byref(rect), None, colour, 0, None) == 0
        c.check(ln.want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 0, tables), what="params == NULL")
    finally:
        for d in (a, b, c, whole_a, whole_b):
            d.free()
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 3. calls back to back

def test_calls_back_to_back(ctx):
    """more calls than the staging ring has slots, every one with another item table, no sync between them"""
    bpc, layout = 10, I444
    rng = np.random.default_rng(32500)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    a = make_source(ctx, rng, 330, 102, layout, bpc, "twin-only")
    b = make_source(ctx, rng, 2040, 48, layout, bpc, "raster")
    try:
        tables_ = [[Item(*a, None, (30, 11)), Item(*a, None, (95, 51)), Item(*a, (20, 10, 64, 90), (112, 9))],
                   [Item(*b, None, (2040, 8))] * 3,
                   [Item(*a, (14, 14, 300, 12), (7, 40)), Item(*b, (8, 0, 2032, 48), (8, 8))],
                   [Item(*a, None, (21, 9))],
                   [Item(*b, None, (257, 8)), Item(*a, (0, 0, 256, 102), (1, 1))],
                   [Item(*a, (0, 0, 80, 3), (4, 4)), Item(*a, None, (30, 11)), Item(*b, (8, 0, 2032, 48), (8, 3))]]
        assert len(tables_) > N_BATCH_STAGE
        dests = [[it.dest(ctx, K4, F16) for it in t] for t in tables_]
        ctx.sync()
        for t, ds in zip(tables_, dests):
            ctx.export_rgb_linear_reduced_batch([d.surface for d in ds], [it.pic for it in t], colour, [it.rect for it in t], 1)
        for k, (t, ds) in enumerate(zip(tables_, dests)):
            for it, d in zip(t, ds):
                d.check(it.want(K4, F16, 1, tables), what="call %d of %d back to back" % (k, len(tables_)))
                d.free()
    finally:
        a[0].free()
        b[0].free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 4. refusals

class RawBatch:
    """the C call on arrays of the test's own, so that a test can damage any field"""

    def __init__(self, ctx, colour, pics, sizes, fmts, samples, crops=None):
        self.ctx, self.n, self.colour = ctx, len(pics), colour
        self.dests = [Dest(ctx, s[0], s[1], p.layout, p.bpc, f, sm) for p, s, f, sm in zip(pics, sizes, fmts, samples)]
        self.dst = (SurfaceDesc * self.n)(*[d.surface.desc for d in self.dests])
        self.src = (C.POINTER(Picture) * self.n)(*[C.pointer(p.pic) for p in pics])
        self.crop = (api.SurfaceRect * self.n)(*[api.SurfaceRect(*c) for c in crops]) if crops is not None else None

    def call(self, params=None, n=None, with_bad=True, dst=True, src=True, flt=0, colour="own"):
        bad = C.c_int(-7)
        rc = self.ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced_batch(self.ctx.h, self.n if n is None else n, self.dst if dst else None, self.src if src else None,
                                                                           self.crop, C.byref(params) if params is not None else None,
                                                                           self.colour if colour == "own" else colour, flt, C.byref(bad) if with_bad else None)
        return rc, bad.value

    def refused(self, code, bad_item, what, **kw):
        """the code and *bad_item; the same code with bad_item == NULL; every destination of the batch still holds the sentinel only"""
        rc, bad = self.call(**kw)
        assert (rc, bad) == (-code, bad_item), (what, rc, bad, code, bad_item)
        rc, _ = self.call(with_bad=False, **kw)
        assert rc == -code, (what, rc)
        for d in self.dests:
            d.check(None, what="a refused batch: " + what)

    def free(self):
        for d in self.dests:
            d.free()


def test_refusals(ctx):
    w, h = 514, 102
    rng = np.random.default_rng(32600)
    pic = make_source(ctx, rng, w, h, I420, 10, "raster")[0]
    pic8 = make_source(ctx, rng, w, h, I420, 8, "raster")[0]
    pic12 = make_source(ctx, rng, w, h, I420, 12, "raster")[0]
    tall = make_source(ctx, rng, 64, 514, I420, 10, "raster")[0]
    colour = ctx.colour(*tc.random_tables(rng, 10), bpc=10)
    colour8 = ctx.colour(*tc.random_tables(rng, 8), bpc=8)
    neg = tc.random_tables(rng, 10)[0]
    neg[100] = -neg[100]
    no_q = ctx.colour(neg, bpc=10)
    whole, good = (0, 0, w, h), (30, 200)          # 17:1 across, up down

    def set_stride(desc):
        desc.stride[0] = desc.stride[0] - 2

    def null_plane(desc):
        desc.data[0] = None
    item_faults = [("ratio above 256 across", ENOTSUP, (2, 200), whole, None, pic), ("ratio above 256 down", ENOTSUP, (64, 2), (0, 0, 64, 514), None, tall),
                   ("odd crop origin at 4:2:0", EINVAL, good, (1, 0, 95, 51), None, pic), ("crop outside the picture", EINVAL, good, (500, 0, 100, 51), None, pic),
                   ("NULL plane pointer", EINVAL, good, whole, null_plane, pic), ("bad stride", EINVAL, good, whole, set_stride, pic),
                   ("a 12-bit picture under a 10-bit handle", EINVAL, good, whole, None, pic12), ("an 8-bit picture under a 10-bit handle", EINVAL, good, whole, None, pic8)]
    try:
        for what, code, size, crop, change, p in item_faults:
            for at in (0, 2, 4):          # at the front, in the middle, at the end
                sizes, crops, pics = [good] * 5, [whole] * 5, [pic] * 5
                sizes[at], crops[at], pics[at] = size, crop, p
                b = RawBatch(ctx, colour, pics, sizes, [K3] * 5, [F16] * 5, crops)
                if change:
                    change(b.dst[at])
                b.refused(code, at, "%s at item %d" % (what, at))
                b.free()
        b = RawBatch(ctx, colour, [pic] * 5, [good, good, (2, 200), good, good], [K3] * 5, [F16] * 5, [whole, whole, whole, (1, 0, 95, 51), whole])
        b.refused(ENOTSUP, 2, "two faults")
        b.free()
        b = RawBatch(ctx, colour, [pic] * 3, [good] * 3, [K3] * 3, [N] * 3)
        b.refused(EINVAL, 0, "an integer sample")
        b.refused(EINVAL, 0, "scale with a native sample", params=RgbParams(1, 1, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)))
        b.free()
        b = RawBatch(ctx, colour, [pic] * 3, [good] * 3, [K3] * 3, [F16] * 3)
        b.refused(EINVAL, 0, "chroma_pos 3", params=RgbParams(3, 0))
        b.refused(EINVAL, 0, "a handle of another depth", colour=colour8)
        b.refused(EINVAL, 0, "a handle without q", colour=no_q)
        # the call as a whole
        b.refused(EINVAL, -1, "n < 0", n=-1)
        b.refused(EINVAL, -1, "n > MAX", n=SURFACE_BATCH_MAX + 1)
        b.refused(EINVAL, -1, "NULL dst", dst=False)
        b.refused(EINVAL, -1, "NULL src", src=False)
        b.refused(EINVAL, -1, "a NULL colour", colour=None)
        b.refused(EINVAL, -1, "a NULL colour with n == 0", colour=None, n=0)
        b.refused(EINVAL, -1, "a NULL colour in front of a NULL dst", colour=None, dst=False)
        for flt in (1, -1):
            b.refused(ENOTSUP, -1, "an unknown filter", flt=flt)
            b.refused(EINVAL, -1, "an unknown filter behind n < 0", flt=flt, n=-1)
            b.refused(ENOTSUP, -1, "an unknown filter in front of a NULL dst", flt=flt, dst=False)
            b.refused(ENOTSUP, -1, "an unknown filter in front of a NULL colour", flt=flt, colour=None)
        assert ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced_batch(None, 3, b.dst, b.src, None, None, colour, 0, None) == -EINVAL
        for at in (0, 1, 2):
            b.src[at] = C.POINTER(Picture)()
            b.refused(EINVAL, at, "NULL src[%d]" % at)
            b.refused(EINVAL, -1, "a NULL colour in front of a NULL src[%d]" % at, colour=None)
            b.src[at] = C.pointer(pic.pic)
        # n == 0 returns 0 and writes nothing, with or without arrays
        assert b.call(n=0) == (0, -1) and b.call(n=0, dst=False, src=False) == (0, -1)
        for d in b.dests:
            d.check(None, what="n == 0")
        assert b.call(params=RgbParams(1, 0)) == (0, -1)          # ... and the same arrays with nothing wrong are accepted
        ctx.sync()
        b.free()
        for at in (1, 3):          # what must be uniform: the lowest item that differs from item 0
            fmts, samples = [K3] * 4, [F16] * 4
            fmts[at] = K4
            b = RawBatch(ctx, colour, [pic] * 4, [good] * 4, fmts, samples)
            b.refused(EINVAL, at, "mixed format")
            b.free()
            fmts, samples = [K3] * 4, [F16] * 4
            samples[at] = F32
            b = RawBatch(ctx, colour, [pic] * 4, [good] * 4, fmts, samples)
            b.refused(EINVAL, at, "mixed sample")
            b.free()
        # the Python layer names the item
        d = [Dest(ctx, 30, 200, I420, 10, K3, F16), Dest(ctx, 2, 200, I420, 10, K3, F16)]
        with pytest.raises(api.HipError, match=r"item 1\b.*errno %d" % ENOTSUP):
            ctx.export_rgb_linear_reduced_batch([x.surface for x in d], [pic, pic], colour)
        with pytest.raises(ValueError):
            ctx.export_rgb_linear_reduced_batch([x.surface for x in d], [pic], colour)
        with pytest.raises(ValueError):
            ctx.export_rgb_linear_reduced_batch([x.surface for x in d], [pic, pic], None)
        for x in d:
            x.check(None, what="a refused batch")
            x.free()
    finally:
        ctx.sync()
        for p in (pic, pic8, pic12, tall):
            p.free()
        for hd in (colour, colour8, no_q):
            ctx.colour_destroy(hd)


# ------------------------------------------------------------------------------------------------ 5. Python and torch

def test_python_method_against_the_c_call(ctx):
    bpc, layout = 10, I420
    rng = np.random.default_rng(32700)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    a = make_source(ctx, rng, 330, 102, layout, bpc, "retiled")
    b = make_source(ctx, rng, 33, 5, layout, bpc, "twin-only")
    items = [Item(*a, (20, 10, 300, 90), (21, 7)), Item(*b, None, (264, 40)), Item(*a, None, (165, 51))]
    scale, bias = [2.0, 1.0, 0.5], [-1.0, 0.0, 1.0]
    py = [it.dest(ctx, K4, F16) for it in items]
    raw = RawBatch(ctx, colour, [it.pic for it in items], [it.size for it in items], [K4] * 3, [F16] * 3, [it.rect for it in items])
    try:
        ctx.export_rgb_linear_reduced_batch([d.surface for d in py], [it.pic for it in items], colour, [it.rect for it in items], chroma_pos=api.CHROMA_COLOCATED,
                                            scale=scale, bias=bias, filter=api.RESIZE_BILINEAR)
        assert raw.call(params=RgbParams(2, 1, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias))) == (0, -1)
        kw = dict(scale=[f32(v) for v in scale], bias=[f32(v) for v in bias])
        for it, d, r in zip(items, py, raw.dests):
            same_bytes(d, r)
            d.check(it.want(K4, F16, 2, tables, **kw), what="Context.export_rgb_linear_reduced_batch")
    finally:
        raw.free()
        for d in py:
            d.free()
        a[0].free()
        b[0].free()
        ctx.colour_destroy(colour)


def _torch_child():
    """(a process of its own, for the reason tests/test_surface.py gives)"""
    import torch
    w, h, bpc, layout = 520, 180, 10, I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(32800)
    lin, m, enc, has_matrix, has_enc = api.colour_tables(tctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)          # PQ / BT.2020 to sRGB / BT.709
    assert has_matrix and has_enc
    tables = (lin, m.reshape(9), enc)
    colour = tctx.colour_for(bpc, 16, 9, 13, 1, 203.0, 1000.0)
    crops = [None, (20, 10, 64, 90), (14, 14, 33, 21), (0, 0, 512, 160)]
    rects = [c if c is not None else (0, 0, w, h) for c in crops]
    srcs = [make_source(tctx, rng, w, h, layout, bpc, state, extremes=True) for state in ("twin-only", "raster", "twin-only", "retiled")]
    pics = [s[0] for s in srcs]
    scale, bias = [1.0 / s for s in (0.229, 0.224, 0.225)], [-mu / s for mu, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    kw = dict(scale=[f32(v) for v in scale], bias=[f32(v) for v in bias])

    def bits(t):
        return t.cpu().numpy().view(np.uint16)

    t = torch.full((4, 3, 24, 40), 7.0, dtype=torch.float16, device="cuda")
    api.export_colour_batch_to_tensor(pics, t, colour, crops=rects, chroma_pos=api.CHROMA_VERTICAL, linear_light=True)
    tctx.sync()
    for k, (pic, vis) in enumerate(srcs):
        want = ln.want_of(vis, layout, bpc, 40, 24, crops[k], P, F16, 1, tables)
        assert all(np.array_equal(bits(t[k, c]), want[c].view(np.uint16)) for c in range(3)), "(4, 3, 24, 40) item %d" % k
    t = torch.full((4, 24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
    api.export_colour_batch_to_tensor(pics, t, colour, crops=rects, chroma_pos=api.CHROMA_VERTICAL, scale=scale, bias=bias, linear_light=True)
    tctx.sync()
    for k, (pic, vis) in enumerate(srcs):
        want = ln.want_of(vis, layout, bpc, 40, 24, crops[k], K4, F16, 1, tables, **kw)[0]
        assert np.array_equal(bits(t[k]).reshape(24, 40 * 4), want.view(np.uint16)), "(4, 24, 40, 4) item %d" % k
    for crop in (None, (0, 0, 512, 160)):
        t = torch.full((24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
        api.export_colour_to_tensor(pics[0], t, colour, crop=crop, chroma_pos=api.CHROMA_VERTICAL, scale=scale, bias=bias, linear_light=True)
        tctx.sync()
        want = ln.want_of(srcs[0][1], layout, bpc, 40, 24, crop, K4, F16, 1, tables, **kw)[0]
        assert np.array_equal(bits(t).reshape(24, 40 * 4), want.view(np.uint16)), "HWC float16 tensor, crop %s" % (crop,)
        t = torch.empty((3, 24, 40), dtype=torch.float32, device="cuda")
        api.export_colour_to_tensor(pics[0], t, colour, crop=crop, linear_light=True)
        tctx.sync()
        want = ln.want_of(srcs[0][1], layout, bpc, 40, 24, crop, P, F32, 0, tables)
        assert all(np.array_equal(t[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)) for k in range(3)), "CHW float32 tensor, crop %s" % (crop,)
    assert [p.pic.twin_ok for p in pics] == [api.TWIN_ONLY, 0, api.TWIN_ONLY, 1]
    tctx.sync()
    for pic, _ in srcs:
        pic.free()
    tctx.colour_destroy(colour)
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_colour_to_tensor_in_linear_light():
    """export_colour_batch_to_tensor and export_colour_to_tensor with linear_light=True from 520x180 PQ / BT.2020 pictures to sRGB"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
