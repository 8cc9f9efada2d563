"""Batched tensor export: dav1d_hip_surface_export_rgb_scaled_batch (dav1d_amd/csrc/surface_batch.hip).

For every item the call must write the bytes, at the addresses, that dav1d_hip_surface_export_rgb_scaled writes for it, and no other byte.  The
expectation is the numpy restatement the suite has already (test_surface_rgb_scaled.want_of: the scaler with Python integers fed into the RGB
restatement); every comparison is exact, every destination is filled with 0xA5 first and compared byte by byte, padding and the gaps between the
items of a shared buffer included.  Every case runs on the emulated build and, under -m gpu, on the device.

How many workgroups an item takes is groups_of() below, from test_surface_rgb_scaled.cell_of: the cases of section 4
assert from it that they are what they claim to be."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import util
import test_surface_rgb as tr
from dav1d_amd import api
from dav1d_amd._lib import Picture, RgbParams, SURFACE_BATCH_MAX
from dav1d_amd._lib import Surface as SurfaceDesc
from test_surface import Dest
from test_surface_rgb_scaled import WORST, cell_of, even_crop, same_bytes, want_of
from test_surface_scaled import CROPS, GEOMS, scaled_planes, ss_of
from util import make_source

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16
SENTINEL = 0xA5


def imagenet(bpc):
    mx = (1 << bpc) - 1
    return [np.float32(1.0 / (mx * s)) for s in tr.IMAGENET_STD], [np.float32(-m / s) for m, s in zip(tr.IMAGENET_MEAN, tr.IMAGENET_STD)]


def groups_of(crop, size, layout, pos):
    """workgroups of one item: the cells (cell_of) that tile the scaled chroma planes (the luma plane at 4:0:0)"""
    ssh, ssv = ss_of(layout)
    cw, ch = cell_of(crop[2], crop[3], size[0], size[1], ssh, ssv, pos)
    cdw, cdh = (size[0] + ssh) >> ssh, (size[1] + ssv) >> ssv
    return -(-cdw // cw) * -(-cdh // ch)


class Item:
    def __init__(self, pic, vis, crop, size):
        self.pic, self.vis, self.size = pic, vis, size
        self.crop = even_crop(crop, pic.layout) if crop is not None else None
        self._planes = None

    @property
    def rect(self):
        return self.crop if self.crop is not None else (0, 0, self.pic.w, self.pic.h)

    def want(self, fmt, sample, pos, **kw):
        if self._planes is None:
            self._planes = scaled_planes(self.vis, self.pic.layout, self.size[0], self.size[1], self.crop)
        return want_of(self.vis, self.pic.layout, self.pic.bpc, self.size[0], self.size[1], self.crop, fmt, sample, pos, self._planes, **kw)

    def dest(self, ctx, fmt, sample, **kw):
        return Dest(ctx, self.size[0], self.size[1], self.pic.layout, self.pic.bpc, fmt, sample, **kw)


def run_and_check(ctx, items, fmt, sample, pos, scale=None, bias=None, what=""):
    """one batch into a Dest per item; every Dest is checked against the numpy expectation"""
    dests = [it.dest(ctx, fmt, sample) for it in items]
    try:
        ctx.export_rgb_scaled_batch([d.surface for d in dests], [it.pic for it in items], [it.rect for it in items], pos, scale, bias)
        kw = {} if scale is None else dict(scale=scale, bias=bias)
        for k, (it, d) in enumerate(zip(items, dests)):
            d.check(it.want(fmt, sample, pos, **kw), what="%s item %d of %d: %dx%d crop %s -> %s, %d bpc layout %d format %d sample %d chroma_pos %d"
                    % (what, k, len(items), it.pic.w, it.pic.h, it.crop, it.size, it.pic.bpc, it.pic.layout, fmt, sample, pos))
    finally:
        for d in dests:
            d.free()


# ------------------------------------------------------------------------------------------------ 1. a mixed batch is its single calls

def combos(bpc):
    out = [(P, N, 0, False), (P, N, 1, False), (P, N, 2, False), (K3, N, 1, False), (K4, F16, 1, True), (P, F32, 2, False)]
    return out + ([(P, M, 1, False)] if bpc > 8 else [])


@pytest.mark.parametrize("layout", [I400, I420, I422, I444], ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_a_mixed_batch_is_its_single_calls(ctx, bpc, layout):
    """different pictures, sizes, crops, all three ratio classes, the picture's own size, a 1-column and a 1-row output in ONE batch; one source has
    another layout (4:4:4 among 4:2:0 and the like) and, at 16 bits, the other bit depth: 1 / max, the MSB16 shift and alpha are the item's own"""
    rng = np.random.default_rng(15000 + 10 * bpc + layout)
    other_layout, other_bpc = (I420 if layout == I444 else I444), {8: 8, 10: 12, 12: 10}[bpc]
    a = make_source(ctx, rng, 190, 102, layout, bpc, "raster", extremes=True)
    b = make_source(ctx, rng, 333, 77, layout, bpc, "raster")
    c = make_source(ctx, rng, 64, 64, other_layout, other_bpc, "raster")
    try:
        assert GEOMS[0] == ((190, 102), (95, 51)) and GEOMS[1] == ((190, 102), (47, 13)) and GEOMS[3] == ((333, 77), (42, 10)) and GEOMS[6] == ((64, 64), (32, 32))
        items = [Item(*a, None, (95, 51)),                  # up to 2:1
                 Item(*b, None, (42, 10)),                  # up to 8:1, another picture
                 Item(*a, *CROPS[0]),                       # (10, 6, 133, 71) -> (60, 33): up to 4:1
                 Item(*c, None, (32, 32)),                  # another layout, another depth
                 Item(*a, None, (190, 102)),                # the picture's own size
                 Item(*a, *CROPS[2]),                       # a 1-column output
                 Item(*a, None, (47, 13)),
                 Item(*a, *CROPS[3]),                       # a 1-row output
                 Item(*a, *CROPS[1]),
                 Item(*a, *CROPS[5])]
        assert items[5].size[0] == 1 and items[7].size[1] == 1
        classes = {cell_of(it.rect[2], it.rect[3], it.size[0], it.size[1], 0, 0, 0)[0] for it in items}
        assert classes == {128, 64, 32}, "all three ratio classes"
        for fmt, sample, pos, norm in combos(bpc):
            scale, bias = imagenet(bpc) if norm else (None, None)
            run_and_check(ctx, items, fmt, sample, pos, scale, bias, what="mixed batch")
    finally:
        for pic, _ in (a, b, c):
            pic.free()


# ------------------------------------------------------------------------------------------------ 2. mixed picture states

@pytest.mark.parametrize("bpc", [8, 10])
def test_mixed_picture_states(ctx, bpc):
    """raster, twin-only and retiled pictures interleaved in one batch (two launches, a table slice each); no picture changes its state"""
    rng = np.random.default_rng(15200 + bpc)
    states = ["raster", "twin-only", "retiled", "twin-only", "raster", "retiled", "twin-only"]
    srcs = {s: make_source(ctx, rng, 190, 102, I420, bpc, s) for s in set(states)}
    geoms = [(None, (95, 51)), CROPS[0], CROPS[1], (None, (47, 13)), CROPS[5], (None, (24, 13)), CROPS[4]]
    try:
        items = [Item(*srcs[s], crop, size) for s, (crop, size) in zip(states, geoms)]
        before = {s: (srcs[s][0].pic.twin_ok, [srcs[s][0].pic.twin[pl] for pl in range(3)]) for s in srcs}
        assert [before[s][0] for s in ("raster", "retiled", "twin-only")] == [0, 1, api.TWIN_ONLY]
        scale, bias = imagenet(bpc)
        run_and_check(ctx, [it for it in items if it.pic.pic.twin_ok == api.TWIN_ONLY], P, N, 1, what="twin-only alone")
        run_and_check(ctx, items, K4, F16, 1, scale, bias, what="mixed states")
        run_and_check(ctx, items, P, N, 2, what="mixed states")
        # 8. device time: the call before this line is a batch of both states, two launches between one pair of events (the emulator has no clock)
        ms = ctx.last_kernel_ms()
        assert ms > 0.0 if ctx.backend == "hip" else ms >= 0.0
        assert {s: (srcs[s][0].pic.twin_ok, [srcs[s][0].pic.twin[pl] for pl in range(3)]) for s in srcs} == before
    finally:
        for pic, _ in srcs.values():
            pic.free()


# ------------------------------------------------------------------------------------------------ 3. one source, many crops, one buffer

class Shared:
    """n items in slices of ONE device buffer, `gap` bytes of sentinel behind each item; image() is what the whole buffer must hold"""

    def __init__(self, ctx, n, w, h, layout, bpc, fmt, sample, gap):
        self.ctx, self.n, self.fmt = ctx, n, fmt
        self.shapes, self.dtype = api.surface_planes(w, h, layout, bpc, fmt, sample)
        es = self.dtype.itemsize
        self.row = [cols * es for _, cols in self.shapes]
        self.plane_at = np.concatenate([[0], np.cumsum([rows * rb for (rows, _), rb in zip(self.shapes, self.row)])])
        self.item_bytes = int(self.plane_at[-1]) + gap
        self.buf = ctx.buffer(256 + n * self.item_bytes)
        assert ctx.lib.dav1d_hip_memset(ctx.h, self.buf.ptr, SENTINEL, self.buf.nbytes) == 0
        self.lead = -self.buf.ptr % 256
        self.surfaces = [api.Surface.wrap(ctx, [self.buf.ptr + self.lead + k * self.item_bytes + int(self.plane_at[pl]) for pl in range(len(self.shapes))],
                                          self.row, w, h, layout, bpc, fmt, sample) for k in range(n)]

    def check(self, wants, what=""):
        """wants[k]: the planes of item k, or None for an item that must be untouched"""
        image = np.full(self.buf.nbytes, SENTINEL, np.uint8)
        for k, want in enumerate(wants):
            for pl, (rows, cols) in enumerate(self.shapes if want is not None else []):
                at = self.lead + k * self.item_bytes + int(self.plane_at[pl])
                image[at:at + rows * self.row[pl]] = np.ascontiguousarray(want[pl]).view(np.uint8).reshape(-1)
        self.ctx.sync()
        got = self.buf.download(np.uint8)
        if not np.array_equal(got, image):
            bad = np.flatnonzero(got != image)
            at = int(bad[0]) - self.lead
            raise AssertionError("%s: %d bytes differ, first at byte %d of item %d (an item is %d bytes): got %d, want %d"
                                 % (what, len(bad), at % self.item_bytes, at // self.item_bytes, self.item_bytes, got[bad[0]], image[bad[0]]))

    def free(self):
        self.buf.free()


@pytest.mark.parametrize("fmt,sample", [(P, N), (K4, F16)], ids=["n3hw", "nhw4"])
def test_one_source_many_crops_one_buffer(ctx, fmt, sample):
    """6 crops of one picture into slices of one buffer laid out as (6, 3, h, w) / (6, h, w, 4) with a batch stride larger than an image"""
    (w, h), (dw, dh), bpc, layout = (190, 102), (19, 12), 10, I420
    crops = [(10, 6, 133, 71), (64, 8, 126, 94), (2, 2, 37, 23), (0, 0, 152, 96), (100, 50, 19, 12), (30, 40, 38, 24)]
    pic, vis = make_source(ctx, np.random.default_rng(15300), w, h, layout, bpc, "twin-only", extremes=True)
    sh = Shared(ctx, len(crops), dw, dh, layout, bpc, fmt, sample, gap=40)
    try:
        ctx.export_rgb_scaled_batch(sh.surfaces, [pic] * len(crops), crops, 1)
        sh.check([want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, 1) for crop in crops], what="six crops, one buffer")
        assert pic.pic.twin_ok == api.TWIN_ONLY
    finally:
        sh.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 4. where a workgroup finds its item

def test_one_item_is_the_single_call(ctx):
    (w, h), crop, (dw, dh), bpc, layout = (190, 102), (10, 6, 133, 71), (60, 33), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(15400), w, h, layout, bpc, "twin-only")
    a, b, c = (Dest(ctx, dw, dh, layout, bpc, K4, F16) for _ in range(3))
    whole_a, whole_b = Dest(ctx, 95, 51, layout, bpc, K4, F16), Dest(ctx, 95, 51, layout, bpc, K4, F16)
    try:
        pic.export_rgb_scaled(a.surface, crop, 2)
        ctx.export_rgb_scaled_batch([b.surface], [pic], [crop], 2)
        same_bytes(a, b)
        b.check(want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 2), what="n == 1")
        pic.export_rgb_scaled(whole_a.surface, None, 2)
        ctx.export_rgb_scaled_batch([whole_b.surface], [pic], None, 2)          # crop == NULL: every item whole
        same_bytes(whole_a, whole_b)
        # the raw call with params == NULL: the defaults of the single call
        src = (C.POINTER(Picture) * 1)(C.pointer(pic.pic))
        rect = api.SurfaceRect(*crop)
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled_batch(ctx.h, 1, C.byref(c.surface.desc), src, C.byref(rect), None, None) == 0
        c.check(want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 0), what="params == NULL")
    finally:
        for d in (a, b, c, whole_a, whole_b):
            d.free()
        pic.free()


@pytest.mark.parametrize("state", ["raster", "twin-only"])
def test_one_many_one_one_many(ctx, state):
    """workgroup counts per item of 1, many, 1, 1, many: the 1s in front, between and last but one; many = two cells per axis"""
    bpc, layout, pos = 10, I420, 1
    (W, H), big_crop, big_size = WORST[0]
    rng = np.random.default_rng(15410)
    big = make_source(ctx, rng, W, H, layout, bpc, state)
    small = make_source(ctx, rng, 64, 64, layout, bpc, state)
    try:
        one = [((0, 0, 24, 24), (12, 12)), ((16, 8, 40, 32), (10, 4)), ((2, 2, 16, 16), (8, 8))]
        items = [Item(*small, *one[0]), Item(*big, big_crop, big_size), Item(*small, *one[1]), Item(*small, *one[2]), Item(*big, (0, 0, 544, 96), (272, 24))]
        counts = [groups_of(it.rect, it.size, layout, pos) for it in items]
        assert counts[0] == counts[2] == counts[3] == 1 and counts[1] == 4 and counts[4] == 4, counts
        cw, ch = cell_of(big_crop[2], big_crop[3], big_size[0], big_size[1], 1, 1, pos)
        assert big_size[0] // 2 > cw and big_size[1] // 2 > ch, "two cells per axis"
        run_and_check(ctx, items, P, N, pos, what="1, many, 1, 1, many " + state)
        run_and_check(ctx, items + items[:1], K3, N, pos, what="... and a 1 last " + state)
    finally:
        big[0].free()
        small[0].free()


def tiny_crops(n):
    """n 16 x 16 crops of a 190 x 102 picture at even origins (130 different ones, then again)"""
    return [(2 * (k % 13) * 6 + 2 * ((k // 130) % 4), 2 * ((k // 13) % 10) * 4, 16, 16) for k in range(n)]


@pytest.mark.parametrize("n", [130, SURFACE_BATCH_MAX], ids=["130", "max"])
def test_many_items_of_one_workgroup(ctx, n):
    """more items than a wave has lanes, a non-power-of-two n, and the largest n: 8 x 8 outputs from 16 x 16 crops of one picture into one buffer"""
    (w, h), (dw, dh), bpc, layout, pos = (190, 102), (8, 8), 8, I420, 2
    pic, vis = make_source(ctx, np.random.default_rng(15420), w, h, layout, bpc, "twin-only")
    sh = Shared(ctx, n, dw, dh, layout, bpc, P, N, gap=8)
    try:
        crops = tiny_crops(n)
        assert all(groups_of(crop, (dw, dh), layout, pos) == 1 for crop in crops[:130]) and len(set(crops)) >= 130
        assert all(x0 + 16 <= w and y0 + 16 <= h for x0, y0, _, _ in crops)
        wants = {}
        for crop in crops:
            if crop not in wants:
                wants[crop] = want_of(vis, layout, bpc, dw, dh, crop, P, N, pos)
        ctx.export_rgb_scaled_batch(sh.surfaces, [pic] * n, crops, pos)
        sh.check([wants[crop] for crop in crops], what="%d items" % n)
    finally:
        sh.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. calls back to back

def test_calls_back_to_back(ctx):
    """more batch calls than the staging ring has slots, every one with another item table, no sync between them: a table overwritten while its batch
    is in flight shows as another call's pixels (on the emulator this checks the plumbing only)"""
    bpc, layout = 10, I420
    rng = np.random.default_rng(15500)
    a = make_source(ctx, rng, 190, 102, layout, bpc, "twin-only")
    b = make_source(ctx, rng, 333, 77, layout, bpc, "raster")
    try:
        tables = [[Item(*a, None, (95, 51)), Item(*a, *CROPS[0]), Item(*b, None, (64, 33))],
                  [Item(*b, None, (42, 10)), Item(*a, *CROPS[1])],
                  [Item(*a, *CROPS[5]), Item(*a, None, (47, 13)), Item(*b, None, (100, 12)), Item(*a, None, (24, 13))],
                  [Item(*a, *CROPS[4]), Item(*b, None, (64, 33))],
                  [Item(*a, None, (95, 51))],
                  [Item(*b, None, (100, 12)), Item(*a, *CROPS[0]), Item(*a, *CROPS[5])]]
        dests = [[it.dest(ctx, K4, F16) for it in t] for t in tables]
        ctx.sync()
        for t, ds in zip(tables, dests):
            ctx.export_rgb_scaled_batch([d.surface for d in ds], [it.pic for it in t], [it.rect for it in t], 1)
        for k, (t, ds) in enumerate(zip(tables, dests)):
            for it, d in zip(t, ds):
                d.check(it.want(K4, F16, 1), what="call %d of %d back to back" % (k, len(tables)))
                d.free()
    finally:
        a[0].free()
        b[0].free()


# ------------------------------------------------------------------------------------------------ 6. refusals

class RawBatch:
    """the C call on arrays of the test's own, so that a test can damage any field"""

    def __init__(self, ctx, pics, sizes, fmts, samples, crops=None):
        self.ctx, self.n = ctx, len(pics)
        self.dests = [Dest(ctx, s[0], s[1], p.layout, p.bpc, f, sm) for p, s, f, sm in zip(pics, sizes, fmts, samples)]
        self.dst = (SurfaceDesc * self.n)(*[d.surface.desc for d in self.dests])
        self.src = (C.POINTER(Picture) * self.n)(*[C.pointer(p.pic) for p in pics])
        self.crop = (api.SurfaceRect * self.n)(*[api.SurfaceRect(*c) for c in crops]) if crops is not None else None

    def call(self, params=None, n=None, with_bad=True, dst=True, src=True):
        bad = C.c_int(-7)
        rc = self.ctx.lib.dav1d_hip_surface_export_rgb_scaled_batch(self.ctx.h, self.n if n is None else n, self.dst if dst else None, self.src if src else None, self.crop,
                                                                   C.byref(params) if params is not None else None, C.byref(bad) if with_bad else None)
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
    w, h = 190, 102
    rng = np.random.default_rng(15600)
    pic = make_source(ctx, rng, w, h, I420, 10, "raster")[0]
    pic8 = make_source(ctx, rng, w, h, I420, 8, "raster")[0]
    whole, good = (0, 0, w, h), (95, 51)

    def set_stride(desc):
        desc.stride[0] = desc.stride[0] - 2

    def null_plane(desc):
        desc.data[0] = None
    # (code, size, crop, what is done to the item's descriptor)
    item_faults = [("ratio above 8", ENOTSUP, (23, 51), whole, None), ("upscaling", ENOTSUP, (191, 102), whole, None),
                   ("odd crop origin at 4:2:0", EINVAL, good, (1, 0, 95, 51), None), ("crop outside the picture", EINVAL, (50, 51), (100, 0, 100, 51), None),
                   ("NULL plane pointer", EINVAL, good, whole, null_plane), ("bad stride", EINVAL, good, whole, set_stride)]
    try:
        for what, code, size, crop, change in item_faults:
            for at in (0, 2, 4):
                sizes, crops = [good] * 5, [whole] * 5
                sizes[at], crops[at] = size, crop
                b = RawBatch(ctx, [pic] * 5, sizes, [K3] * 5, [N] * 5, crops)
                if change:
                    change(b.dst[at])
                b.refused(code, at, "%s at item %d" % (what, at))
                b.free()
        # two faults: the lowest item's code
        b = RawBatch(ctx, [pic] * 5, [good, good, (23, 51), good, good], [K3] * 5, [N] * 5, [whole, whole, whole, (1, 0, 95, 51), whole])
        b.refused(ENOTSUP, 2, "two faults")
        b.free()
        # what params refuse is refused for item 0
        b = RawBatch(ctx, [pic] * 3, [good] * 3, [K3] * 3, [N] * 3)
        b.refused(EINVAL, 0, "chroma_pos 3", params=RgbParams(3, 0))
        b.refused(EINVAL, 0, "scale with a native sample", params=RgbParams(1, 1, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)))
        # the call as a whole
        b.refused(EINVAL, -1, "n < 0", n=-1)
        b.refused(EINVAL, -1, "n > MAX", n=SURFACE_BATCH_MAX + 1)
        b.refused(EINVAL, -1, "NULL dst", dst=False)
        b.refused(EINVAL, -1, "NULL src", src=False)
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled_batch(None, 3, b.dst, b.src, None, None, None) == -EINVAL
        for at in (0, 1, 2):
            b.src[at] = C.POINTER(Picture)()
            b.refused(EINVAL, at, "NULL src[%d]" % at)
            b.src[at] = C.pointer(pic.pic)
        # n == 0 returns 0 and writes nothing, with or without arrays
        assert b.call(n=0) == (0, -1) and b.call(n=0, dst=False, src=False) == (0, -1)
        for d in b.dests:
            d.check(None, what="n == 0")
        # ... and the same arrays with nothing wrong are accepted
        assert b.call(params=RgbParams(1, 0)) == (0, -1)
        ctx.sync()
        b.free()
        # what must be uniform: the lowest item that differs from item 0
        for at in (1, 3):
            fmts, samples, pics = [K3] * 4, [N] * 4, [pic] * 4
            fmts[at] = K4
            b = RawBatch(ctx, pics, [good] * 4, fmts, samples)
            b.refused(EINVAL, at, "mixed format")
            b.free()
            fmts, samples = [K3] * 4, [N] * 4
            samples[at] = F16
            b = RawBatch(ctx, pics, [good] * 4, fmts, samples)
            b.refused(EINVAL, at, "mixed sample")
            b.free()
            pics = [pic] * 4
            pics[at] = pic8
            b = RawBatch(ctx, pics, [good] * 4, [K3] * 4, [F16] * 4)
            b.refused(EINVAL, at, "an 8-bit source among 10-bit ones")
            b.free()
        # the Python layer names the item
        d = [Dest(ctx, 95, 51, I420, 10, K3, N), Dest(ctx, 23, 51, I420, 10, K3, N)]
        with pytest.raises(api.HipError, match=r"item 1\b.*errno %d" % ENOTSUP):
            ctx.export_rgb_scaled_batch([x.surface for x in d], [pic, pic])
        with pytest.raises(ValueError):
            ctx.export_rgb_scaled_batch([x.surface for x in d], [pic])
        for x in d:
            x.check(None, what="a refused batch")
            x.free()
    finally:
        pic.free()
        pic8.free()


def test_a_picture_of_another_device_is_refused():
    """-EXDEV for the item whose picture lives on the emulator's second device (tests/conftest.py)"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        far = other.picture(64, 64, I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        near = ctx.picture(64, 64, I420, 10)
        for at in (0, 1, 2):
            pics = [near] * 3
            pics[at] = far
            b = RawBatch(ctx, pics, [(32, 32)] * 3, [K3] * 3, [F16] * 3)
            b.refused(EXDEV, at, "a picture of another device at item %d" % at)
            b.free()
        near.free()
        ctx.lib.dav1d_hip_context_use(other.h)
        far.free()
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 7. Python

def test_python_method_against_the_c_call(ctx):
    bpc, layout = 10, I420
    rng = np.random.default_rng(15700)
    a = make_source(ctx, rng, 190, 102, layout, bpc, "retiled")
    b = make_source(ctx, rng, 333, 77, layout, bpc, "twin-only")
    items = [Item(*a, *CROPS[0]), Item(*b, None, (64, 33)), Item(*a, None, (95, 51))]
    scale, bias = [2.0, 1.0, 0.5], [-1.0, 0.0, 1.0]
    py = [it.dest(ctx, K4, F16) for it in items]
    raw = RawBatch(ctx, [it.pic for it in items], [it.size for it in items], [K4] * 3, [F16] * 3, [it.rect for it in items])
    try:
        ctx.export_rgb_scaled_batch([d.surface for d in py], [it.pic for it in items], [it.rect for it in items], chroma_pos=api.CHROMA_COLOCATED, scale=scale, bias=bias)
        assert raw.call(params=RgbParams(2, 1, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias))) == (0, -1)
        f32 = dict(scale=[np.float32(v) for v in scale], bias=[np.float32(v) for v in bias])
        for it, d, r in zip(items, py, raw.dests):
            same_bytes(d, r)
            d.check(it.want(K4, F16, 2, **f32), what="Context.export_rgb_scaled_batch")
    finally:
        raw.free()
        for d in py:
            d.free()
        a[0].free()
        b[0].free()


class FakeTensor:
    """what export_batch_to_tensor asks of a tensor before it reaches the library: a device tensor of a shape, contiguous unless strides are given"""
    is_cuda = True

    def __init__(self, shape, strides=None, is_cuda=True):
        self.shape, self.is_cuda = tuple(shape), is_cuda
        self._strides = strides if strides is not None else [int(np.prod(shape[k + 1:])) for k in range(len(shape))]
        self.dtype = "fake"

    def dim(self):
        return len(self.shape)

    def stride(self, k):
        return self._strides[k]

    def element_size(self):
        return 2


def test_export_batch_to_tensor_value_errors():
    """what is refused before anything reaches the library, each case by its own message: the stand-in says it is a contiguous device tensor, so
    only the rule under test can refuse it (the child process of test_export_batch_to_tensor repeats the cases on real device tensors)"""
    pics = [object()] * 4
    rect = [(0, 0, 96, 54)]
    for match, tensor, n_pics, crops in (("read as", FakeTensor((4, 3, 54, 3)), 4, None), ("read as", FakeTensor((4, 3, 54, 4)), 4, None),
                                         ("takes 4 pictures", FakeTensor((4, 3, 54, 96)), 3, None), ("takes 4 pictures", FakeTensor((4, 3, 54, 96)), 4, rect * 3),
                                         ("takes 4 pictures", FakeTensor((4, 54, 96, 4)), 4, rect * 5),
                                         ("has shape", FakeTensor((4, 2, 54, 96)), 4, None), ("has shape", FakeTensor((3, 54, 96)), 3, None),
                                         ("has shape", FakeTensor((4, 54, 96, 5)), 4, None), ("has shape", FakeTensor((4, 3, 54, 96, 1)), 4, None),
                                         ("device tensor", FakeTensor((4, 3, 54, 96), is_cuda=False), 4, None),
                                         ("unit stride", FakeTensor((4, 3, 54, 96), [3 * 54 * 192, 54 * 192, 192, 2]), 4, None),
                                         ("channels next to each other", FakeTensor((4, 54, 96, 4), [54 * 96 * 8, 96 * 8, 8, 1]), 4, None)):
        with pytest.raises(ValueError, match=match):
            api.export_batch_to_tensor(pics[:n_pics], tensor, crops=crops)


def _torch_child():
    """(a process of its own, for the reason tests/test_surface.py gives)"""
    import torch
    w, h, layout = 190, 102, I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(15800)
    crops = [None, (10, 6, 133, 71), (64, 8, 126, 94), (0, 0, 96, 54)]
    rects = [c if c is not None else (0, 0, w, h) for c in crops]

    def bits(t):
        return t.cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])

    for bpc, dtype, sample in ((10, torch.float16, F16), (8, torch.uint8, N)):
        srcs = [make_source(tctx, rng, w, h, layout, bpc, state, extremes=True) for state in ("twin-only", "raster", "twin-only", "retiled")]
        pics = [s[0] for s in srcs]
        # (4, 3, 54, 96): planes
        t = torch.full((4, 3, 54, 96), 7, dtype=dtype, device="cuda")
        api.export_batch_to_tensor(pics, t, crops=rects)
        tctx.sync()
        for k, (pic, vis) in enumerate(srcs):
            want = want_of(vis, layout, bpc, 96, 54, crops[k], P, sample, 0)
            assert all(np.array_equal(bits(t[k, c]), want[c].view(bits(t).dtype)) for c in range(3)), "(4, 3, 54, 96) %s item %d" % (dtype, k)
        if bpc == 8:
            with_none = torch.full((4, 3, 51, 95), 7, dtype=dtype, device="cuda")
            api.export_batch_to_tensor(pics, with_none, chroma_pos=api.CHROMA_VERTICAL)          # crops=None: every picture whole
            tctx.sync()
            want = want_of(srcs[3][1], layout, bpc, 95, 51, None, P, sample, 1)
            assert all(np.array_equal(bits(with_none[3, c]), want[c]) for c in range(3)), "crops=None"
            for pic, _ in srcs:
                pic.free()
            continue
        # (4, 54, 96, 4) with ImageNet scale / bias
        mx = (1 << bpc) - 1
        scale, bias = [1.0 / (mx * s) for s in tr.IMAGENET_STD], [-m / s for m, s in zip(tr.IMAGENET_MEAN, tr.IMAGENET_STD)]
        f32 = dict(scale=[np.float32(v) for v in scale], bias=[np.float32(v) for v in bias])
        t = torch.full((4, 54, 96, 4), 7.0, dtype=dtype, device="cuda")
        api.export_batch_to_tensor(pics, t, crops=rects, chroma_pos=api.CHROMA_VERTICAL, scale=scale, bias=bias)
        tctx.sync()
        for k, (pic, vis) in enumerate(srcs):
            want = want_of(vis, layout, bpc, 96, 54, crops[k], K4, F16, 1, **f32)[0]
            assert np.array_equal(bits(t[k]).reshape(54, 96 * 4), want.view(np.uint16)), "(4, 54, 96, 4) item %d" % k
        # a non-contiguous batch view: every other image of a larger tensor, the ones between keep their fill
        big = torch.full((8, 3, 54, 96), 7.0, dtype=dtype, device="cuda")
        api.export_batch_to_tensor(pics, big[::2], crops=rects, chroma_pos=api.CHROMA_COLOCATED)
        tctx.sync()
        for k, (pic, vis) in enumerate(srcs):
            want = want_of(vis, layout, bpc, 96, 54, crops[k], P, F16, 2)
            assert all(np.array_equal(bits(big[2 * k, c]), want[c].view(np.uint16)) for c in range(3)), "big[::2] item %d" % k
            assert bool((big[2 * k + 1] == 7.0).all()), "the image behind item %d was written" % k
        for shape, kw in (((4, 3, 54, 3), {}), ((4, 3, 54, 96), dict(crops=rects[:3])), ((4, 3, 54, 96), dict(pics=pics[:3]))):
            try:
                api.export_batch_to_tensor(kw.pop("pics", pics), torch.empty(shape, dtype=dtype, device="cuda"), **kw)
            except ValueError:
                pass
            else:
                raise AssertionError("shape %s %s was accepted" % (shape, kw))
        try:
            api.export_batch_to_tensor(pics, torch.empty((4, 3, 54, 96, 2), dtype=dtype, device="cuda")[..., 0])
        except ValueError:
            pass
        else:
            raise AssertionError("rows without unit stride were accepted")
        assert [p.pic.twin_ok for p in pics] == [api.TWIN_ONLY, 0, api.TWIN_ONLY, 1]
        for pic, _ in srcs:
            pic.free()
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_batch_to_tensor():
    """export_batch_to_tensor into (4, 3, 54, 96) float16, (4, 54, 96, 4) float16 with ImageNet scale / bias, (4, 3, 54, 96) uint8 from 8-bit pictures,
    a non-contiguous batch view big[::2], and the ValueError cases on device tensors"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
