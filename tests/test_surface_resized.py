"""Resized tensor-ready RGB: dav1d_hip_surface_export_rgb_resized / dav1d_hip_surface_rgb_resized_rows_needed (dav1d_amd/csrc/surface_resize.hip,
DESIGN.md 10.7).

The call must write byte for byte what dav1d_hip_surface_export_rgb writes from the picture Q whose planes are R of the crop windows: per plane and per
axis the area scaler where the axis goes down or keeps its length, linear interpolation with half-sample centres where it goes up.  The expectation is
numpy only: r_weights() restates the "up" half of R from include/dav1d_hip.h with Python integers (test_surface_scaled.axis_weights serves d <= s),
resized_planes() runs the two passes, test_surface_rgb.expect does the rest — the way test_surface_rgb_scaled.want_of composes.  Every comparison is
exact; every destination is filled with 0xA5 first and compared byte by byte, padding included (test_surface.Dest).  Every case with `ctx` runs on the
emulated build and, under -m gpu, on the device.  The emulator has no clock: a positive device time is asked for on the device only."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import util
import test_surface_rgb as tr
import test_surface_scaled as tsc
from dav1d_amd import api
from dav1d_amd._lib import RgbParams
from test_surface import Dest
from test_surface_rgb_scaled import cell_of, even_crop, same_bytes
from test_surface_scaled import source_from, ss_of, windows
from util import make_source

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16
BIG = (190, 102)

# ((picture), crop or None, (output)): every geometry class of the single call
GEOMS = [((40, 24), None, (80, 48)),                    # exactly 2x
         ((33, 5), None, (264, 40)),                    # exactly 8x: two cells across, more than two down
         ((95, 51), None, (96, 52)),                    # barely up
         ((37, 13), None, (101, 47)),                   # odd everything
         (BIG, (14, 14, 40, 80), (264, 20)),            # up across, down down; the 4:2:0 chroma window starts at 7 mod 8 on both axes
         (BIG, (14, 14, 176, 12), (44, 40)),            # down across, up down
         (BIG, (14, 14, 33, 21), (70, 50)),             # up on both axes from 7 mod 8 (4:2:0 chroma)
         (BIG, (7, 7, 33, 21), (70, 50)),               # ... from 7 mod 8 where the layout does not subsample the axis
         (BIG, (189, 0, 1, 1), (9, 7)),                 # one sample
         (BIG, (20, 10, 2, 30), (7, 30)),               # a two-sample axis next to an identity
         (BIG, (20, 10, 30, 2), (30, 5)),
         (BIG, (0, 0, 40, 3), (40, 4))]                 # at 4:2:0 luma 3 -> 4 and chroma 2 -> 2


# ------------------------------------------------------------------------------------------------ the oracle (numpy, Python integers)

@functools.lru_cache(None)
def r_weights(s, d):
    """per output of an axis (s source samples to d): (first tap, weights) of R, from the definition"""
    if d <= s:
        return tsc.axis_weights(s, d)
    out = []
    for o in range(d):
        n, den = (2 * o + 1) * s - d, 2 * d
        i0 = n // den                      # floor, -1 .. s - 1
        r = n - i0 * den
        w1 = (r * 4096 + d) // den
        taps = {}
        for i, w in ((i0, 4096 - w1), (i0 + 1, w1)):
            k = min(max(i, 0), s - 1)
            if w:
                taps[k] = taps.get(k, 0) + w
        ks = sorted(taps)
        out.append((ks[0], tuple(taps[k] for k in ks)))
    return out


def resize_plane(plane, dw, dh):
    sh, sw = plane.shape
    p = plane.astype(np.int64)
    t = np.empty((dh, sw), np.int64)
    for j, (i0, ws) in enumerate(r_weights(sh, dh)):
        t[j] = (sum(w * p[i0 + k] for k, w in enumerate(ws)) + 8) >> 4
    out = np.empty((dh, dw), np.int64)
    for o, (i0, ws) in enumerate(r_weights(sw, dw)):
        out[:, o] = (sum(w * t[:, i0 + k] for k, w in enumerate(ws)) + (1 << 19)) >> 20
    return out.astype(plane.dtype)


def plane_axes(layout, w, h, dw, dh):
    """(s, d) across and down, for luma and (if any) chroma"""
    ssh, ssv = ss_of(layout)
    out = [((w, dw), (h, dh))]
    if layout != I400:
        out.append((((w + ssh) >> ssh, (dw + ssh) >> ssh), ((h + ssv) >> ssv, (dh + ssv) >> ssv)))
    return out


def resized_planes(vis, layout, dw, dh, crop=None):
    crop = crop or (0, 0, vis[0].shape[1], vis[0].shape[0])
    out = []
    for pl, win in enumerate(windows(vis, layout, crop)):
        ssh, ssv = ss_of(layout) if pl else (0, 0)
        out.append(resize_plane(win, (dw + ssh) >> ssh, (dh + ssv) >> ssv))
    return out


def want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, planes=None, **kw):
    planes = planes if planes is not None else resized_planes(vis, layout, dw, dh, crop)
    return tr.expect(planes, layout, bpc, fmt, sample, pos, **kw)


def check(ctx, pic, want, dw, dh, fmt, sample, crop=None, pos=0, scale=None, bias=None, rows=(0, 1 << 30), what="", **kw):
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export_rgb_resized(d.surface, crop, pos, scale, bias, rows[0], rows[1])
        d.check(want, what="%s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d chroma_pos %d" % (what, pic.w, pic.h, dw, dh, crop, pic.bpc, pic.layout,
                                                                                                       fmt, sample, pos))
    finally:
        d.free()


def imagenet(bpc):
    mx = (1 << bpc) - 1
    return [np.float32(1.0 / (mx * s)) for s in tr.IMAGENET_STD], [np.float32(-m / s) for m, s in zip(tr.IMAGENET_MEAN, tr.IMAGENET_STD)]


# ------------------------------------------------------------------------------------------------ 1. weights (CPU only)

def axes_used():
    out = set()
    for (w, h), crop, (dw, dh) in GEOMS:
        for layout in (I400, I420, I422, I444):
            c = even_crop(crop, layout) if crop else (0, 0, w, h)
            for ax in plane_axes(layout, c[2], c[3], dw, dh):
                out.update(ax)
    return out | {(1, 5), (2, 16), (7, 8), (13, 29), (31, 33), (50, 51), (50, 399), (9, 72), (8, 16), (3, 4), (5000, 5001)}


def test_weights_of_every_axis_used():
    """4096 in sum, every weight positive after merging, one or two taps on consecutive indices inside [0, s); the 2:1 taps of the definition"""
    ups = 0
    for s, d in sorted(axes_used()):
        ws = r_weights(s, d)
        assert len(ws) == d
        if d <= s:
            continue
        ups += 1
        last = 0
        for i0, w in ws:
            assert sum(w) == 4096 and min(w) > 0 and len(w) in (1, 2), (s, d, i0, w)
            assert 0 <= i0 and i0 + len(w) <= s and i0 >= last, (s, d, i0, w)
            last = i0
        assert ws[0] == (0, (4096,)) and ws[-1] == (s - 1, (4096,))
    assert ups > 20
    w = r_weights(8, 16)
    assert w[4] == (1, (1024, 3072)) and w[5] == (2, (3072, 1024)) and w[0] == (0, (4096,)) and w[15] == (7, (4096,))          # samples 1, 2 and 2, 3
    assert all(w[2 * k] == (k - 1, (1024, 3072)) and w[2 * k + 1] == (k, (3072, 1024)) for k in range(1, 7))
    assert all(i0 == 0 and ws == (4096,) for i0, ws in r_weights(1, 5))


# ------------------------------------------------------------------------------------------------ 2. closeness to the real thing (CPU only)

def _interpolate_child():
    """R on whole planes, both axes up, against torch.nn.functional.interpolate(mode="bilinear", align_corners=False) in float64, on the CPU.
    The bound is derived, not measured: 0.5 for the final rounding, a weight rounding of at most 1 / 8192 of the sample range per axis (max / 4096
    for both) and 2^-8 for the intermediate with 8 fraction bits."""
    import torch
    rng = np.random.default_rng(16050)
    for bpc in (8, 10, 12):
        mx = (1 << bpc) - 1
        tol = 0.5 + mx / 4096 + 2.0 ** -8
        assert tol < 1.51
        worst = 0.0
        for (sw, sh), (dw, dh) in (((40, 24), (80, 48)), ((33, 5), (264, 40)), ((95, 51), (96, 52)), ((37, 13), (101, 47)), ((1, 1), (9, 7)), ((2, 3), (7, 30)),
                                   ((50, 13), (399, 29))):
            for content in ("random", "two-valued"):
                plane = rng.integers(0, mx + 1, (sh, sw)) if content == "random" else rng.integers(0, 2, (sh, sw)) * mx
                plane = plane.astype(np.uint16)
                got = resize_plane(plane, dw, dh).astype(np.int64)
                assert got.min() >= 0 and got.max() <= mx
                ref = torch.nn.functional.interpolate(torch.from_numpy(plane.astype(np.float64))[None, None], size=(dh, dw), mode="bilinear", align_corners=False)
                err = float(np.abs(got - ref[0, 0].numpy()).max())
                worst = max(worst, err)
                assert err <= tol, (bpc, sw, sh, dw, dh, content, err, tol)
        print("bpc %d: largest distance %.3f codes, bound %.3f" % (bpc, worst, tol))
    print("interpolate-child ok")


def test_close_to_bilinear_interpolation():
    """(a process of its own: torch brings its own HIP runtime, and this process may have opened the device through the library)"""
    pytest.importorskip("torch")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "interpolate-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "interpolate-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 3. every geometry class

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [I400, I420, I422, I444], ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_geometry(ctx, bpc, layout, state):
    """planar native at chroma_pos 0 / 1 / 2"""
    pics = {}
    two_cells = False
    ssh, ssv = ss_of(layout)
    try:
        for (w, h), crop, (dw, dh) in GEOMS:
            if (w, h) not in pics:
                pics[w, h] = make_source(ctx, np.random.default_rng(16100 + 100 * bpc + 10 * layout + w), w, h, layout, bpc, state)
            pic, vis = pics[w, h]
            crop = even_crop(crop, layout) if crop else None
            rect = crop or (0, 0, w, h)
            planes = resized_planes(vis, layout, dw, dh, crop)
            for pos in (0, 1, 2):
                cw, ch = cell_of(rect[2], rect[3], dw, dh, ssh, ssv, pos)
                ring = (ssh or ssv) and pos
                two_cells |= bool(ring and planes[-1].shape[1] > cw and planes[-1].shape[0] > ch)
                check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, P, N, pos, planes), dw, dh, P, N, crop, pos, what=state)
            assert pic.pic.twin_ok == (api.TWIN_ONLY if state == "twin-only" else 0)
        if layout in (I420, I422):
            assert two_cells, "no case spans two owned cells per axis with a ring"
    finally:
        for pic, _ in pics.values():
            pic.free()


def test_the_geometries_are_what_they_claim():
    """from the sizes alone: the 8x case spans two owned cells with a ring across and more than two down; the crops at (14, 14) put the 4:2:0 chroma window
    at 7 mod 8; luma and chroma fall on different sides in the last case; every up / down / identity pairing of the axes occurs"""
    (w, h), _, (dw, dh) = GEOMS[1]
    for pos in (1, 2):
        cw, ch = cell_of(w, h, dw, dh, 1, 1, pos)
        assert (cw, ch) == {1: (124, 6), 2: (124, 7)}[pos] and dw // 2 > cw and dh // 2 > 2 * ch
    assert all((c[0] >> 1) & 7 == 7 and (c[1] >> 1) & 7 == 7 for _, c, _ in GEOMS[4:7]) and GEOMS[7][1][0] & 7 == 7 and GEOMS[7][1][1] & 7 == 7
    luma, chroma = plane_axes(I420, 40, 3, 40, 4)
    assert luma[1] == (3, 4) and chroma[1] == (2, 2)
    kinds = set()
    for (w, h), crop, (dw, dh) in GEOMS:
        c = crop or (0, 0, w, h)
        kinds.add(((dw > c[2]) - (dw < c[2]), (dh > c[3]) - (dh < c[3])))
    assert {(1, 1), (1, -1), (-1, 1), (1, 0), (0, 1)} <= kinds


# ------------------------------------------------------------------------------------------------ 4. nothing outside the crop is read

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [I420, I444], ids=["i420", "i444"])
def test_nothing_outside_the_crop_is_read(ctx, layout, state):
    """an interior crop of a picture whose samples outside the crop are 0 or max gives the bytes of the picture that is the crop alone"""
    bpc, (cw, ch), (x0, y0), (dw, dh) = 10, (38, 22), (22, 14), (101, 47)
    mx = (1 << bpc) - 1
    alone, vis = make_source(ctx, np.random.default_rng(16200 + layout), cw, ch, layout, bpc, state, extremes=True)
    big = ctx.picture(96, 64, layout, bpc)
    ssh, ssv = ss_of(layout)
    padded = []
    for pl in range(big.n_planes):
        sh, sv = (ssh, ssv) if pl else (0, 0)
        shape = big.padded_shape(pl)
        a = (((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) & 1) * mx).astype(big.dtype)
        a[y0 >> sv:(y0 >> sv) + vis[pl].shape[0], x0 >> sh:(x0 >> sh) + vis[pl].shape[1]] = vis[pl]
        padded.append(a)
    big.free()
    pic, _ = source_from(ctx, padded, 96, 64, layout, bpc, state)
    try:
        for fmt, sample, pos in ((P, N, 0), (P, N, 1), (K4, F16, 2)):
            a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            alone.export_rgb_resized(a.surface, None, pos)
            pic.export_rgb_resized(b.surface, (x0, y0, cw, ch), pos)
            same_bytes(a, b)
            b.check(want_of(vis, layout, bpc, dw, dh, None, fmt, sample, pos), what="the crop alone")
            a.free()
            b.free()
    finally:
        alone.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. anchors

@pytest.mark.parametrize("state", ["raster", "twin-only"])
def test_down_everywhere_is_export_rgb_scaled(ctx, state):
    """d <= s on both axes of every plane: the bytes of dav1d_hip_surface_export_rgb_scaled, library against library"""
    w, h, bpc, layout = 190, 102, 10, I420
    pic, _ = make_source(ctx, np.random.default_rng(16300), w, h, layout, bpc, state, extremes=True)
    try:
        for crop, (dw, dh) in ((None, (95, 51)), (None, (47, 13)), ((10, 6, 133, 71), (24, 13)), (None, (189, 101)), ((10, 6, 133, 71), (133, 71))):
            for fmt, sample, pos in ((P, N, 1), (K4, F16, 2)):
                a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
                pic.export_rgb_scaled(a.surface, crop, pos)
                pic.export_rgb_resized(b.surface, crop, pos)
                same_bytes(a, b)
                a.free()
                b.free()
    finally:
        pic.free()


def test_same_size_is_export_rgb(ctx):
    w, h, bpc, layout = 190, 102, 10, I420
    pic, _ = make_source(ctx, np.random.default_rng(16310), w, h, layout, bpc, "twin-only", extremes=True)
    try:
        for fmt, sample, pos in ((P, N, 1), (K3, F16, 2), (K4, F32, 1)):
            a, b = Dest(ctx, w, h, layout, bpc, fmt, sample), Dest(ctx, w, h, layout, bpc, fmt, sample)
            pic.export_rgb(a.surface, pos)
            pic.export_rgb_resized(b.surface, None, pos)
            same_bytes(a, b)
            a.free()
            b.free()
    finally:
        pic.free()


def test_exact_double_of_a_ramp(ctx):
    """2x at 4:4:4 with the identity matrix, a ramp of 4 per column in Y and of 8 per row in U: output 2k is (s[k - 1] + 3 s[k]) / 4, output 2k + 1 is
    (3 s[k] + s[k + 1]) / 4, the first and last outputs are the edge samples"""
    w, h, bpc, layout = 40, 24, 10, I444
    fill = lambda pl, s: np.broadcast_to(np.arange(s[1])[None, :] * 4 if pl == 0 else np.arange(s[0])[:, None] * 8 if pl == 1 else np.full(s, 512), s)
    pic, vis = tr.make_picture(ctx, w, h, layout, bpc, "raster", fill)
    d = Dest(ctx, 2 * w, 2 * h, layout, bpc, P, N, matrix=0)
    try:
        pic.export_rgb_resized(d.surface, None, 0)
        cols = np.array([0] + [c for k in range(w - 1) for c in (4 * k + 1, 4 * k + 3)] + [4 * (w - 1)])
        rows = np.array([0] + [c for k in range(h - 1) for c in (8 * k + 2, 8 * k + 6)] + [8 * (h - 1)])
        want = [np.full((2 * h, 2 * w), 512, np.uint16), np.broadcast_to(cols[None, :], (2 * h, 2 * w)).astype(np.uint16),
                np.broadcast_to(rows[:, None], (2 * h, 2 * w)).astype(np.uint16)]          # R, G, B = V, Y, U
        assert all(np.array_equal(a, b) for a, b in zip(want, want_of(vis, layout, bpc, 2 * w, 2 * h, None, P, N, 0, matrix=0)))
        d.check(want, what="2x of a ramp")
    finally:
        d.free()
        pic.free()


@pytest.mark.parametrize("value", [0, 1, 511, 1023])
def test_constants_stay_constant(ctx, value):
    """at every geometry of section 3, 4:4:4 with the identity matrix: every output sample is the value"""
    bpc, layout = 10, I444
    pics = {}
    try:
        for (w, h), crop, (dw, dh) in GEOMS:
            if (w, h) not in pics:
                pics[w, h] = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", lambda pl, s: np.full(s, value))
            want = [np.full((dh, dw), value, np.uint16)] * 3
            check(ctx, pics[w, h][0], want, dw, dh, P, N, crop, 1, what="constant %d" % value, matrix=0)
    finally:
        for pic, _ in pics.values():
            pic.free()


# ------------------------------------------------------------------------------------------------ 6. formats and samples

@pytest.mark.parametrize("fmt", [P, K3, K4], ids=["planar", "rgb", "rgba"])
@pytest.mark.parametrize("bpc", [8, 10])
def test_formats_and_samples(ctx, bpc, fmt):
    """one geometry that goes up on both axes and one that is mixed, every sample type, with and without normalisation"""
    layout = I420
    mx = (1 << bpc) - 1
    pic, vis = make_source(ctx, np.random.default_rng(16400 + bpc), BIG[0], BIG[1], layout, bpc, "twin-only", extremes=True)
    try:
        for crop, (dw, dh) in (((14, 14, 33, 21), (75, 47)), ((14, 14, 176, 12), (44, 40))):
            planes = resized_planes(vis, layout, dw, dh, crop)
            for sample in (N, M, F32, F16):
                if sample == M and bpc == 8:
                    continue
                want = want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, 1, planes)
                if fmt == K4:
                    alpha = {N: mx, M: mx << (16 - bpc), F32: 1.0, F16: 1.0}[sample]
                    assert (want[0][:, 3::4] == alpha).all()
                check(ctx, pic, want, dw, dh, fmt, sample, crop, 1, what="sample")
                if sample in (F32, F16):
                    scale, bias = imagenet(bpc)
                    check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, 1, planes, scale=scale, bias=bias), dw, dh, fmt, sample, crop, 1, scale, bias,
                          what="normalised")
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 7. bands and rows needed

@pytest.mark.parametrize("band", [2, 6, 16])
@pytest.mark.parametrize("fmt,sample", [(P, N), (K4, F16)], ids=["planar", "rgba-f16"])
def test_bands(ctx, fmt, sample, band):
    """destination bands at chroma_pos 1: each alone leaves every other row at the sentinel, their union equals the one call"""
    (w, h), (dw, dh), bpc, layout = (37, 13), (101, 47), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(16500), w, h, layout, bpc, "twin-only")
    want = want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 1)
    try:
        whole = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
        for r0 in range(0, dh, band):
            r1 = min(r0 + band, dh)
            d = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            pic.export_rgb_resized(d.surface, None, 1, row0=r0, row1=r1)
            d.check(want, rows=[(r0, r1)] * len(want), what="band [%d, %d)" % (r0, r1))
            d.free()
            pic.export_rgb_resized(whole.surface, None, 1, row0=r0, row1=r1 if r1 < dh else 1 << 30)
        whole.check(want, what="the union of the bands")
        whole.free()
    finally:
        pic.free()


def rows_of(r, s, d):
    """rows [0, r) of a plane need rows [0, rows_of) of its window"""
    if r <= 0:
        return 0
    if d <= s:
        return -(-r * s // d)
    return min(s, ((2 * (r - 1) + 1) * s - d) // (2 * d) + 2)


def rows_needed(h, crop, dh, ssv, pos, r1, mono=False):
    y0, ch = crop[1], crop[3]
    r = min(dh, r1 + 2) if ssv and pos else min(dh, r1)
    need = y0 + rows_of(r, ch, dh)
    if not mono:
        dch, sh = (dh + ssv) >> ssv, (ch + ssv) >> ssv
        need = max(need, ((y0 >> ssv) + rows_of(dch if r >= dh else r >> ssv, sh, dch)) << ssv)
    return min(h, need)


@pytest.mark.parametrize("crop,size", [((10, 6, 60, 30), (150, 88)), (None, (380, 150)), ((10, 6, 133, 11), (60, 88))], ids=["crop", "whole", "mixed"])
def test_rows_needed_is_safe_and_tight(ctx, crop, size):
    """For every band end r1: a copy of the source whose luma rows at and below rgb_resized_rows_needed(r1), and the chroma rows under them, hold other
    values gives the same rows [0, r1); with one row fewer than the helper says at least one band of the sweep changes.  The answer is the restated rule
    of include/dav1d_hip.h for r1 + 2 rows: the chroma row below the band is resized as well."""
    (w, h), (dw, dh), bpc, layout, pos = BIG, size, 10, I420, 1
    pic, vis = make_source(ctx, np.random.default_rng(16600), w, h, layout, bpc, "raster")
    padded = [v.base for v in vis]
    want = want_of(vis, layout, bpc, dw, dh, crop, K3, N, pos)
    surface = Dest(ctx, dw, dh, layout, bpc, K3, N)
    tight = False
    try:
        last = 0
        for r1 in list(range(6, dh, 14)) + [dh]:
            need = pic.rgb_resized_rows_needed(surface.surface, crop, pos, r1)
            assert last <= need <= h
            last = need
            assert need == rows_needed(h, crop or (0, 0, w, h), dh, 1, pos, r1)
            assert pic.rgb_resized_rows_needed(surface.surface, crop, 0, r1) == rows_needed(h, crop or (0, 0, w, h), dh, 1, 0, r1)
            for rows, same in ((need, True), (need - 1, False)):
                other = [p.copy() for p in padded]
                other[0][rows:] ^= 0x155
                for pl in (1, 2):          # safe: the chroma rows wholly below; tight: from the chroma row that luma row `rows` belongs to (the answer can be chroma's)
                    other[pl][(rows + 1) >> 1 if same else rows >> 1:] ^= 0x155
                pic2, _ = source_from(ctx, other, w, h, layout, bpc, "twin-only")
                d = Dest(ctx, dw, dh, layout, bpc, K3, N)
                pic2.export_rgb_resized(d.surface, crop, pos, row0=0, row1=r1)
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
        assert pic.rgb_resized_rows_needed(surface.surface, crop, pos, 0) == 0
        assert pic.rgb_resized_rows_needed(surface.surface, crop, pos, 1 << 30) == (crop[1] + crop[3] + (crop[3] & 1) if crop else h)
    finally:
        surface.free()
        pic.free()


def test_rows_needed_where_nothing_goes_up_is_the_parents(ctx):
    (w, h), bpc, layout = BIG, 10, I420
    pic, _ = make_source(ctx, np.random.default_rng(16650), w, h, layout, bpc, "raster")
    d = Dest(ctx, 47, 33, layout, bpc, K3, N)
    try:
        for crop in (None, (10, 6, 133, 71)):
            for pos in (0, 1, 2):
                for r1 in (0, 2, 10, 32, 33, 1 << 30):
                    assert pic.rgb_resized_rows_needed(d.surface, crop, pos, r1) == pic.rgb_scaled_rows_needed(d.surface, crop, pos, r1)
    finally:
        d.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 8. unaligned destinations; the source is left alone; timed

@pytest.mark.parametrize("pad", [0, 2, 10])
@pytest.mark.parametrize("offset", [0, 2, 6])
def test_unaligned_destinations(ctx, offset, pad):
    """the sample-by-sample store path, whole units and the partial last unit (101 = 12 * 8 + 5 samples)"""
    (w, h), (dw, dh), layout = (37, 13), (101, 47), I420
    for bpc, fmt, sample in ((8, K3, N), (10, K4, F16)):
        pic, vis = make_source(ctx, np.random.default_rng(16700 + bpc), w, h, layout, bpc, "twin-only")
        try:
            check(ctx, pic, want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 2), dw, dh, fmt, sample, None, 2, pad=pad, offset=offset,
                  what="offset %d pad %d" % (offset, pad))
        finally:
            pic.free()


@pytest.mark.parametrize("state", ["twin-only", "raster"])
def test_source_untouched_and_timed(ctx, state):
    (w, h), (dw, dh), bpc, layout = BIG, (75, 47), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(16800), w, h, layout, bpc, state)
    try:
        raster = tsc._raster_bytes(ctx, pic)
        twin = util.twin_bytes(ctx, pic) if state == "twin-only" else None
        ptrs, ok, live = [pic.pic.twin[pl] for pl in range(3)], pic.pic.twin_ok, tsc._live(ctx)
        if state == "twin-only":
            assert (raster == 0x5A).all()
        crop = (14, 14, 33, 21)
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
    w, h = BIG
    rng = np.random.default_rng(16900)
    pics = {key: make_source(ctx, rng, w, h, key[1], key[0], "raster")[0] for key in ((10, I420), (8, I420), (10, I422), (10, I444))}

    def refused(code, fmt=K3, sample=N, size=(95, 51), crop=None, rows=(0, 1 << 30), change=None, key=(10, I420), params=None, helper=True, shape_as=None, flt=0, **kw):
        pic = pics[key]
        d = Dest(ctx, size[0], size[1], key[1], key[0], shape_as[0] if shape_as else fmt, shape_as[1] if shape_as else sample, **kw)
        d.surface.desc.format, d.surface.desc.sample = fmt, sample
        if change:
            change(d.surface.desc)
        rect = C.byref(api.SurfaceRect(*crop)) if crop is not None else None
        p = C.byref(params) if params is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_rgb_resized(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), rect, p, flt, rows[0], rows[1])
        assert rc == -code, (rc, code, fmt, sample, crop, size, rows)
        d.check(None, what="a refused export")
        if helper:
            assert ctx.lib.dav1d_hip_surface_rgb_resized_rows_needed(C.byref(d.surface.desc), C.byref(pic.pic), rect, p, flt, rows[1]) == -code
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
        for size in ((95, 51), (200, 110)):          # a size the parent serves, and one only this call does
            # what dav1d_hip_surface_export_rgb refuses
            for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, 5, -1):
                refused(EINVAL, fmt, N, shape_as=(P, N), size=size)
            for sample in (4, -1):
                refused(EINVAL, K3, sample, shape_as=(K3, N), size=size)
            for fmt in (P, K3, K4):
                refused(EINVAL, fmt, M, key=(8, I420), shape_as=(fmt, F16), size=size)             # MSB16 at 8 bpc
                for sample in (N, M):                                                             # normalisation is for float samples
                    refused(EINVAL, fmt, sample, params=RgbParams(1, 1, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)), size=size)
                for pos in (-1, 3):
                    refused(EINVAL, fmt, F16, params=RgbParams(pos, 0), size=size)
                refused(EINVAL, fmt, N, change=setter("w", 0), size=size)
                refused(EINVAL, fmt, N, change=null_plane(0), size=size)
                refused(EINVAL, fmt, F16, change=stride(0, -2), size=size)
                refused(EINVAL, fmt, F32, change=stride(0, +2), pad=4, size=size)
                refused(EINVAL, fmt, N, matrix=0, size=size)                                       # identity needs 4:4:4
                refused(EINVAL, fmt, N, rows=(1, 32), helper=False, size=size)                     # odd band rows
                refused(EINVAL, fmt, N, rows=(0, 33), size=size)
                for m in (2, 4, 8, 14, -1):
                    refused(ENOTSUP, fmt, N, matrix=m, size=size)
            refused(EINVAL, P, N, change=null_plane(2), size=size)
        assert ctx.lib.dav1d_hip_surface_export_rgb_resized(None, None, None, None, None, 0, 0, 2) == -EINVAL
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
        refused(EINVAL, crop=(1, 0, 95, 51), size=(200, 110))
        # ... and the ratios above 8 downwards, whatever the other axis does
        refused(ENOTSUP, size=(23, 51))
        refused(ENOTSUP, size=(95, 12))
        refused(ENOTSUP, size=(23, 200))
        refused(ENOTSUP, size=(300, 12))
        # an unknown filter, alone and behind an older refusal (whose code wins)
        for flt in (1, -1, 7):
            refused(ENOTSUP, flt=flt)
            refused(ENOTSUP, flt=flt, size=(200, 110))
            refused(EINVAL, flt=flt, crop=(1, 0, 95, 51))
        # the existing calls still refuse what they refused
        for size in ((191, 102), (190, 103)):
            d = Dest(ctx, size[0], size[1], I420, 10, K3, N)
            planar = Dest(ctx, size[0], size[1], I420, 10, api.SURFACE_PLANAR, N)
            desc, p = C.byref(d.surface.desc), C.byref(pics[10, I420].pic)
            assert ctx.lib.dav1d_hip_surface_export_rgb_scaled(ctx.h, desc, p, None, None, 0, 1 << 30) == -ENOTSUP
            assert ctx.lib.dav1d_hip_surface_rgb_scaled_rows_needed(desc, p, None, None, 1 << 30) == -ENOTSUP
            assert ctx.lib.dav1d_hip_surface_export_scaled(ctx.h, C.byref(planar.surface.desc), p, None, 0, 1 << 30) == -ENOTSUP
            src = (C.POINTER(api.Picture) * 1)(C.pointer(pics[10, I420].pic))
            assert ctx.lib.dav1d_hip_surface_export_rgb_scaled_batch(ctx.h, 1, desc, src, None, None, None) == -ENOTSUP
            for x in (d, planar):
                x.check(None, what="a refused export")
                x.free()
        # what is accepted: the same surfaces with nothing wrong, odd origins where the layout does not subsample the axis
        for key, crop, size in (((10, I420), None, (191, 102)), ((10, I420), None, (190, 103)), ((10, I422), (0, 1, 95, 51), (200, 51)),
                                ((10, I444), (1, 1, 95, 51), (24, 110)), ((8, I420), (0, 0, 184, 96), (23, 200))):
            for fmt in (P, K3, K4):
                d = Dest(ctx, size[0], size[1], key[1], key[0], fmt, F16, matrix=0 if key[1] == I444 else 6)
                pics[key].export_rgb_resized(d.surface, crop, 2)
                assert pics[key].rgb_resized_rows_needed(d.surface, crop, 2, 1 << 30) == (crop[1] + crop[3] if crop else h)
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
        d = Dest(ctx, 96, 96, I420, 10, K3, F16)
        assert ctx.lib.dav1d_hip_surface_export_rgb_resized(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, None, 0, 0, 96) == -EXDEV
        d.check(None, what="a refused export")
        d.free()
        ctx.lib.dav1d_hip_context_use(other.h)
        pic.free()
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 10. Python

def test_python_methods(ctx):
    (w, h), (dw, dh), bpc, layout = BIG, (224, 224), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(17000), w, h, layout, bpc, "retiled")
    s = ctx.surface(dw, dh, layout, bpc, K4, F16)
    try:
        s.fill(0xA5)
        crop = (10, 2, 64, 100)
        assert api.RESIZE_BILINEAR == 0
        pic.export_rgb_resized(s, crop=crop, chroma_pos=api.CHROMA_COLOCATED, scale=[2.0, 1.0, 0.5], bias=[-1.0, 0.0, 1.0], filter=api.RESIZE_BILINEAR)
        got = s.download()[0]
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 2, scale=[np.float32(v) for v in (2.0, 1.0, 0.5)], bias=[np.float32(v) for v in (-1.0, 0.0, 1.0)])[0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        assert pic.rgb_resized_rows_needed(s, crop, 1, 1 << 30) == 102
        assert pic.rgb_resized_rows_needed(s, crop, 1, 10) == rows_needed(h, crop, dh, 1, 1, 10) == 8          # luma 2 + 6, chroma (1 + 3) << 1
        assert pic.rgb_resized_rows_needed(s, crop, 0, 40) == rows_needed(h, crop, dh, 1, 0, 40) == 22         # chroma (1 + 10) << 1 (luma 2 + 19)
        with pytest.raises(api.HipError):
            pic.rgb_resized_rows_needed(s, (1, 0, 95, 51), 1, 10)
        with pytest.raises(api.HipError, match="errno %d" % ENOTSUP):
            pic.export_rgb_resized(s, crop, filter=3)
        with pytest.raises(api.HipError, match="errno %d" % ENOTSUP):
            pic.export_rgb_scaled(s, crop)
    finally:
        s.free()
        pic.free()


def test_export_to_tensor_value_errors():
    """interp= is refused before anything reaches the library: without resize=True, with grain or colour, with a name that is no filter"""
    from test_surface_batch import FakeTensor
    t = FakeTensor((3, 54, 96))
    for kw in (dict(interp="bilinear"), dict(interp="bilinear", resize=True, grain=object()), dict(interp="bilinear", colour=object()),
               dict(interp="bilinear", resize=True, colour=object()), dict(interp="bicubic", resize=True)):
        with pytest.raises(ValueError):
            api.export_to_tensor(object(), t, **kw)
    with pytest.raises(ValueError):
        api.export_batch_to_tensor([object()] * 4, FakeTensor((4, 3, 54, 96)), interp="bicubic")


if __name__ == "__main__":
    if sys.argv[1:] == ["interpolate-child"]:
        _interpolate_child()
