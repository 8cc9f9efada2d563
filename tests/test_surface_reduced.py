"""Thumbnail-scale tensor-ready RGB: dav1d_hip_surface_export_rgb_reduced / dav1d_hip_surface_rgb_reduced_rows_needed (dav1d_amd/csrc/surface_reduce.hip,
DESIGN.md 10.8).

The call must write byte for byte what dav1d_hip_surface_export_rgb writes from the picture Q whose planes are R' of the crop windows: per plane and
per axis the area rule S at EVERY ratio up to 256:1 where the axis goes down or keeps its length, R's linear interpolation where it goes up.  The
expectation is numpy only: area_weights() restates S from include/dav1d_hip.h with Python integers and without the 8:1 limit
(test_surface_resized.r_weights serves d > s), reduced_planes() runs the two passes, test_surface_rgb.expect does the rest.  Every comparison is
exact; every destination is filled with 0xA5 first and compared byte by byte, padding included (test_surface.Dest).  Every case with `ctx` runs on the
emulated build and, under -m gpu, on the device.  The emulator has no clock: a positive device time is asked for on the device only.

A plane axis of 513 -> 2 or 2049 -> 8 cannot reach the call (w <= 256 dst->w bounds every plane): the weights test covers them on the CPU, the calls
get 511 -> 2 and 2047 -> 8, whose outputs have 256 and 257 taps."""
import ctypes as C
import functools

import numpy as np
import pytest

import util
import test_surface_rgb as tr
import test_surface_resized as rs
import test_surface_scaled as tsc
from dav1d_amd import api
from dav1d_amd._lib import RgbParams
from test_surface import Dest
from test_surface_rgb_scaled import even_crop, same_bytes
from test_surface_scaled import source_from, ss_of, windows
from util import make_source

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16
BIG = (330, 120)
RD_NCOL, RD_OW = 2048, 256          # the reducer's cell (dav1d_amd/csrc/surface_reduce.hip): source columns, outputs across

# ((picture), crop or None, (output)): every geometry class
GEOMS = [((73, 73), None, (9, 9)),                      # 10 taps, the first ratio past the old limit; at 4:2:0 chroma is 37 -> 5, under 8:1
         ((100, 100), None, (11, 11)),
         ((2047, 40), None, (8, 3)),                    # 257 taps across, two cells across
         ((40, 511), None, (3, 2)),                     # 256 taps down
         ((2048, 16), None, (8, 2)),                    # exactly 256:1 across
         ((256, 256), None, (1, 1)),                    # 256 -> 1, a 1 x 1 destination
         (BIG, (14, 14, 300, 100), (7, 9)),             # 300 -> 7; the 4:2:0 chroma window starts at 7 mod 8 on both axes
         (BIG, (7, 7, 300, 100), (7, 9)),               # ... from 7 mod 8 where the layout does not subsample the axis
         (BIG, (0, 0, 80, 3), (4, 4)),                  # 20:1 across while down goes up (at 4:2:0 luma 3 -> 4, chroma 2 -> 2)
         (BIG, (0, 0, 3, 80), (4, 4)),                  # ... and the reverse
         (BIG, (2, 2, 72, 81), (9, 9)),                 # exactly 8:1 across, 9:1 down
         (BIG, None, (300, 13))]                        # more than RD_OW outputs across next to 9.2:1 down: two cells across whatever the ratio


# ------------------------------------------------------------------------------------------------ the oracle (numpy, Python integers)

@functools.lru_cache(None)
def area_weights(s, d):
    """per output of an axis (s source samples to d <= s): (first tap, weights) of S, from the definition — any ratio"""
    assert 1 <= d <= s
    out = []
    for o in range(d):
        a, b = o * s, (o + 1) * s
        i0, i1 = a // d, (b + d - 1) // d - 1
        prev, ws = 0, []
        for k in range(i0, i1 + 1):
            q = ((min(b, (k + 1) * d) - a) * 4096 + s // 2) // s
            ws.append(q - prev)
            prev = q
        out.append((i0, tuple(ws)))
    return out


def axis_weights(s, d):
    return area_weights(s, d) if d <= s else rs.r_weights(s, d)


def reduce_plane(plane, dw, dh, with_t=False):
    sh, sw = plane.shape
    p = plane.astype(np.int64)
    t = np.empty((dh, sw), np.int64)
    for j, (i0, ws) in enumerate(axis_weights(sh, dh)):
        t[j] = ((np.array(ws, np.int64)[:, None] * p[i0:i0 + len(ws)]).sum(0) + 8) >> 4
    assert t.max() < 1 << 20
    out = np.empty((dh, dw), np.int64)
    for o, (i0, ws) in enumerate(axis_weights(sw, dw)):
        acc = (np.array(ws, np.int64)[None, :] * t[:, i0:i0 + len(ws)]).sum(1) + (1 << 19)
        assert acc.max() < 1 << 32
        out[:, o] = acc >> 20
    return (out.astype(plane.dtype), t) if with_t else out.astype(plane.dtype)


def reduced_planes(vis, layout, dw, dh, crop=None):
    crop = crop or (0, 0, vis[0].shape[1], vis[0].shape[0])
    out = []
    for pl, win in enumerate(windows(vis, layout, crop)):
        ssh, ssv = ss_of(layout) if pl else (0, 0)
        out.append(reduce_plane(win, (dw + ssh) >> ssh, (dh + ssv) >> ssv))
    return out


def want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, planes=None, **kw):
    planes = planes if planes is not None else reduced_planes(vis, layout, dw, dh, crop)
    return tr.expect(planes, layout, bpc, fmt, sample, pos, **kw)


def check(ctx, pic, want, dw, dh, fmt, sample, crop=None, pos=0, scale=None, bias=None, rows=(0, 1 << 30), what="", **kw):
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export_rgb_reduced(d.surface, crop, pos, scale, bias, rows[0], rows[1])
        d.check(want, what="%s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d chroma_pos %d" % (what, pic.w, pic.h, dw, dh, crop, pic.bpc, pic.layout,
                                                                                                       fmt, sample, pos))
    finally:
        d.free()


def cells_across(s, d):
    """the reducer's cells across an axis that goes down (job_cell of surface_reduce.hip)"""
    ow = max(1, min(RD_OW, (RD_NCOL - 9) * d // s))
    return -(-d // ow)


# ------------------------------------------------------------------------------------------------ 1. weights (CPU only)

def axes_used():
    out = set()
    for (w, h), crop, (dw, dh) in GEOMS:
        for layout in (I400, I420, I422, I444):
            c = even_crop(crop, layout) if crop else (0, 0, w, h)
            for ax in rs.plane_axes(layout, c[2], c[3], dw, dh):
                out.update(ax)
    return out | {(513, 2), (2049, 8), (257, 1), (256, 1), (7680, 224), (4320, 224), (7680, 30), (3840, 15), (511, 2), (1000, 999), (5, 5)}


def test_weights_of_every_axis_used():
    """never negative, 4096 in sum, at most ceil(s / d) + 1 <= 257 taps inside [0, s), a fully covered sample weighs at least 15; up to 8:1 they are
    test_surface_scaled's"""
    downs = 0
    for s, d in sorted(axes_used()):
        if d > s:
            continue
        downs += 1
        ws = area_weights(s, d)
        assert len(ws) == d
        for o, (i0, w) in enumerate(ws):
            assert sum(w) == 4096 and min(w) >= 0 and len(w) <= -(-s // d) + 1 <= 258 and 0 <= i0 and i0 + len(w) <= s, (s, d, o, i0, w)
            assert len(w) <= 257 or s > 256 * d
            for k, wk in enumerate(w):
                if (i0 + k) * d >= o * s and (i0 + k + 1) * d <= (o + 1) * s and s <= 257 * d:
                    assert wk >= 15, (s, d, o, k, wk)
        if s <= 8 * d:
            assert ws == tsc.axis_weights(s, d)
    assert downs > 25
    assert max(len(w) for _, w in area_weights(513, 2)) == 257 and max(len(w) for _, w in area_weights(2049, 8)) == 257
    assert max(len(w) for _, w in area_weights(2047, 8)) == 257 and max(len(w) for _, w in area_weights(511, 2)) == 256
    assert area_weights(256, 1) == [(0, (16,) * 256)]
    assert area_weights(5, 5) == [(k, (4096,)) for k in range(5)]


def test_the_geometries_are_what_they_claim():
    """from the sizes alone"""
    luma, chroma = rs.plane_axes(I420, 73, 73, 9, 9)
    assert luma[0] == (73, 9) and chroma[0] == (37, 5) and 73 > 8 * 9 and 37 <= 8 * 5
    assert all((c[0] >> 1) & 7 == 7 and (c[1] >> 1) & 7 == 7 for _, c, _ in GEOMS[6:7]) and GEOMS[7][1][0] & 7 == 7 and GEOMS[7][1][1] & 7 == 7
    luma, chroma = rs.plane_axes(I420, 80, 3, 4, 4)
    assert luma == ((80, 4), (3, 4)) and chroma == ((40, 2), (2, 2))
    assert rs.plane_axes(I420, 3, 80, 4, 4)[0] == ((3, 4), (80, 4))
    assert rs.plane_axes(I400, 72, 81, 9, 9)[0] == ((72, 9), (81, 9))
    assert cells_across(2047, 8) == 2 and cells_across(330, 300) == 2          # two cells across; a cell is four rows down at these sizes
    i0 = [i for i, _ in area_weights(73, 9)]
    n = [len(w) for _, w in area_weights(73, 9)]
    assert any(i0[k] + n[k] - 1 == i0[k + 1] for k in range(8)), "no source row feeds two output rows"


# ------------------------------------------------------------------------------------------------ 2. closeness to an exact area mean (CPU only)

def box_matrix(s, d):
    """exact box integration: row o holds the shares of the samples of [o s / d, (o + 1) s / d)"""
    m = np.zeros((d, s))
    for o in range(d):
        a, b = o * s / d, (o + 1) * s / d
        for i in range(int(a), min(s, int(np.ceil(b)))):
            m[o, i] = (min(b, i + 1) - max(a, i)) * d / s
    return m


MEASURED = {}


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_close_to_the_area_mean(bpc):
    """R' against a float64 area mean on noise and on a ramp plus noise, at 34:1, 255.5:1 and 256:1.  The bound is derived, not measured.  A cumulative
    weight q_k is the exact one times 4096 rounded to an integer, so it is off by at most 1 / 8192 of the whole; by Abel summation the weighted sum of
    an axis is off by at most sum |P[k + 1] - P[k]| / 8192 over the taps of the output.  Down: that, per column, plus 2^-9 for the intermediate, which keeps 8
    of the 12 fraction bits; those errors pass the second axis with weights that sum to 1.  Across: the same rule on the
    intermediate as computed, and 0.5 for the final rounding."""
    rng = np.random.default_rng(18050 + bpc)
    mx = (1 << bpc) - 1
    worst = {}
    for (s, d) in ((238, 7), (511, 2), (512, 2)):
        by, bx = box_matrix(s, d), box_matrix(s, d)
        for content in ("noise", "ramp+noise"):
            if content == "noise":
                plane = rng.integers(0, mx + 1, (s, s))
            else:
                ramp = (np.arange(s)[:, None] + np.arange(s)[None, :]) * (0.8 * mx / (2 * s))
                plane = np.clip(ramp + rng.normal(0, mx / 64, (s, s)), 0, mx).round()
            plane = plane.astype(np.uint16)
            got, t = reduce_plane(plane, d, d, with_t=True)
            ref = by @ plane.astype(np.float64) @ bx.T
            p = plane.astype(np.float64)
            tv = t / 256.0
            bound = np.empty((d, d))
            for j, (j0, wj) in enumerate(area_weights(s, d)):
                err_down = np.abs(np.diff(p[j0:j0 + len(wj)], axis=0)).sum(0) / 8192 + 2.0 ** -9          # per column
                for o, (i0, wo) in enumerate(area_weights(s, d)):
                    bound[j, o] = 0.5 + bx[o] @ err_down + np.abs(np.diff(tv[j, i0:i0 + len(wo)])).sum() / 8192
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bound + 1e-9).all(), (bpc, s, d, content, float(err.max()), float(bound.max()))
            key = ("%.1f:1" % (s / d), content)
            worst[key] = max(worst.get(key, (0, 0)), (float(err.max()), float(bound.max())))
    MEASURED[bpc] = worst
    for key, (e, b) in sorted(worst.items()):
        print("bpc %d %s %s: largest distance %.3f codes, bound there at most %.3f" % (bpc, key[0], key[1], e, b))


# ------------------------------------------------------------------------------------------------ 3. every geometry class

@pytest.mark.parametrize("state", util.STATES)
@pytest.mark.parametrize("layout", [I400, I420, I422, I444], ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_geometry(ctx, bpc, layout, state):
    """planar native at chroma_pos 0 / 1 / 2; every third geometry per case, rotating so that every geometry meets every depth, layout and state"""
    pics = {}
    rot = (bpc // 2 + layout + util.STATES.index(state)) % 3
    try:
        for (w, h), crop, (dw, dh) in GEOMS[rot::3]:
            if (w, h) not in pics:
                pics[w, h] = make_source(ctx, np.random.default_rng(18100 + 100 * bpc + 10 * layout + w), w, h, layout, bpc, state, extremes=True)
            pic, vis = pics[w, h]
            crop = even_crop(crop, layout) if crop else None
            planes = reduced_planes(vis, layout, dw, dh, crop)
            for pos in (0, 1, 2):
                check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, P, N, pos, planes), dw, dh, P, N, crop, pos, what=state)
            assert pic.pic.twin_ok == {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}[state]
    finally:
        for pic, _ in pics.values():
            pic.free()


# ------------------------------------------------------------------------------------------------ 4. overflow guards, anchors

@pytest.mark.parametrize("value", [0, 1, 2047, 4095])
def test_constants_stay_constant_at_256_to_1(ctx, value):
    """12 bits, 256:1 and 255.5:1 on both axes, 4:4:4 with the identity matrix: the sums reach their largest values and every output is the value"""
    bpc, layout = 12, I444
    for (w, h), (dw, dh) in (((512, 512), (2, 2)), ((511, 511), (2, 2)), ((256, 256), (1, 1))):
        pic, _ = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", lambda pl, s: np.full(s, value))
        try:
            check(ctx, pic, [np.full((dh, dw), value, np.uint16)] * 3, dw, dh, P, N, None, 1, what="constant %d" % value, matrix=0)
        finally:
            pic.free()


@pytest.mark.parametrize("state", ["raster", "twin-only"])
def test_up_to_8_to_1_is_export_rgb_resized(ctx, state):
    """no plane axis above 8:1: the bytes of dav1d_hip_surface_export_rgb_resized, library against library"""
    w, h, bpc, layout = 190, 102, 10, I420
    pic, _ = make_source(ctx, np.random.default_rng(18300), w, h, layout, bpc, state, extremes=True)
    try:
        for crop, (dw, dh) in ((None, (95, 51)), (None, (24, 13)), ((10, 6, 133, 71), (224, 9)), (None, (200, 110)), ((10, 6, 133, 71), (133, 71)), (None, (190, 102))):
            for fmt, sample, pos in ((P, N, 1), (K4, F16, 2)):
                a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
                pic.export_rgb_resized(a.surface, crop, pos)
                pic.export_rgb_reduced(b.surface, crop, pos)
                same_bytes(a, b)
                a.free()
                b.free()
    finally:
        pic.free()


def test_exact_16_to_1_of_boxes(ctx):
    """a picture that is constant within each 16 x 16 box, 4:4:4 with the identity matrix: the box values come back"""
    w, h, bpc, layout = 208, 112, 10, I444
    rng = np.random.default_rng(18310)
    boxes = [rng.integers(0, 1024, (h // 16, w // 16)) for _ in range(3)]
    pic, vis = tr.make_picture(ctx, w, h, layout, bpc, "raster", lambda pl, s: boxes[pl][np.minimum(np.arange(s[0]) // 16, h // 16 - 1)[:, None], np.minimum(np.arange(s[1]) // 16, w // 16 - 1)[None, :]])
    try:
        want = [boxes[2].astype(np.uint16), boxes[0].astype(np.uint16), boxes[1].astype(np.uint16)]          # R, G, B = V, Y, U
        assert all(np.array_equal(a, b) for a, b in zip(want, want_of(vis, layout, bpc, w // 16, h // 16, None, P, N, 0, matrix=0)))
        check(ctx, pic, want, w // 16, h // 16, P, N, None, 0, what="16:1 of boxes", matrix=0)
    finally:
        pic.free()


def test_the_older_calls_still_refuse_9_to_1(ctx):
    w, h = 73, 73
    pic, vis = make_source(ctx, np.random.default_rng(18320), w, h, I420, 10, "raster")
    d, planar = Dest(ctx, 9, 9, I420, 10, K3, N), Dest(ctx, 9, 9, I420, 10, api.SURFACE_PLANAR, N)
    try:
        desc, p = C.byref(d.surface.desc), C.byref(pic.pic)
        src = (C.POINTER(api.Picture) * 1)(C.pointer(pic.pic))
        assert ctx.lib.dav1d_hip_surface_export_rgb_resized(ctx.h, desc, p, None, None, 0, 0, 1 << 30) == -ENOTSUP
        assert ctx.lib.dav1d_hip_surface_rgb_resized_rows_needed(desc, p, None, None, 0, 1 << 30) == -ENOTSUP
        assert ctx.lib.dav1d_hip_surface_export_rgb_resized_batch(ctx.h, 1, desc, src, None, None, 0, None) == -ENOTSUP
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled(ctx.h, desc, p, None, None, 0, 1 << 30) == -ENOTSUP
        assert ctx.lib.dav1d_hip_surface_export_rgb_scaled_batch(ctx.h, 1, desc, src, None, None, None) == -ENOTSUP
        assert ctx.lib.dav1d_hip_surface_export_scaled(ctx.h, C.byref(planar.surface.desc), p, None, 0, 1 << 30) == -ENOTSUP
        for x in (d, planar):
            x.check(None, what="a refused export")
        pic.export_rgb_reduced(d.surface, None, 1)
        d.check(want_of(vis, I420, 10, 9, 9, None, K3, N, 1), what="the shape the new call serves")
    finally:
        d.free()
        planar.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. nothing outside the crop is read

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [I420, I444], ids=["i420", "i444"])
def test_nothing_outside_the_crop_is_read(ctx, layout, state):
    """an interior crop of a picture whose samples outside the crop are 0 or max gives the bytes of the picture that is the crop alone"""
    bpc, (cw, ch), (x0, y0), (dw, dh) = 10, (200, 90), (22, 14), (7, 9)
    mx = (1 << bpc) - 1
    alone, vis = make_source(ctx, np.random.default_rng(18200 + layout), cw, ch, layout, bpc, state, extremes=True)
    big = ctx.picture(256, 128, layout, bpc)
    ssh, ssv = ss_of(layout)
    padded = []
    for pl in range(big.n_planes):
        sh, sv = (ssh, ssv) if pl else (0, 0)
        shape = big.padded_shape(pl)
        a = (((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) & 1) * mx).astype(big.dtype)
        a[y0 >> sv:(y0 >> sv) + vis[pl].shape[0], x0 >> sh:(x0 >> sh) + vis[pl].shape[1]] = vis[pl]
        padded.append(a)
    big.free()
    pic, _ = source_from(ctx, padded, 256, 128, layout, bpc, state)
    try:
        for fmt, sample, pos in ((P, N, 0), (P, N, 1), (K4, F16, 2)):
            a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            alone.export_rgb_reduced(a.surface, None, pos)
            pic.export_rgb_reduced(b.surface, (x0, y0, cw, ch), pos)
            same_bytes(a, b)
            b.check(want_of(vis, layout, bpc, dw, dh, None, fmt, sample, pos), what="the crop alone")
            a.free()
            b.free()
    finally:
        alone.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 6. formats and samples

@pytest.mark.parametrize("fmt", [P, K3, K4], ids=["planar", "rgb", "rgba"])
@pytest.mark.parametrize("bpc", [8, 10])
def test_formats_and_samples(ctx, bpc, fmt):
    """one geometry that goes down past 8:1 on both axes and one that is mixed, every sample type, with and without normalisation"""
    layout = I420
    mx = (1 << bpc) - 1
    pic, vis = make_source(ctx, np.random.default_rng(18400 + bpc), BIG[0], BIG[1], layout, bpc, "twin-only", extremes=True)
    try:
        for crop, (dw, dh) in (((14, 14, 300, 100), (21, 11)), ((0, 0, 240, 12), (12, 40))):
            planes = reduced_planes(vis, layout, dw, dh, crop)
            for sample in (N, M, F32, F16):
                if sample == M and bpc == 8:
                    continue
                want = want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, 1, planes)
                if fmt == K4:
                    alpha = {N: mx, M: mx << (16 - bpc), F32: 1.0, F16: 1.0}[sample]
                    assert (want[0][:, 3::4] == alpha).all()
                check(ctx, pic, want, dw, dh, fmt, sample, crop, 1, what="sample")
                if sample in (F32, F16):
                    scale, bias = rs.imagenet(bpc)
                    check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, 1, planes, scale=scale, bias=bias), dw, dh, fmt, sample, crop, 1, scale, bias,
                          what="normalised")
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 7. bands and rows needed

@pytest.mark.parametrize("band", [2, 6, 16])
@pytest.mark.parametrize("fmt,sample", [(P, N), (K4, F16)], ids=["planar", "rgba-f16"])
def test_bands(ctx, fmt, sample, band):
    """destination bands at chroma_pos 1: each alone leaves every other row at the sentinel, their union equals the one call"""
    (w, h), (dw, dh), bpc, layout = (200, 330), (21, 35), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(18500), w, h, layout, bpc, "twin-only")
    want = want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 1)
    try:
        whole = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
        for r0 in range(0, dh, band):
            r1 = min(r0 + band, dh)
            d = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            pic.export_rgb_reduced(d.surface, None, 1, row0=r0, row1=r1)
            d.check(want, rows=[(r0, r1)] * len(want), what="band [%d, %d)" % (r0, r1))
            d.free()
            pic.export_rgb_reduced(whole.surface, None, 1, row0=r0, row1=r1 if r1 < dh else 1 << 30)
        whole.check(want, what="the union of the bands")
        whole.free()
    finally:
        pic.free()


@pytest.mark.parametrize("crop,size", [((10, 6, 300, 100), (30, 11)), (None, (33, 9)), ((10, 6, 40, 110), (60, 12))], ids=["crop", "whole", "mixed"])
def test_rows_needed_is_safe_and_tight(ctx, crop, size):
    """For every band end r1: a copy of the source whose luma rows at and below rgb_reduced_rows_needed(r1), and the chroma rows under them, hold other
    values gives the same rows [0, r1): the band reads none of them.  With one row fewer than the helper says at least one band of the sweep changes.
    The answer is test_surface_resized's restatement of the rule, which knows no limit of the ratio."""
    (w, h), (dw, dh), bpc, layout, pos = BIG, size, 10, I420, 1
    pic, vis = make_source(ctx, np.random.default_rng(18600), w, h, layout, bpc, "raster")
    padded = [v.base for v in vis]
    want = want_of(vis, layout, bpc, dw, dh, crop, K3, N, pos)
    surface = Dest(ctx, dw, dh, layout, bpc, K3, N)
    tight = False
    try:
        last = 0
        for r1 in list(range(2, dh, 4)) + [dh]:
            need = pic.rgb_reduced_rows_needed(surface.surface, crop, pos, r1)
            assert last <= need <= h
            last = need
            assert need == rs.rows_needed(h, crop or (0, 0, w, h), dh, 1, pos, r1)
            assert pic.rgb_reduced_rows_needed(surface.surface, crop, 0, r1) == rs.rows_needed(h, crop or (0, 0, w, h), dh, 1, 0, r1)
            for rows, same in ((need, True), (need - 1, False)):
                other = [p.copy() for p in padded]
                other[0][rows:] ^= 0x155
                for pl in (1, 2):
                    other[pl][(rows + 1) >> 1 if same else rows >> 1:] ^= 0x155
                pic2, _ = source_from(ctx, other, w, h, layout, bpc, "twin-only")
                d = Dest(ctx, dw, dh, layout, bpc, K3, N)
                pic2.export_rgb_reduced(d.surface, crop, pos, row0=0, row1=r1)
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
        assert pic.rgb_reduced_rows_needed(surface.surface, crop, pos, 0) == 0
        assert pic.rgb_reduced_rows_needed(surface.surface, crop, pos, 1 << 30) == (crop[1] + crop[3] + (crop[3] & 1) if crop else h)
    finally:
        surface.free()
        pic.free()


def test_rows_needed_up_to_8_to_1_is_the_resized_calls(ctx):
    (w, h), bpc, layout = BIG, 10, I420
    pic, _ = make_source(ctx, np.random.default_rng(18650), w, h, layout, bpc, "raster")
    try:
        for size in ((47, 33), (400, 150)):
            d = Dest(ctx, size[0], size[1], layout, bpc, K3, N)
            for crop in (None, (10, 6, 133, 71)):
                for pos in (0, 1, 2):
                    for r1 in (0, 2, 10, 32, size[1], 1 << 30):
                        assert pic.rgb_reduced_rows_needed(d.surface, crop, pos, r1) == pic.rgb_resized_rows_needed(d.surface, crop, pos, r1)
            d.free()
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 8. unaligned destinations; the source is left alone; timed

@pytest.mark.parametrize("pad", [0, 2, 10])
@pytest.mark.parametrize("offset", [0, 2, 6])
def test_unaligned_destinations(ctx, offset, pad):
    """the sample-by-sample store path, whole units and the partial last unit (21 = 2 * 8 + 5 samples)"""
    (w, h), (dw, dh), layout = (300, 100), (21, 11), I420
    for bpc, fmt, sample in ((8, K3, N), (10, K4, F16)):
        pic, vis = make_source(ctx, np.random.default_rng(18700 + bpc), w, h, layout, bpc, "twin-only")
        try:
            check(ctx, pic, want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 2), dw, dh, fmt, sample, None, 2, pad=pad, offset=offset,
                  what="offset %d pad %d" % (offset, pad))
        finally:
            pic.free()


@pytest.mark.parametrize("state", ["twin-only", "raster"])
def test_source_untouched_and_timed(ctx, state):
    (w, h), (dw, dh), bpc, layout = BIG, (21, 11), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(18800), w, h, layout, bpc, state)
    try:
        raster = tsc._raster_bytes(ctx, pic)
        twin = util.twin_bytes(ctx, pic) if state == "twin-only" else None
        ptrs, ok = [pic.pic.twin[pl] for pl in range(3)], pic.pic.twin_ok
        if state == "twin-only":
            assert (raster == 0x5A).all()
        crop = (14, 14, 300, 100)
        check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 1), dw, dh, K4, F16, crop, 1, what=state)          # (the scratch is made here)
        live = tsc._live(ctx)
        check(ctx, pic, want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 1), dw, dh, K4, F16, crop, 1, what=state)
        ms = ctx.last_kernel_ms()
        assert ms > 0.0 if ctx.backend == "hip" else ms >= 0.0
        assert tsc._live(ctx) == live, "the call allocated an object in the steady state"
        assert pic.pic.twin_ok == ok and [pic.pic.twin[pl] for pl in range(3)] == ptrs
        assert np.array_equal(tsc._raster_bytes(ctx, pic), raster)
        if twin is not None:
            assert np.array_equal(util.twin_bytes(ctx, pic), twin)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 9. errors

def test_errors(ctx):
    w, h = 514, 102
    rng = np.random.default_rng(18900)
    pics = {key: make_source(ctx, rng, w, h, key[1], key[0], "raster")[0] for key in ((10, I420), (8, I420), (10, I422), (10, I444))}
    tall = make_source(ctx, rng, 64, 514, I420, 10, "raster")[0]

    def refused(code, fmt=K3, sample=N, size=(50, 12), crop=None, rows=(0, 1 << 30), change=None, key=(10, I420), params=None, helper=True, shape_as=None, flt=0, pic=None,
                **kw):
        pic = pic or pics[key]
        d = Dest(ctx, size[0], size[1], key[1], key[0], shape_as[0] if shape_as else fmt, shape_as[1] if shape_as else sample, **kw)
        d.surface.desc.format, d.surface.desc.sample = fmt, sample
        if change:
            change(d.surface.desc)
        rect = C.byref(api.SurfaceRect(*crop)) if crop is not None else None
        p = C.byref(params) if params is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_rgb_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), rect, p, flt, rows[0], rows[1])
        assert rc == -code, (rc, code, fmt, sample, crop, size, rows)
        d.check(None, what="a refused export")
        if helper:
            assert ctx.lib.dav1d_hip_surface_rgb_reduced_rows_needed(C.byref(d.surface.desc), C.byref(pic.pic), rect, p, flt, rows[1]) == -code
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
        for size in ((95, 51), (50, 12), (600, 110)):          # a size the resized call serves, one only this call does, one that goes up
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
                refused(EINVAL, fmt, N, rows=(1, 8), helper=False, size=size)                      # odd band rows
                refused(EINVAL, fmt, N, rows=(0, 9), size=size)
                for m in (2, 4, 8, 14, -1):
                    refused(ENOTSUP, fmt, N, matrix=m, size=size)
            refused(EINVAL, P, N, change=null_plane(2), size=size)
        assert ctx.lib.dav1d_hip_surface_export_rgb_reduced(None, None, None, None, None, 0, 0, 2) == -EINVAL
        # what dav1d_hip_surface_export_scaled refuses: the crop
        refused(EINVAL, crop=(500, 0, 100, 51))
        refused(EINVAL, crop=(0, 60, 95, 51))
        refused(EINVAL, crop=(-2, 0, 95, 51))
        refused(EINVAL, crop=(0, -2, 95, 51))
        refused(EINVAL, crop=(0, 0, 0, 51))
        refused(EINVAL, crop=(0, 0, 95, 0))
        refused(EINVAL, crop=(1, 0, 95, 51))
        refused(EINVAL, crop=(0, 1, 95, 51))
        refused(EINVAL, crop=(1, 0, 95, 51), key=(10, I422))
        # ... and the ratios above 256 downwards, whatever the other axis does
        refused(ENOTSUP, size=(2, 12))
        refused(ENOTSUP, size=(2, 51))
        refused(ENOTSUP, size=(2, 200))
        refused(ENOTSUP, size=(64, 2), pic=tall)
        refused(ENOTSUP, size=(8, 2), pic=tall)
        refused(ENOTSUP, size=(200, 2), pic=tall)
        refused(ENOTSUP, size=(1, 1), crop=(0, 0, 258, 2))
        # an unknown filter, alone and behind an older refusal (whose code wins)
        for flt in (1, -1, 7):
            refused(ENOTSUP, flt=flt)
            refused(ENOTSUP, flt=flt, size=(600, 110))
            refused(ENOTSUP, flt=flt, size=(2, 12))
            refused(EINVAL, flt=flt, crop=(1, 0, 95, 51))
        # what is accepted: the same surfaces with nothing wrong, 256:1 exactly, odd origins where the layout does not subsample the axis
        for key, crop, size in (((10, I420), None, (50, 12)), ((10, I420), (2, 0, 512, 102), (2, 12)), ((10, I422), (0, 1, 95, 51), (200, 3)),
                                ((10, I444), (1, 1, 95, 51), (3, 110)), ((8, I420), (0, 0, 184, 96), (23, 200)), ((10, I420), (0, 0, 256, 2), (1, 1))):
            for fmt in (P, K3, K4):
                d = Dest(ctx, size[0], size[1], key[1], key[0], fmt, F16, matrix=0 if key[1] == I444 else 6)
                pics[key].export_rgb_reduced(d.surface, crop, 2)
                assert pics[key].rgb_reduced_rows_needed(d.surface, crop, 2, 1 << 30) == (crop[1] + crop[3] if crop else h)
                ctx.sync()
                d.free()
    finally:
        for p in pics.values():
            p.free()
        tall.free()


def test_a_picture_of_another_device_is_refused():
    """-EXDEV by the check the frame calls use, on the emulator's two devices (tests/conftest.py)"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        pic = other.picture(128, 128, I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        d = Dest(ctx, 9, 9, I420, 10, K3, F16)
        assert ctx.lib.dav1d_hip_surface_export_rgb_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, None, 0, 0, 96) == -EXDEV
        assert ctx.lib.dav1d_hip_surface_export_rgb_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, None, 3, 0, 96) == -ENOTSUP          # the filter comes first
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
    (w, h), (dw, dh), bpc, layout = BIG, (14, 9), 10, I420
    pic, vis = make_source(ctx, np.random.default_rng(19000), w, h, layout, bpc, "retiled")
    s = ctx.surface(dw, dh, layout, bpc, K4, F16)
    try:
        s.fill(0xA5)
        crop = (10, 2, 300, 100)
        assert api._lib.SYMBOLS.count("dav1d_hip_surface_export_rgb_reduced") == 1
        pic.export_rgb_reduced(s, crop=crop, chroma_pos=api.CHROMA_COLOCATED, scale=[2.0, 1.0, 0.5], bias=[-1.0, 0.0, 1.0], filter=api.RESIZE_BILINEAR)
        got = s.download()[0]
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 2, scale=[np.float32(v) for v in (2.0, 1.0, 0.5)], bias=[np.float32(v) for v in (-1.0, 0.0, 1.0)])[0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        assert pic.rgb_reduced_rows_needed(s, crop, 1, 1 << 30) == 102
        assert pic.rgb_reduced_rows_needed(s, crop, 1, 4) == rs.rows_needed(h, crop, dh, 1, 1, 4) == 2 + 67
        with pytest.raises(api.HipError):
            pic.rgb_reduced_rows_needed(s, (1, 0, 95, 51), 1, 10)
        with pytest.raises(api.HipError, match="errno %d" % ENOTSUP):
            pic.export_rgb_reduced(s, crop, filter=3)
        with pytest.raises(api.HipError, match="errno %d" % ENOTSUP):
            pic.export_rgb_resized(s, crop)
    finally:
        s.free()
        pic.free()


def test_export_to_tensor_value_errors():
    """interp="area" is refused before anything reaches the library where interp="bilinear" is; "bicubic" still is no filter"""
    from test_surface_batch import FakeTensor
    t = FakeTensor((3, 54, 96))
    for kw in (dict(interp="area"), dict(interp="area", resize=True, grain=object()), dict(interp="area", colour=object()),
               dict(interp="area", resize=True, colour=object()), dict(interp="bicubic", resize=True)):
        with pytest.raises(ValueError):
            api.export_to_tensor(object(), t, **kw)
    with pytest.raises(ValueError):
        api.export_batch_to_tensor([object()] * 4, FakeTensor((4, 3, 54, 96)), interp="bicubic")
