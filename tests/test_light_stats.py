"""Per-picture light statistics on the device (dav1d_hip_picture_light_stats and the dav1d_hip_light_stats_* calls; dav1d_amd/csrc/surface_stats.hip,
DESIGN.md 10.13): a histogram of a picture's luminance over the index of a toned handle's gain, the pixels above 1.0, the pixels at or below 0 and the
largest light.

Every comparison of counts is exact.  The oracle is the suite's own numpy: test_surface_rgb.rgb_values on the crop window for the integers, the
handle's lin, test_surface_tone.tone for the index (its arithmetic restated here for Y, with .astype(f32) behind every product and sum, and
asserted equal to it) and np.bincount.  Every case with `ctx` runs on the emulated build and, under -m gpu, on the device; the host helpers are checked
without a backend."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import util
import test_surface as ts
import test_surface_colour as tc
import test_surface_rgb as tr
import test_surface_scaled as tsc
import test_surface_tone as tn
from dav1d_amd import _lib, api
from dav1d_amd._lib import LightStatsData, SurfaceRect

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
F32, F16 = api.SAMPLE_F32, api.SAMPLE_F16
ENC_N = tc.ENC_N
f32 = np.float32
ONES = np.full(ENC_N, 0x3C00, np.uint16)
SIZES = [(67, 35), (130, 66), (1030, 130)]          # odd and one cell; two cells across; past one 1024-column span and more cells than a workgroup has waves


# ------------------------------------------------------------------------------------------------ the definition, restated

def window(vis, layout, crop):
    """the planes of the crop window W = (x0, y0, w, h) taken as a picture of its own"""
    if crop is None:
        return vis
    x0, y0, w, h = crop
    ss_h, ss_v = tr.subsampling(layout)
    out = [vis[0][y0:y0 + h, x0:x0 + w]]
    if layout != I400:
        out += [v[y0 >> ss_v:(y0 + h + ss_v) >> ss_v, x0 >> ss_h:(x0 + w + ss_h) >> ss_h] for v in vis[1:]]
    return out


def luminance(l, k):
    """step 1b's Y and h on three float32 planes of light; h is test_surface_tone.tone's"""
    k = np.asarray(k, f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = [(k[j] * l[j]).astype(f32) for j in range(3)]
        y = ((p[0] + p[1]).astype(f32) + p[2]).astype(f32)
        x = np.where(y > 0, np.where(y < 1, y, f32(1)), f32(0)).astype(f32)
        h = x.astype(np.float16).view(np.uint16)
    index = []
    tn.tone(l, k, ONES, index)
    assert np.array_equal(index[0], h)
    return y, h


def np_stats(vis, layout, bpc, lin, k, crop=None, matrix=1, full_range=0, pos=0, rows=None):
    """what an accumulator holds after one call on a zeroed one"""
    lin = np.asarray(lin, f32)
    l = [lin[v] for v in tr.rgb_values(window(vis, layout, crop), layout, bpc, matrix, full_range, pos)]
    if rows is not None:
        l = [c[rows[0]:rows[1]] for c in l]
    if not l[0].size:
        return {"n": 0, "n_above": 0, "n_nonpos": 0, "max_light": f32(-np.inf), "hist": np.zeros(ENC_N, np.uint64)}
    y, h = luminance(l, k)
    return {"n": int(y.size), "n_above": int((y > 1).sum()), "n_nonpos": int((~(y > 0)).sum()),
            "max_light": f32(max(c.max() for c in l)), "hist": np.bincount(h.ravel(), minlength=ENC_N).astype(np.uint64)}


def plus(a, b):
    return {"n": a["n"] + b["n"], "n_above": a["n_above"] + b["n_above"], "n_nonpos": a["n_nonpos"] + b["n_nonpos"],
            "max_light": max(a["max_light"], b["max_light"]), "hist": a["hist"] + b["hist"]}


def same(got, want, what=""):
    assert (got["n"], got["n_above"], got["n_nonpos"]) == (want["n"], want["n_above"], want["n_nonpos"]), what
    assert got["max_light"] == want["max_light"], (what, got["max_light"], want["max_light"])
    bad = np.flatnonzero(got["hist"] != want["hist"])
    assert not bad.size, (what, bad[:8], got["hist"][bad[:8]], want["hist"][bad[:8]])
    assert int(got["hist"].sum()) == got["n"], what


def random_light(rng, bpc):
    """lin finite, of either sign, away from the denormals; k in [-1, 1]"""
    lin = (rng.uniform(-8, 8, 1 << bpc) * np.exp2(rng.integers(-8, 1, 1 << bpc))).astype(f32)
    lin[np.abs(lin) < 2.0 ** -20] = f32(0.25)
    while True:          # coefficients of both signs, no denormal products, and a sum that takes grey (4:0:0: R = G = B) past 1 as well
        k = rng.uniform(-1, 1, 3).astype(f32)
        if (k > 0).any() and (k < 0).any() and (np.abs(k) >= 2.0 ** -10).all() and abs(float(k.sum())) >= 0.3:
            return lin, k


def live(ctx):
    return tsc._live(ctx), int(ctx.lib.dav1d_hip_light_stats_alive())


# ------------------------------------------------------------------------------------------------ 1. the sweep

CASES = [(bpc, layout, state) for bpc in (8, 10, 12) for layout in (I400, I420, I422, I444) for state in util.STATES]


def deal(i):
    """size, crop, matrix, full_range, chroma_pos of case i"""
    bpc, layout, state = CASES[i]
    w, h = SIZES[(i + i // 3) % 3]
    pos = (i + i // 12) % 3
    matrix = (0, 1, 9)[(i // 3 + i // 12) % 3] if layout == I444 else (1, 9)[i % 2]
    full_range = (i // 2) % 2
    crop = None
    if state != "raster":          # odd width and height, x0 / y0 even and no multiple of 8
        x0, y0 = 2 + 4 * (i % 3), 2 + 4 * ((i // 3) % 2)
        crop = (x0, y0, (w - x0 - 2) | 1, (h - y0 - 2) | 1)
    return w, h, crop, matrix, full_range, pos


def test_the_cases_meet_every_value_of_every_option():
    met = [CASES[i] + deal(i) for i in range(len(CASES))]
    assert {m[0] for m in met} == {8, 10, 12} and {m[1] for m in met} == {I400, I420, I422, I444} and {m[2] for m in met} == set(util.STATES)
    assert {(m[3], m[4]) for m in met} == set(SIZES) and {m[6] for m in met} == {0, 1, 9} and {m[7] for m in met} == {0, 1} and {m[8] for m in met} == {0, 1, 2}
    for layout in (I420, I422):          # the layouts whose taps chroma_pos changes: every position, both ranges, every size
        mine = [m for m in met if m[1] == layout]
        assert {m[8] for m in mine} == {0, 1, 2} and {m[7] for m in mine} == {0, 1} and {(m[3], m[4]) for m in mine} == set(SIZES)
    crops = [m for m in met if m[2] == "twin-only"]
    assert all(m[5] is not None and m[5][0] % 8 and m[5][1] % 8 and m[5][2] % 2 and m[5][3] % 2 for m in crops)
    assert {m[1] for m in crops} == {I400, I420, I422, I444} and {(m[3], m[4]) for m in crops} == set(SIZES)
    for m in met:
        if m[5] is not None:
            x0, y0, cw, ch = m[5]
            assert cw > 0 and ch > 0 and x0 + cw <= m[3] and y0 + ch <= m[4]
    assert (1030 + 63) // 64 * ((130 + 7) // 8) > 8 and 1030 > 1024


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%dbit-l%d-%s" % c for c in CASES])
def test_random_tables(ctx, case):
    bpc, layout, state = CASES[case]
    w, h, crop, matrix, full_range, pos = deal(case)
    rng = np.random.default_rng(50000 + case)
    lin, k = random_light(rng, bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, state, extremes=True)
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    try:
        want = np_stats(vis, layout, bpc, lin, k, crop, matrix, full_range, pos)
        assert 0 < want["n_above"] and 0 < want["n_nonpos"] and want["n_above"] + want["n_nonpos"] < want["n"], "Y lies below 0, inside and above 1"
        st.add(pic, colour, k, crop=crop, matrix=matrix, full_range=full_range, chroma_pos=pos)
        same(st.read(), want, "%dx%d crop %s matrix %d range %d chroma_pos %d" % (w, h, crop, matrix, full_range, pos))
        assert pic.pic.twin_ok == {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}[state]
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


# ------------------------------------------------------------------------------------------------ 2. additivity

def test_a_fresh_accumulator_reads_as_zero(ctx):
    before = live(ctx)
    st = ctx.light_stats()
    assert live(ctx) == (before[0], before[1] + 1)
    got = st.read()
    assert (got["n"], got["n_above"], got["n_nonpos"]) == (0, 0, 0) and got["max_light"] == -np.inf and not got["hist"].any() and got["hist"].size == ENC_N
    assert st.mean() == 0.0
    with pytest.raises(api.HipError, match="errno %d" % EINVAL):
        st.rank(0.5)
    st.free()
    assert live(ctx) == before


@pytest.mark.parametrize("pos", [1, 2])
def test_the_bands_of_a_picture_add_up_to_the_picture(ctx, pos):
    w, h, layout, bpc = 130, 66, I420, 10
    rng = np.random.default_rng(50100 + pos)
    lin, k = random_light(rng, bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    colour, st, band = ctx.colour(lin, bpc=bpc), ctx.light_stats(), ctx.light_stats()
    crop = (6, 2, 121, 63)
    try:
        for cr in (None, crop):
            rows = (cr or (0, 0, w, h))[3]
            whole = np_stats(vis, layout, bpc, lin, k, cr, pos=pos)
            st.reset()
            for r0, r1 in ((0, 2), (2, 34), (34, rows), (rows + 1 & ~1, rows + 9), (40, 1 << 30)):
                r1c = max(min(r1, rows), min(r0, rows))
                st.add(pic, colour, k, crop=cr, chroma_pos=pos, row0=r0, row1=r1)
                band.reset()
                band.add(pic, colour, k, crop=cr, chroma_pos=pos, row0=r0, row1=r1)
                same(band.read(), np_stats(vis, layout, bpc, lin, k, cr, pos=pos, rows=(r0, r1c)), "band [%d, %d) alone, crop %s" % (r0, r1, cr))
            same(st.read(), plus(whole, np_stats(vis, layout, bpc, lin, k, cr, pos=pos, rows=(40, rows))), "three bands (and one of them again), crop %s" % (cr,))
            st.reset()
            st.add(pic, colour, k, crop=cr, chroma_pos=pos, row0=-5)
            same(st.read(), whole, "the whole picture, rows clamped")
    finally:
        st.free()
        band.free()
        ctx.colour_destroy(colour)
        pic.free()


def test_two_pictures_in_one_accumulator_and_reset_between_them(ctx):
    rng = np.random.default_rng(50200)
    lin8, k8 = random_light(rng, 8)
    lin10, k10 = random_light(rng, 10)
    a, va = util.make_source(ctx, rng, 67, 35, I422, 8, "raster")
    b, vb = util.make_source(ctx, rng, 130, 66, I420, 10, "twin-only")
    ca, cb, st = ctx.colour(lin8, bpc=8), ctx.colour(lin10, bpc=10), ctx.light_stats()
    try:
        wa, wb = np_stats(va, I422, 8, lin8, k8, pos=2), np_stats(vb, I420, 10, lin10, k10, pos=1, matrix=9, full_range=1)
        st.add(a, ca, k8, chroma_pos=2)          # no sync in between
        st.add(b, cb, k10, chroma_pos=1, matrix=9, full_range=1)
        same(st.read(), plus(wa, wb), "two pictures")
        st.reset()
        st.add(b, cb, k10, chroma_pos=1, matrix=9, full_range=1)
        same(st.read(), wb, "the second alone after a reset")
        st.reset()
        got = st.read()
        assert got["n"] == 0 and got["max_light"] == -np.inf and not got["hist"].any()
    finally:
        st.free()
        ctx.colour_destroy(ca)
        ctx.colour_destroy(cb)
        a.free()
        b.free()


# ------------------------------------------------------------------------------------------------ 3. concentration

def test_a_flat_picture_is_one_bin(ctx):
    """133,900 pixels, more than 2^16, in one bin: every lane of every wave agrees with its first"""
    w, h, bpc = 1030, 130, 10
    rng = np.random.default_rng(50300)
    lin = tc.random_tables(rng, bpc)[0]
    pic, vis = tr.make_picture(ctx, w, h, I420, bpc, "twin-only", lambda pl, s: np.full(s, (400, 500, 600)[pl]))
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    try:
        k = np.array([0.01, 0.02, 0.005], f32)
        want = np_stats(vis, I420, bpc, lin, k, pos=1)
        assert w * h == 133900 > 1 << 16 and want["hist"].max() == w * h and 0 < int(np.argmax(want["hist"])) < 0x3C00
        st.add(pic, colour, k, chroma_pos=1)
        same(st.read(), want, "flat")
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


def test_a_checkerboard_of_two_luminances(ctx):
    """neighbouring lanes and neighbouring pixels of a lane disagree: two bins, half the pixels each; then every eighth column: the lanes agree, the pixels of a lane do not"""
    w, h, bpc = 130, 66, 8
    lin = np.linspace(0, 1, 1 << bpc).astype(f32)
    k = np.array([0.25, 0.5, 0.125], f32)
    yy, xx = np.mgrid[0:128, 0:256]
    for name, board in (("checkerboard", (xx + yy) & 1), ("columns", (xx & 7) == 3), ("rows", yy & 1)):
        pic, vis = tr.make_picture(ctx, w, h, I400, bpc, "raster", lambda pl, s: np.where(board[:s[0], :s[1]], 200, 40))
        colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
        try:
            want = np_stats(vis, I400, bpc, lin, k, full_range=1)
            assert np.count_nonzero(want["hist"]) == 2, name
            st.add(pic, colour, k, full_range=1)
            same(st.read(), want, name)
        finally:
            st.free()
            ctx.colour_destroy(colour)
            pic.free()


def test_codes_that_walk_every_value(ctx):
    """many bins: 4:4:4 with matrix 0, so the samples are the codes, R walking every value along a row"""
    w, h, bpc = 1030, 18, 12
    lin = (np.arange(1 << bpc) / f32(4095)).astype(f32)
    pic, vis = tr.make_picture(ctx, w, h, I444, bpc, "twin-only", lambda pl, s: (np.arange(s[0] * s[1]).reshape(s) * (1, 3, 5)[pl]) % (1 << bpc))
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    try:
        k = np.array([1, 0, 0], f32)
        want = np_stats(vis, I444, bpc, lin, k, matrix=0)
        assert np.count_nonzero(want["hist"]) > 3000
        st.add(pic, colour, k, matrix=0)
        same(st.read(), want, "walk")
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


# ------------------------------------------------------------------------------------------------ 4. the edges of Y

def test_edges_of_the_luminance_index(ctx):
    """4:4:4 with matrix 0: every pixel of a flat picture is (code, 0, 0), k = (1, 0, 0) and lin[0] = +0, so Y = lin[code] exactly; one picture per value"""
    w, h, bpc = 24, 4, 8
    special = dict(tn_special())
    lin = np.zeros(1 << bpc, f32)
    for i, (v, _) in enumerate(special.values()):
        lin[i + 1] = v
        assert float(lin[i + 1]) == v, "the special values are float32 values"
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    try:
        for i, (name, (v, e)) in enumerate(special.items()):
            pic, vis = tr.make_picture(ctx, w, h, I444, bpc, "twin-only", lambda pl, s: np.full(s, i + 1 if pl == 2 else 0))          # planes Y, U, V are G, B, R
            st.reset()
            st.add(pic, colour, [1, 0, 0], matrix=0)
            got = st.read()
            same(got, np_stats(vis, I444, bpc, lin, [1, 0, 0], matrix=0), name)
            assert got["hist"][e] == w * h and got["n_above"] == (w * h if v > 1 else 0) and got["n_nonpos"] == (0 if v > 0 else w * h), name
            assert got["max_light"] == max(f32(v), f32(0)), name
            pic.free()
    finally:
        st.free()
        ctx.colour_destroy(colour)


def tn_special():
    """the values of test_surface_tone.test_edges_of_the_luminance_index and the bin each falls into, with +0"""
    return {
        "one": (1.0, 0x3C00), "just below one": (float(np.nextafter(f32(1), f32(0))), 0x3C00), "just above one": (float(np.nextafter(f32(1), f32(2))), 0x3C00),
        "the last half below one": (1 - 2.0 ** -11, 0x3BFF), "sixteen": (16.0, 0x3C00), "the smallest subnormal": (2.0 ** -24, 1), "the tie with zero": (2.0 ** -25, 0),
        "just above that tie": (2.0 ** -25 * (1 + 2.0 ** -20), 1), "a tie between halves, down": (0.5 + 2.0 ** -12, 0x3800), "a tie between halves, up": (0.5 + 3 * 2.0 ** -12, 0x3802),
        "a tie between subnormals, down": (2.5 * 2.0 ** -24, 2), "a tie between subnormals, up": (3.5 * 2.0 ** -24, 4), "the largest subnormal": (1023 * 2.0 ** -24, 0x3FF),
        "negative": (-0.75, 0), "plus zero": (0.0, 0),
    }


def test_minus_zero_nan_and_both_overflows(ctx):
    """Y = -0.0 (k of minus zeros on positive light), NaN (inf - inf: large finite k of opposite signs on light of 2 .. 16), +inf and -inf"""
    w, h, bpc = 67, 35, 10
    rng = np.random.default_rng(50400)
    lin = rng.uniform(2, 16, 1 << bpc).astype(f32)
    pic, vis = tc._gbr_picture(ctx, w, h, bpc, lambda pl, s: rng.integers(0, 1 << bpc, size=s))
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    big, n = 3e38, w * h
    try:
        l = [lin[v] for v in tr.rgb_values(vis, I444, bpc, 0, 0, 0)]
        for name, k, e, above, nonpos in (("-0.0", [-0.0, -0.0, -0.0], 0, 0, n), ("NaN", [big, -big, 0.0], 0, 0, n), ("+inf", [big, big, 0.0], 0x3C00, n, 0), ("-inf", [-big, -big, 0.0], 0, 0, n)):
            y, _ = luminance(l, k)
            assert {"-0.0": (y == 0).all() and np.signbit(y).all(), "NaN": np.isnan(y).all(), "+inf": np.isposinf(y).all(), "-inf": np.isneginf(y).all()}[name], name
            st.reset()
            st.add(pic, colour, k, matrix=0)
            got = st.read()
            same(got, np_stats(vis, I444, bpc, lin, k, matrix=0), name)
            assert got["hist"][e] == n and (got["n_above"], got["n_nonpos"]) == (above, nonpos), name
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. independence

def test_a_tone_part_of_the_handle_is_ignored_and_the_source_stays(ctx):
    w, h, layout, bpc = 131, 19, I420, 10
    rng = np.random.default_rng(50500)
    lin, m, enc = tc.random_tables(rng, bpc)
    k = np.array([0.3, -0.2, 0.1], f32)
    plain, toned = ctx.colour(lin, m, enc, bpc=bpc), ctx.colour(lin, m, enc, bpc=bpc, tone=tn.random_tone(rng))
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    a, b = ctx.light_stats(), ctx.light_stats()
    try:
        twin, raster = util.twin_bytes(ctx, pic), tsc._raster_bytes(ctx, pic)
        a.add(pic, plain, k, chroma_pos=1)
        b.add(pic, toned, k, chroma_pos=1)
        want = np_stats(vis, layout, bpc, lin, k, pos=1)
        same(a.read(), want, "un-toned handle")
        same(b.read(), want, "toned handle")
        assert pic.pic.twin_ok == api.TWIN_ONLY
        assert np.array_equal(util.twin_bytes(ctx, pic), twin) and np.array_equal(tsc._raster_bytes(ctx, pic), raster)
    finally:
        a.free()
        b.free()
        ctx.colour_destroy(plain)
        ctx.colour_destroy(toned)
        pic.free()


def test_exports_around_a_stats_call_write_their_usual_bytes(ctx):
    """export, stats, export, stats with no sync in between"""
    w, h, layout, bpc = 131, 19, I420, 10
    rng = np.random.default_rng(50600)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    colour = ctx.colour(lin, m, enc, bpc=bpc, tone=tp)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    st = ctx.light_stats()
    d = [ts.Dest(ctx, w, h, layout, bpc, K4, F16), ts.Dest(ctx, w, h, layout, bpc, P, F32)]
    try:
        ctx.sync()
        pic.export_rgb_colour(d[0].surface, colour, 1)
        st.add(pic, colour, tp[0], chroma_pos=1)
        pic.export_rgb_colour(d[1].surface, colour, 2)
        st.add(pic, colour, tp[0], chroma_pos=2, row0=2, row1=10)
        d[0].check(tn.expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, tp), what="the export in front of the stats call")
        d[1].check(tn.expect(vis, layout, bpc, P, F32, 2, lin, m, enc, tp), what="the export behind it")
        same(st.read(), plus(np_stats(vis, layout, bpc, lin, tp[0], pos=1), np_stats(vis, layout, bpc, lin, tp[0], pos=2, rows=(2, 10))), "between exports")
        assert ctx.last_kernel_ms() >= 0.0
    finally:
        for x in d:
            x.free()
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


# ------------------------------------------------------------------------------------------------ 6. refusals

def _raw(ctx, st, pic, colour, k, crop=None, matrix=1, full_range=0, pos=0, row0=0, row1=1 << 30, c=True):
    kk = (C.c_float * 3)(*[float(v) for v in k]) if k is not None else None
    return ctx.lib.dav1d_hip_picture_light_stats(ctx.h if c else None, st, C.byref(pic) if pic is not None else None,
                                                 C.byref(SurfaceRect(*crop)) if crop is not None else None, matrix, full_range, pos, colour, kk, row0, row1)


def test_refusals_in_their_order(ctx):
    w, h, layout, bpc = 66, 34, I420, 10
    rng = np.random.default_rng(50700)
    lin, k = random_light(rng, bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    colour, other_depth, st = ctx.colour(lin, bpc=bpc), ctx.colour(lin[:256], bpc=8), ctx.light_stats()
    try:
        st.add(pic, colour, k, row1=4)
        held, before = st.read(), live(ctx)
        st._data = None
        good = dict(st=st.h, pic=pic.pic, colour=colour, k=k)

        def call(**kw):
            a = dict(good, **kw)
            return _raw(ctx, a.pop("st"), a.pop("pic"), a.pop("colour"), a.pop("k"), **a)
        nan_k, bad_pic = [0.5, np.nan, 0.5], _lib.Picture.from_buffer_copy(pic.pic)
        bad_pic.bpc = 9
        assert call(row0=8, row1=8) == 0 and call(row0=20, row1=10) == 0 and call(row0=h, row1=h + 10) == 0, "an empty row range is 0 and counts nothing"
        # 1. NULL arguments, in front of everything else
        for kw in (dict(c=False), dict(st=None), dict(pic=None), dict(colour=None), dict(k=None)):
            assert call(**kw) == -EINVAL and call(matrix=2, **kw) == -EINVAL, kw
        # 2. the picture, the crop, the matrix, chroma_pos and the rows, with the export's codes and in its order, in front of 3, 4 and 5
        for later in ({}, dict(k=nan_k), dict(colour=other_depth)):
            assert call(pic=bad_pic, matrix=2, **later) == -EINVAL
            assert call(matrix=2, **later) == -ENOTSUP and call(matrix=2, crop=(1, 0, 8, 8), **later) == -ENOTSUP and call(matrix=2, pos=3, **later) == -ENOTSUP
            assert call(matrix=0, **later) == -EINVAL, "matrix 0 needs 4:4:4"
            assert call(pos=3, **later) == -EINVAL and call(pos=-1, **later) == -EINVAL
            assert call(row0=1, **later) == -EINVAL and call(row1=7, **later) == -EINVAL and call(row1=h - 1, **later) == -EINVAL
            for crop in ((1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 0, 8), (0, 0, 8, -1), (-2, 0, 8, 8), (60, 0, 8, 8), (0, 30, 8, 8)):
                assert call(crop=crop, **later) == -EINVAL, crop
            assert call(crop=(0, 0, 9, 9), row1=7, **later) == -EINVAL, "an odd row1 is W's end or nothing"
        # 3. and 4.
        for bad in (np.nan, np.inf, -np.inf):
            for i in range(3):
                kk = [0.5, 0.5, 0.5]
                kk[i] = bad
                assert call(k=kk) == -EINVAL and call(k=kk, colour=other_depth) == -EINVAL
        assert call(colour=other_depth) == -EINVAL
        assert live(ctx) == before
        same(st.read(), held, "the accumulator after the refusals")
        assert call(crop=(0, 0, 9, 9), row0=8, row1=9) == 0          # (W's end)
        st._data = None
        assert st.read()["n"] == held["n"] + 9
    finally:
        st.free()
        ctx.colour_destroy(colour)
        ctx.colour_destroy(other_depth)
        pic.free()


def test_refused_calls_leave_the_accumulator_alone(ctx):
    w, h, layout, bpc = 66, 34, I420, 10
    rng = np.random.default_rng(50800)
    lin, k = random_light(rng, bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "raster")
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    try:
        st.add(pic, colour, k)
        want = np_stats(vis, layout, bpc, lin, k)
        for kw in (dict(matrix=2), dict(matrix=0), dict(pos=3), dict(row0=1), dict(crop=(1, 0, 8, 8)), dict(crop=(0, 0, 80, 8))):
            assert _raw(ctx, st.h, pic.pic, colour, k, **kw) < 0
        assert _raw(ctx, st.h, pic.pic, colour, [np.nan, 0, 0]) == -EINVAL
        st._data = None
        same(st.read(), want, "after refused calls")
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


def test_another_devices_picture_handle_and_accumulator_are_refused():
    """-EXDEV on the emulator's two devices (tests/conftest.py), behind everything else"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        rng = np.random.default_rng(50900)
        lin, k = random_light(rng, 10)
        foreign_colour, foreign_st, foreign_pic = other.colour(lin, bpc=10), other.light_stats(), other.picture(64, 64, I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        pic, colour, st = ctx.picture(64, 64, I420, 10), ctx.colour(lin, bpc=10), ctx.light_stats()
        assert _raw(ctx, st.h, pic.pic, colour, k) == 0
        for kw in (dict(pic=foreign_pic.pic), dict(colour=foreign_colour), dict(st=foreign_st.h)):
            a = dict(dict(st=st.h, pic=pic.pic, colour=colour), **kw)
            assert _raw(ctx, a["st"], a["pic"], a["colour"], k) == -EXDEV, kw
            assert _raw(ctx, a["st"], a["pic"], a["colour"], [np.nan, 0, 0]) == -EINVAL and _raw(ctx, a["st"], a["pic"], a["colour"], k, matrix=2) == -ENOTSUP, kw
        assert ctx.lib.dav1d_hip_light_stats_reset(ctx.h, foreign_st.h) == -EXDEV
        assert ctx.lib.dav1d_hip_light_stats_read(ctx.h, foreign_st.h, C.byref(LightStatsData())) == -EXDEV
        got = foreign_st.read()
        assert got["n"] == 0 and not got["hist"].any()
        assert st.read()["n"] == 64 * 64
        for x in (pic, st):
            x.free()
        ctx.colour_destroy(colour)
        ctx.lib.dav1d_hip_context_use(other.h)
        foreign_pic.free()
        foreign_st.free()
        other.colour_destroy(foreign_colour)
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


def test_null_arguments_of_the_other_calls(ctx):
    st = ctx.light_stats()
    lib = ctx.lib
    try:
        assert lib.dav1d_hip_light_stats_create(None, C.byref(C.c_void_p())) == -EINVAL and lib.dav1d_hip_light_stats_create(ctx.h, None) == -EINVAL
        assert lib.dav1d_hip_light_stats_reset(None, st.h) == -EINVAL and lib.dav1d_hip_light_stats_reset(ctx.h, None) == -EINVAL
        assert lib.dav1d_hip_light_stats_read(None, st.h, C.byref(LightStatsData())) == -EINVAL and lib.dav1d_hip_light_stats_read(ctx.h, None, C.byref(LightStatsData())) == -EINVAL
        assert lib.dav1d_hip_light_stats_read(ctx.h, st.h, None) == -EINVAL
        assert lib.dav1d_hip_light_stats_destroy(ctx.h, None) == 0
    finally:
        st.free()


# ------------------------------------------------------------------------------------------------ 7. the host helpers

@pytest.fixture(scope="module")
def hostlib():
    return _lib.load(util.emu_lib_path())


def _record(hist):
    d = LightStatsData()
    np.ctypeslib.as_array(d.hist)[:] = hist
    d.n = int(hist.sum())
    return d


def test_rank_against_cumsum(hostlib):
    rng = np.random.default_rng(51000)
    for trial in range(6):
        hist = np.zeros(ENC_N, np.uint64)
        idx = rng.choice(ENC_N, size=(3, 40, 2000, ENC_N)[trial % 4], replace=False)
        hist[idx] = rng.integers(1, (1 << 40) if trial & 1 else 50, idx.size).astype(np.uint64)
        d, cum, n = _record(hist), np.cumsum(hist), int(hist.sum())
        ranks = {1, n, n // 2, n // 3 + 1, max(1, int(np.ceil(0.999 * n)))} | {int(c) for c in cum[idx[:20]]} | {int(c) + 1 for c in cum[idx[:20]] if c < n}
        for rank in ranks:
            h = C.c_int(-1)
            assert hostlib.dav1d_hip_light_stats_rank(C.byref(d), rank, C.byref(h)) == 0
            assert h.value == int(np.searchsorted(cum, np.uint64(rank), side="left")), (trial, rank)
            assert hist[h.value] > 0
        h = C.c_int(-7)
        assert hostlib.dav1d_hip_light_stats_rank(C.byref(d), 0, C.byref(h)) == -EINVAL and hostlib.dav1d_hip_light_stats_rank(C.byref(d), n + 1, C.byref(h)) == -EINVAL
        assert hostlib.dav1d_hip_light_stats_rank(None, 1, C.byref(h)) == -EINVAL and hostlib.dav1d_hip_light_stats_rank(C.byref(d), 1, None) == -EINVAL and h.value == -7


def test_mean_is_the_ascending_double_sum(hostlib):
    rng = np.random.default_rng(51100)
    value = np.arange(ENC_N, dtype=np.uint16).view(np.float16).astype(np.float64)
    for trial in range(4):
        hist = rng.integers(0, (1 << 30) if trial & 1 else 3, ENC_N).astype(np.uint64)
        total = 0.0
        for h in range(ENC_N):          # ascending, one addition at a time: what the header says
            total += float(hist[h]) * float(value[h])
        assert hostlib.dav1d_hip_light_stats_mean(C.byref(_record(hist))) == total / float(hist.sum()), trial
    one = np.zeros(ENC_N, np.uint64)
    one[0x3800] = 5
    assert hostlib.dav1d_hip_light_stats_mean(C.byref(_record(one))) == 0.5
    assert hostlib.dav1d_hip_light_stats_mean(C.byref(LightStatsData())) == 0.0 and hostlib.dav1d_hip_light_stats_mean(None) == 0.0


def test_python_rank_and_mean(ctx):
    w, h, layout, bpc = 67, 35, I420, 10
    rng = np.random.default_rng(51200)
    lin = tc.random_tables(rng, bpc)[0]
    k = np.array([0.02, 0.05, 0.01], f32)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "raster")
    colour, st = ctx.colour(lin, bpc=bpc), ctx.light_stats()
    try:
        for name in ("dav1d_hip_picture_light_stats", "dav1d_hip_light_stats_rank", "dav1d_hip_light_stats_mean", "dav1d_hip_colour_update_tone"):
            assert api._lib.SYMBOLS.count(name) == 1
        st.add(pic, colour, k)
        want = np_stats(vis, layout, bpc, lin, k)
        cum = np.cumsum(want["hist"])
        for fraction in (0.0, 0.5, 0.999, 1.0):
            assert st.rank(fraction) == int(np.searchsorted(cum, max(1, int(np.ceil(fraction * want["n"]))), side="left")), fraction
        value = np.arange(ENC_N, dtype=np.uint16).view(np.float16).astype(np.float64)
        assert abs(st.mean() - float((want["hist"] * value).sum()) / want["n"]) <= 1e-12
        with pytest.raises(ValueError):
            st.add(pic, colour, [1, 2])
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            st.add(pic, colour, [np.nan, 0, 0])
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


# ------------------------------------------------------------------------------------------------ 8. end to end: a measured peak

def measured_peak_chain(ctx, rng):
    """A PQ / BT.2020 10-bit picture through a handle made for a nominal peak of 1000 nits: its 99.9th-percentile bin from the device, in nits (the helper's
    lin counts light in units of its peak with an encoded output, so k = K 1000 / 10000 makes the index luminance in units of 10,000 nits), clamped to at
    least white_nits, becomes peak_nits of dav1d_hip_colour_tables_toned; that call's k and gain, rescaled by 1000 / peak to the unit of the live handle's
    lin, go into it through dav1d_hip_colour_update_tone; an export follows.  The bytes are those of the same chain computed from the numpy histogram."""
    w, h, layout, bpc, white, nominal = 130, 66, I420, 10, 203.0, 1000.0
    lin, m, enc, has_matrix, has_enc, K, gain, has_gain = api.colour_tables_toned(ctx.lib, bpc, 16, 9, 13, 1, white, nominal)
    assert has_matrix and has_enc and has_gain and lin[-1] == f32(10000.0 / nominal)
    k_stats = (K.astype(np.float64) * nominal / 10000.0).astype(f32)
    pic, vis = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", lambda pl, s: rng.integers(64, 680, size=s) if pl == 0 else rng.integers(480, 544, size=s))
    colour, st = ctx.colour(lin, m, enc, bpc=bpc, tone=(K, gain)), ctx.light_stats()
    try:
        st.add(pic, colour, k_stats, matrix=9, chroma_pos=1)
        value = np.arange(ENC_N, dtype=np.uint16).view(np.float16).astype(np.float64)
        parts = []
        for source in ("device", "numpy"):
            if source == "device":
                bin_ = st.rank(0.999)
            else:
                ws = np_stats(vis, layout, bpc, lin, k_stats, matrix=9, pos=1)
                bin_ = int(np.searchsorted(np.cumsum(ws["hist"]), max(1, int(np.ceil(0.999 * ws["n"]))), side="left"))
            peak = max(white, float(value[bin_]) * 10000.0)
            assert white < peak < nominal, peak
            _, _, enc2, _, _, K2, gain2, _ = api.colour_tables_toned(ctx.lib, bpc, 16, 9, 13, 1, white, peak)
            assert np.array_equal(enc2, enc), "the pure transfer does not know the peak"
            scale = nominal / peak
            parts.append(((K2.astype(np.float64) * scale).astype(f32), (gain2.view(np.float16).astype(np.float64) * scale).astype(np.float16).view(np.uint16)))
        assert not np.array_equal(parts[1][1], gain)
        ctx.colour_update_tone(colour, parts[0])
        tc.export_and_check(ctx, pic, colour, tn.expect(vis, layout, bpc, K4, F16, 1, lin, m.reshape(9), enc, parts[1], matrix=9), K4, F16, "measured peak", pos=1, matrix=9)
    finally:
        st.free()
        ctx.colour_destroy(colour)
        pic.free()


def test_a_measured_peak_end_to_end(ctx):
    measured_peak_chain(ctx, np.random.default_rng(51300))


def _child():
    ctx = api.Context(0)
    ctx.backend = "hip"
    measured_peak_chain(ctx, np.random.default_rng(51300))
    ctx.close()
    print("child ok")


@pytest.mark.gpu
def test_a_measured_peak_end_to_end_in_a_process_of_its_own():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    if sys.argv[1:] == ["child"]:
        _child()
