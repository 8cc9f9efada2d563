"""Linear-light scaling for the colour-managed tensor export: dav1d_hip_surface_export_rgb_linear_reduced and dav1d_hip_surface_rgb_linear_rows_needed
(dav1d_amd/csrc/surface_linear.hip).

The crop window W is converted to integer R, G, B at its own size, every code is replaced by its light in fixed point (q of the handle), the light is
averaged with the 12-bit weights of R' in one exact integer sum A per channel, and l = float32(A) * 2^(e - 55) goes through steps 2 to 4 of the
colour-managed export.  The oracle is composed from what exists and adds no pixel arithmetic of its own: test_surface_rgb.rgb_values on
test_surface_scaled.windows for the integers, test_surface_reduced.axis_weights for the taps, int64 sums for A, numpy's uint64 -> float32 and an exact
power of two for l, test_surface_colour.stage (fed l through an identity-indexed table) and finish for the rest.  Every comparison is exact; every
destination is filled with 0xA5 first and compared byte by byte, padding included.  Every case with `ctx` runs on the emulated build and, under -m gpu,
on the device."""
import ctypes as C

import numpy as np
import pytest

import util
import test_surface_colour as tc
import test_surface_reduced as rd
import test_surface_resized as rs
import test_surface_rgb as tr
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
f32 = np.float32
BIG = (330, 120)
LN_NCOL, LN_OW = 1024, 256          # the cell of surface_linear.hip: source columns, outputs across

# ((picture), crop or None, (output)): test_surface_reduced.GEOMS as they stand, the resized classes, odd crops at 4:2:0
OWN = [(BIG, (8, 4, 24, 24), (40, 40)),               # up on both axes
       (BIG, (0, 0, 2, 2), (5, 3)),                   # two-sample axes going up
       (BIG, (4, 2, 1, 1), (1, 1)),                   # one-sample axes
       (BIG, (0, 0, 200, 2), (1, 2)),                 # 200 -> 1 next to 2 -> 2
       (BIG, (10, 6, 133, 71), (133, 71)),            # d == s from a crop, odd width and height
       (BIG, (10, 6, 133, 71), (19, 9)),              # odd crop width and height going down: the last luma column / row has a chroma sample of its own
       (BIG, (2, 2, 21, 9), (21, 5)),                 # ... where W's last chroma column is the fourth of a unit of 8, not its last
       ((190, 102), None, (96, 54))]                  # under 8:1 on every axis
GEOMS = list(rd.GEOMS) + OWN

STAGES = ["lin", "lin+matrix", "all"]
COMBOS = [(st, fmt, sample, norm, pos) for pos in (0, 1, 2) for norm in (0, 1) for sample in (F32, F16) for fmt in (P, K3, K4) for st in STAGES]
CASES = [(bpc, layout, state) for bpc in (8, 10, 12) for layout in (I400, I420, I422, I444) for state in util.STATES]


def combo_of(case, gi):
    return COMBOS[((case * len(GEOMS) + gi) * 37) % len(COMBOS)]          # 37 and 108 share no factor


# ------------------------------------------------------------------------------------------------ the oracle, composed

def q_of(lin):
    """the light table in fixed point and its exponent, from the definition; None where an entry is negative"""
    lin = np.asarray(lin, f32)
    if (lin < 0).any():
        return None, 0
    m = lin.max()
    e = int(np.frexp(np.float64(m))[1]) if m > 0 else 0
    q = np.rint(np.ldexp(lin.astype(np.float64), 31 - e))
    assert q.max() < 2 ** 31
    return q.astype(np.uint32), e


def sums(vis, layout, bpc, dw, dh, crop, pos, q, matrix=1, full_range=0):
    """A_c: the exact integers, three (dh, dw) int64 planes"""
    crop = crop or (0, 0, vis[0].shape[1], vis[0].shape[0])
    values = tr.rgb_values(windows(vis, layout, crop), layout, bpc, matrix, full_range, pos)
    wy, wx = rd.axis_weights(crop[3], dh), rd.axis_weights(crop[2], dw)
    out = []
    for v in values:
        assert v.shape == (crop[3], crop[2])
        light = q.astype(np.int64)[v]
        t = np.empty((dh, crop[2]), np.int64)
        for j, (i0, ws) in enumerate(wy):
            assert sum(ws) == 4096
            t[j] = (np.array(ws, np.int64)[:, None] * light[i0:i0 + len(ws)]).sum(0)
        assert t.max() < 1 << 43
        a = np.empty((dh, dw), np.int64)
        for o, (i0, ws) in enumerate(wx):
            assert sum(ws) == 4096
            a[:, o] = (np.array(ws, np.int64)[None, :] * t[:, i0:i0 + len(ws)]).sum(1)
        assert a.min() >= 0 and a.max() < 1 << 55
        out.append(a)
    return out


def light_of(a, e):
    """l = float32(A) * 2^(e - 55): numpy's uint64 -> float32 rounds to nearest even, the power of two is exact"""
    return [np.ldexp(x.astype(np.uint64).astype(f32), e - 55).astype(f32) for x in a]


def after_light(l, sample, fmt, m=None, enc=None, scale=None, bias=None):
    """steps 2 to 4 through test_surface_colour.stage, which indexes a table: the table is l itself"""
    n = l[0].size
    table = np.concatenate([x.ravel() for x in l])
    index = [np.arange(k * n, (k + 1) * n).reshape(l[0].shape) for k in range(3)]
    planes, alpha = tc.finish(tc.stage(index, table, m, enc), sample, scale, bias)
    return tr.arrange(planes, alpha, fmt)


def want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tables, matrix=1, full_range=0, scale=None, bias=None):
    lin, m, enc = tables
    q, e = q_of(lin)
    return after_light(light_of(sums(vis, layout, bpc, dw, dh, crop, pos, q, matrix, full_range), e), sample, fmt, m, enc, scale, bias)


def check(ctx, pic, colour, want, dw, dh, fmt, sample, crop=None, pos=0, scale=None, bias=None, rows=(0, 1 << 30), what="", **kw):
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export_rgb_linear_reduced(d.surface, colour, crop, pos, scale, bias, rows[0], rows[1])
        d.check(want, what="%s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d chroma_pos %d" % (what, pic.w, pic.h, dw, dh, crop, pic.bpc, pic.layout,
                                                                                                       fmt, sample, pos))
    finally:
        d.free()


def cells_across(s, d):
    """the cells across an axis that goes down (linear_item_fill of surface_linear.hip)"""
    ow = max(1, min(LN_OW, (LN_NCOL - 9) * d // s))
    return -(-d // ow)


# ------------------------------------------------------------------------------------------------ 1. the case list, the table, closeness (CPU only)

def test_the_cases_meet_every_combination():
    assert len(COMBOS) == 108 and len(CASES) == 36
    met = {}
    for case in range(len(CASES)):
        for gi in range(len(GEOMS)):
            met.setdefault(combo_of(case, gi), set()).add(CASES[case])
    assert set(met) == set(COMBOS) and min(len(v) for v in met.values()) >= 4
    for what, index in (("stage", 0), ("format", 1), ("sample", 2), ("normalisation", 3), ("chroma_pos", 4)):
        for gi in range(len(GEOMS)):          # every geometry meets every value of every option
            assert {combo_of(case, gi)[index] for case in range(len(CASES))} == {c[index] for c in COMBOS}, (what, gi)


def test_the_geometries_are_what_they_claim():
    """from the sizes alone"""
    assert GEOMS[:len(rd.GEOMS)] == rd.GEOMS
    assert cells_across(2047, 8) >= 2 and max(len(w) for _, w in rd.area_weights(2047, 8)) == 257          # 257 taps over more than one cell
    assert (2048, 16) == rd.GEOMS[4][0] and rd.GEOMS[4][2][0] * 256 == 2048 and max(len(w) for _, w in rd.area_weights(511, 2)) == 256
    assert rd.GEOMS[5] == ((256, 256), None, (1, 1)) and rd.GEOMS[11][2][0] > LN_OW
    assert all((c[0] >> 1) & 7 == 7 and (c[1] >> 1) & 7 == 7 for _, c, _ in rd.GEOMS[6:7]) and rd.GEOMS[7][1][0] & 7 == 7
    up, two, one, mixed, same, odd, odd2, under = OWN
    assert up[2][0] > up[1][2] and up[2][1] > up[1][3] and two[1][2:] == (2, 2) and one[1][2:] == (1, 1)
    assert rs.plane_axes(I444, 3, 80, 4, 4)[0] == ((3, 4), (80, 4)) and rs.plane_axes(I444, 80, 3, 4, 4)[0] == ((80, 4), (3, 4))          # (in rd.GEOMS)
    assert same[1][2:] == same[2]
    for g in (same, odd, odd2):          # the last luma column and row share their chroma sample with nothing
        assert g[1][2] & 1 and g[1][3] & 1 and not g[1][0] & 1 and not g[1][1] & 1
    # W's last chroma column, which the column behind it is clamped to: the last of a unit of 8 samples, and the last of a unit's first half
    assert ((odd[1][0] + odd[1][2] - 1) >> 1) & 7 == 7 and ((odd2[1][0] + odd2[1][2] - 1) >> 1) & 7 == 3 and (BIG[0] + 1) >> 1 > 100
    assert all(d <= s <= 8 * d for s, d in ((190, 96), (102, 54)))


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_q_from_the_definition(bpc):
    """q < 2^31, the largest entry keeps 31 bits, a power-of-two lin is exact"""
    rng = np.random.default_rng(30000 + bpc)
    lin = tc.random_tables(rng, bpc)[0]
    q, e = q_of(lin)
    assert q.max() >= 1 << 30 and q.max() < 1 << 31 and lin.max() < 2.0 ** e <= 2 * lin.max()
    assert np.abs(q.astype(np.float64) * 2.0 ** (e - 31) - lin.astype(np.float64)).max() <= 2.0 ** (e - 32)
    q2, e2 = q_of(np.full(1 << bpc, 0.25, f32))
    assert e2 == -1 and (q2 == 1 << 30).all()
    assert q_of(np.zeros(1 << bpc, f32))[1] == 0 and not q_of(np.zeros(1 << bpc, f32))[0].any()
    lin[5] = -lin[5]
    assert q_of(lin)[0] is None


@pytest.mark.parametrize("bpc,crop,size", [(10, (0, 0, 330, 120), (9, 7)), (12, (10, 6, 133, 71), (19, 9)), (8, (8, 4, 24, 24), (40, 40)), (10, (0, 0, 256, 102), (1, 1))])
def test_close_to_the_float64_mean(bpc, crop, size):
    """numpy only.  Against sum wy wx lin / 2^24 in float64 with the same weights, per output sample: |l - exact| <= 2^(e - 32) + ulp(l) / 2 — the
    quantisation of q (half a unit of 2^(e - 31) per sample, carried through weights that sum to one) plus the one rounding to binary32"""
    rng = np.random.default_rng(30100 + bpc)
    lin = tc.random_tables(rng, bpc)[0]
    q, e = q_of(lin)
    w, h = BIG
    vis = [rng.integers(0, 1 << bpc, (h, w)) for _ in range(3)]
    a = sums(vis, I444, bpc, size[0], size[1], crop, 0, q)
    exact = sums(vis, I444, bpc, size[0], size[1], crop, 0, np.arange(1 << bpc))          # the codes' own sums: the taps and weights, reused below
    values = tr.rgb_values(windows(vis, I444, crop), I444, bpc, 1, 0, 0)
    wy, wx = rd.axis_weights(crop[3], size[1]), rd.axis_weights(crop[2], size[0])
    for ch, l in enumerate(light_of(a, e)):
        light = lin.astype(np.float64)[values[ch]]
        mean = np.array([[sum(wa * wb * light[i0 + ka, k0 + kb] for ka, wa in enumerate(ws) for kb, wb in enumerate(wk)) for k0, wk in wx] for i0, ws in wy]) / 2.0 ** 24
        ulp = np.spacing(l.astype(f32)).astype(np.float64)
        assert (np.abs(l.astype(np.float64) - mean) <= 2.0 ** (e - 32) + ulp / 2 + mean * 2.0 ** -50).all()          # (the last term: the float64 sum itself)
    assert exact[0].max() < 1 << (24 + bpc)


# ------------------------------------------------------------------------------------------------ 2. every geometry, every combination

@pytest.mark.parametrize("case", range(len(CASES)), ids=["%dbit-l%d-%s" % c for c in CASES])
def test_every_geometry(ctx, case):
    """every geometry in every depth, layout and picture state; the stage, format, sample, normalisation and chroma_pos are dealt over them in turn"""
    bpc, layout, state = CASES[case]
    rng = np.random.default_rng(30200 + case)
    lin, m, enc = tc.random_tables(rng, bpc)
    tables = {"lin": (lin, None, None), "lin+matrix": (lin, m, None), "all": (lin, m, enc)}
    handles = {st: ctx.colour(*tables[st], bpc=bpc) for st in STAGES}
    pics = {}
    try:
        for gi, ((w, h), crop, (dw, dh)) in enumerate(GEOMS):
            if (w, h) not in pics:
                pics[w, h] = make_source(ctx, np.random.default_rng(30300 + 100 * bpc + 10 * layout + w), w, h, layout, bpc, state, extremes=True)
            pic, vis = pics[w, h]
            crop = even_crop(crop, layout) if crop else None
            st, fmt, sample, norm, pos = combo_of(case, gi)
            scale = [f32(v) for v in rng.uniform(0.5, 2, 3)] if norm else None
            bias = [f32(v) for v in rng.uniform(-1, 1, 3)] if norm else None
            want = want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tables[st], scale=scale, bias=bias)
            check(ctx, pic, handles[st], want, dw, dh, fmt, sample, crop, pos, scale, bias, what="%s %s norm %d" % (state, st, norm))
            assert pic.pic.twin_ok == {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}[state]
    finally:
        ctx.sync()
        for pic, _ in pics.values():
            pic.free()
        for hd in handles.values():
            ctx.colour_destroy(hd)


# ------------------------------------------------------------------------------------------------ 3. anchors with a formula of their own

@pytest.mark.parametrize("bpc,layout,state", [(10, I420, "twin-only"), (8, I422, "raster"), (12, I444, "retiled")])
def test_same_size_with_a_dyadic_lin_is_export_rgb_colour_on_the_crop(ctx, bpc, layout, state):
    """d == s: one tap of 4096 x 4096, A = q 2^24; a lin of dyadic entries within 2^7 of its largest has q exact and below 2^24 significant bits,
    so l == lin[code] and the bytes are dav1d_hip_surface_export_rgb_colour's on the picture that is the crop"""
    rng = np.random.default_rng(30400 + bpc)
    _, m, enc = tc.random_tables(rng, bpc)
    lin = (rng.integers(1 << 16, 1 << 23, 1 << bpc) * 2.0 ** -20).astype(f32)          # in [2^-4, 8): within 2^7, 23 bits each
    assert lin.max() / lin.min() <= 128
    colour = ctx.colour(lin, m, enc, bpc=bpc)
    (w, h), crop = BIG, even_crop((10, 6, 133, 71), layout)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, state, extremes=True)
    alone, _ = source_from(ctx, [np.ascontiguousarray(v) for v in padded_windows(ctx, vis, layout, bpc, crop)], crop[2], crop[3], layout, bpc, "raster")
    try:
        for fmt, sample, pos in ((P, F32, 1), (K4, F16, 2), (K3, F16, 0)):
            a, b = Dest(ctx, crop[2], crop[3], layout, bpc, fmt, sample), Dest(ctx, crop[2], crop[3], layout, bpc, fmt, sample)
            alone.export_rgb_colour(a.surface, colour, pos)
            pic.export_rgb_linear_reduced(b.surface, colour, crop, pos)
            same_bytes(a, b)
            a.free()
            b.free()
    finally:
        pic.free()
        alone.free()
        ctx.colour_destroy(colour)


def padded_windows(ctx, vis, layout, bpc, crop):
    """the crop's windows in padded planes of a picture of the crop's size"""
    probe = ctx.picture(crop[2], crop[3], layout, bpc)
    out = []
    for pl, win in enumerate(windows(vis, layout, crop)):
        a = np.zeros(probe.padded_shape(pl), probe.dtype)
        a[:win.shape[0], :win.shape[1]] = win
        out.append(a)
    probe.free()
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_a_ramp_gives_the_unrounded_mean_of_the_codes(ctx, bpc):
    """lin[v] = v 2^-bpc, identity matrix at 4:4:4: q[v] = v 2^(31 - bpc) and A == 2^(31 - bpc) sum w v exactly; l is that sum's float32"""
    rng = np.random.default_rng(30500 + bpc)
    lin = (np.arange(1 << bpc) * 2.0 ** -bpc).astype(f32)
    q, e = q_of(lin)
    assert e == 0 and np.array_equal(q, np.arange(1 << bpc, dtype=np.uint32) << (31 - bpc))
    (w, h), crop, (dw, dh) = BIG, (14, 14, 300, 100), (21, 11)
    pic, vis = make_source(ctx, rng, w, h, I444, bpc, "twin-only", extremes=True)
    colour = ctx.colour(lin, bpc=bpc)
    try:
        a = sums(vis, I444, bpc, dw, dh, crop, 0, q, matrix=0)
        codes = sums(vis, I444, bpc, dw, dh, crop, 0, np.arange(1 << bpc, dtype=np.uint32), matrix=0)
        assert all(np.array_equal(x, y << (31 - bpc)) for x, y in zip(a, codes))
        want = [np.ldexp(y.astype(np.uint64).astype(f32), -24 - bpc).astype(f32) for y in codes]
        check(ctx, pic, colour, want, dw, dh, P, F32, crop, 0, what="ramp", matrix=0)
    finally:
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("value", [0, 1, 2047, 4095])
def test_a_constant_picture_at_12_bits_and_256_to_1(ctx, value):
    """4:4:4 with the identity matrix: the sums reach their largest values; every sample is enc[f16(float(q[v] << 24) * 2^(e - 55))]"""
    bpc, layout = 12, I444
    rng = np.random.default_rng(30600)
    lin, _, enc = tc.random_tables(rng, bpc)
    q, e = q_of(lin)
    colour = ctx.colour(lin, enc=enc, bpc=bpc)
    l = np.ldexp(f32(np.uint64(int(q[value]) << 24)), e - 55)
    want16 = enc[np.asarray(min(max(l, f32(0)), f32(1)), f32).astype(np.float16).view(np.uint16)]
    try:
        for (w, h), (dw, dh) in (((256, 256), (1, 1)), ((1024, 16), (4, 2))):
            pic, _ = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", lambda pl, s: np.full(s, value))
            try:
                check(ctx, pic, colour, [np.full((dh, dw), want16, np.uint16)] * 3, dw, dh, P, F16, None, 1, what="constant %d" % value, matrix=0)
            finally:
                pic.free()
    finally:
        ctx.colour_destroy(colour)


def test_a_permutation_matrix_swaps_the_planes(ctx):
    (w, h), (dw, dh), bpc, layout = BIG, (21, 11), 10, I420
    rng = np.random.default_rng(30700)
    lin = tc.random_tables(rng, bpc)[0]
    plain, swapped = ctx.colour(lin, bpc=bpc), ctx.colour(lin, matrix=[0, 0, 1, 0, 1, 0, 1, 0, 0], bpc=bpc)
    pic, _ = make_source(ctx, rng, w, h, layout, bpc, "raster")
    a, b = ctx.surface(dw, dh, layout, bpc, P, F32), ctx.surface(dw, dh, layout, bpc, P, F32)
    try:
        pic.export_rgb_linear_reduced(a, plain, None, 1)
        pic.export_rgb_linear_reduced(b, swapped, None, 1)
        x, y = a.download(), b.download()
        assert all(np.array_equal(x[k].view(np.uint32), y[2 - k].view(np.uint32)) for k in range(3))
        assert not np.array_equal(x[0], x[2])
    finally:
        a.free()
        b.free()
        pic.free()
        ctx.colour_destroy(plain)
        ctx.colour_destroy(swapped)


@pytest.mark.parametrize("layout", [I400, I444])
def test_ties_of_the_conversion_to_binary32(ctx, layout):
    """a 2 x 1 picture to 1 x 1: the weights are 2048 x 4096, A = 2^23 (q0 + q1), and binary32 has steps of 2^30 from 2^53 on.  With q = 2^30 and
    0x40 A is 2^53 + 2^29, half a step above the even 2^53: down.  With 2^30 and 0xC0 A is 2^53 + 3 2^29, half a step above the odd 2^53 + 2^30: up to
    2^53 + 2^31.  (The issue behind this file names 0x80 and 0x180 for the two ties; under its own weights those give 2^53 + 2^30 and 2^53 + 3 2^30,
    which binary32 holds exactly.  They are kept as cases — the conversion must not move them — next to the two that are ties.)"""
    bpc = 8
    lin = np.zeros(256, f32)
    for second, want_a in ((0x80, (1 << 53) + (1 << 30)), (0x180, (1 << 53) + 3 * (1 << 30)), (0x40, 1 << 53), (0xC0, (1 << 53) + (1 << 31))):
        lin[:] = 0
        lin[255], lin[10], lin[20] = 1 - 2.0 ** -24, 0.5, second * 2.0 ** -31          # (the largest entry sets e = 0)
        q, e = q_of(lin)
        assert e == 0 and q[10] == 1 << 30 and q[20] == second
        colour = ctx.colour(lin, bpc=bpc)
        pic, vis = tr.make_picture(ctx, 2, 1, layout, bpc, "raster", lambda pl, s: np.tile(np.array([10, 20]), (s[0], (s[1] + 1) // 2))[:, :s[1]])
        try:
            full = Dest(ctx, 1, 1, layout, bpc, P, F32, matrix=0 if layout == I444 else 1, full_range=1)
            pic.export_rgb_linear_reduced(full.surface, colour)
            a = sums(vis, layout, bpc, 1, 1, None, 0, q, matrix=0 if layout == I444 else 1, full_range=1)
            if layout == I444:
                assert all(int(x[0, 0]) == (1 << 23) * ((1 << 30) + second) for x in a)
                assert all(f32(np.uint64(int(x[0, 0]))) == f32(want_a) for x in a)
            full.check(light_of(a, e), what="tie %x" % second)
            full.free()
        finally:
            pic.free()
            ctx.colour_destroy(colour)


@pytest.mark.parametrize("size", [(160, 60), (9, 3)], ids=["2to1", "34to1"])
def test_a_checkerboard_of_pq_codes_is_brighter_than_the_mean_of_its_codes(ctx, size):
    """The point of the feature: a one-pixel checkerboard of PQ codes 64 / 940 (10 bit, grey), PQ / BT.2020 to sRGB / BT.709.  The new call equals its
    oracle and every sample is strictly above dav1d_hip_surface_export_rgb_colour_reduced's, which averages the codes"""
    bpc, layout, (w, h) = 10, I420, (320, 120)
    assert (w // size[0] in (2,) and h // size[1] == 2) or (w > 34 * size[0] and h > 34 * size[1])
    lin, m, enc, has_matrix, has_enc = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
    assert has_matrix and has_enc
    tables = (lin, m.reshape(9), enc)
    colour = ctx.colour(*tables, bpc=bpc)

    def fill(pl, s):
        if pl:
            return np.full(s, 512)
        return np.where((np.arange(s[0])[:, None] + np.arange(s[1])[None, :]) & 1, 940, 64)
    pic, vis = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", fill)
    a, b = ctx.surface(size[0], size[1], layout, bpc, P, F32), ctx.surface(size[0], size[1], layout, bpc, P, F32)
    try:
        check(ctx, pic, colour, want_of(vis, layout, bpc, size[0], size[1], None, P, F32, 1, tables), size[0], size[1], P, F32, None, 1, what="checkerboard")
        pic.export_rgb_linear_reduced(a, colour, None, 1)
        pic.export_rgb_colour_reduced(b, colour, None, 1)
        x, y = a.download(), b.download()
        assert all((x[k] > y[k]).all() for k in range(3))
    finally:
        a.free()
        b.free()
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 4. bands and rows needed

def rows_needed(h, crop, dh, ssv, pos, r1):
    """the definition: the luma rows the taps down of rows [0, r1) take, and with sited chroma at 4:2:0 the chroma row below"""
    if r1 <= 0:
        return 0
    r1 = min(r1, dh)
    taps = rd.axis_weights(crop[3], dh)
    n = crop[1] + max(i0 + len(ws) for i0, ws in taps[:r1])
    return n if not pos or not ssv else min(crop[1] + crop[3], n + 2)


@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("geom", [((200, 330), None, (21, 35)), ((190, 102), None, (96, 54)), (BIG, (8, 4, 24, 24), (40, 40))], ids=["over", "under", "up"])
def test_bands(ctx, geom, pos):
    """even destination bands: each alone leaves every other row at the sentinel, their union is the one call"""
    (w, h), crop, (dw, dh) = geom
    bpc, layout = 10, I420
    rng = np.random.default_rng(30800)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    fmt, sample = (P, F32) if pos == 1 else (K4, F16)
    want = want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tables)
    try:
        for band in (2, 6, 16):
            whole = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            for r0 in range(0, dh, band):
                r1 = min(r0 + band, dh)
                d = Dest(ctx, dw, dh, layout, bpc, fmt, sample)
                pic.export_rgb_linear_reduced(d.surface, colour, crop, pos, row0=r0, row1=r1)
                d.check(want, rows=[(r0, r1)] * len(want), what="band [%d, %d)" % (r0, r1))
                d.free()
                pic.export_rgb_linear_reduced(whole.surface, colour, crop, pos, row0=r0, row1=r1 if r1 < dh else 1 << 30)
            whole.check(want, what="the union of the bands of %d" % band)
            whole.free()
    finally:
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("crop,size", [((10, 6, 300, 100), (30, 11)), (None, (96, 40)), ((10, 6, 40, 110), (60, 12)), ((10, 6, 40, 20), (60, 50))], ids=["over", "under", "mixed", "up"])
def test_a_band_reads_no_row_at_or_beyond_rows_needed(ctx, crop, size, pos):
    """For every band end r1: a copy of the source whose luma rows at and beyond dav1d_hip_surface_rgb_linear_rows_needed(r1), and the chroma rows
    under them, hold other values gives the same rows [0, r1)"""
    (w, h), (dw, dh), bpc, layout = BIG, size, 10, I420
    rng = np.random.default_rng(30900)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "raster")
    padded = [v.base for v in vis]
    want = want_of(vis, layout, bpc, dw, dh, crop, K3, F16, pos, tables)
    surface = Dest(ctx, dw, dh, layout, bpc, K3, F16)
    try:
        assert pic.rgb_linear_rows_needed(surface.surface, crop, pos, 0) == 0 and pic.rgb_linear_rows_needed(surface.surface, crop, pos, -4) == 0
        for r1 in list(range(2, dh, 4)) + [dh]:
            need = pic.rgb_linear_rows_needed(surface.surface, crop, pos, r1)
            assert need == rows_needed(h, crop or (0, 0, w, h), dh, 1, pos, r1)
            other = [p.copy() for p in padded]
            other[0][need:] ^= 0x155
            for pl in (1, 2):
                other[pl][(need + 1) >> 1:] ^= 0x155
            pic2, _ = source_from(ctx, other, w, h, layout, bpc, "twin-only" if r1 & 2 else "raster")
            d = Dest(ctx, dw, dh, layout, bpc, K3, F16)
            pic2.export_rgb_linear_reduced(d.surface, colour, crop, pos, row0=0, row1=r1)
            d.check(want, rows=[(0, r1)], what="rows from %d on changed, band [0, %d)" % (need, r1))
            d.free()
            pic2.free()
    finally:
        surface.free()
        pic.free()
        ctx.colour_destroy(colour)


def test_rows_needed_refuses_what_the_export_refuses(ctx):
    pic = ctx.picture(514, 102, I420, 10)
    try:
        for size, crop, sample, flt, pos, r1, code in (((2, 12), None, F16, 0, 0, 2, ENOTSUP), ((50, 12), (1, 0, 95, 51), F16, 0, 0, 2, EINVAL), ((50, 12), None, N, 0, 0, 2, EINVAL),
                                                       ((50, 12), None, F16, 3, 0, 2, ENOTSUP), ((50, 12), None, F16, 0, 3, 2, EINVAL), ((50, 12), None, F16, 0, 1, 3, EINVAL)):
            s = ctx.surface(size[0], size[1], I420, 10, K3, sample)
            with pytest.raises(api.HipError, match="errno %d" % code):
                pic.rgb_linear_rows_needed(s, crop, pos, r1, filter=flt)
            s.free()
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. memory and state

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [I420, I444], ids=["i420", "i444"])
def test_nothing_outside_the_crop_takes_part(ctx, layout, state):
    """an interior crop (odd width and height) of a picture whose samples outside the crop are 0 or max gives the bytes of the picture that is the crop alone"""
    bpc, (cw, ch), (x0, y0) = 10, (199, 89), (22, 14)
    mx = (1 << bpc) - 1
    rng = np.random.default_rng(31000 + layout)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    alone, vis = make_source(ctx, rng, cw, ch, layout, bpc, state, extremes=True)
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
        for (dw, dh), fmt, sample, pos in (((7, 9), P, F32, 1), ((100, 45), K4, F16, 2), ((230, 100), K3, F16, 1), ((199, 89), P, F16, 1)):
            a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            alone.export_rgb_linear_reduced(a.surface, colour, None, pos)
            pic.export_rgb_linear_reduced(b.surface, colour, (x0, y0, cw, ch), pos)
            same_bytes(a, b)
            b.check(want_of(vis, layout, bpc, dw, dh, None, fmt, sample, pos, tables), what="the crop alone")
            a.free()
            b.free()
    finally:
        alone.free()
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("pad", [0, 2, 10])
@pytest.mark.parametrize("offset", [0, 2, 6])
def test_unaligned_destinations(ctx, offset, pad):
    """destinations off every alignment and with padded strides; sentinel gaps between the rows"""
    (w, h), (dw, dh), layout = (300, 100), (21, 11), I420
    for bpc, fmt, sample, k in ((8, K3, F16, 1), (10, K4, F16, 1), (10, K4, F32, 2), (10, P, F32, 2)):          # (k: offset and pad stay multiples of the sample)
        rng = np.random.default_rng(31100 + bpc)
        tables = tc.random_tables(rng, bpc)
        colour = ctx.colour(*tables, bpc=bpc)
        pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
        try:
            check(ctx, pic, colour, want_of(vis, layout, bpc, dw, dh, None, fmt, sample, 2, tables), dw, dh, fmt, sample, None, 2, pad=pad * k, offset=offset * k,
                  what="offset %d pad %d" % (offset * k, pad * k))
        finally:
            pic.free()
            ctx.colour_destroy(colour)


@pytest.mark.parametrize("state", ["twin-only", "raster"])
def test_source_untouched_and_timed(ctx, state):
    """no object is allocated by the second call, the picture keeps its state, its pointers and every byte of its raster planes and its twin"""
    (w, h), (dw, dh), bpc, layout = BIG, (21, 11), 10, I420
    rng = np.random.default_rng(31200)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, state)
    try:
        raster = tsc._raster_bytes(ctx, pic)
        twin = util.twin_bytes(ctx, pic) if state == "twin-only" else None
        ptrs, ok = [pic.pic.twin[pl] for pl in range(3)], pic.pic.twin_ok
        crop = (14, 14, 300, 100)
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 1, tables)
        for _ in range(5):          # (every slot of the staging ring is made here)
            check(ctx, pic, colour, want, dw, dh, K4, F16, crop, 1, what=state)
        live = tsc._live(ctx)
        check(ctx, pic, colour, want, dw, dh, K4, F16, crop, 1, what=state)
        ms = ctx.last_kernel_ms()
        assert ms > 0.0 if ctx.backend == "hip" else ms >= 0.0
        assert tsc._live(ctx) == live, "the call allocated an object in the steady state"
        assert pic.pic.twin_ok == ok and [pic.pic.twin[pl] for pl in range(3)] == ptrs
        assert np.array_equal(tsc._raster_bytes(ctx, pic), raster)
        if twin is not None:
            assert np.array_equal(util.twin_bytes(ctx, pic), twin)
    finally:
        pic.free()
        ctx.colour_destroy(colour)


def test_six_exports_back_to_back_on_one_handle(ctx):
    """no sync in between: more calls than the staging ring has slots"""
    (w, h), bpc, layout = BIG, 10, I420
    rng = np.random.default_rng(31300)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pics = [make_source(ctx, rng, w, h, layout, bpc, "twin-only" if k & 1 else "raster") for k in range(3)]
    configs = [(None, (21, 11), P, F32, 0), ((14, 14, 300, 100), (96, 54), K3, F16, 1), ((8, 4, 24, 24), (40, 40), K4, F16, 2), (None, (400, 150), P, F16, 1),
               ((0, 0, 80, 3), (4, 4), K4, F32, 0), (None, (330, 120), K3, F32, 2)]
    dests = [Dest(ctx, dw, dh, layout, bpc, fmt, sample) for _, (dw, dh), fmt, sample, _ in configs]
    try:
        ctx.sync()
        for k, (crop, _, fmt, sample, pos) in enumerate(configs):
            pics[k % 3][0].export_rgb_linear_reduced(dests[k].surface, colour, crop, pos)
        ctx.sync()
        for k, (crop, (dw, dh), fmt, sample, pos) in enumerate(configs):
            dests[k].check(want_of(pics[k % 3][1], layout, bpc, dw, dh, crop, fmt, sample, pos, tables), what="export %d of six" % k)
        ctx.colour_destroy(colour)
        colour = None
    finally:
        for d in dests:
            d.free()
        for p, _ in pics:
            p.free()
        if colour is not None:
            ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 6. the table of a handle

@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_q_of_a_handle(ctx, bpc):
    """q and e of a handle against numpy: random tables, an all-zero lin, and a lin with one negative entry — which has no q, is refused by the new
    calls and still served by dav1d_hip_surface_export_rgb_colour"""
    rng = np.random.default_rng(31400 + bpc)
    lin = tc.random_tables(rng, bpc)[0]
    for table in (lin, np.zeros(1 << bpc, f32), lin * f32(2.0 ** -140), np.full(1 << bpc, 2.0 ** 127, f32)):
        h = ctx.colour(table, bpc=bpc)
        q, e = ctx.colour_light_table(h, bpc)
        wq, we = q_of(table)
        assert e == we and np.array_equal(q, wq)
        ctx.colour_destroy(h)
    neg = lin.copy()
    neg[7] = -neg[7]
    h = ctx.colour(neg, bpc=bpc)
    pic, vis = make_source(ctx, rng, 64, 32, I444, bpc, "raster")
    d, e = Dest(ctx, 8, 4, I444, bpc, P, F32), Dest(ctx, 64, 32, I444, bpc, P, F32)
    try:
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            ctx.colour_light_table(h, bpc)
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            pic.export_rgb_linear_reduced(d.surface, h)
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            ctx.export_rgb_linear_reduced_batch([d.surface], [pic], h)
        d.check(None, what="a refused export")
        pic.export_rgb_colour(e.surface, h)
        e.check(tc.expect(vis, I444, bpc, P, F32, 0, neg), what="a lin with a negative entry through export_rgb_colour")
    finally:
        d.free()
        e.free()
        pic.free()
        ctx.colour_destroy(h)


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refusals(ctx):
    """every refusal in the header's order, each with nothing written: a later fault never hides an earlier one"""
    w, h = 514, 102
    rng = np.random.default_rng(31500)
    pics = {key: make_source(ctx, rng, w, h, key[1], key[0], "raster")[0] for key in ((10, I420), (8, I420), (10, I422), (10, I444))}
    tall = make_source(ctx, rng, 64, 514, I420, 10, "raster")[0]
    colours = {bpc: ctx.colour(*tc.random_tables(rng, bpc), bpc=bpc) for bpc in (8, 10)}
    no_q = {}
    for bpc in (8, 10):
        lin = tc.random_tables(rng, bpc)[0]
        lin[3] = -lin[3]
        no_q[bpc] = ctx.colour(lin, bpc=bpc)

    def refused(code, fmt=K3, sample=F16, size=(50, 12), crop=None, rows=(0, 1 << 30), change=None, key=(10, I420), params=None, shape_as=None, flt=0, pic=None,
                colour="own", **kw):
        pic = pic or pics[key]
        d = Dest(ctx, size[0], size[1], key[1], key[0], shape_as[0] if shape_as else fmt, shape_as[1] if shape_as else sample, **kw)
        d.surface.desc.format, d.surface.desc.sample = fmt, sample
        if change:
            change(d.surface.desc)
        rect = C.byref(api.SurfaceRect(*crop)) if crop is not None else None
        p = C.byref(params) if params is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), rect, p, colours[key[0]] if colour == "own" else colour,
                                                                 flt, rows[0], rows[1])
        assert rc == -code, (rc, code, fmt, sample, crop, size, rows)
        d.check(None, what="a refused export")
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
        for size in ((95, 51), (50, 12), (600, 110)):          # under 8:1, over it, going up
            # 1. what dav1d_hip_surface_export_rgb_reduced refuses, with its codes — also with no handle, a wrong one and one without q, which come later
            for colour in ("own", None, colours[8], no_q[10]):
                for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, 5, -1):
                    refused(EINVAL, fmt, F16, shape_as=(P, F16), size=size, colour=colour)
                for sample in (4, -1):
                    refused(EINVAL, K3, sample, shape_as=(K3, F16), size=size, colour=colour)
            for fmt in (P, K3, K4):
                refused(EINVAL, fmt, M, key=(8, I420), shape_as=(fmt, F16), size=size)             # MSB16 at 8 bpc
                for sample in (N, M):                                                             # normalisation is for float samples
                    refused(EINVAL, fmt, sample, params=RgbParams(1, 1, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)), shape_as=(fmt, F16), size=size)
                for pos in (-1, 3):
                    refused(EINVAL, fmt, F16, params=RgbParams(pos, 0), size=size)
                refused(EINVAL, fmt, F16, change=setter("w", 0), size=size)
                refused(EINVAL, fmt, F16, change=null_plane(0), size=size)
                refused(EINVAL, fmt, F16, change=stride(0, -2), size=size)
                refused(EINVAL, fmt, F32, change=stride(0, +2), pad=4, size=size)
                refused(EINVAL, fmt, F16, matrix=0, size=size)                                     # identity needs 4:4:4
                refused(EINVAL, fmt, F16, rows=(1, 8), size=size)                                  # odd band rows
                refused(EINVAL, fmt, F16, rows=(0, 9), size=size)
                for m in (2, 4, 8, 14, -1):
                    refused(ENOTSUP, fmt, F16, matrix=m, size=size, colour=None)
            refused(EINVAL, P, F16, change=null_plane(2), size=size)
        assert ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced(None, None, None, None, None, None, 0, 0, 2) == -EINVAL
        # ... the crop
        for crop in ((500, 0, 100, 51), (0, 60, 95, 51), (-2, 0, 95, 51), (0, -2, 95, 51), (0, 0, 0, 51), (0, 0, 95, 0), (1, 0, 95, 51), (0, 1, 95, 51)):
            refused(EINVAL, crop=crop)
        refused(EINVAL, crop=(1, 0, 95, 51), key=(10, I422))
        # ... the ratios above 256 downwards, whatever the other axis does, and in front of a missing handle, an integer sample and a handle without q
        for colour, sample in (("own", F16), (None, F16), ("own", N), (no_q[10], F16)):
            refused(ENOTSUP, size=(2, 12), colour=colour, sample=sample)
            refused(ENOTSUP, size=(2, 200), colour=colour, sample=sample)
            refused(ENOTSUP, size=(64, 2), pic=tall, colour=colour, sample=sample)
            refused(ENOTSUP, size=(1, 1), crop=(0, 0, 258, 2), colour=colour, sample=sample)
        # ... the unknown filter, alone, behind an older refusal (whose code wins) and in front of this call's own
        for flt in (1, -1, 7):
            refused(ENOTSUP, flt=flt)
            refused(ENOTSUP, flt=flt, size=(600, 110))
            refused(EINVAL, flt=flt, crop=(1, 0, 95, 51))
            refused(ENOTSUP, flt=flt, colour=None)
            refused(ENOTSUP, flt=flt, sample=N)
            refused(ENOTSUP, flt=flt, colour=colours[8])
            refused(ENOTSUP, flt=flt, colour=no_q[10])
        # 2. -EINVAL for a NULL colour, then an integer sample, then a handle of another depth, then a handle without q
        for size in ((95, 51), (50, 12), (600, 110)):
            for fmt in (P, K3, K4):
                refused(EINVAL, fmt, F16, colour=None, size=size)
                refused(EINVAL, fmt, N, colour=None, size=size)
                for sample in (N, M):
                    refused(EINVAL, fmt, sample, size=size)
                    refused(EINVAL, fmt, sample, size=size, colour=colours[8])
                refused(EINVAL, fmt, N, key=(8, I420), size=size)
                refused(EINVAL, fmt, F32, colour=colours[8], size=size)
                refused(EINVAL, fmt, F32, key=(8, I420), colour=colours[10], size=size)
                refused(EINVAL, fmt, F32, colour=no_q[10], size=size)
                refused(EINVAL, fmt, F16, key=(8, I420), colour=no_q[8], size=size)
                refused(EINVAL, fmt, F16, key=(8, I420), colour=no_q[10], size=size)
        # what is accepted: the same surfaces with nothing wrong, 256:1 exactly, odd origins where the layout does not subsample the axis
        for key, crop, size in (((10, I420), None, (50, 12)), ((10, I420), (2, 0, 512, 102), (2, 12)), ((10, I422), (0, 1, 95, 51), (200, 3)),
                                ((10, I444), (1, 1, 95, 51), (3, 110)), ((8, I420), (0, 0, 184, 96), (23, 200)), ((10, I420), (0, 0, 256, 2), (1, 1))):
            for fmt in (P, K3, K4):
                d = Dest(ctx, size[0], size[1], key[1], key[0], fmt, F16, matrix=0 if key[1] == I444 else 6)
                pics[key].export_rgb_linear_reduced(d.surface, colours[key[0]], crop, 2)
                ctx.sync()
                d.free()
    finally:
        ctx.sync()
        for p in pics.values():
            p.free()
        tall.free()
        for hd in list(colours.values()) + list(no_q.values()):
            ctx.colour_destroy(hd)


def test_a_picture_and_a_handle_of_another_device_are_refused():
    """-EXDEV on the emulator's two devices (tests/conftest.py): for the picture first, then for the handle; behind every -EINVAL of the call, the
    handle without q included"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        rng = np.random.default_rng(31600)
        foreign = other.colour(*tc.random_tables(rng, 10), bpc=10)
        foreign8 = other.colour(*tc.random_tables(rng, 8), bpc=8)
        neg = tc.random_tables(rng, 10)[0]
        neg[0] = -neg[0]
        foreign_neg = other.colour(neg, bpc=10)
        far = other.picture(128, 128, I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        own = ctx.colour(*tc.random_tables(rng, 10), bpc=10)
        near = ctx.picture(128, 128, I420, 10)
        d = Dest(ctx, 9, 9, I420, 10, K3, F16)
        n = Dest(ctx, 9, 9, I420, 10, K3, N)

        def call(dest, pic, colour, flt=0):
            return ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced(ctx.h, C.byref(dest.surface.desc), C.byref(pic.pic), None, None, colour, flt, 0, 96)
        assert call(d, far, own) == -EXDEV                 # the picture
        assert call(d, near, foreign) == -EXDEV            # the handle
        assert call(d, far, foreign) == -EXDEV
        assert call(d, far, own, flt=3) == -ENOTSUP        # the filter comes first
        assert call(d, far, None) == -EINVAL and call(n, far, own) == -EINVAL and call(d, far, foreign8) == -EINVAL and call(d, near, foreign8) == -EINVAL
        assert call(d, far, foreign_neg) == -EINVAL and call(d, near, foreign_neg) == -EINVAL
        bad = C.c_int(-7)
        from dav1d_amd._lib import Picture
        src = (C.POINTER(Picture) * 2)(C.pointer(near.pic), C.pointer(far.pic))
        dst = (type(d.surface.desc) * 2)(d.surface.desc, d.surface.desc)
        assert ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced_batch(ctx.h, 2, dst, src, None, None, own, 0, C.byref(bad)) == -EXDEV and bad.value == 1
        assert ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced_batch(ctx.h, 2, dst, src, None, None, foreign, 0, C.byref(bad)) == -EXDEV and bad.value == 0
        for x in (d, n):
            x.check(None, what="a refused export")
            x.free()
        near.free()
        ctx.colour_destroy(own)
        ctx.lib.dav1d_hip_context_use(other.h)
        far.free()
        for hd in (foreign, foreign8, foreign_neg):
            other.colour_destroy(hd)
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 8. Python

def test_python_methods(ctx):
    (w, h), (dw, dh), bpc, layout = BIG, (14, 9), 10, I420
    rng = np.random.default_rng(31700)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "retiled")
    s = ctx.surface(dw, dh, layout, bpc, K4, F16)
    try:
        s.fill(0xA5)
        crop = (10, 2, 300, 100)
        for name in ("dav1d_hip_surface_export_rgb_linear_reduced", "dav1d_hip_surface_export_rgb_linear_reduced_batch", "dav1d_hip_surface_rgb_linear_rows_needed",
                     "dav1d_hip_colour_light_table"):
            assert api._lib.SYMBOLS.count(name) == 1
        pic.export_rgb_linear_reduced(s, colour, crop=crop, chroma_pos=api.CHROMA_COLOCATED, scale=[2.0, 1.0, 0.5], bias=[-1.0, 0.0, 1.0], filter=api.RESIZE_BILINEAR)
        got = s.download()[0]
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 2, tables, scale=[f32(v) for v in (2.0, 1.0, 0.5)], bias=[f32(v) for v in (-1.0, 0.0, 1.0)])[0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        with pytest.raises(api.HipError, match="errno %d" % ENOTSUP):
            pic.export_rgb_linear_reduced(s, colour, crop, filter=3)
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            pic.export_rgb_linear_reduced(s, None, crop)
    finally:
        s.free()
        pic.free()
        ctx.colour_destroy(colour)


def test_linear_light_is_a_keyword_that_changes_no_check():
    """the two tensor functions check shapes the same way with linear_light=True, before anything reaches the library"""
    from test_surface_batch import FakeTensor
    for kw in ({}, dict(linear_light=True)):
        for match, tensor in (("read as", FakeTensor((3, 54, 3))), ("has shape", FakeTensor((2, 54, 96))), ("device tensor", FakeTensor((3, 54, 96), is_cuda=False)),
                              ("unit stride", FakeTensor((3, 54, 96), [54 * 192, 192, 2]))):
            with pytest.raises(ValueError, match=match):
                api.export_colour_to_tensor(object(), tensor, object(), **kw)
        with pytest.raises(ValueError, match="colour handle"):
            api.export_colour_to_tensor(object(), FakeTensor((3, 54, 96)), None, **kw)
        with pytest.raises(ValueError, match="takes 4 pictures"):
            api.export_colour_batch_to_tensor([object()] * 3, FakeTensor((4, 3, 54, 96)), object(), **kw)
        with pytest.raises(ValueError, match="colour handle"):
            api.export_colour_batch_to_tensor([object()] * 4, FakeTensor((4, 3, 54, 96)), None, **kw)
