"""The tone part of a colour handle (dav1d_hip_colour_create_toned, dav1d_hip_colour_tables_toned; dav1d_amd/csrc/surface_colour.h)
through dav1d_hip_surface_export_rgb_colour: step 1b, a gain that depends on the pixel's luminance and multiplies all three channels in front of the
matrix.  tests/test_surface_tone_sized.py takes the same handles through the sized calls and the batches.

The oracle is composed from what the suite has — test_surface_rgb.rgb_values for the integers, test_surface_colour.stage / finish for steps 2 to 4 (fed
the light through an identity-indexed table, as test_surface_linear.after_light does), test_surface_rgb.arrange — and adds one piece of arithmetic:
`tone`, the numpy restatement of step 1b in float32 with .astype(f32) behind every product and sum.  Every comparison of exported bytes is exact;
every destination is filled with 0xA5 first and compared byte by byte, padding included.  Every case with `ctx` runs on the emulated build and, under
-m gpu, on the device; the tables of dav1d_hip_colour_tables_toned are host arithmetic and are checked without a backend."""
import ctypes as C

import numpy as np
import pytest

import util
import test_surface as ts
import test_surface_colour as tc
import test_surface_linear as ln
import test_surface_rgb as tr
import test_surface_scaled as tsc
from dav1d_amd import _lib, api
from dav1d_amd._lib import ColourDesc, ColourTone

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
F32, F16 = api.SAMPLE_F32, api.SAMPLE_F16
ENC_N = tc.ENC_N
f32 = np.float32
ONES = np.full(ENC_N, 0x3C00, np.uint16)


# ------------------------------------------------------------------------------------------------ step 1b, restated

def tone(l, k, gain, index=None):
    """step 1b on three float32 planes of light: l' — and, in `index` (a list), the entries of gain that were read"""
    k, gain = np.asarray(k, f32), np.asarray(gain, np.uint16)
    assert all(x.dtype == f32 for x in l) and k.shape == (3,) and gain.shape == (ENC_N,)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = [(k[j] * l[j]).astype(f32) for j in range(3)]
        y = ((p[0] + p[1]).astype(f32) + p[2]).astype(f32)
        x = np.where(y > 0, np.where(y < 1, y, f32(1)), f32(0)).astype(f32)
        h = x.astype(np.float16).view(np.uint16)
        assert h.max() <= 0x3C00
        g = gain[h].view(np.float16).astype(f32)
        out = [(c * g).astype(f32) for c in l]
    if index is not None:
        index.append(h)
    return out


def random_tone(rng):
    """k in [-1, 1] (Y negative, inside [0, 1] and above 1 within one picture) and a gain of random finite halves of either sign, NOT monotone: an
    index that is off by one shows"""
    k = rng.uniform(-1, 1, 3).astype(f32)
    k[np.abs(k) < 2.0 ** -10] = f32(0.5)          # (no denormal products)
    gain = rng.integers(0, 0x7C00, ENC_N).astype(np.uint16) | (rng.integers(0, 2, ENC_N).astype(np.uint16) << 15)
    return k, gain


def light(vis, layout, bpc, pos, lin, matrix=1, full_range=0):
    return [np.asarray(lin, f32)[v] for v in tr.rgb_values(vis, layout, bpc, matrix, full_range, pos)]


def expect(vis, layout, bpc, fmt, sample, pos, lin, m=None, enc=None, tone_part=None, matrix=1, full_range=0, scale=None, bias=None, index=None):
    l = light(vis, layout, bpc, pos, lin, matrix, full_range)
    if tone_part is not None:
        l = tone(l, *tone_part, index=index)
    return ln.after_light(l, sample, fmt, m, enc, scale, bias)


def toned(ctx, lin, m=None, enc=None, tone_part=None, bpc=None):
    return ctx.colour(lin, m, enc, bpc=bpc, tone=tone_part)


# ------------------------------------------------------------------------------------------------ 1. random tables against numpy

def test_the_cases_meet_every_combination():
    """the deal of test_surface_colour.test_random_tables, with a tone part on every handle"""
    n = len(tc.CASES) * len(tr.SIZES) * 4
    assert len(tc.COMBOS) == 144 and n >= 2 * len(tc.COMBOS)
    met = {}
    for k in range(n):
        met.setdefault(tc.COMBOS[(k * 37) % len(tc.COMBOS)], set()).add(tc.CASES[k // 16])
    assert set(met) == set(tc.COMBOS) and min(len(v) for v in met.values()) >= 2
    assert {c[0] for c in tc.CASES} == {8, 10, 12} and {c[1] for c in tc.CASES} == {I400, I420, I422, I444} and {c[2] for c in tc.CASES} == {"raster", "twin-only"}
    assert {c[0] for c in tc.COMBOS} == set(tc.STAGES) and {c[1] for c in tc.COMBOS} == {P, K3, K4} and {c[2] for c in tc.COMBOS} == {F32, F16}
    assert {c[3] for c in tc.COMBOS} == {0, 1} and {c[4] for c in tc.COMBOS} == {0, 1, 2}


def test_the_random_tone_part_reaches_below_inside_and_above():
    """numpy only: with k in [-1, 1] and lin in [2^-20, 16) one picture has Y < 0, 0 < Y < 1 and Y > 1, and the gain is not monotone"""
    rng = np.random.default_rng(40000)
    lin = tc.random_tables(rng, 10)[0]
    for _ in range(8):
        k, gain = random_tone(rng)
        if (k > 0).any() and (k < 0).any():
            break
    vis = [rng.integers(0, 1024, (19, 131)) for _ in range(3)]
    index = []
    tone(light(vis, I444, 10, 0, lin), k, gain, index)
    h = index[0]
    assert (h == 0).any() and (h == 0x3C00).any() and ((h > 0) & (h < 0x3C00)).any()
    assert (np.diff(gain.view(np.float16).astype(f32)) < 0).any() and (np.diff(gain.view(np.float16).astype(f32)) > 0).any()


@pytest.mark.parametrize("case", range(len(tc.CASES)), ids=["%dbit-l%d-%s" % c for c in tc.CASES])
def test_random_tables(ctx, case):
    bpc, layout, state = tc.CASES[case]
    rng = np.random.default_rng(40100 + case)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = random_tone(rng)
    handles = {st: toned(ctx, *tc.tables_of(st, lin, m, enc), tone_part=tp, bpc=bpc) for st in tc.STAGES}
    try:
        for si, (w, h) in enumerate(tr.SIZES):
            pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, state, extremes=w > 100)
            try:
                for j in range(4):
                    st, fmt, sample, norm, pos = tc.COMBOS[((case * 16 + si * 4 + j) * 37) % len(tc.COMBOS)]
                    scale = [f32(v) for v in rng.uniform(0.5, 2, 3)] if norm else None
                    bias = [f32(v) for v in rng.uniform(-1, 1, 3)] if norm else None
                    want = expect(vis, layout, bpc, fmt, sample, pos, *tc.tables_of(st, lin, m, enc), tone_part=tp, scale=scale, bias=bias)
                    tc.export_and_check(ctx, pic, handles[st], want, fmt, sample,
                                        "toned %dx%d %d bpc layout %d %s, %s format %d sample %d norm %d chroma_pos %d" % (w, h, bpc, layout, state, st, fmt, sample, norm, pos),
                                        pos=pos, scale=scale, bias=bias)
                assert pic.pic.twin_ok == (api.TWIN_ONLY if state == "twin-only" else 0)
            finally:
                pic.free()
    finally:
        ctx.sync()
        for hd in handles.values():
            ctx.colour_destroy(hd)


# ------------------------------------------------------------------------------------------------ 2. exact anchors

def _export(ctx, pic, colour, fmt, sample, pos=1, **kw):
    d = ts.Dest(ctx, pic.w, pic.h, pic.layout, pic.bpc, fmt, sample, **kw)
    pic.export_rgb_colour(d.surface, colour, pos)
    ctx.sync()
    return d


def _same(a, b):
    assert all(np.array_equal(x, y) for x, y in zip(tc._bytes_of(a), tc._bytes_of(b)))


@pytest.mark.parametrize("bpc,layout,state", [(8, I420, "twin-only"), (10, I422, "raster"), (12, I444, "twin-only")])
def test_a_gain_of_ones_writes_the_bytes_of_the_untoned_handle(ctx, bpc, layout, state):
    """l * 1.0 is l: the three multiplications change no bit, whatever Y is"""
    rng = np.random.default_rng(40200 + bpc)
    lin, m, enc = tc.random_tables(rng, bpc)
    plain, ones = ctx.colour(lin, m, enc, bpc=bpc), toned(ctx, lin, m, enc, (random_tone(rng)[0], ONES), bpc)
    pic, vis = util.make_source(ctx, rng, 131, 19, layout, bpc, state, extremes=True)
    try:
        for fmt, sample in ((P, F32), (K4, F16), (K3, F16)):
            a, b = _export(ctx, pic, plain, fmt, sample), _export(ctx, pic, ones, fmt, sample)
            _same(a, b)
            b.check(tc.expect(vis, layout, bpc, fmt, sample, 1, lin, m, enc), what="gain of ones")
            a.free()
            b.free()
    finally:
        pic.free()
        ctx.colour_destroy(plain)
        ctx.colour_destroy(ones)


def test_zero_k_and_a_gain_of_two_is_a_doubled_lin(ctx):
    """k = (0, 0, 0): Y = +0 for every pixel, gain[0] = 2.0 is read and l * 2 is exact for a lin free of denormals: the bytes of an un-toned handle
    whose lin is doubled.  Every other entry of gain is 3.0: a read elsewhere shows"""
    bpc, layout = 10, I420
    rng = np.random.default_rng(40300)
    lin, m, enc = tc.random_tables(rng, bpc)
    assert (np.abs(lin) >= 2.0 ** -100).all()
    gain = np.full(ENC_N, 0x4200, np.uint16)
    gain[0] = 0x4000
    doubled, two = ctx.colour((lin * f32(2)).astype(f32), m, enc, bpc=bpc), toned(ctx, lin, m, enc, ([0, 0, 0], gain), bpc)
    pic, vis = util.make_source(ctx, rng, 131, 19, layout, bpc, "twin-only", extremes=True)
    try:
        for fmt, sample in ((P, F32), (K4, F16)):
            a, b = _export(ctx, pic, doubled, fmt, sample), _export(ctx, pic, two, fmt, sample)
            _same(a, b)
            b.check(expect(vis, layout, bpc, fmt, sample, 1, lin, m, enc, ([0, 0, 0], gain)), what="k = 0")
            a.free()
            b.free()
    finally:
        pic.free()
        ctx.colour_destroy(doubled)
        ctx.colour_destroy(two)


def _create_raw(ctx, lin, m, enc, bpc, tone_ptr="null"):
    """dav1d_hip_colour_create_toned itself; tone_ptr "null": t == NULL"""
    keep = [np.ascontiguousarray(lin, f32), np.ascontiguousarray(enc, np.uint16)]
    d = ColourDesc(bpc=bpc, lin=keep[0].ctypes.data_as(C.POINTER(C.c_float)), has_matrix=1, enc=keep[1].ctypes.data_as(C.POINTER(C.c_uint16)))
    d.m[:] = [float(v) for v in m]
    h = C.c_void_p()
    assert ctx.lib.dav1d_hip_colour_create_toned(ctx.h, C.byref(d), None if tone_ptr == "null" else tone_ptr, C.byref(h)) == 0
    return h


def test_create_toned_with_a_null_tone_is_colour_create(ctx):
    bpc, layout = 10, I420
    rng = np.random.default_rng(40400)
    lin, m, enc = tc.random_tables(rng, bpc)
    old, new = ctx.colour(lin, m, enc, bpc=bpc), _create_raw(ctx, lin, m, enc, bpc)
    pic, vis = util.make_source(ctx, rng, 131, 19, layout, bpc, "raster")
    try:
        for fmt, sample in ((P, F32), (K4, F16)):
            a, b = _export(ctx, pic, old, fmt, sample), _export(ctx, pic, new, fmt, sample)
            _same(a, b)
            b.check(tc.expect(vis, layout, bpc, fmt, sample, 1, lin, m, enc), what="t == NULL")
            a.free()
            b.free()
        qa, ea = ctx.colour_light_table(old, bpc)
        qb, eb = ctx.colour_light_table(new, bpc)
        assert ea == eb and np.array_equal(qa, qb)
    finally:
        pic.free()
        ctx.colour_destroy(old)
        ctx.colour_destroy(new)


def test_toned_and_untoned_handles_alternate_back_to_back(ctx):
    """six exports on one context with no sync in between, a toned, an un-toned and a second toned handle in turn: each writes its own bytes (a
    table that stayed behind from the launch before would show)"""
    w, h, bpc, layout = 131, 19, 10, I420
    rng = np.random.default_rng(40500)
    lin, m, enc = tc.random_tables(rng, bpc)
    tps = [random_tone(rng), None, random_tone(rng)]
    handles = [toned(ctx, lin, m, enc, tp, bpc) for tp in tps]
    pics = [util.make_source(ctx, rng, w, h, layout, bpc, "twin-only" if k & 1 else "raster") for k in range(3)]
    configs = [(P, F32, 0), (K3, F16, 1), (K4, F16, 2), (P, F16, 1), (K4, F32, 0), (K3, F32, 2)]
    dests = [ts.Dest(ctx, w, h, layout, bpc, fmt, sample) for fmt, sample, _ in configs]
    try:
        ctx.sync()
        for k, (fmt, sample, pos) in enumerate(configs):          # no sync in between
            pics[k % 3][0].export_rgb_colour(dests[k].surface, handles[k % 2 if k < 4 else 2 - k % 2], pos)
        ctx.sync()
        for k, (fmt, sample, pos) in enumerate(configs):
            dests[k].check(expect(pics[k % 3][1], layout, bpc, fmt, sample, pos, lin, m, enc, tps[k % 2 if k < 4 else 2 - k % 2]), what="export %d of six" % k)
    finally:
        for d in dests:
            d.free()
        for p, _ in pics:
            p.free()
        for hd in handles:
            ctx.colour_destroy(hd)


# ------------------------------------------------------------------------------------------------ 3. edges of the index

def test_edges_of_the_luminance_index(ctx):
    """4:4:4 with matrix 0, so that the codes are the samples: every pixel is (code, 0, 0) with k = (1, 0, 0) and lin[0] = 0, so Y = lin[code] exactly;
    gain[h] is the half whose value is h / 4 + 1 for the entries the cases name — distinct, exact in binary16 — and 7 elsewhere; lin'[code] = Y * g
    reaches the output unchanged (no matrix, no enc, F32), so which entry was read is visible per case"""
    w, h, bpc = 131, 19, 8
    special = {
        "one": (1.0, 0x3C00), "just below one": (float(np.nextafter(f32(1), f32(0))), 0x3C00), "just above one": (float(np.nextafter(f32(1), f32(2))), 0x3C00),
        "the last half below one": (1 - 2.0 ** -11, 0x3BFF), "sixteen": (16.0, 0x3C00), "the smallest subnormal": (2.0 ** -24, 1), "the tie with zero": (2.0 ** -25, 0),
        "just above that tie": (2.0 ** -25 * (1 + 2.0 ** -20), 1), "a tie between halves, down": (0.5 + 2.0 ** -12, 0x3800), "a tie between halves, up": (0.5 + 3 * 2.0 ** -12, 0x3802),
        "a tie between subnormals, down": (2.5 * 2.0 ** -24, 2), "a tie between subnormals, up": (3.5 * 2.0 ** -24, 4), "the largest subnormal": (1023 * 2.0 ** -24, 0x3FF),
        "negative": (-0.75, 0),
    }
    lin = np.zeros(1 << bpc, f32)          # code 0: +0
    for i, (v, _) in enumerate(special.values()):
        lin[i + 1] = v
        assert float(lin[i + 1]) == v, "the special values are float32 values"
    entries = sorted({e for _, e in special.values()})
    gain = np.full(ENC_N, 0x4700, np.uint16)          # 7.0 wherever no case reads
    for j, e in enumerate(entries):
        gain[e] = np.float16(1 + j / 4).view(np.uint16)
    value_of = {e: f32(1 + j / 4) for j, e in enumerate(entries)}
    tp = (np.array([1, 0, 0], f32), gain)
    rng = np.random.default_rng(40600)

    def fill(pl, s):          # planes Y, U, V are G, B, R
        return rng.integers(0, len(special) + 1, size=s) if pl == 2 else np.zeros(s, np.int64)
    pic, vis = tr.make_picture(ctx, w, h, I444, bpc, "twin-only", fill)
    colour = toned(ctx, lin, tone_part=tp, bpc=bpc)
    try:
        codes = tr.rgb_values(vis, I444, bpc, 0, 0, 0)
        assert set(codes[0].ravel()) == set(range(len(special) + 1)) and not codes[1].any() and not codes[2].any(), "every special entry is met"
        index = []
        want = expect(vis, I444, bpc, P, F32, 0, lin, tone_part=tp, matrix=0, index=index)
        for i, (name, (v, e)) in enumerate(special.items()):
            at = codes[0] == i + 1
            assert (index[0][at] == e).all(), name
            assert (want[0][at] == f32(v) * value_of[e]).all(), name
        assert (index[0][codes[0] == 0] == 0).all() and (want[0][codes[0] == 0] == 0).all()
        for sample in (F32, F16):
            d = _export(ctx, pic, colour, P, sample, pos=0, matrix=0)
            d.check(expect(vis, I444, bpc, P, sample, 0, lin, tone_part=tp, matrix=0), what="special entries, sample %d" % sample)
            d.free()
    finally:
        pic.free()
        ctx.colour_destroy(colour)


def test_minus_zero_and_nan_read_entry_zero(ctx):
    """Y = -0.0 (k = (-0.0, -0.0, -0.0) on positive light) and Y = NaN (k = (3e38, -3e38, 0) on light of 2 .. 16: p_0 + p_1 is inf - inf) read gain[0]; Y =
    +inf (k = (3e38, 3e38, 0)) reads gain[0x3C00].  gain[0] = 2, gain[0x3C00] = 0.5, 3 elsewhere"""
    w, h, bpc = 131, 19, 10
    rng = np.random.default_rng(40700)
    lin = rng.uniform(2, 16, 1 << bpc).astype(f32)
    gain = np.full(ENC_N, 0x4200, np.uint16)
    gain[0], gain[0x3C00] = 0x4000, 0x3800
    pic, vis = tc._gbr_picture(ctx, w, h, bpc, lambda pl, s: rng.integers(0, 1 << bpc, size=s))
    big = 3e38
    try:
        l = light(vis, I444, bpc, 0, lin, matrix=0)
        for name, k, entry, factor in (("-0.0", [-0.0, -0.0, -0.0], 0, 2), ("NaN", [big, -big, 0.0], 0, 2), ("+inf", [big, big, 0.0], 0x3C00, 0.5), ("-inf", [-big, -big, 0.0], 0, 2)):
            k = np.array(k, f32)
            with np.errstate(over="ignore", invalid="ignore"):
                y = (((k[0] * l[0]).astype(f32) + (k[1] * l[1]).astype(f32)).astype(f32) + (k[2] * l[2]).astype(f32)).astype(f32)
            assert {"-0.0": (y == 0).all() and np.signbit(y).all(), "NaN": np.isnan(y).all(), "+inf": np.isposinf(y).all(), "-inf": np.isneginf(y).all()}[name], name
            index = []
            want = expect(vis, I444, bpc, P, F32, 0, lin, tone_part=(k, gain), matrix=0, index=index)
            assert (index[0] == entry).all(), name
            assert all((want[c] == l[c] * f32(factor)).all() for c in range(3)), name
            colour = toned(ctx, lin, tone_part=(k, gain), bpc=bpc)
            try:
                d = _export(ctx, pic, colour, P, F32, pos=0, matrix=0)
                d.check(want, what="Y = %s" % name)
                d.free()
            finally:
                ctx.colour_destroy(colour)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 4. workgroups that loop, 5. bands, sentinels, the source

def test_workgroups_that_loop(ctx):
    w, h, layout, bpc = 1030, 130, I420, 10
    rng = np.random.default_rng(40800)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = random_tone(rng)
    colour = toned(ctx, lin, m, enc, tp, bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        assert (((w + 1) >> 1) + 63) // 64 == 9 and (((h + 1) >> 1) + 7) // 8 == 9
        want = expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, tp)
        for cells in (2, 3, 64):
            ctx.set_option("colour_cells", cells)
            tc.export_and_check(ctx, pic, colour, want, K4, F16, "toned %dx%d, colour_cells %d" % (w, h, cells), pos=1)
    finally:
        ctx.set_option("colour_cells", 0)
        ctx.sync()
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("pos", [1, 2])
def test_bands_sentinels_and_the_source(ctx, pos):
    """three bands write the bytes of the whole-surface call, a band alone leaves every other byte of the destination at the sentinel (Dest.check
    compares the padding as well), and the source keeps its state and every byte"""
    w, h, bpc, layout = 131, 19, 10, I420
    rng = np.random.default_rng(40900 + pos)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = random_tone(rng)
    colour = toned(ctx, lin, m, enc, tp, bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        twin = util.twin_bytes(ctx, pic)
        raster = tsc._raster_bytes(ctx, pic)
        for fmt, sample in ((P, F32), (K4, F16)):
            want = expect(vis, layout, bpc, fmt, sample, pos, lin, m, enc, tp)
            d = ts.Dest(ctx, w, h, layout, bpc, fmt, sample)
            for r0, r1 in ((0, 2), (2, 10), (10, h)):
                pic.export_rgb_colour(d.surface, colour, pos, row0=r0, row1=r1)
            d.check(want, what="three bands, chroma_pos %d format %d" % (pos, fmt))
            d.free()
            d = ts.Dest(ctx, w, h, layout, bpc, fmt, sample, pad=8)
            pic.export_rgb_colour(d.surface, colour, pos, row0=2, row1=10)
            d.check(want, rows=[(2, 10)] * len(want), what="band [2, 10) alone")
            d.free()
        assert pic.pic.twin_ok == api.TWIN_ONLY
        assert np.array_equal(util.twin_bytes(ctx, pic), twin) and np.array_equal(tsc._raster_bytes(ctx, pic), raster)
    finally:
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 7. create refusals

def test_create_refusals(ctx):
    """everything dav1d_hip_colour_create refuses, in its order, in front of the tone part's own; nothing is allocated by a refused call"""
    rng = np.random.default_rng(41000)
    lin, m, enc = tc.random_tables(rng, 10)
    k0, gain0 = random_tone(rng)

    def create(bpc=10, lin=lin, m=m, enc=enc, has_matrix=1, out=True, desc=True, k=k0, gain=gain0, tone_part=True):
        d = ColourDesc(bpc=bpc, has_matrix=has_matrix)
        keep = [np.ascontiguousarray(lin, f32) if lin is not None else None, np.ascontiguousarray(enc, np.uint16) if enc is not None else None,
                np.ascontiguousarray(gain, np.uint16) if gain is not None else None]
        if keep[0] is not None:
            d.lin = keep[0].ctypes.data_as(C.POINTER(C.c_float))
        if keep[1] is not None:
            d.enc = keep[1].ctypes.data_as(C.POINTER(C.c_uint16))
        d.m[:] = [float(v) for v in m]
        t = ColourTone(k=(C.c_float * 3)(*[float(v) for v in k]))
        if keep[2] is not None:
            t.gain = keep[2].ctypes.data_as(C.POINTER(C.c_uint16))
        h = C.c_void_p()
        before = tsc._live(ctx)
        rc = ctx.lib.dav1d_hip_colour_create_toned(ctx.h, C.byref(d) if desc else None, C.byref(t) if tone_part else None, C.byref(h) if out else None)
        if rc == 0:
            ctx.colour_destroy(h)
        else:
            assert not h.value
        assert tsc._live(ctx) == before, "a refused (or destroyed) handle left an object behind"
        return rc

    def poked(a, i, v):
        b = np.array(a)
        b.reshape(-1)[i] = v
        return b
    bad_k, bad_gain = poked(k0, 1, np.nan), poked(gain0, 5, 0x7C00)
    assert create() == 0 and create(enc=None) == 0 and create(has_matrix=0) == 0 and create(tone_part=False) == 0
    # the old refusals, with and without a tone part, and in front of a bad one
    for kw in ({}, dict(tone_part=False), dict(gain=None), dict(k=bad_k), dict(gain=bad_gain)):
        assert create(lin=None, **kw) == -EINVAL
        assert create(desc=False, **kw) == -EINVAL and create(out=False, **kw) == -EINVAL
        for bpc in (0, 9, 11, 16, -8):
            assert create(bpc=bpc, **kw) == -EINVAL
        for bad in (np.inf, -np.inf, np.nan):
            assert create(lin=poked(lin, 1023, bad), **kw) == -EINVAL and create(lin=poked(lin, 0, bad), **kw) == -EINVAL
            assert create(m=poked(m, 8, bad), **kw) == -EINVAL
        for bad in (0x7C00, 0xFC00, 0x7E00, 0xFFFF):
            assert create(enc=poked(enc, ENC_N - 1, bad), **kw) == -EINVAL and create(enc=poked(enc, 0, bad), **kw) == -EINVAL
    # the tone part's own
    assert create(gain=None) == -EINVAL
    for bad in (np.inf, -np.inf, np.nan):
        for i in range(3):
            assert create(k=poked(k0, i, bad)) == -EINVAL
    for bad in (0x7C00, 0xFC00, 0x7E00, 0xFFFF):
        assert create(gain=poked(gain0, ENC_N - 1, bad)) == -EINVAL and create(gain=poked(gain0, 0, bad)) == -EINVAL
    assert create(gain=poked(gain0, 7, 0x7BFF)) == 0 and create(gain=poked(gain0, 7, 0xFBFF)) == 0          # the largest finite halves, either sign
    assert create(k=[-3e38, 0.0, -0.0]) == 0
    assert ctx.lib.dav1d_hip_colour_create_toned(None, None, None, None) == -EINVAL


def test_a_toned_handle_of_another_device_is_refused():
    """-EXDEV on the emulator's two devices (tests/conftest.py), as for an un-toned handle"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        rng = np.random.default_rng(41100)
        foreign = toned(other, *tc.random_tables(rng, 10), tone_part=random_tone(rng), bpc=10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        pic = ctx.picture(64, 64, I420, 10)
        d = ts.Dest(ctx, 64, 64, I420, 10, K3, F16)
        assert ctx.lib.dav1d_hip_surface_export_rgb_colour(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, foreign, 0, 64) == -EXDEV
        assert ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, None, foreign, 0, 0, 64) == -EXDEV
        assert ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), None, None, foreign, 0, 0, 64) == -EXDEV
        d.check(None, what="a refused export")
        d.free()
        pic.free()
        other.colour_destroy(foreign)
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 8. dav1d_hip_colour_tables_toned (host arithmetic)

@pytest.fixture(scope="module")
def hostlib():
    return _lib.load(util.emu_lib_path())


ROWS = ((8, 9, 1, 203.0, 1000.0), (13, 9, 1, 203.0, 1000.0), (1, 1, 12, 100.0, 100.0), (4, 12, 9, 80.0, 4000.0), (14, 9, 9, 203.0, 203.0))          # test_tables_against_numpy's
HLG_ROWS = tuple((trc_out, 9, 1, 203.0, peak) for peak in (400.0, 1000.0, 2000.0) for trc_out in (8, 13))


def np_tone_tables(trc_in, pri_in, trc_out, white, peak):
    """k, gain, has_gain and the pure enc, in double"""
    p = peak / white
    K = np.array([float(v) for v in tc.exact_rgb_to_xyz(pri_in)[1]], np.float64)
    k = (K / p if trc_out == 8 else K).astype(f32)
    gamma = 1.2 + 0.42 * np.log10(peak / 1000.0) if trc_in == 18 else 1.0
    x = np.arange(ENC_N, dtype=np.uint16).view(np.float16).astype(np.float64)
    if trc_out == 8:
        if trc_in != 18:
            return k, ONES, False, None
        with np.errstate(divide="ignore"):
            return k, np.minimum(x ** (gamma - 1), 65504.0).astype(np.float16).view(np.uint16), True, None
    y = x ** gamma * p
    with np.errstate(invalid="ignore", divide="ignore"):
        g = y * (1 + y / (p * p)) / (1 + y) / x
    g[0] = p if gamma == 1.0 else 0.0 if gamma > 1.0 else 65504.0
    return k, np.minimum(g, 65504.0).astype(np.float16).view(np.uint16), True, tc.np_oetf(trc_out, x).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_toned_tables_against_numpy(hostlib, bpc):
    """lin, m and k within one unit in the last place of float32, enc and gain within one binary16 pattern: both sides are double computations rounded once"""
    for trc_in in tc.SDR_IN + (16, 18):
        for trc_out, pri_in, pri_out, white, peak in ROWS + (HLG_ROWS if trc_in == 18 else ()):
            lin, m, enc, has_matrix, has_enc, k, gain, has_gain = api.colour_tables_toned(hostlib, bpc, trc_in, pri_in, trc_out, pri_out, white, peak)
            wl, wm, _ = tc.np_tables(bpc, trc_in, pri_in, trc_out, pri_out, white, peak)
            wk, wg, w_has, we = np_tone_tables(trc_in, pri_in, trc_out, white, peak)
            what = (bpc, trc_in, pri_in, trc_out, pri_out, white, peak)
            assert tc.ulps_f32(lin, wl) <= 1 and tc.ulps_f32(k, wk) <= 1, what
            assert has_matrix == (wm is not None) and has_enc == (we is not None) and has_gain == w_has, what
            assert has_gain == ((trc_in == 18) if trc_out == 8 else True), what
            if wm is not None:
                assert tc.ulps_f32(m, wm) <= 1, what
            else:
                assert np.array_equal(m, np.eye(3, dtype=f32))
            assert np.abs(gain.astype(np.int64) - wg.astype(np.int64)).max() <= 1, what          # (positive halves: the patterns count units in the last place)
            assert ((gain & 0x7C00) != 0x7C00).all(), what
            if we is not None:
                assert np.abs(enc.astype(np.int64) - we.astype(np.int64)).max() <= 1, what
                assert gain[0x3C00] == 0x3C00, what
                assert enc[0] == 0 and enc[0x3C00] == 0x3C00 and (np.diff(enc.astype(np.int64)) >= 0).all(), what
            else:
                assert not has_gain or gain[0x3C00] == 0x3C00, what
            # the tables the old helper fills are the old helper's
            ol, om, oe, o_hm, o_he = api.colour_tables(hostlib, bpc, trc_in, pri_in, trc_out, pri_out, white, peak)
            assert np.array_equal(ol.view(np.uint32), lin.view(np.uint32)) and np.array_equal(om, m) and (o_hm, o_he) == (has_matrix, has_enc), what
            if has_enc and white == peak:
                assert np.abs(enc.astype(np.int64) - oe.astype(np.int64)).max() <= 1, what


def test_k_is_the_luminance_row(hostlib):
    k = api.colour_tables_toned(hostlib, 10, 16, 9, 13, 1, 203.0, 1000.0)[5]
    assert np.abs(k.astype(np.float64) - [0.2627, 0.6780, 0.0593]).max() <= 5e-5 and abs(float(k.astype(np.float64).sum()) - 1) <= 1e-6
    k8 = api.colour_tables_toned(hostlib, 10, 16, 9, 8, 1, 203.0, 1000.0)[5]
    assert np.abs(k8.astype(np.float64) * (1000.0 / 203.0) - k.astype(np.float64)).max() <= 1e-7
    k709 = api.colour_tables_toned(hostlib, 10, 13, 1, 13, 1, 100.0, 100.0)[5]
    assert np.abs(k709.astype(np.float64) - [0.2126, 0.7152, 0.0722]).max() <= 5e-5


def test_gains_reach_p_and_stay_finite(hostlib):
    for white, peak in ((203.0, 1000.0), (100.0, 10000.0), (80.0, 4000.0), (203.0, 203.0)):
        gain = api.colour_tables_toned(hostlib, 10, 16, 9, 13, 1, white, peak)[6]
        g = gain.view(np.float16).astype(np.float64)
        assert np.isfinite(g).all() and g[0] == np.float16(peak / white) and g.max() == g[0] and g[0x3C00] == 1.0
        assert (np.diff(g) <= 0).all(), "the gain of the roll-off falls with the luminance"


def test_the_old_tables_are_what_they_were(hostlib):
    """dav1d_hip_colour_tables against np_tables, and a few entries as recorded"""
    lin, m, enc, _, _ = api.colour_tables(hostlib, 10, 16, 9, 13, 1, 203.0, 1000.0)
    wl, wm, we = tc.np_tables(10, 16, 9, 13, 1, 203.0, 1000.0)
    assert tc.ulps_f32(lin, wl) <= 1 and tc.ulps_f32(m, wm) <= 1 and np.abs(enc.astype(np.int64) - we.astype(np.int64)).max() <= 1
    assert enc[0] == 0 and enc[0x3C00] == 0x3C00 and lin[0] == 0 and lin[1023] == f32(10000.0 / 1000.0)


def test_toned_tables_refusals(hostlib):
    lin, m, enc, k, gain = np.zeros(4096, f32), np.zeros(9, f32), np.zeros(ENC_N, np.uint16), np.zeros(3, f32), np.zeros(ENC_N, np.uint16)
    hm, he, hg = C.c_int(), C.c_int(), C.c_int()

    def call(bpc=10, trc_in=16, pri_in=9, trc_out=13, pri_out=1, white=203.0, peak=1000.0, lin=lin, k=k, gain=gain, hg=hg):
        return hostlib.dav1d_hip_colour_tables_toned(bpc, trc_in, pri_in, trc_out, pri_out, white, peak, lin.ctypes.data if lin is not None else None, m.ctypes.data,
                                                     C.byref(hm), enc.ctypes.data, C.byref(he), k.ctypes.data if k is not None else None,
                                                     gain.ctypes.data if gain is not None else None, C.byref(hg) if hg is not None else None)
    assert call() == 0
    for trc in (0, 2, 3, 5, 7, 9, 10, 11, 12, 17, 19, -1):
        assert call(trc_in=trc) == -ENOTSUP
    for trc in (0, 2, 16, 18, 17, -1):
        assert call(trc_out=trc) == -ENOTSUP
    for pri in (0, 2, 4, 5, 6, 7, 8, 10, 11, 22, -1):
        assert call(pri_in=pri) == -ENOTSUP and call(pri_out=pri) == -ENOTSUP
    assert call(white=0.0) == -EINVAL and call(white=-1.0) == -EINVAL and call(white=float("nan")) == -EINVAL
    assert call(peak=202.0) == -EINVAL and call(peak=float("nan")) == -EINVAL and call(peak=float("inf")) == -EINVAL
    assert call(peak=203.0) == 0
    for bpc in (0, 9, 16):
        assert call(bpc=bpc) == -EINVAL
    assert call(lin=None) == -EINVAL
    assert call(k=None) == -EINVAL and call(gain=None) == -EINVAL and call(hg=None) == -EINVAL


# ------------------------------------------------------------------------------------------------ 9. hue

SATURATED = [(1023, 64, 64), (700, 520, 480), (64, 900, 64), (100, 100, 1000), (900, 900, 100), (800, 200, 900), (1023, 1023, 1023), (700, 650, 600)]


def _saturated_picture(ctx, bpc, w=64, h=8):
    """4:4:4 with matrix 0: column x holds the code triple SATURATED[x % 8] as (R, G, B)"""
    def fill(pl, s):          # planes Y, U, V are G, B, R
        ch = {0: 1, 1: 2, 2: 0}[pl]
        return np.tile(np.array([t[ch] for t in SATURATED]), (s[0], (s[1] + 7) // 8))[:, :s[1]]
    return tr.make_picture(ctx, w, h, I444, bpc, "twin-only", fill)


def test_the_hue_of_saturated_highlights_is_kept(ctx):
    """The point of the feature.  PQ / BT.2020 to LINEAR BT.709 with the helper's tables: no enc, so nothing clips, and the tone part is the gain alone.
    (The helper gives has_gain = 0 for PQ to linear — there is no OOTF and linear output is not tone-mapped — so the gain here is the roll-off's own,
    the gain of the helper's sRGB tables over p; k is scaled to the linear unit.)  R' : G' : B' equals (m l)_R : (m l)_G : (m l)_B within 4 float32 ulps per
    channel — one rounding of the gain product and the five of a matrix row.  The same picture through the OLD helper's sRGB tables, whose tone
    curve runs per channel, does not keep it: the ratio G / R of the linearised output is off by more than 10 % for the saturated red"""
    bpc, white, peak = 10, 203.0, 1000.0
    p = peak / white
    lin, m, _, has_matrix, has_enc, k8, ones, has_gain = api.colour_tables_toned(ctx.lib, bpc, 16, 9, 8, 1, white, peak)
    assert has_matrix and not has_enc and not has_gain and np.array_equal(ones, ONES)
    _, _, _, _, _, k, gain, has_gain = api.colour_tables_toned(ctx.lib, bpc, 16, 9, 13, 1, white, peak)
    assert has_gain
    pic, vis = _saturated_picture(ctx, bpc)
    a = ctx.surface(pic.w, pic.h, I444, bpc, P, F32, matrix=0)
    # the helper's own tone part for linear output, forced into a handle: a gain of 1.0 — the gain product is exact and the ratios are (m l)'s own
    own = toned(ctx, lin, m, None, (k8, ones), bpc)
    pic.export_rgb_colour(a, own, 0)
    l = light(vis, I444, bpc, 0, lin, matrix=0)
    exact = tc.stage([np.arange(l[0].size).reshape(l[0].shape) + c * l[0].size for c in range(3)], np.concatenate([x.ravel() for x in l]), m.reshape(9))
    assert all(tc.ulps_f32(x, y) <= 4 for x, y in zip(a.download(), exact))
    ctx.colour_destroy(own)
    # lin is in white units and k8 = K / p, so the index is luminance in peak units: the roll-off alone is tone(x p) / (x p), the sRGB route's gain over p
    gain = (gain.view(np.float16).astype(np.float64) / p).astype(np.float16).view(np.uint16)
    colour = toned(ctx, lin, m, None, (k8, gain), bpc)
    try:
        pic.export_rgb_colour(a, colour, 0)
        got = [x.astype(np.float64) for x in a.download()]
        l = light(vis, I444, bpc, 0, lin, matrix=0)
        ml = [x.astype(np.float64) for x in tc.stage([np.arange(l[0].size).reshape(l[0].shape) + c * l[0].size for c in range(3)],
                                                     np.concatenate([x.ravel() for x in l]), m.reshape(9))]
        index = []
        tone(l, k8, gain, index)
        g = gain[index[0]].view(np.float16).astype(np.float64)
        assert g.min() < 0.5 and g.max() < 1, "the highlights are rolled off"
        for c in range(3):
            # o'_c / g == (m l)_c within 4 ulps of the larger of the row's products (a row that cancels has the ulps of its terms)
            rows = np.abs(np.stack([m.reshape(3, 3)[c, j] * l[j].astype(np.float64) for j in range(3)])).max(axis=0)
            ulp = np.spacing(np.maximum(rows, np.abs(ml[c])).astype(f32)).astype(np.float64)
            assert (np.abs(got[c] / g - ml[c]) <= 4 * ulp).all(), c
        # the red of the issue: in (4.0, 0.4, 0.2)-like proportion, out in the same proportion
        x = 0          # SATURATED[0]
        want_ratio = ml[1][0, x] / ml[0][0, x]
        assert abs(got[1][0, x] / got[0][0, x] - want_ratio) <= 1e-5 * abs(want_ratio)
        # ... and per channel, through the old helper's tables, linearised again: not kept
        olin, om, oenc, _, _ = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, white, peak)
        old = ctx.colour(olin, om, oenc, bpc=bpc)
        b = ctx.surface(pic.w, pic.h, I444, bpc, P, F32, matrix=0)
        pic.export_rgb_colour(b, old, 0)
        srgb = [x.astype(np.float64) for x in b.download()]
        back = [tc.np_inverse_oetf(13, s) for s in srgb]
        col = 1          # SATURATED[1] = (700, 520, 480), a red of about (4, 0.25, 0.25) white units in BT.709: no channel of m l is negative, none clips at zero
        old_ml = [x[0, col] for x in ml]
        assert min(old_ml) > 0
        kept = ml[1][0, col] / ml[0][0, col]
        was = back[1][0, col] / back[0][0, col]
        assert abs(was / kept - 1) > 0.10, (was, kept)
        now = got[1][0, col] / got[0][0, col]
        assert abs(now / kept - 1) <= 1e-5
        b.free()
        ctx.colour_destroy(old)
    finally:
        a.free()
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 10. Python

def test_python_colour_with_a_tone_part(ctx):
    w, h, bpc, layout = 131, 19, 10, I420
    rng = np.random.default_rng(41200)
    lin, m, enc = tc.random_tables(rng, bpc)
    k, gain = random_tone(rng)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        for name in ("dav1d_hip_colour_create_toned", "dav1d_hip_colour_tables_toned"):
            assert api._lib.SYMBOLS.count(name) == 1
        want = expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, (k, gain))
        for g in (gain, gain.view(np.float16)):          # uint16 patterns, or halves
            hd = ctx.colour(lin, m, enc, tone=(list(k), g))
            tc.export_and_check(ctx, pic, hd, want, K4, F16, "Context.colour(tone=)", pos=1)
            ctx.colour_destroy(hd)
        with pytest.raises(ValueError):
            ctx.colour(lin, tone=(k, gain[:100]))
        with pytest.raises(ValueError):
            ctx.colour(lin, tone=(k[:2], gain))
        with pytest.raises(ValueError):
            ctx.colour(np.zeros(1000, f32), tone=(k, gain))
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            ctx.colour(lin, tone=([np.nan, 0, 0], gain))
    finally:
        pic.free()


def test_python_colour_for_luminance(ctx):
    """colour_for(luminance=True) is colour_tables_toned + colour(tone=); PQ / BT.2020 to sRGB / BT.709 and HLG to linear (the OOTF)"""
    w, h, bpc, layout = 131, 19, 10, I420
    rng = np.random.default_rng(41300)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    try:
        for trc_in, trc_out in ((16, 13), (18, 8), (18, 13), (13, 8)):
            lin, m, enc, has_matrix, has_enc, k, gain, has_gain = api.colour_tables_toned(ctx.lib, bpc, trc_in, 9, trc_out, 1, 203.0, 1000.0)
            assert has_matrix and has_enc == (trc_out != 8) and has_gain == (trc_out != 8 or trc_in == 18)
            hd = ctx.colour_for(bpc, trc_in, 9, trc_out, 1, 203.0, 1000.0, luminance=True)
            want = expect(vis, layout, bpc, K4, F16, 1, lin, m.reshape(9), enc if has_enc else None, (k, gain) if has_gain else None, matrix=9)
            tc.export_and_check(ctx, pic, hd, want, K4, F16, "colour_for(luminance=True) %d -> %d" % (trc_in, trc_out), pos=1, matrix=9)
            ctx.colour_destroy(hd)
        with pytest.raises(api.HipError):
            ctx.colour_for(10, 17, 9, luminance=True)
        # the default is the old route
        lin, m, enc, _, _ = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
        hd = ctx.colour_for(bpc, 16, 9, 13, 1, 203.0, 1000.0)
        tc.export_and_check(ctx, pic, hd, tc.expect(vis, layout, bpc, K4, F16, 1, lin, m.reshape(9), enc, matrix=9), K4, F16, "colour_for", pos=1, matrix=9)
        ctx.colour_destroy(hd)
    finally:
        pic.free()
