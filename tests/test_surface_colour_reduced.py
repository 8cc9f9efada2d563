"""Colour-managed tensor export at any size: dav1d_hip_surface_export_rgb_colour_reduced (dav1d_amd/csrc/surface_colour_reduce.hip).

The call must write byte for byte what dav1d_hip_surface_export_rgb_colour writes from the picture Q whose planes are R' of the crop windows.  Nothing
numerical is new, so nothing is restated here: the expectation is test_surface_colour.expect (the colour stage in numpy) applied to
test_surface_reduced.reduced_planes (R' with Python integers).  Every comparison is exact; every destination is filled with 0xA5 first and compared byte
by byte, padding included (test_surface.Dest).  Every case with `ctx` runs on the emulated build and, under -m gpu, on the device."""
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
from dav1d_amd._lib import Picture, RgbParams
from test_surface import Dest
from test_surface_rgb_scaled import even_crop, same_bytes
from test_surface_scaled import source_from, ss_of
from util import make_source

EINVAL, ENOTSUP, EXDEV = 22, 95, 18
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16
f32 = np.float32
BIG = (330, 120)
MAX_SAMPLES = 2047 * 48          # no picture of this file is larger

# ((picture), crop or None, (output)): every geometry class
GEOMS = [((73, 73), None, (9, 9)),                      # luma over 8:1; at 4:2:0 chroma is 37 -> 5, under it
         ((2047, 40), None, (8, 3)),                    # 257 taps across, two reducer cells across
         ((2048, 16), None, (8, 2)),                    # exactly 256:1 across
         (BIG, (14, 14, 300, 100), (7, 9)),             # 300 -> 7; the 4:2:0 chroma window starts at 7 mod 8 on both axes
         (BIG, (7, 7, 300, 100), (7, 9)),               # ... from 7 mod 8 where the layout does not subsample the axis
         ((190, 102), None, (96, 54)),                  # under 8:1 on every axis
         (BIG, (10, 6, 133, 71), (133, 71)),            # d == s from a crop
         (BIG, (8, 4, 24, 24), (40, 40)),               # 24 -> 40 on both axes: up
         (BIG, (0, 0, 3, 80), (4, 4)),                  # up across with 20:1 down
         (BIG, (0, 0, 80, 3), (4, 4)),                  # ... the reverse; h 3 -> 4 at 4:2:0 is luma up with chroma 2 -> 2
         (BIG, (4, 2, 1, 1), (1, 1)),                   # one-sample axes
         (BIG, (0, 0, 2, 2), (5, 3)),                   # two-sample axes going up
         (BIG, (0, 0, 200, 2), (1, 2))]                 # 200 -> 1 next to 2 -> 2

STAGES = ["lin", "lin+matrix", "all"]
COMBOS = [(st, fmt, sample, norm, pos) for pos in (0, 1, 2) for norm in (0, 1) for sample in (F32, F16) for fmt in (P, K3, K4) for st in STAGES]
CASES = [(bpc, layout, state) for bpc in (8, 10, 12) for layout in (I400, I420, I422, I444) for state in util.STATES]


def combo_of(case, gi):
    return COMBOS[((case * len(GEOMS) + gi) * 37) % len(COMBOS)]          # 37 and 108 share no factor


def want_of(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tables, planes=None, **kw):
    planes = planes if planes is not None else rd.reduced_planes(vis, layout, dw, dh, crop)
    return tc.expect(planes, layout, bpc, fmt, sample, pos, *tables, **kw)


def check(ctx, pic, colour, want, dw, dh, fmt, sample, crop=None, pos=0, scale=None, bias=None, rows=(0, 1 << 30), what="", **kw):
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export_rgb_colour_reduced(d.surface, colour, crop, pos, scale, bias, rows[0], rows[1])
        d.check(want, what="%s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d chroma_pos %d" % (what, pic.w, pic.h, dw, dh, crop, pic.bpc, pic.layout,
                                                                                                       fmt, sample, pos))
    finally:
        d.free()


def wrapped_picture(ctx, surface, layout, bpc):
    """a planar native surface of the context described as a raster picture"""
    pic = Picture()
    for k, ((rows, cols), st) in enumerate(zip(surface.shapes, surface.strides)):
        pic.p[k].data, pic.p[k].stride, pic.p[k].w, pic.p[k].h = surface.bufs[k].ptr, st, cols, rows
    pic.bpc, pic.layout = bpc, layout
    return api.DevicePicture.view(ctx, pic, surface.shapes[0][1], surface.shapes[0][0], layout, bpc)


# ------------------------------------------------------------------------------------------------ 1. the case list (CPU only)

def test_the_cases_meet_every_combination():
    assert len(COMBOS) == 108 and len(CASES) == 36
    met, geom_met = {}, {}
    for case, (bpc, layout, state) in enumerate(CASES):
        for gi in range(len(GEOMS)):
            met.setdefault(combo_of(case, gi), set()).add((bpc, layout, state))
            geom_met.setdefault(gi, set()).add((bpc, layout, state))
    assert set(met) == set(COMBOS) and min(len(v) for v in met.values()) >= 4
    assert all(v == set(CASES) for v in geom_met.values())
    for what, index in (("stage", 0), ("format", 1), ("sample", 2), ("normalisation", 3), ("chroma_pos", 4)):
        for gi in range(len(GEOMS)):          # every geometry meets every value of every option
            assert {combo_of(case, gi)[index] for case in range(len(CASES))} == {c[index] for c in COMBOS}, (what, gi)
    assert all(w * h <= MAX_SAMPLES for (w, h), _, _ in GEOMS)


def test_the_geometries_are_what_they_claim():
    """from the sizes alone"""
    luma, chroma = rs.plane_axes(I420, 73, 73, 9, 9)
    assert luma[0] == (73, 9) and chroma[0] == (37, 5) and 73 > 8 * 9 and 37 <= 8 * 5
    assert rd.cells_across(2047, 8) == 2 and max(len(w) for _, w in rd.area_weights(2047, 8)) == 257
    assert GEOMS[2][0][0] == 256 * GEOMS[2][2][0]
    assert all((c[0] >> 1) & 7 == 7 and (c[1] >> 1) & 7 == 7 for _, c, _ in GEOMS[3:4]) and GEOMS[4][1][0] & 7 == 7 and GEOMS[4][1][1] & 7 == 7
    assert 300 > 8 * 7 and GEOMS[3][1][2] == 300 and GEOMS[3][2][0] == 7
    for layout in (I400, I420, I422, I444):
        assert all(d <= s <= 8 * d and d < s for axes in rs.plane_axes(layout, 190, 102, 96, 54) for s, d in axes)
        assert all(s == d for axes in rs.plane_axes(layout, 133, 71, 133, 71) for s, d in axes)
        assert all(d > s for axes in rs.plane_axes(layout, 24, 24, 40, 40) for s, d in axes)
    assert rs.plane_axes(I444, 3, 80, 4, 4)[0] == ((3, 4), (80, 4)) and rs.plane_axes(I444, 80, 3, 4, 4)[0] == ((80, 4), (3, 4))
    luma, chroma = rs.plane_axes(I420, 80, 3, 4, 4)
    assert luma[1] == (3, 4) and chroma[1] == (2, 2)
    assert rs.plane_axes(I420, 1, 1, 1, 1) == [((1, 1), (1, 1)), ((1, 1), (1, 1))] and rs.plane_axes(I444, 2, 2, 5, 3)[0] == ((2, 5), (2, 3))


# ------------------------------------------------------------------------------------------------ 2. every geometry, every combination

@pytest.mark.parametrize("case", range(len(CASES)), ids=["%dbit-l%d-%s" % c for c in CASES])
def test_every_geometry(ctx, case):
    """every geometry in every depth, layout and picture state; the stage, format, sample, normalisation and chroma_pos are dealt over them in turn"""
    bpc, layout, state = CASES[case]
    rng = np.random.default_rng(20000 + case)
    lin, m, enc = tc.random_tables(rng, bpc)
    tables = {"lin": (lin, None, None), "lin+matrix": (lin, m, None), "all": (lin, m, enc)}
    handles = {st: ctx.colour(*tables[st], bpc=bpc) for st in STAGES}
    pics = {}
    try:
        for gi, ((w, h), crop, (dw, dh)) in enumerate(GEOMS):
            if (w, h) not in pics:
                pics[w, h] = make_source(ctx, np.random.default_rng(20100 + 100 * bpc + 10 * layout + w), w, h, layout, bpc, state, extremes=True)
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

@pytest.mark.parametrize("w,h,bpc,layout,state", [(190, 102, 10, I420, "twin-only"), (73, 37, 8, I422, "raster"), (131, 19, 12, I444, "retiled")])
def test_the_whole_picture_at_its_own_size_is_export_rgb_colour(ctx, w, h, bpc, layout, state):
    rng = np.random.default_rng(20200 + bpc)
    colour = ctx.colour(*tc.random_tables(rng, bpc), bpc=bpc)
    pic, _ = make_source(ctx, rng, w, h, layout, bpc, state, extremes=True)
    try:
        for fmt, sample, pos in ((P, F32, 1), (K4, F16, 2), (K3, F16, 0)):
            a, b = Dest(ctx, w, h, layout, bpc, fmt, sample), Dest(ctx, w, h, layout, bpc, fmt, sample)
            pic.export_rgb_colour(a.surface, colour, pos)
            pic.export_rgb_colour_reduced(b.surface, colour, None, pos)
            same_bytes(a, b)
            a.free()
            b.free()
    finally:
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("state", ["raster", "twin-only"])
def test_up_to_8_to_1_is_export_scaled_then_export_rgb_colour(ctx, state):
    """d <= s <= 8 d on every plane axis: the bytes of the only other route to them — dav1d_hip_surface_export_scaled into native planes, those
    planes described as a picture, dav1d_hip_surface_export_rgb_colour from it.  Library against library."""
    w, h, bpc, layout = 190, 102, 10, I420
    rng = np.random.default_rng(20300)
    scale, bias = [f32(2), f32(0.5), f32(1)], [f32(-1), f32(0.25), f32(0)]
    colour = ctx.colour(*tc.random_tables(rng, bpc), bpc=bpc)
    pic, _ = make_source(ctx, rng, w, h, layout, bpc, state, extremes=True)
    try:
        for crop, (dw, dh) in ((None, (96, 54)), (None, (24, 13)), ((10, 6, 133, 71), (133, 71)), (None, (95, 51)), ((10, 6, 133, 71), (17, 9))):
            rect = crop or (0, 0, w, h)
            assert all(d <= s <= 8 * d for axes in rs.plane_axes(layout, rect[2], rect[3], dw, dh) for s, d in axes)
            q = ctx.surface(dw, dh, layout, bpc, api.SURFACE_PLANAR, N)
            pic.export_scaled(q, crop)
            qpic = wrapped_picture(ctx, q, layout, bpc)
            for fmt, sample, pos, norm in ((P, F32, 1, False), (K4, F16, 2, True)):
                a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
                qpic.export_rgb_colour(a.surface, colour, pos, scale if norm else None, bias if norm else None)
                pic.export_rgb_colour_reduced(b.surface, colour, crop, pos, scale if norm else None, bias if norm else None)
                same_bytes(a, b)
                a.free()
                b.free()
            ctx.sync()
            q.free()
    finally:
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("bpc,layout,state", [(8, I420, "twin-only"), (10, I420, "raster"), (12, I422, "twin-only")])
def test_a_linear_ramp_writes_the_bytes_of_export_rgb_reduced(ctx, bpc, layout, state):
    """lin[v] = float32(v) * float32(1 / max) without matrix and enc is the float sample of dav1d_hip_surface_export_rgb_reduced; with a
    normalisation whose scale is a power of two times that factor the product rounds the same way (test_surface_colour's ramp anchor)"""
    (w, h), mx = BIG, (1 << bpc) - 1
    rng = np.random.default_rng(20400 + bpc)
    colour = ctx.colour(np.arange(1 << bpc).astype(f32) * f32(1.0 / mx), bpc=bpc)
    pic, _ = make_source(ctx, rng, w, h, layout, bpc, state, extremes=True)
    try:
        for crop, (dw, dh) in (((14, 14, 300, 100), (21, 11)), (None, (96, 54)), ((8, 4, 24, 24), (40, 40))):
            for fmt, sample in ((P, F32), (K4, F16)):
                for norm in (None, ([f32(4.0), f32(0.5), f32(1.0)], [f32(-0.25), f32(0.125), f32(-3.0)])):
                    a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
                    if norm is None:
                        pic.export_rgb_reduced(a.surface, crop, 1)
                        pic.export_rgb_colour_reduced(b.surface, colour, crop, 1)
                    else:
                        pic.export_rgb_reduced(a.surface, crop, 1, [s * f32(1.0 / mx) for s in norm[0]], norm[1])
                        pic.export_rgb_colour_reduced(b.surface, colour, crop, 1, norm[0], norm[1])
                    same_bytes(a, b)
                    a.free()
                    b.free()
    finally:
        pic.free()
        ctx.colour_destroy(colour)


def test_a_permutation_matrix_swaps_the_planes(ctx):
    (w, h), (dw, dh), bpc, layout = BIG, (21, 11), 10, I420
    rng = np.random.default_rng(20500)
    lin = tc.random_tables(rng, bpc)[0]
    plain, swapped = ctx.colour(lin, bpc=bpc), ctx.colour(lin, matrix=[0, 0, 1, 0, 1, 0, 1, 0, 0], bpc=bpc)
    pic, _ = make_source(ctx, rng, w, h, layout, bpc, "raster")
    a, b = ctx.surface(dw, dh, layout, bpc, P, F32), ctx.surface(dw, dh, layout, bpc, P, F32)
    try:
        pic.export_rgb_colour_reduced(a, plain, None, 1)
        pic.export_rgb_colour_reduced(b, swapped, None, 1)
        x, y = a.download(), b.download()
        assert all(np.array_equal(x[k].view(np.uint32), y[2 - k].view(np.uint32)) for k in range(3))
        assert not np.array_equal(x[0], x[2])
    finally:
        a.free()
        b.free()
        pic.free()
        ctx.colour_destroy(plain)
        ctx.colour_destroy(swapped)


@pytest.mark.parametrize("value", [0, 1, 2047, 4095])
def test_a_constant_picture_at_12_bits_and_256_to_1(ctx, value):
    """4:4:4 with the identity matrix: the reducer's sums reach their largest values, every code of Q is the value, every sample enc[f16(lin[v])]"""
    bpc, layout = 12, I444
    rng = np.random.default_rng(20600)
    lin, _, enc = tc.random_tables(rng, bpc)
    colour = ctx.colour(lin, enc=enc, bpc=bpc)
    want16 = enc[np.asarray(min(max(lin[value], f32(0)), f32(1)), f32).astype(np.float16).view(np.uint16)]
    try:
        for (w, h), (dw, dh) in (((256, 256), (1, 1)), ((1024, 16), (4, 2))):
            assert w == 256 * dw and w * h <= MAX_SAMPLES
            pic, _ = tr.make_picture(ctx, w, h, layout, bpc, "twin-only", lambda pl, s: np.full(s, value))
            try:
                check(ctx, pic, colour, [np.full((dh, dw), want16, np.uint16)] * 3, dw, dh, P, F16, None, 1, what="constant %d" % value, matrix=0)
                f = np.full((dh, dw), np.asarray(want16, np.uint16).view(np.float16).astype(f32), f32)
                check(ctx, pic, colour, [f] * 3, dw, dh, P, F32, None, 1, what="constant %d" % value, matrix=0)
            finally:
                pic.free()
    finally:
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 4. workgroups that loop

@pytest.mark.parametrize("w,h,layout,bpc", [(515, 65, I420, 10), (260, 33, I444, 8)], ids=["420-10bit", "444-8bit"])
def test_workgroups_that_loop(ctx, w, h, layout, bpc):
    """a Q of 9 x 9 cells, ragged on both axes (the picture twice up): the library's own choice of cells per wave and, through the option
    colour_cells, 2, 3 and 64 — waves that loop, a last workgroup of few cells, one workgroup for the whole of Q: the same bytes"""
    rng = np.random.default_rng(20700 + w)
    lin, m, enc = tc.random_tables(rng, bpc)
    colour = ctx.colour(lin, m, enc, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    dw, dh = 2 * w, 2 * h
    try:
        ssh, ssv = ss_of(layout)
        assert (((dw + ssh) >> ssh) + 63) // 64 == 9 and (((dh + ssv) >> ssv) + 7) // 8 == 9
        want = want_of(vis, layout, bpc, dw, dh, None, K4, F16, 1, (lin, m, enc))
        for cells in (0, 2, 3, 64):
            ctx.set_option("colour_cells", cells)
            check(ctx, pic, colour, want, dw, dh, K4, F16, None, 1, what="colour_cells %d" % cells)
    finally:
        ctx.set_option("colour_cells", 0)
        ctx.sync()
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 5. bands and rows needed

@pytest.mark.parametrize("pos", [1, 2])
@pytest.mark.parametrize("geom", [((200, 330), None, (21, 35)), ((190, 102), None, (96, 54)), (BIG, (8, 4, 24, 24), (40, 40))], ids=["over", "under", "up"])
def test_bands(ctx, geom, pos):
    """even destination bands: each alone leaves every other row at the sentinel, their union is the one call"""
    (w, h), crop, (dw, dh) = geom
    bpc, layout = 10, I420
    rng = np.random.default_rng(20800)
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
                pic.export_rgb_colour_reduced(d.surface, colour, crop, pos, row0=r0, row1=r1)
                d.check(want, rows=[(r0, r1)] * len(want), what="band [%d, %d)" % (r0, r1))
                d.free()
                pic.export_rgb_colour_reduced(whole.surface, colour, crop, pos, row0=r0, row1=r1 if r1 < dh else 1 << 30)
            whole.check(want, what="the union of the bands of %d" % band)
            whole.free()
    finally:
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("pos", [1, 2])
@pytest.mark.parametrize("crop,size", [((10, 6, 300, 100), (30, 11)), (None, (96, 40)), ((10, 6, 40, 110), (60, 12))], ids=["over", "under", "mixed"])
def test_a_band_reads_no_row_at_or_beyond_rows_needed(ctx, crop, size, pos):
    """For every band end r1: a copy of the source whose luma rows at and beyond dav1d_hip_surface_rgb_reduced_rows_needed(r1), and the chroma rows
    under them, hold other values gives the same rows [0, r1)"""
    (w, h), (dw, dh), bpc, layout = BIG, size, 10, I420
    rng = np.random.default_rng(20900)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "raster")
    padded = [v.base for v in vis]
    want = want_of(vis, layout, bpc, dw, dh, crop, K3, F16, pos, tables)
    surface = Dest(ctx, dw, dh, layout, bpc, K3, F16)
    try:
        for r1 in list(range(2, dh, 4)) + [dh]:
            need = pic.rgb_reduced_rows_needed(surface.surface, crop, pos, r1)
            assert need == rs.rows_needed(h, crop or (0, 0, w, h), dh, 1, pos, r1)
            other = [p.copy() for p in padded]
            other[0][need:] ^= 0x155
            for pl in (1, 2):
                other[pl][(need + 1) >> 1:] ^= 0x155
            pic2, _ = source_from(ctx, other, w, h, layout, bpc, "twin-only" if r1 & 2 else "raster")
            d = Dest(ctx, dw, dh, layout, bpc, K3, F16)
            pic2.export_rgb_colour_reduced(d.surface, colour, crop, pos, row0=0, row1=r1)
            d.check(want, rows=[(0, r1)], what="rows from %d on changed, band [0, %d)" % (need, r1))
            d.free()
            pic2.free()
    finally:
        surface.free()
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 6. memory and state

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", [I420, I444], ids=["i420", "i444"])
def test_nothing_outside_the_crop_is_read(ctx, layout, state):
    """an interior crop of a picture whose samples outside the crop are 0 or max gives the bytes of the picture that is the crop alone"""
    bpc, (cw, ch), (x0, y0) = 10, (200, 90), (22, 14)
    mx = (1 << bpc) - 1
    rng = np.random.default_rng(21000 + layout)
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
        for (dw, dh), fmt, sample, pos in (((7, 9), P, F32, 1), ((100, 45), K4, F16, 2), ((230, 100), K3, F16, 1)):
            a, b = Dest(ctx, dw, dh, layout, bpc, fmt, sample), Dest(ctx, dw, dh, layout, bpc, fmt, sample)
            alone.export_rgb_colour_reduced(a.surface, colour, None, pos)
            pic.export_rgb_colour_reduced(b.surface, colour, (x0, y0, cw, ch), pos)
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
    """the sample-by-sample store path, whole units and the partial last unit (21 = 2 * 8 + 5 samples); sentinel gaps between the rows"""
    (w, h), (dw, dh), layout = (300, 100), (21, 11), I420
    for bpc, fmt, sample, k in ((8, K3, F16, 1), (10, K4, F16, 1), (10, P, F32, 2)):          # (k: offset and pad stay multiples of the sample)
        rng = np.random.default_rng(21100 + bpc)
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
    """the way test_surface_reduced.test_source_untouched_and_timed observes it: no object is allocated by the second call, the picture keeps its
    state, its pointers and every byte of its raster planes and its twin"""
    (w, h), (dw, dh), bpc, layout = BIG, (21, 11), 10, I420
    rng = np.random.default_rng(21200)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, state)
    try:
        raster = tsc._raster_bytes(ctx, pic)
        twin = util.twin_bytes(ctx, pic) if state == "twin-only" else None
        ptrs, ok = [pic.pic.twin[pl] for pl in range(3)], pic.pic.twin_ok
        if state == "twin-only":
            assert (raster == 0x5A).all()
        crop = (14, 14, 300, 100)
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 1, tables)
        check(ctx, pic, colour, want, dw, dh, K4, F16, crop, 1, what=state)          # (the scratch is made here)
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
    """no sync in between; the fourth Q (1000 x 400 at 4:2:0, 1.2 MB) outgrows the scratch the first made, the later ones reuse the larger one"""
    (w, h), bpc, layout = BIG, 10, I420
    rng = np.random.default_rng(21300)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pics = [make_source(ctx, rng, w, h, layout, bpc, "twin-only" if k & 1 else "raster") for k in range(3)]
    configs = [(None, (21, 11), P, F32, 0), ((14, 14, 300, 100), (96, 54), K3, F16, 1), ((8, 4, 24, 24), (40, 40), K4, F16, 2), (None, (1000, 400), P, F16, 1),
               ((0, 0, 80, 3), (4, 4), K4, F32, 0), (None, (330, 120), K3, F32, 2)]
    assert 1000 * 400 * 2 * 3 // 2 > 1 << 20
    dests = [Dest(ctx, dw, dh, layout, bpc, fmt, sample) for _, (dw, dh), fmt, sample, _ in configs]
    try:
        ctx.sync()
        for k, (crop, _, fmt, sample, pos) in enumerate(configs):
            pics[k % 3][0].export_rgb_colour_reduced(dests[k].surface, colour, crop, pos)
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


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refusals(ctx):
    """every refusal in the header's order, each with nothing written: a later fault never hides an earlier one"""
    w, h = 514, 102
    rng = np.random.default_rng(21400)
    pics = {key: make_source(ctx, rng, w, h, key[1], key[0], "raster")[0] for key in ((10, I420), (8, I420), (10, I422), (10, I444))}
    tall = make_source(ctx, rng, 64, 514, I420, 10, "raster")[0]
    colours = {bpc: ctx.colour(*tc.random_tables(rng, bpc), bpc=bpc) for bpc in (8, 10)}

    def refused(code, fmt=K3, sample=F16, size=(50, 12), crop=None, rows=(0, 1 << 30), change=None, key=(10, I420), params=None, shape_as=None, flt=0, pic=None,
                colour="own", **kw):
        pic = pic or pics[key]
        d = Dest(ctx, size[0], size[1], key[1], key[0], shape_as[0] if shape_as else fmt, shape_as[1] if shape_as else sample, **kw)
        d.surface.desc.format, d.surface.desc.sample = fmt, sample
        if change:
            change(d.surface.desc)
        rect = C.byref(api.SurfaceRect(*crop)) if crop is not None else None
        p = C.byref(params) if params is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), rect, p, colours[key[0]] if colour == "own" else colour,
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
            # 1. what dav1d_hip_surface_export_rgb_reduced refuses, with its codes — also with no handle and a wrong one, which come later
            for colour in ("own", None, colours[8]):
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
        assert ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced(None, None, None, None, None, None, 0, 0, 2) == -EINVAL
        # ... the crop
        for crop in ((500, 0, 100, 51), (0, 60, 95, 51), (-2, 0, 95, 51), (0, -2, 95, 51), (0, 0, 0, 51), (0, 0, 95, 0), (1, 0, 95, 51), (0, 1, 95, 51)):
            refused(EINVAL, crop=crop)
        refused(EINVAL, crop=(1, 0, 95, 51), key=(10, I422))
        # ... the ratios above 256 downwards, whatever the other axis does, and in front of a missing handle and an integer sample
        for colour, sample in (("own", F16), (None, F16), ("own", N)):
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
        # 2. -EINVAL for a NULL colour, then an integer sample, then a handle of another depth
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
        # what is accepted: the same surfaces with nothing wrong, 256:1 exactly, odd origins where the layout does not subsample the axis
        for key, crop, size in (((10, I420), None, (50, 12)), ((10, I420), (2, 0, 512, 102), (2, 12)), ((10, I422), (0, 1, 95, 51), (200, 3)),
                                ((10, I444), (1, 1, 95, 51), (3, 110)), ((8, I420), (0, 0, 184, 96), (23, 200)), ((10, I420), (0, 0, 256, 2), (1, 1))):
            for fmt in (P, K3, K4):
                d = Dest(ctx, size[0], size[1], key[1], key[0], fmt, F16, matrix=0 if key[1] == I444 else 6)
                pics[key].export_rgb_colour_reduced(d.surface, colours[key[0]], crop, 2)
                ctx.sync()
                d.free()
    finally:
        ctx.sync()
        for p in pics.values():
            p.free()
        tall.free()
        for hd in colours.values():
            ctx.colour_destroy(hd)


def test_a_picture_and_a_handle_of_another_device_are_refused():
    """-EXDEV on the emulator's two devices (tests/conftest.py): for the picture first, then for the handle; behind every -EINVAL of the call"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        rng = np.random.default_rng(21500)
        foreign = other.colour(*tc.random_tables(rng, 10), bpc=10)
        foreign8 = other.colour(*tc.random_tables(rng, 8), bpc=8)
        far = other.picture(128, 128, I420, 10)
        ctx.lib.dav1d_hip_context_use(ctx.h)
        own = ctx.colour(*tc.random_tables(rng, 10), bpc=10)
        near = ctx.picture(128, 128, I420, 10)
        d = Dest(ctx, 9, 9, I420, 10, K3, F16)
        n = Dest(ctx, 9, 9, I420, 10, K3, N)

        def call(dest, pic, colour, flt=0):
            return ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced(ctx.h, C.byref(dest.surface.desc), C.byref(pic.pic), None, None, colour, flt, 0, 96)
        assert call(d, far, own) == -EXDEV                 # the picture
        assert call(d, near, foreign) == -EXDEV            # the handle
        assert call(d, far, foreign) == -EXDEV
        assert call(d, far, own, flt=3) == -ENOTSUP        # the filter comes first
        assert call(d, far, None) == -EINVAL and call(n, far, own) == -EINVAL and call(d, far, foreign8) == -EINVAL and call(d, near, foreign8) == -EINVAL
        bad = C.c_int(-7)
        src = (C.POINTER(Picture) * 2)(C.pointer(near.pic), C.pointer(far.pic))
        dst = (type(d.surface.desc) * 2)(d.surface.desc, d.surface.desc)
        assert ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced_batch(ctx.h, 2, dst, src, None, None, own, 0, C.byref(bad)) == -EXDEV and bad.value == 1
        assert ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced_batch(ctx.h, 2, dst, src, None, None, foreign, 0, C.byref(bad)) == -EXDEV and bad.value == 0
        for x in (d, n):
            x.check(None, what="a refused export")
            x.free()
        near.free()
        ctx.colour_destroy(own)
        ctx.lib.dav1d_hip_context_use(other.h)
        far.free()
        other.colour_destroy(foreign)
        other.colour_destroy(foreign8)
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()


# ------------------------------------------------------------------------------------------------ 8. Python

def test_python_methods(ctx):
    (w, h), (dw, dh), bpc, layout = BIG, (14, 9), 10, I420
    rng = np.random.default_rng(21600)
    tables = tc.random_tables(rng, bpc)
    colour = ctx.colour(*tables, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "retiled")
    s = ctx.surface(dw, dh, layout, bpc, K4, F16)
    try:
        s.fill(0xA5)
        crop = (10, 2, 300, 100)
        assert api._lib.SYMBOLS.count("dav1d_hip_surface_export_rgb_colour_reduced") == 1
        pic.export_rgb_colour_reduced(s, colour, crop=crop, chroma_pos=api.CHROMA_COLOCATED, scale=[2.0, 1.0, 0.5], bias=[-1.0, 0.0, 1.0], filter=api.RESIZE_BILINEAR)
        got = s.download()[0]
        want = want_of(vis, layout, bpc, dw, dh, crop, K4, F16, 2, tables, scale=[f32(v) for v in (2.0, 1.0, 0.5)], bias=[f32(v) for v in (-1.0, 0.0, 1.0)])[0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
        with pytest.raises(api.HipError, match="errno %d" % ENOTSUP):
            pic.export_rgb_colour_reduced(s, colour, crop, filter=3)
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            pic.export_rgb_colour_reduced(s, None, crop)
    finally:
        s.free()
        pic.free()
        ctx.colour_destroy(colour)


def test_the_older_tensor_functions_still_raise():
    """export_to_tensor and export_batch_to_tensor keep every ValueError they have for colour= with resize / interp; the new functions check shapes
    the same way before anything reaches the library"""
    from test_surface_batch import FakeTensor
    t = FakeTensor((3, 54, 96))
    for kw in (dict(interp="area", colour=object()), dict(interp="area", resize=True, colour=object()), dict(interp="bilinear", resize=True, colour=object()),
               dict(resize=True, colour=object()), dict(crop=(0, 0, 96, 54), colour=object())):
        with pytest.raises(ValueError):
            api.export_to_tensor(object(), t, **kw)
    with pytest.raises(TypeError):
        api.export_batch_to_tensor([object()] * 4, FakeTensor((4, 3, 54, 96)), colour=object())
    for match, tensor in (("read as", FakeTensor((3, 54, 3))), ("read as", FakeTensor((3, 54, 4))), ("has shape", FakeTensor((2, 54, 96))),
                          ("has shape", FakeTensor((54, 96, 5))), ("has shape", FakeTensor((4, 3, 54, 96))), ("device tensor", FakeTensor((3, 54, 96), is_cuda=False)),
                          ("unit stride", FakeTensor((3, 54, 96), [54 * 192, 192, 2])), ("next to each other", FakeTensor((54, 96, 4), [96 * 8, 8, 1]))):
        with pytest.raises(ValueError, match=match):
            api.export_colour_to_tensor(object(), tensor, object())
    with pytest.raises(ValueError, match="colour handle"):
        api.export_colour_to_tensor(object(), t, None)
    for match, tensor, n_pics in (("read as", FakeTensor((4, 3, 54, 3)), 4), ("takes 4 pictures", FakeTensor((4, 3, 54, 96)), 3), ("has shape", FakeTensor((4, 2, 54, 96)), 4),
                                  ("has shape", FakeTensor((3, 54, 96)), 3), ("device tensor", FakeTensor((4, 3, 54, 96), is_cuda=False), 4),
                                  ("unit stride", FakeTensor((4, 3, 54, 96), [3 * 54 * 192, 54 * 192, 192, 2]), 4)):
        with pytest.raises(ValueError, match=match):
            api.export_colour_batch_to_tensor([object()] * n_pics, tensor, object())
    with pytest.raises(ValueError, match="colour handle"):
        api.export_colour_batch_to_tensor([object()] * 4, FakeTensor((4, 3, 54, 96)), None)
