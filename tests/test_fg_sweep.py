"""Film grain, ENUMERATED: the geometry of the apply kernel, every (lag, shift, layout) of the template generator and the ends of the
arithmetic (csrc/fg.hip) against the oracle's dav1d_apply_grain / template generator, byte for byte.

tests/test_filmgrain.py runs four picture sizes and one random draw of ar_coeff_lag, the shifts and overlap per case.  The apply
kernel has a fast path for whole quads of four pixels and a per-pixel path for the rest, overlap extents clamped by the block,
workgroups of four blocks whose last one in a row holds waves past the end, and chroma blocks of height (bh + sy) >> sy: this
module lists the sizes where those change.  What the cases cover is collected in a set FIRST and the set is asserted; the
conditions are computed from the geometry of the specification (32 x 32 luma blocks, (w + ss) >> ss chroma) restated here or
taken from the oracle's outputs, never read from the code under test.

* test_every_width_and_height_class -- I400 / I420 / I422 / I444 x 8 / 10 / 12 bit.  hip: widths {1 .. 9, 31 .. 35, 63 .. 67,
  127 .. 131} x heights {1, 2, 3, 31 .. 35, 63, 65}; emu: every width at heights {1, 33} and every height at widths {1, 35, 129}.
  overlap, chroma_scaling_from_luma and clip_to_restricted_range (with is_id both ways) rotate so that every (layout, overlap)
  meets every width and every height and all twelve combinations occur.  Both fg_apply and the prepare / apply-prepared pair write
  into pictures that are random beforehand, and the whole padded planes are compared: what the reference does not write keeps its
  value.  Asserted from geometry: every bw mod 4 in the last block of a row (luma and chroma), whole chroma quads whose luma reach
  4 << sx ends inside and outside the luma width, bh == 1 and bw == 1 with overlap below / right of another block, rows of 1, 4
  and 5 blocks.  Asserted on the oracle alone: the output differs from the source in every plane that gets grain, in EVERY case
  (the grain seed of a case is the first of a fixed sequence for which the oracle's output does; a 1 x 1 picture can draw a zero).
* test_every_lag_shift_and_layout -- templates for ar_coeff_lag 0 .. 3 x ar_coeff_shift 6 .. 9 x grain_scale_shift 0 .. 3 x the
  four layouts, AR coefficients from a seed and at the corners (all -128 >> 2, all 127 >> 2, alternating; hip: the product, emu:
  the family rotates so that it meets every value of each other parameter); the oracle's templates
  hold grain_min and grain_max; num_y_points 0 with chroma points, num_uv_points 0 for either plane, templates and application
  (the plane without grain is a copy of the source); then the application on a
  67 x 35 picture per (lag, layout) with scaling_shift 8 .. 11.
* test_extremal_content_and_scaling -- sources all 0, all bitdepth_max, checkerboard, and the restricted-range limits +- 1; scaling
  functions of 1 point and of 14 (10 for chroma) points, of value 0 and 255; uv_mult, uv_luma_mult, uv_offset at the corners of
  their ranges (the second chroma plane at the opposite corner).  By a Python restatement over the cases that use the multipliers,
  (combined >> 6) + offset leaves [0, bitdepth_max] at both ends in both chroma planes; the oracle's outputs hold
  0 and bitdepth_max, and with the restricted clip both of its limits, in luma and in chroma.

The fused grain of the surface export has its own module (tests/test_surface_grain.py).  Cost: DESIGN.md 11.  An emulator trap ends
the pytest process: run this module in a pytest call of its own first."""
import ctypes as C
import itertools

import numpy as np
import pytest

import util
from dav1d_amd import api
from test_filmgrain import fg_driver, random_fg

LAYOUTS = {"i400": api.LAYOUT_I400, "i420": api.LAYOUT_I420, "i422": api.LAYOUT_I422, "i444": api.LAYOUT_I444}
WIDTHS = list(range(1, 10)) + list(range(31, 36)) + list(range(63, 68)) + list(range(127, 132))
HEIGHTS = [1, 2, 3, 31, 32, 33, 34, 35, 63, 65]
SEEDS = [(7919 * k + 1) & 0xffff for k in range(24)]       # grain seeds a case tries in turn


def subsampling(layout):
    return int(layout in (api.LAYOUT_I420, api.LAYOUT_I422)), int(layout == api.LAYOUT_I420)


def grained_planes(data, layout):
    out = [0] if data.num_y_points else []
    if layout != api.LAYOUT_I400:
        out += [pl for pl in (1, 2) if data.num_uv_points[pl - 1] or data.chroma_scaling_from_luma]
    return out


def visible(layout, w, h, pl):
    sx, sy = subsampling(layout)
    return ((h + sy) >> sy, (w + sx) >> sx) if pl else (h, w)


def oracle_apply(lib, bpc, layout, w, h, data, is_id, src, dst0):
    """the oracle's dav1d_apply_grain from copies of `src` into copies of `dst0` (padded planes)"""
    want, inp = [p.copy() for p in dst0], [p.copy() for p in src]
    n = len(src)
    outp = (C.c_void_p * 3)(*([p.ctypes.data for p in want] + [None] * (3 - n)))
    inpp = (C.c_void_p * 3)(*([p.ctypes.data for p in inp] + [None] * (3 - n)))
    lib.apply_grain(bpc, C.byref(data), w, h, layout, is_id, outp, inpp, want[0].strides[0], want[1].strides[0] if n == 3 else 0)
    return want


def compare_routes(ctx, bpc, layout, w, h, data, is_id, src, dst0, want, what):
    """fg_apply and fg_prepare + fg_apply_prepared into pictures holding dst0.  A plane that gets grain is compared whole, padding
    included; one that does not is a copy of the source over its visible size, and keeps its rows below it (the reference copies
    whole rows of the stride there, so the columns to their right say nothing)."""
    n = len(src)
    sp, dp = ctx.picture(w, h, layout, bpc), ctx.picture(w, h, layout, bpc)
    for pl in range(n):
        sp.upload(pl, src[pl])
    grained = grained_planes(data, layout)
    for split in (False, True):
        for pl in range(n):
            dp.upload(pl, dst0[pl])
        if split:
            g = ctx.fg_prepare(data, bpc, layout)
            ctx.fg_apply_prepared(dp, sp, g, is_id)
            ctx.fg_grain_destroy(g)
        else:
            ctx.fg_apply(dp, sp, data, is_id)
        for pl in range(n):
            got = dp.download(pl)
            vh, vw = visible(layout, w, h, pl)
            if pl in grained:
                bad = np.argwhere(got != want[pl])
            else:
                bad = np.argwhere(got[:vh, :vw] != src[pl][:vh, :vw])
                if not len(bad):
                    bad = np.argwhere(got[vh:] != dst0[pl][vh:]) + [vh, 0]
            if len(bad):
                yy, xx = bad[0]
                raise AssertionError("%s, %s: plane %d (visible %d x %d) at (%d,%d) is %d, the oracle has %d (source %d, before the call %d); %d pixels differ" % (
                    what, "prepare + apply" if split else "fg_apply", pl, vw, vh, xx, yy, got[yy, xx], want[pl][yy, xx], src[pl][yy, xx], dst0[pl][yy, xx], len(bad)))
    sp.free(); dp.free()


def random_planes(rng, bpc, layout, w, h):
    sx, sy = subsampling(layout)
    ph, pw = (h + 127) & ~127, (w + 127) & ~127
    shapes = [(ph, pw)] + ([(ph >> sy, pw >> sx)] * 2 if layout != api.LAYOUT_I400 else [])
    return [rng.integers(0, 1 << bpc, size=s).astype(util.pix_dtype(bpc)) for s in shapes]


# ------------------------------------------------------------------ 1. every width and height class

def geometry_cases(full):
    sizes = [(w, h) for w in WIDTHS for h in HEIGHTS] if full else \
            sorted({(w, h) for w in WIDTHS for h in (1, 33)} | {(w, h) for w in (1, 35, 129) for h in HEIGHTS})
    cases = []
    for w, h in sizes:
        wi, hi = WIDTHS.index(w), HEIGHTS.index(h)
        k = wi + hi
        cases.append((w, h, k & 1, (wi + (hi >> 1)) & 1, (wi + 2 * hi + (k >> 1)) % 3))      # overlap, csfl, clip mode (0 off, 1 on, 2 on with is_id)
    return cases


def assert_geometry_coverage(cases, layout, full):
    sx, sy = subsampling(layout)
    chroma = layout != api.LAYOUT_I400
    ws, hs = {c[0] for c in cases}, {c[1] for c in cases}
    assert ws == set(WIDTHS) and hs == set(HEIGHTS) and len({c[:2] for c in cases}) == len(cases)
    if full:
        assert {c[:2] for c in cases} == set(itertools.product(WIDTHS, HEIGHTS))
    else:
        assert {c[:2] for c in cases} == set(itertools.product(WIDTHS, (1, 33))) | set(itertools.product((1, 35, 129), HEIGHTS))
    assert {(c[2], c[0]) for c in cases} == set(itertools.product((0, 1), WIDTHS)), "not every (overlap, width)"
    assert {(c[2], c[1]) for c in cases} == set(itertools.product((0, 1), HEIGHTS)), "not every (overlap, height)"
    assert {c[2:] for c in cases} == set(itertools.product((0, 1), (0, 1), (0, 1, 2))), "not every (overlap, csfl, clip mode)"
    last = lambda n, step: (n - 1) % step + 1          # extent of the last block of a row / column
    assert {last(w, 32) % 4 for w in ws} == {0, 1, 2, 3}
    assert {-(-w // 32) for w in ws} >= {1, 4, 5}, "rows of 1, 4 and 5 blocks"
    assert any(ov and h > 32 and last(h, 32) == 1 for w, h, ov, _, _ in cases), "bh == 1 below another block row, with overlap"
    assert any(ov and w > 32 and last(w, 32) == 1 for w, h, ov, _, _ in cases), "bw == 1 right of another block, with overlap"
    if chroma:
        cw = lambda w: (w + sx) >> sx
        assert {last(cw(w), 32 >> sx) % 4 for w in ws} == {0, 1, 2, 3}
        assert any(ov and cw(w) > (32 >> sx) and last(cw(w), 32 >> sx) == 1 for w, h, ov, _, _ in cases)
        assert any(ov and h > 32 and (last(h, 32) + sy) >> sy == 1 for w, h, ov, _, _ in cases)
        assert {(last(h, 32) + sy) >> sy for h in hs} >= {1, 2, 16 if sy else 32}
        # a whole chroma quad [x, x + 4) reaches luma column (x + 4) << sx: inside the luma width, and (odd widths of a
        # horizontally sub-sampled layout whose chroma width is a multiple of 4) one past it
        reach = {((x + 4) << sx) <= w for w in ws for x in range(0, cw(w) - 3, 4)}
        assert reach == ({True, False} if sx else {True})


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_width_and_height_class(ctx, layout, bpc):
    lib = fg_driver()
    name, layout = layout, LAYOUTS[layout]
    cases = geometry_cases(ctx.backend == "hip")
    assert_geometry_coverage(cases, layout, ctx.backend == "hip")
    rng = np.random.default_rng(4100 + 10 * bpc + layout)
    for w, h, overlap, csfl, clip in cases:
        data = random_fg(rng, bpc, 0)
        data.overlap_flag, data.clip_to_restricted_range = overlap, int(clip > 0)
        data.chroma_scaling_from_luma = csfl if layout != api.LAYOUT_I400 else 0
        if csfl or layout == api.LAYOUT_I400:          # the frame header carries no chroma points then
            data.num_uv_points[0] = data.num_uv_points[1] = 0
        is_id = int(clip == 2)
        # strong scaling (values 128 .. 255 at shift 8): the noise of a pixel is seldom 0, so that a plane of one pixel can change
        data.scaling_shift = 8
        for i in range(14):
            data.y_points[i][1] |= 128
        for pl, i in itertools.product(range(2), range(10)):
            data.uv_points[pl][i][1] |= 128
        src, dst0 = random_planes(rng, bpc, layout, w, h), random_planes(rng, bpc, layout, w, h)
        grained = grained_planes(data, layout)
        assert grained == list(range(len(src)))
        for seed in SEEDS:          # on the oracle alone: every plane that gets grain comes out different from the source
            data.seed = seed
            want = oracle_apply(lib, bpc, layout, w, h, data, is_id, src, dst0)
            if all(not np.array_equal(want[pl][:vh, :vw], src[pl][:vh, :vw]) for pl in grained for vh, vw in [visible(layout, w, h, pl)]):
                break
        else:
            raise AssertionError("%s %d bpc %d x %d: no seed of the sequence changes every plane" % (name, bpc, w, h))
        compare_routes(ctx, bpc, layout, w, h, data, is_id, src, dst0, want,
                       "%s %d bpc %d x %d overlap %d csfl %d clip %d is_id %d" % (name, bpc, w, h, overlap, csfl, int(clip > 0), is_id))


# ------------------------------------------------------------------ 2. every lag, shift and layout

COEF_FAMILIES = ["seed", "all -128 >> 2", "all 127 >> 2", "alternating"]


def set_ar_coefs(data, rng, family):
    for i in range(25):
        v = {"seed": int(rng.integers(-128, 128)) >> 2, "all -128 >> 2": -128 >> 2, "all 127 >> 2": 127 >> 2,
             "alternating": (127 >> 2) if i & 1 else (-128 >> 2)}[family]
        if i < 24:
            data.ar_coeffs_y[i] = v
        for pl in range(2):
            data.ar_coeffs_uv[pl][i] = v if family != "seed" else int(rng.integers(-128, 128)) >> 2


def check_templates(ctx, lib, bpc, layout, data, what):
    want = np.zeros((3, 74, 82), np.int16)
    lib.generate_grain(bpc, C.byref(data), layout, want.ctypes.data)
    got = ctx.fg_generate_grain(data, bpc, layout)
    n = 1 if layout == api.LAYOUT_I400 else 3
    for pl in range(n):
        bad = np.argwhere(got[pl] != want[pl])
        assert not len(bad), "%s: template %d at %s is %d, the oracle has %d (%d differ)" % (what, pl, bad[0], got[pl][tuple(bad[0])], want[pl][tuple(bad[0])], len(bad))
    return want[:n]


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_lag_shift_and_layout(ctx, bpc):
    lib = fg_driver()
    rng = np.random.default_rng(4200 + bpc)
    rows = [(lag, sh, gss, name, fam) for lag in range(4) for sh in range(6, 10) for gss in range(4) for name in LAYOUTS for fam in COEF_FAMILIES]
    if ctx.backend == "emu":          # the coefficient family rotates instead of multiplying: every pair of it with another parameter stays
        rows = [r for r in rows if COEF_FAMILIES.index(r[4]) == (r[0] + r[1] + r[2] + list(LAYOUTS).index(r[3])) % 4]
    assert len(set(rows)) == 4 * 4 * 4 * 4 * (4 if ctx.backend == "hip" else 1)
    assert {r[:4] for r in rows} == set(itertools.product(range(4), range(6, 10), range(4), LAYOUTS))
    for i in range(4):
        assert {(r[i], r[4]) for r in rows} == set(itertools.product(sorted({r[i] for r in rows}), COEF_FAMILIES))
    grain_min, grain_max = -(128 << (bpc - 8)), (128 << (bpc - 8)) - 1
    lows, highs = set(), set()
    for lag, sh, gss, name, fam in rows:
        layout = LAYOUTS[name]
        data = random_fg(rng, bpc, 0)
        data.ar_coeff_lag, data.ar_coeff_shift, data.grain_scale_shift = lag, sh, gss
        set_ar_coefs(data, rng, fam)
        if layout == api.LAYOUT_I400:
            data.num_uv_points[0] = data.num_uv_points[1] = 0
        want = check_templates(ctx, lib, bpc, layout, data, "%s %d bpc lag %d shift %d scale shift %d, %s" % (name, bpc, lag, sh, gss, fam))
        for pl in range(len(want)):
            lows |= {(name, pl)} if want[pl].min() == grain_min else set()
            highs |= {(name, pl)} if want[pl].max() == grain_max else set()
        assert want.min() >= grain_min and want.max() <= grain_max
    planes = {(name, pl) for name in LAYOUTS for pl in range(1 if name == "i400" else 3)}
    assert lows == planes and highs == planes, "the oracle's templates do not reach both grain clips in every plane of every layout"
    # planes that get no template: no luma points with chroma points, no points for one chroma plane
    for name, (ny, nuv) in itertools.product(("i420", "i422", "i444"), ((0, (3, 4)), (2, (0, 5)), (2, (6, 0)))):
        data = random_fg(rng, bpc, 0)
        data.num_y_points, data.num_uv_points[0], data.num_uv_points[1] = ny, nuv[0], nuv[1]
        check_templates(ctx, lib, bpc, LAYOUTS[name], data, "%s %d bpc, %d luma and %s chroma points" % (name, bpc, ny, nuv))
        # ... and applied: such a plane comes out as a copy of the source, nothing below its visible rows is written
        src, dst0 = random_planes(rng, bpc, LAYOUTS[name], 67, 35), random_planes(rng, bpc, LAYOUTS[name], 67, 35)
        assert len(grained_planes(data, LAYOUTS[name])) == 2
        want = oracle_apply(lib, bpc, LAYOUTS[name], 67, 35, data, 0, src, dst0)
        compare_routes(ctx, bpc, LAYOUTS[name], 67, 35, data, 0, src, dst0, want, "%s %d bpc, %d luma and %s chroma points" % (name, bpc, ny, nuv))
    # application per (lag, layout, scaling_shift)
    w, h = 67, 35
    for lag, name, shift in itertools.product(range(4), LAYOUTS, range(8, 12)):
        layout = LAYOUTS[name]
        data = random_fg(rng, bpc, 0)
        data.ar_coeff_lag, data.scaling_shift = lag, shift
        if layout == api.LAYOUT_I400:
            data.num_uv_points[0] = data.num_uv_points[1] = 0
        src, dst0 = random_planes(rng, bpc, layout, w, h), random_planes(rng, bpc, layout, w, h)
        want = oracle_apply(lib, bpc, layout, w, h, data, 0, src, dst0)
        compare_routes(ctx, bpc, layout, w, h, data, 0, src, dst0, want, "%s %d bpc lag %d scaling_shift %d" % (name, bpc, lag, shift))


# ------------------------------------------------------------------ 3. extremal content and scaling

def extremal_sources(bpc, shapes):
    """name -> planes: constant planes and a checkerboard of 0 / bitdepth_max, over the whole padded planes"""
    b, mx = bpc - 8, (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    out = {"all 0": [np.zeros(s, pd) for s in shapes], "all max": [np.full(s, mx, pd) for s in shapes]}
    yy, xx = np.indices(shapes[0])
    out["checkerboard"] = [(((yy[:s[0], :s[1]] + xx[:s[0], :s[1]]) & 1) * mx).astype(pd) for s in shapes]
    for v in (16, 235, 240):
        for d in (-1, 1):
            out["%d %+d" % (v, d)] = [np.full(s, (v << b) + d, pd) for s in shapes]
    return out


def set_scaling(data, npoints, value):
    """scaling functions of `npoints` points (at most 10 for chroma) of one value"""
    data.num_y_points = npoints
    for i in range(14):
        data.y_points[i][0], data.y_points[i][1] = (i * 255) // 13 if npoints > 1 else 128, value
    for pl in range(2):
        data.num_uv_points[pl] = min(npoints, 10)
        for i in range(10):
            data.uv_points[pl][i][0], data.uv_points[pl][i][1] = (i * 255) // 9 if npoints > 1 else 128, value


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_extremal_content_and_scaling(ctx, bpc):
    lib = fg_driver()
    rng = np.random.default_rng(4300 + bpc)
    b, mx = bpc - 8, (1 << bpc) - 1
    w, h = 67, 35
    layout = api.LAYOUT_I420
    shapes = [p.shape for p in random_planes(rng, bpc, layout, w, h)]
    sources = extremal_sources(bpc, shapes)
    assert set(sources) == {"all 0", "all max", "checkerboard", "16 -1", "16 +1", "235 -1", "235 +1", "240 -1", "240 +1"}
    corners = list(itertools.product((-128, 127), (-128, 127), (-256, 255)))          # uv_mult, uv_luma_mult, uv_offset
    cases, below, above = [], set(), set()
    vh, vw = visible(layout, w, h, 1)
    for k, (((sname, src), (npoints, value)), clip) in enumerate(itertools.product(itertools.product(sources.items(), ((1, 0), (1, 255), (14, 0), (14, 255))), (0, 1, 2))):
        um, ulm, uo = corners[k % 8]
        csfl = int(k % 5 == 4)
        cases.append((sname, npoints, value, clip, um, ulm, uo, csfl))
        if csfl:          # the multipliers are not used then
            continue
        # (combined >> 6) + offset before its clip, on every visible chroma pixel of both planes (4:2:0: luma is the rounded average
        # of two pixels of one row, the last one repeated past an odd width); plane 2 takes the opposite corner in uv_mult and uv_offset
        luma = np.concatenate([src[0][:h:2, :w], src[0][:h:2, w - 1:w]], axis=1).astype(np.int64)
        lum = (luma[:, 0:2 * vw:2] + luma[:, 1:2 * vw:2] + 1) >> 1
        for pl, (m, lm, o) in ((1, (um, ulm, uo)), (2, (-um - 1, ulm, -uo - 1))):
            v = ((lum * lm + src[pl][:vh, :vw].astype(np.int64) * m) >> 6) + o * (1 << b)
            below |= {pl} if (v < 0).any() else set()
            above |= {pl} if (v > mx).any() else set()
    assert {c[4:7] for c in cases if not c[7]} == set(corners) and {(c[0], c[1], c[2]) for c in cases} == set(itertools.product(sources, (1, 14), (0, 255)))
    assert {(c[0], c[3]) for c in cases} == set(itertools.product(sources, (0, 1, 2)))
    assert below == above == {1, 2}, "the clip of (combined >> 6) + offset to [0, bitdepth_max] is not reached at both ends in both chroma planes"
    seen, runs = {}, []
    for sname, npoints, value, clip, um, ulm, uo, csfl in cases:
        data = random_fg(rng, bpc, 0)
        set_scaling(data, npoints, value)
        data.scaling_shift, data.clip_to_restricted_range = 8, int(clip > 0)
        data.chroma_scaling_from_luma = csfl
        for pl in range(2):
            data.uv_mult[pl], data.uv_luma_mult[pl], data.uv_offset[pl] = (um, ulm, uo) if pl == 0 else (-um - 1, ulm, -uo - 1)
        is_id = int(clip == 2)
        src = sources[sname]
        dst0 = random_planes(rng, bpc, layout, w, h)
        want = oracle_apply(lib, bpc, layout, w, h, data, is_id, src, dst0)
        for pl in range(3):
            vh, vw = visible(layout, w, h, pl)
            seen.setdefault((clip, min(pl, 1)), set()).update(np.unique(want[pl][:vh, :vw]).tolist())
        runs.append((data, is_id, src, dst0, want, "%s, %d points of %d, clip %d, uv (%d, %d, %d), %d bpc" % (sname, npoints, value, clip, um, ulm, uo, bpc)))
    # on the oracle's outputs alone: both ends of every clip, in luma and in chroma
    for chroma in (0, 1):
        assert {0, mx} <= seen[0, chroma], "no clip: plane type %d lacks 0 or bitdepth_max" % chroma
        assert min(seen[1, chroma]) == 16 << b and max(seen[1, chroma]) == (240 if chroma else 235) << b
        assert min(seen[2, chroma]) == 16 << b and max(seen[2, chroma]) == 235 << b
    for data, is_id, src, dst0, want, what in runs:
        compare_routes(ctx, bpc, layout, w, h, data, is_id, src, dst0, want, what)
