"""CDEF, ENUMERATED: every strength pair, direction and damping, the ties of the direction search, extreme pixels beside missing
neighbours and the ways units fall into strips -- against the oracle, under BOTH kernels (the strips, and cdef_unit = 1).

tests/test_cdef.py draws strengths, edges and content at random and uploads dst as a copy of src.  Here dst is pre-filled with a
pattern that differs from src: the expected picture is that pattern outside the listed units, src inside listed units on planes that
do not filter, the oracle's output where they do -- so a kernel that wrote anything over unlisted units, or left a listed unit
unwritten, fails.  The reference reads a block's right-hand neighbours through the destination pointer, so each unit is filtered in
a scratch copy of the source planes and its blocks are copied out.  What each test ran is collected in a set FIRST and the set is
asserted, so the coverage below is a checked fact:

* test_every_strength_direction_and_damping -- oriented stripes plus graded noise; direction and variance are READ FROM THE ORACLE's
  cdef_dir.  All four layouts x 8 / 10 / 12 bit (a superset of the (bpc, layout) list of test_cdef.py, which the other tests here keep
  to).  hip: the full product y_pri 0 .. 15 x y_sec {0, 1, 2, 4} x oracle direction 0 .. 7 x damping 3 .. 6 (+ bitdepth_min_8), one
  call per damping; the chroma pair is the luma pair rotated by a fixed offset, so chroma sees all 64 pairs too.  emu: every (pri,
  sec) pair per plane type, and as pairs every
  (pri, damping), (sec, damping), (direction, pri > 0), (direction, sec > 0).  Both: var == 0 occurs; every adjust_strength index
  i = 0 .. 12 occurs with y_pri > 0 (horizontal stripes of growing amplitude); on 4:2:2 every luma direction occurs with uv_pri > 0
  (the remap).  dirvar is compared wherever a primary strength is set.
* test_direction_ties_and_extremes -- constant 0 / mid / max, checkerboards of 0 and max with period 1 and 2, a single max pixel in 0 at
  each of the 64 positions and the inverse, transpose-, mirror- and 180-degree-symmetric blocks, rows-only and columns-only stripes of
  0 / max, with y_pri = uv_pri = 15 << bd8.  A numpy restatement of the eight costs (labels only) agrees with the oracle's direction
  and variance on every unit, and by it the set holds units whose best cost is shared by two or more directions for at least four
  different winning directions.
* test_extremal_pixels_next_to_missing_neighbours -- all 16 `edges` x content {all 0, all max, checkerboard 0 / max, max block in a 0
  surround, 0 block in a max surround, isolated low peaks on 0, isolated shallow valleys in max (where the clamp to the local
  range decides)} x (pri, sec) in {(15,4), (1,1), (15,0), (0,4), (0,1), (1,0)} << bd8 on luma and chroma x damping
  {3, 6} + bd8, 8 / 10 / 12 bit, 4:2:0 and 4:4:4; both BOT_REP flags where edges & 8.  The same product on hip and emu (on emu the packed
  int16 helpers trap when an operand leaves its range).
* test_strip_compositions -- unit rows built from named templates, every template asserted per layout: 1, 15, 16, 17, 32 and 33 listed
  units in a row; gaps of 1 and of several unlisted units inside a run; a unit in mid-row without HAVE_LEFT; a unit whose predecessor
  lacks HAVE_RIGHT; top / bottom flags changing in mid-row; a run in which no unit filters chroma; one chroma-filtering unit among
  luma-only ones; a listed unit with all four strengths 0; rep-flag changes in mid-row.

An emulator trap ends the pytest process: run this module in a pytest call of its own first.  Cost: DESIGN.md 11."""
import itertools

import numpy as np
import pytest

import util
import synth_frames as synth
from test_cdef import oracle_cdef_unit
from dav1d_amd import api

SEC = [0, 1, 2, 4]
LAYOUTS_EMU = [(8, api.LAYOUT_I420), (10, api.LAYOUT_I420), (12, api.LAYOUT_I420), (8, api.LAYOUT_I444), (10, api.LAYOUT_I444),
               (8, api.LAYOUT_I422), (10, api.LAYOUT_I422), (10, api.LAYOUT_I400)]          # the list of tests/test_cdef.py
LAYOUTS_ALL = [(bpc, layout) for layout in (api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444) for bpc in (8, 10, 12)]
REP_Y, REP_UV = 8, 16          # DAV1D_HIP_CDEF_BOT_REP_*
LEFT, RIGHT, TOP, BOTTOM = 1, 2, 4, 8


def subsampling(layout):
    return int(layout != api.LAYOUT_I444), int(layout == api.LAYOUT_I420)


def task_row(bx, by, y_pri, y_sec, uv_pri, uv_sec, edges, flags, bd8):
    return (bx, by, y_pri << bd8, y_sec << bd8, uv_pri << bd8, uv_sec << bd8, edges, flags, 0, 0, (0, 0, 0, 0))


def picture_edges(bx, by, bw, bh):
    return (LEFT if bx > 0 else 0) | (RIGHT if bx < bw - 1 else 0) | (TOP if by > 0 else 0) | (BOTTOM if by < bh - 1 else 0)


class Case:
    pass


def prepare(bpc, layout, planes, rows, damping, rng):
    """rows -> CDEF tasks and the expected picture; the oracle's (direction, variance) per task in .dv"""
    oracle = util.default_oracle()
    c = Case()
    c.bpc, c.layout, c.planes, c.damping = bpc, layout, planes, damping
    n_pl = len(planes)
    ss_hor, ss_ver = subsampling(layout)
    c.tasks = tasks = np.zeros(len(rows), api.CDEF_TASK)
    for k, r in enumerate(rows):
        tasks[k] = r
    assert len({(int(t["bx"]), int(t["by"])) for t in tasks}) == len(tasks)
    h, w = planes[0].shape
    fill = [np.where(f == p, f ^ 1, f) for f, p in zip(synth.make_planes(rng, w, h, bpc, smooth=False, layout=layout), planes)]
    c.fill = synth.copy_planes(fill)          # differs from src in every pixel
    c.want = synth.copy_planes(c.fill)
    work = synth.copy_planes(planes)
    c.want_dv = np.zeros(len(tasks), np.uint32)
    for k, t in enumerate(tasks):
        d, v = oracle_cdef_unit(oracle, bpc, planes, work, t, damping, layout)
        c.want_dv[k] = d | (v << 3)
        for pl in range(n_pl):
            bw_, bh_ = (8, 8) if pl == 0 else (8 >> ss_hor, 8 >> ss_ver)
            x0, y0 = int(t["bx"]) * bw_, int(t["by"]) * bh_
            c.want[pl][y0:y0 + bh_, x0:x0 + bw_] = work[pl][y0:y0 + bh_, x0:x0 + bw_]
            work[pl][y0:y0 + bh_, x0:x0 + bw_] = planes[pl][y0:y0 + bh_, x0:x0 + bw_]
    c.dv = [(int(v) & 7, int(v) >> 3) for v in c.want_dv]
    return c


def compare(ctx, c):
    """both kernels against the expected picture of prepare()"""
    bpc, layout, planes, tasks, damping, fill, want = c.bpc, c.layout, c.planes, c.tasks, c.damping, c.fill, c.want
    n_pl = len(planes)
    ss_hor, ss_ver = subsampling(layout)
    h, w = planes[0].shape
    pri_any = (tasks["y_pri"] > 0) | (tasks["uv_pri"] > 0)
    src_pic, dst_pic = ctx.picture(w, h, layout, bpc), ctx.picture(w, h, layout, bpc)
    dirvar = ctx.buffer(4 * len(tasks))
    try:
        for pl in range(n_pl):
            src_pic.upload(pl, planes[pl])
        for unit_kernel in (0, 1):
            ctx.set_option("cdef_unit", unit_kernel)
            for pl in range(n_pl):
                dst_pic.upload(pl, fill[pl])
            dirvar.zero()
            ctx.cdef_batch(dst_pic, src_pic, tasks, damping, dirvar)
            for pl in range(n_pl):
                got = dst_pic.download(pl)
                bad = np.argwhere(got != want[pl])
                if len(bad):
                    yy, xx = (int(v) for v in bad[0])
                    ux, uy = (xx // 8, yy // 8) if pl == 0 else (xx // (8 >> ss_hor), yy // (8 >> ss_ver))
                    hit = [tuple(t)[:8] for t in tasks if t["bx"] == ux and t["by"] == uy]
                    raise AssertionError("cdef_unit=%d damping %d plane %d differs at (x %d, y %d): got %d want %d src %d fill %d (%d px); task %s"
                                         % (unit_kernel, damping, pl, xx, yy, got[yy, xx], want[pl][yy, xx], planes[pl][yy, xx], fill[pl][yy, xx],
                                            len(bad), hit or "unit (%d, %d) is not listed" % (ux, uy)))
            got_dv = dirvar.download(np.uint32, len(tasks))
            assert np.array_equal(got_dv[pri_any], c.want_dv[pri_any]), "cdef_unit=%d: direction / variance side output" % unit_kernel
    finally:
        ctx.set_option("cdef_unit", 0)          # the shared fixture does not reset this option
        for o in (src_pic, dst_pic, dirvar):
            o.free()


def noise_planes(rng, w, h, bpc, layout):
    return synth.make_planes(rng, w, h, bpc, smooth=False, layout=layout)


# ------------------------------------------------------------------ the direction search, restated for labels only

def line_index(direction, x, y):
    """which line of `direction` pixel (x, y) of an 8x8 block lies on (AV1 spec 7.15.2)"""
    return [y + x, y + (x >> 1), y, 3 + y - (x >> 1), 7 + y - x, 3 - (y >> 1) + x, x, (y >> 1) + x][direction]


def direction_costs(block, bpc):
    px = (np.asarray(block, np.int64) >> (bpc - 8)) - 128
    div = [840, 420, 280, 210, 168, 140, 120]
    cost = []
    for d in range(8):
        n = 15 if d in (0, 4) else 8 if d in (2, 6) else 11
        s = np.zeros(n, np.int64)
        for y, x in itertools.product(range(8), range(8)):
            s[line_index(d, x, y)] += px[y, x]
        if n == 8:
            wgt = [105] * 8
        elif n == 15:
            wgt = [div[k] if k < 7 else 105 if k == 7 else div[14 - k] for k in range(15)]
        else:
            wgt = [div[2 * k + 1] if k < 3 else 105 if k < 8 else div[2 * (10 - k) + 1] for k in range(11)]
        cost.append(int((s * s * np.array(wgt)).sum()))
    return cost


def direction_and_variance(block, bpc):
    cost = direction_costs(block, bpc)
    best = max(cost)
    d = cost.index(best)
    return d, (best - cost[d ^ 4]) >> 10, sum(1 for c in cost if c == best)


def oriented_block(rng, direction, amp, noise, bpc):
    mid = 1 << (bpc - 1)
    y, x = np.mgrid[0:8, 0:8]
    idx = np.vectorize(lambda xx, yy: line_index(direction, int(xx), int(yy)))(x, y)
    b = mid + np.where((idx >> 1) & 1, amp, -amp) + (rng.integers(-noise, noise + 1, size=(8, 8)) if noise else 0)
    return np.clip(b, 0, (1 << bpc) - 1)


AMPLITUDES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 14, 16, 20, 23, 28, 32, 40, 45, 56, 64, 80, 90, 100, 105, 110, 115, 120, 123, 125, 126, 127]


def strength_rows(full, damping_idx):
    """[(bx, by, pri, sec, wanted direction)] of one call: hip the product pri x sec x direction, emu pri x direction with sec rotating"""
    rows = []
    if full:
        for by, bx in itertools.product(range(16), range(32)):
            rows.append((bx, by, bx & 15, SEC[(bx >> 4) | (by >> 3) << 1], by & 7))
    else:
        for by, bx in itertools.product(range(8), range(16)):
            rows.append((bx, by, bx, SEC[(bx + by + damping_idx) & 3], by))
    return rows


@pytest.mark.parametrize("bpc,layout", LAYOUTS_ALL)
def test_every_strength_direction_and_damping(ctx, bpc, layout):
    full = ctx.backend == "hip"
    rng = np.random.default_rng(6100 + bpc + 16 * layout)
    bd8 = bpc - 8
    bw, grid_rows = (32, 16) if full else (16, 8)
    amp_rows = len(AMPLITUDES) // bw
    bh = grid_rows + amp_rows
    w, h = bw * 8, bh * 8
    seen, seen_uv, var_i, var_zero, dirs422, cases = set(), set(), set(), False, set(), []
    for di, damping in enumerate(range(3, 7)):
        planes = noise_planes(rng, w, h, bpc, layout)
        grid = strength_rows(full, di)
        for bx, by, pri, sec, direction in grid:
            amp = [4, 16, 60, 127][(bx + by) & 3] << bd8
            planes[0][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = oriented_block(rng, direction, amp, amp // 4, bpc)
        rows = []
        for bx, by, pri, sec, direction in grid:
            cp = (pri * 4 + SEC.index(sec) + 37) % 64          # the chroma pair: the luma pair rotated
            rows.append(task_row(bx, by, pri, sec, cp >> 2, SEC[cp & 3], picture_edges(bx, by, bw, bh), 0, bd8))
        for k, a in enumerate(AMPLITUDES):          # horizontal stripes of growing amplitude: best - opp from 0 to about 8.8e8
            bx, by = k % bw, grid_rows + k // bw
            blk = np.full((8, 8), 1 << (bpc - 1), np.int64)
            blk[0::2] += a << bd8
            blk[1::2] -= a << bd8
            planes[0][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk
            rows.append(task_row(bx, by, 1 + k % 15, SEC[k & 3], 1 + (k + 7) % 15, SEC[(k + 1) & 3], picture_edges(bx, by, bw, bh), 0, bd8))
        cases.append(prepare(bpc, layout, planes, rows, damping + bd8, rng))
        # ---- what runs, on the oracle's values
        for r, (d, v) in zip(rows, cases[-1].dv):
            y_pri, y_sec, uv_pri, uv_sec = (int(r[k]) >> bd8 for k in (2, 3, 4, 5))
            seen.add((y_pri, y_sec, d if y_pri or uv_pri else None, damping))
            seen_uv.add((uv_pri, uv_sec))
            if y_pri:
                var_zero |= v == 0
                if v:
                    var_i.add(min(int(v >> 6).bit_length() - 1, 12) if v >> 6 else 0)
            if uv_pri:
                dirs422.add(d)
    if full:
        assert {r for r in seen if r[0]} >= set(itertools.product(range(1, 16), SEC, range(8), range(3, 7))), "y_pri x y_sec x oracle direction x damping"
        assert {(p, s, dm) for p, s, d, dm in seen} == set(itertools.product(range(16), SEC, range(3, 7)))
    else:
        assert {(p, s) for p, s, d, dm in seen} == set(itertools.product(range(16), SEC))
        assert {(p, dm) for p, s, d, dm in seen} == set(itertools.product(range(16), range(3, 7)))
        assert {(s, dm) for p, s, d, dm in seen} == set(itertools.product(SEC, range(3, 7)))
        assert {d for p, s, d, dm in seen if p} == set(range(8)) and {d for p, s, d, dm in seen if s and d is not None} == set(range(8))
    if layout != api.LAYOUT_I400:
        assert seen_uv == set(itertools.product(range(16), SEC)), "chroma sees all 64 pairs"
    assert var_zero and var_i == set(range(13)), "var == 0 and every adjust_strength index: %s" % sorted(var_i)
    if layout == api.LAYOUT_I422:
        assert dirs422 == set(range(8)), "every luma direction with uv_pri > 0"
    for c in cases:
        compare(ctx, c)


def tie_blocks(rng, bpc):
    """[(name, 8x8 block)]"""
    mx, mid = (1 << bpc) - 1, 1 << (bpc - 1)
    y, x = np.mgrid[0:8, 0:8]
    out = [("constant", np.full((8, 8), v, np.int64)) for v in (0, mid, mx)]
    for period in (1, 2):
        out.append(("checker", np.where(((x // period) + (y // period)) & 1, mx, 0)))
        out.append(("rows", np.where((y // period) & 1, mx, 0)))
        out.append(("columns", np.where((x // period) & 1, mx, 0)))
    for py, px in itertools.product(range(8), range(8)):
        b = np.zeros((8, 8), np.int64)
        b[py, px] = mx
        out += [("pixel", b), ("hole", mx - b)]
    for k in range(8):
        s = oriented_block(rng, k, (20 + 10 * k) << (bpc - 8), 6 << (bpc - 8), bpc) - mid
        out.append(("transpose-symmetric", np.clip(mid + (s + s.T) // 2, 0, mx)))
        out.append(("mirror-symmetric", np.clip(mid + (s + s[:, ::-1]) // 2, 0, mx)))
        r = rng.integers(0, mx + 1, size=(8, 8))
        out.append(("180-degree-symmetric", (r + r[::-1, ::-1]) // 2))
        out.append(("transpose-symmetric", (r + r.T) // 2))
    return out


@pytest.mark.parametrize("bpc,layout", LAYOUTS_EMU)
def test_direction_ties_and_extremes(ctx, bpc, layout):
    rng = np.random.default_rng(6200 + bpc + 16 * layout)
    bd8 = bpc - 8
    blocks = tie_blocks(rng, bpc)
    bw = 16
    bh = (len(blocks) + bw - 1) // bw
    planes = noise_planes(rng, bw * 8, bh * 8, bpc, layout)
    rows, labels = [], []
    for k, (name, blk) in enumerate(blocks):
        bx, by = k % bw, k // bw
        planes[0][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk
        rows.append(task_row(bx, by, 15, 0, 15, 0, picture_edges(bx, by, bw, bh), 0, bd8))
        labels.append(direction_and_variance(blk, bpc))
    assert {n for n, _ in blocks} == {"constant", "checker", "rows", "columns", "pixel", "hole", "transpose-symmetric", "mirror-symmetric",
                                      "180-degree-symmetric"}
    tied = {d for d, v, n_best in labels if n_best >= 2}
    assert len(tied) >= 4, "best cost shared by two or more directions, winners %s" % sorted(tied)
    case = prepare(bpc, layout, planes, rows, 5 + bd8, rng)
    assert case.dv == [(d, v) for d, v, _ in labels], "the restated costs agree with the oracle's direction and variance on every unit"
    compare(ctx, case)


# "peaks at zero" / "valleys at max": 0 with every third pixel of every third row a step of 2 << bd8 higher, and bitdepth_max with those
# a step lower.  No tap reaches from one such pixel to the next; at (15, 4) the step passes constrain() whole, and the up to 24 / 16 of
# it that the taps sum to overshoots the neighbours even with a tap or two missing (2 - ((2 * 23 - 7) >> 4) < 0): the only contents here
# on which the clamp to the local range (pri and sec both set) decides the output, with pixel 0 resp. bitdepth_max as the bound and the
# missing neighbours' sentinels among the taps.
CONTENTS = ["zero", "max", "checker", "max in zero", "zero in max", "peaks at zero", "valleys at max"]
EXTREME_STRENGTHS = [(15, 4), (1, 1), (15, 0), (0, 4), (0, 1), (1, 0)]


def extreme_window(content, mx, cw, ch):
    """(ch + 4) x (cw + 4): a block with its two-pixel surround"""
    y, x = np.mgrid[0:ch + 4, 0:cw + 4]
    if content == "checker":
        return np.where((x + y) & 1, mx, 0)
    if content in ("peaks at zero", "valleys at max"):
        step = np.where((x % 3 == 0) & (y % 3 == 0), (mx + 1) >> 7, 0)
        return step if content == "peaks at zero" else mx - step
    inside = (x >= 2) & (x < cw + 2) & (y >= 2) & (y < ch + 2)
    block, surround = {"zero": (0, 0), "max": (mx, mx), "max in zero": (mx, 0), "zero in max": (0, mx)}[content]
    return np.where(inside, block, surround)


@pytest.mark.parametrize("layout", [api.LAYOUT_I420, api.LAYOUT_I444])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_extremal_pixels_next_to_missing_neighbours(ctx, bpc, layout):
    rng = np.random.default_rng(6300 + bpc + 16 * layout)
    bd8, mx = bpc - 8, (1 << bpc) - 1
    ss_hor, ss_ver = subsampling(layout)
    product = list(itertools.product(range(16), CONTENTS, EXTREME_STRENGTHS))
    per_row = 32
    bw, bh = 2 * per_row + 1, 2 * ((len(product) + per_row - 1) // per_row) + 1          # units at odd positions: a surround of their own
    ran, cases = set(), []
    for damping in (3, 6):
        planes = noise_planes(rng, bw * 8, bh * 8, bpc, layout)
        rows = []
        for k, (edges, content, (pri, sec)) in enumerate(product):
            bx, by = 1 + 2 * (k % per_row), 1 + 2 * (k // per_row)
            for pl in range(len(planes)):
                cw, ch = (8, 8) if pl == 0 else (8 >> ss_hor, 8 >> ss_ver)
                planes[pl][by * ch - 2:by * ch + ch + 2, bx * cw - 2:bx * cw + cw + 2] = extreme_window(content, mx, cw, ch)
            flags = [0, REP_Y, REP_UV, REP_Y | REP_UV][(k + k // 4) & 3] if edges & BOTTOM else 0
            rows.append(task_row(bx, by, pri, sec, pri, sec, edges, flags, bd8))
            ran.add((edges, content, (pri, sec), damping, flags))
        cases.append(prepare(bpc, layout, planes, rows, damping + bd8, rng))
    assert {r[:4] for r in ran} == {(e, c, s, dm) for e, c, s in product for dm in (3, 6)}
    assert {f for e, c, s, dm, f in ran if e & BOTTOM} == {0, REP_Y, REP_UV, REP_Y | REP_UV} and not any(f for e, c, s, dm, f in ran if not e & BOTTOM)
    for c in cases:
        compare(ctx, c)


# ------------------------------------------------------------------ strips

def strip_templates():
    """{name: [(bx, overrides)]} -- one unit row each; overrides: edges_clear, edges_set_only, y / uv = (pri, sec), flags"""
    t = {}
    for n in (1, 15, 16, 17, 32, 33):
        t["%d listed units" % n] = [(bx, {}) for bx in range(n)]
    t["gap of one"] = [(bx, {}) for bx in range(20) if bx != 7]
    t["gap of several"] = [(bx, {}) for bx in range(24) if not 5 <= bx < 11]
    t["no HAVE_LEFT in mid-row"] = [(bx, {"clear": LEFT} if bx == 9 else {}) for bx in range(3, 22)]
    t["predecessor without HAVE_RIGHT"] = [(bx, {"clear": RIGHT} if bx == 12 else {}) for bx in range(2, 20)]
    t["top and bottom flags change"] = [(bx, {"clear": TOP if 6 <= bx < 11 else BOTTOM if 14 <= bx < 17 else 0}) for bx in range(25)]
    t["no unit filters chroma"] = [(bx, {"uv": (0, 0)}) for bx in range(1, 19)]
    t["one chroma unit among luma-only"] = [(bx, {"uv": (0, 0)} if bx != 10 else {}) for bx in range(1, 19)]
    t["all four strengths 0"] = [(bx, {"y": (0, 0), "uv": (0, 0)} if bx in (4, 5, 17) else {}) for bx in range(20)]
    t["rep flags change"] = [(bx, {"flags": [0, REP_Y, REP_UV, REP_Y | REP_UV, 0][bx // 5]}) for bx in range(25)]
    return t


@pytest.mark.parametrize("bpc,layout", LAYOUTS_EMU)
def test_strip_compositions(ctx, bpc, layout):
    rng = np.random.default_rng(6400 + bpc + 16 * layout)
    bd8 = bpc - 8
    templates = strip_templates()
    bw, bh = 34, len(templates) + 2
    planes = noise_planes(rng, bw * 8, bh * 8, bpc, layout)
    rows, by_name = [], {}
    for by, (name, units) in enumerate(templates.items(), start=1):
        for bx, o in units:
            y = o.get("y", (int(rng.integers(1, 16)), SEC[int(rng.integers(0, 4))]))
            uv = o.get("uv", (int(rng.integers(1, 16)), SEC[int(rng.integers(0, 4))]))
            edges = picture_edges(bx, by, bw, bh) & ~o.get("clear", 0)
            row = task_row(bx, by, y[0], y[1], uv[0], uv[1], edges, o.get("flags", 0), bd8)
            rows.append(row)
            by_name.setdefault(name, []).append(row)
    # ---- every template is there as named
    runs = lambda rs: [len(list(g)) for k, g in itertools.groupby(range(len(rs)), key=lambda i: rs[i][0] - i)]
    for n in (1, 15, 16, 17, 32, 33):
        assert runs(by_name["%d listed units" % n]) == [n]
    assert runs(by_name["gap of one"]) == [7, 12] and runs(by_name["gap of several"]) == [5, 13]
    assert [r[0] for r in by_name["no HAVE_LEFT in mid-row"] if not r[6] & LEFT] == [9]
    assert [r[0] for r in by_name["predecessor without HAVE_RIGHT"] if not r[6] & RIGHT] == [12] and any(r[0] == 13 for r in by_name["predecessor without HAVE_RIGHT"])
    tb = [r[6] & (TOP | BOTTOM) for r in by_name["top and bottom flags change"]]
    assert len({k for k, _ in itertools.groupby(tb)}) == 3 and len(list(itertools.groupby(tb))) == 5
    assert not any(r[4] or r[5] for r in by_name["no unit filters chroma"]) and all(r[2] or r[3] for r in by_name["no unit filters chroma"])
    assert sum(1 for r in by_name["one chroma unit among luma-only"] if r[4] or r[5]) == 1
    assert sum(1 for r in by_name["all four strengths 0"] if not any(r[2:6])) == 3
    assert [k for k, _ in itertools.groupby(r[7] for r in by_name["rep flags change"])] == [0, REP_Y, REP_UV, REP_Y | REP_UV, 0]
    assert len(by_name) == 15
    compare(ctx, prepare(bpc, layout, planes, rows, int(rng.integers(3, 7)) + bd8, rng))
