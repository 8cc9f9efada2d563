"""Deblocking, ENUMERATED: every comparison of a line at its threshold, and every edge of a transform grid at its legal spacing.

tests/test_loopfilter.py compares a random sample: edges 16 pixels apart on 4:2:0, and whether a comparison sits at, below or above
E, I, H or F is left to the content.  The kernel decides a line by up to 21 comparisons and writes it back in wide pieces whose
safety rests on the minimum distance between edges, so this module constructs both.  What each test ran is collected in a set FIRST
and the set is asserted, so the coverage below is a checked fact (the same on hip and emu):

* test_every_decision_at_its_threshold -- 8 / 10 / 12 bit, 4:2:0, column edges and row edges on separate pictures, limit tables of
  sharpness 0 and 3.  Every 4-line unit carries four constructed lines: for (width, quantity, delta) the compared value is its
  threshold + delta pixel LSB, delta in {-1, 0, +1}, with the line's base near 0, at mid-range and near bitdepth_max and the step in
  both directions.  Widths: luma 4 / 8 / 16, chroma 4 / 6; quantities: the three terms of fm, |p2-p1| |q2-q1| (wd > 4), |p3-p2|
  |q3-q2| (wd > 6), each flat8in term, each flat8out term, both hev terms.  Every level 1 .. 63 occurs; a third of the units have
  L == 0 and take the neighbour's level, some have both 0; tasks hold 32 units and fewer.  Asserted: every (plane type, dir, width,
  quantity, delta); every branch {not filtered, 16-wide flat, 8-wide flat from wd 8, 8-wide flat from wd 16 without flat8out, 6-wide
  flat, hev, normal} per (plane type, dir, bpc, table) where the width admits it.  The branch labels come from a few lines of Python
  restating the specification; they are kept honest by the oracle: a "not filtered" line is unchanged in its output, any other line
  changes (every line carries a step of 2 LSB across the edge) and changes no tap outside the span its branch writes.  Lines built for it drive the narrow filters into both pixel clips: among the
  written taps of the hev and of the normal lines the oracle's output holds both 0 and bitdepth_max (asserted on the oracle alone).
* test_edges_at_their_legal_spacing -- all four layouts at 8 and 10 bit, 4:2:0 also at 12 bit; luma 200 x 136 (34 units down a column:
  tasks of 32 + 2).  Every plane is cut into a random grid of legal transform rectangles 4 .. 64 and EVERY interior edge is listed with
  the width the smaller transform across it gives (luma 4 / 8 / >= 16, chroma 4 / >= 8), levels per transform block with a share of
  zero blocks, content test_loopfilter.structured_plane, oracle order all column edges then all row edges, the kernel's list
  permuted.  Asserted: each luma width is at least 15 % of the luma edge units; pairs of 4-wide edges 4 apart, of 8-wide (luma) and
  6-wide (chroma) edges 8 apart and of 16-wide edges 16 apart exist in both directions; more than 1000 pixels change.

Cost: DESIGN.md 11."""
import ctypes as C
import itertools

import numpy as np
import pytest

import util
import synth_frames as synth
from test_loopfilter import make_lut, LutStruct, structured_plane
from dav1d_amd import api

B4_STRIDE, B4_ROWS = 96, 80
COMP = {0: (0, 1), 1: (2, 2), 2: (3, 3)}          # level component per plane and direction (Av1Filter level layout)

# ------------------------------------------------------------------ the specification, restated for labels only

SPAN = {"not filtered": (0, 0), "flat16": (-6, 6), "flat8 from wd 8": (-3, 3), "flat8 from wd 16": (-3, 3), "flat6": (-2, 2), "hev": (-1, 1),
        "normal": (-2, 2)}          # taps [lo, hi) a branch writes; tap 0 is the first pixel of the q side


def branch(t, wd, E, I, H, F):
    """t[k + 7] = tap k, k = -7 .. 6.  AV1 spec 7.14.6 / loop_filter() of the reference."""
    p = lambda i: int(t[6 - i])
    q = lambda i: int(t[7 + i])
    fm = abs(p(1) - p(0)) <= I and abs(q(1) - q(0)) <= I and abs(p(0) - q(0)) * 2 + (abs(p(1) - q(1)) >> 1) <= E
    if wd > 4:
        fm = fm and abs(p(2) - p(1)) <= I and abs(q(2) - q(1)) <= I
    if wd > 6:
        fm = fm and abs(p(3) - p(2)) <= I and abs(q(3) - q(2)) <= I
    if not fm:
        return "not filtered"
    flat_in = wd >= 6 and all(abs(p(i) - p(0)) <= F and abs(q(i) - q(0)) <= F for i in range(1, 3 if wd == 6 else 4))
    flat_out = wd >= 16 and all(abs(p(i) - p(0)) <= F and abs(q(i) - q(0)) <= F for i in (4, 5, 6))
    if flat_in and flat_out:
        return "flat16"
    if flat_in:
        return "flat6" if wd == 6 else "flat8 from wd %d" % wd
    return "hev" if abs(p(1) - p(0)) > H or abs(q(1) - q(0)) > H else "normal"


ADMITTED = {4: {"not filtered", "hev", "normal"}, 6: {"not filtered", "flat6", "hev", "normal"},
            8: {"not filtered", "flat8 from wd 8", "hev", "normal"},
            16: {"not filtered", "flat16", "flat8 from wd 16", "hev", "normal"}}

# ------------------------------------------------------------------ constructed lines

FM = ["fm_p1p0", "fm_q1q0", "fm_E"]
QUANTITIES = {4: FM + ["hev_p", "hev_q"],
              6: FM + ["p2p1", "q2q1", "in_p1", "in_p2", "in_q1", "in_q2", "hev_p", "hev_q"]}
QUANTITIES[8] = QUANTITIES[6] + ["p3p2", "q3q2", "in_p3", "in_q3"]
QUANTITIES[16] = QUANTITIES[8] + ["out_p4", "out_p5", "out_p6", "out_q4", "out_q5", "out_q6"]
assert [len(QUANTITIES[w]) for w in (4, 6, 8, 16)] == [5, 11, 15, 21]
WIDTHS = {0: (4, 8, 16), 1: (4, 6)}


def level_class(quantity):
    """fm terms: any level.  flat terms: I >= 2 F, so that a tap F + 1 away passes fm.  hev terms: L >= 16 (H >= F) and I >= 4 F."""
    return "any" if quantity in FM or quantity[1:] in ("2p1", "2q1", "3p2", "3q2") else "hev" if quantity.startswith("hev") else "flat"


def line_offsets(wd, quantity, delta, sg, E, I, H, F):
    """taps relative to the line's base, [p6 .. p0, q0 .. q6]; the compared quantity is threshold + delta, every other comparison of
    fm stays inside its limit"""
    p, q = [0] * 7, [0] * 7
    side = q if "q" in quantity.split("_")[-1][:1] or quantity in ("fm_q1q0", "q2q1", "q3q2") else p
    other = p if side is q else q
    if quantity in ("fm_p1p0", "fm_q1q0", "p2p1", "q2q1", "p3p2", "q3q2"):
        first = {"fm": 1, "p2": 2, "q2": 2, "p3": 3, "q3": 3}[quantity[:2]]
        for i in range(first, 7):
            side[i] = sg * (I + delta)
    elif quantity == "fm_E":
        # |p0 - q0| * 2 + (|p1 - q1| >> 1) == E + delta with |p1 - p0|, |q1 - q0| as small as the target allows
        # (p1 and q1 move apart for s > 0 and the same way for s < 0: |p1 - q1| = |d + s|, each by at most min(I, 2))
        sol = [(abs(s), s, d) for s in range(-2 * min(I, 2), 2 * min(I, 2) + 1) for d in range(E + 2) if 2 * d + (abs(d + s) >> 1) == E + delta]
        _, s, d = min(sol)
        a, a2 = s // 2, s - s // 2
        for i in range(7):
            q[i] = sg * (d + (a2 if i else 0))
            p[i] = -sg * a if i else 0
    elif quantity.startswith("in_") or quantity.startswith("out_"):
        side[int(quantity[-1])] = sg * (F + delta)
    elif quantity.startswith("hev_"):
        for i in range(1, 7):
            side[i] = sg * (H + delta)
        if wd >= 6:          # not flat, whatever H + delta is: the hev comparison is reached
            for i in range(2, 7):
                other[i] = sg * 3 * F
    elif quantity == "sat_hev_hi":          # base bitdepth_max: p0 + f2 leaves the pixel range
        p[0] = -1
        q[1:] = [-I] * 6
    elif quantity == "sat_hev_lo":          # base 0: q0 - f1 leaves it at the other end
        q[0] = 1
        p[1:] = [I] * 6
    elif quantity == "sat_norm_hi":         # |p1 - p0| = 2 F <= H, > F: p1 + f leaves the range
        p[0] = -2 * F
    elif quantity == "sat_norm_lo":
        q[0] = 2 * F
    else:
        raise KeyError(quantity)
    if quantity != "fm_E" and quantity[:3] != "sat":
        # a step of two pixel LSB across the edge (every compared quantity but the third term of fm lies within one side): whichever
        # branch filters the line changes it, so a line that is wrongly left alone, or wrongly filtered, shows.  Its sign is the one
        # with which p1 - q1 and q0 - p0 do not cancel in the narrow filter.
        q = [v + (2 * sg if side is p else -2 * sg) for v in q]
    return np.array(p[::-1] + q, np.int64)


def threshold_units(ptype):
    """[(wd, level class, [(quantity, delta, sign, base class)] * 4)]: 18 lines per (width, quantity) = delta x base x sign, padded to 20"""
    units = []
    for wd in WIDTHS[ptype]:
        for quantity in QUANTITIES[wd]:
            lines = [(quantity, dl, sg, b) for dl, b, sg in itertools.product((-1, 0, 1), ("lo", "mid", "hi"), (1, -1))]
            lines += lines[7:9]
            units += [(wd, level_class(quantity), lines[k:k + 4]) for k in range(0, 20, 4)]
        units.append((wd, "sat_hev", [("sat_hev_hi", 0, 1, "hi"), ("sat_hev_lo", 0, 1, "lo")] * 2))
        units.append((wd, "sat_norm", [("sat_norm_hi", 0, 1, "hi"), ("sat_norm_lo", 0, 1, "lo")] * 2))
    units += [(WIDTHS[ptype][-1], "zero", [("sat_norm_hi", 0, 1, "hi"), ("sat_norm_lo", 0, 1, "lo")] * 2)] * 2
    return units


ALONG, ACROSS = 160, 256          # luma: 40 units along an edge (tasks of 32 + 8), edges every 16 pixels


def build_threshold_case(bpc, d, sharp, rng):
    bd8, mx = bpc - 8, (1 << bpc) - 1
    F = 1 << bd8
    lut_e, lut_i = make_lut(sharp)
    levels = {"any": list(range(1, 64)), "flat": [L for L in range(1, 64) if lut_i[L] >= 2],
              "hev": [L for L in range(16, 64) if lut_i[L] >= 4], "sat_hev": [12], "sat_norm": [40], "zero": [0]}
    counters = dict.fromkeys(levels, 0)
    w, h = (ACROSS, ALONG) if d == 0 else (ALONG, ACROSS)
    planes = synth.make_planes(rng, w, h, bpc, smooth=False)
    lvl = rng.integers(1, 64, size=(B4_ROWS, B4_STRIDE, 4)).astype(np.uint8)
    records, masks = [], {}
    n = 0
    for pl in range(3):
        ptype = min(pl, 1)
        along = (ALONG >> ptype) // 4
        slot = 0
        for wd, cls, lines in threshold_units(ptype)[(pl == 2)::(2 if pl else 1)]:          # chroma units alternate between U and V
            e, u = divmod(slot, along)
            slot += 1
            c, a = 16 * (e + 1), 4 * u
            assert c + 16 <= (ACROSS >> ptype)
            L = levels[cls][counters[cls] % len(levels[cls])]
            counters[cls] += 1
            comp = COMP[pl][d]
            at = (lambda a4, c4: (a4, c4, comp)) if d == 0 else (lambda a4, c4: (c4, a4, comp))
            mode = n % 3
            n += 1
            if mode == 1 or not L:
                lvl[at(a // 4, c // 4)], lvl[at(a // 4, c // 4 - 1)] = 0, L          # the neighbour's level
            else:
                lvl[at(a // 4, c // 4)] = L
                if mode == 2:
                    lvl[at(a // 4, c // 4 - 1)] = 0
            E, I, H = int(lut_e[L]) << bd8, int(lut_i[L]) << bd8, (L >> 4) << bd8
            for i, (quantity, delta, sg, base) in enumerate(lines):
                o = line_offsets(wd, quantity, delta, sg, E, I, H, F)
                taps = o + (-o.min() if base == "lo" else mx - o.max() if base == "hi" else 1 << (bpc - 1))
                assert taps.min() >= 0 and taps.max() <= mx
                if d == 0:
                    planes[pl][a + i, c - 7:c + 7] = taps
                else:
                    planes[pl][c - 7:c + 7, a + i] = taps
                label = branch(taps, wd, E, I, H, F) if L else "not filtered"
                records.append((pl, a + i, c, wd, quantity, delta, label, L))
            idx = {4: 0, 8: 1, 6: 1, 16: 2}[wd]
            masks.setdefault((pl, c, u // 32), [0, 0, 0])[idx] |= 1 << (u % 32)
    tasks = []
    for (pl, c, seg), vm in sorted(masks.items()):
        sp = planes[pl].strides[0] // planes[pl].itemsize
        x, y = (c, seg * 128) if d == 0 else (seg * 128, c)
        tasks.append((y * sp + x, (y // 4) * B4_STRIDE + x // 4, vm, pl, d, COMP[pl][d], 0))
    t = np.zeros(len(tasks), api.LF_TASK)
    for k, v in enumerate(tasks):
        t[k] = v
    return planes, lvl, t, records, (lut_e, lut_i)


def oracle_lf(oracle, bpc, want, t, lvl, lut_e, lut_i):
    """every column-edge call, then every row-edge call, in place on host copies"""
    lut = LutStruct()
    lut.e[:] = list(lut_e)
    lut.i[:] = list(lut_i)
    bps = want[0].itemsize
    for d in (0, 1):
        for k in range(len(t)):
            if t[k]["dir"] != d:
                continue
            pl = int(t[k]["plane"])
            vm = (C.c_uint32 * 4)(*[int(v) for v in t[k]["vmask"]], 0)
            lp = lvl.ctypes.data + int(t[k]["lvl_off"]) * 4 + int(t[k]["lvl_comp"])
            oracle.call(bpc, "loop_filter_sb", 1 if pl else 0, d, want[pl].ctypes.data + int(t[k]["dst_off"]) * bps,
                        want[pl].strides[0], vm, lp, B4_STRIDE, C.byref(lut), 32)


def run_and_compare(ctx, pic, planes, want, t, lvl, lut_e, lut_i, rng):
    for pl in range(len(planes)):
        pic.upload(pl, planes[pl])
    dlvl = ctx.buffer_from(lvl)
    try:
        ctx.lf_batch(pic, t[rng.permutation(len(t))], dlvl, B4_STRIDE, lut_e, lut_i)
        for pl in range(len(planes)):
            got = pic.download(pl)
            bad = np.argwhere(got != want[pl])
            assert not len(bad), "plane %d differs at (y, x) %s: got %d want %d (%d px)" % (pl, bad[0], got[tuple(bad[0])], want[pl][tuple(bad[0])], len(bad))
    finally:
        dlvl.free()


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_decision_at_its_threshold(ctx, bpc):
    oracle = util.default_oracle()
    rng = np.random.default_rng(5100 + bpc)
    mx = (1 << bpc) - 1
    cases = [(d, sharp) + build_threshold_case(bpc, d, sharp, rng) for d in (0, 1) for sharp in (0, 3)]
    # ---- coverage, before anything is compared
    built = {(min(pl, 1), d, wd, qn, dl) for d, sharp, _, _, _, recs, _ in cases for pl, a, c, wd, qn, dl, label, L in recs if qn[:3] != "sat"}
    assert built == {(pt, d, wd, qn, dl) for pt in (0, 1) for d in (0, 1) for wd in WIDTHS[pt] for qn in QUANTITIES[wd] for dl in (-1, 0, 1)}
    for d, sharp, planes, lvl, t, recs, lut in cases:
        for pt in (0, 1):
            labels = {(wd, label) for pl, a, c, wd, qn, dl, label, L in recs if min(pl, 1) == pt}
            assert labels == {(wd, lb) for wd in WIDTHS[pt] for lb in ADMITTED[wd]}, (d, sharp, pt, sorted(labels))
        assert {L for *_, L in recs} == set(range(64)), "every level, and units whose level and neighbour's level are 0"
        assert {pl for pl, *_ in recs} == {0, 1, 2}
        n_units = {bin(int(v)).count("1") for k in range(len(t)) for v in [np.bitwise_or.reduce(t[k]["vmask"])]}
        assert 32 in n_units and min(n_units) < 32
        own_zero = sum(1 for k in range(len(t)) for u in range(32) if np.bitwise_or.reduce(t[k]["vmask"]) >> u & 1
                       and lvl.reshape(-1, 4)[int(t[k]["lvl_off"]) + u * (1 if d else B4_STRIDE), int(t[k]["lvl_comp"])] == 0)
        assert own_zero >= len(recs) // 4 // 4, "units that take the neighbour's level"
    for d, sharp, planes, lvl, t, recs, (lut_e, lut_i) in cases:
        want = synth.copy_planes(planes)
        oracle_lf(oracle, bpc, want, t, lvl, lut_e, lut_i)
        # ---- the labels are the oracle's: no tap changes outside the span of the branch
        written = {}
        for pl, a, c, wd, qn, dl, label, L in recs:
            win = (lambda p: p[a, c - 7:c + 7]) if d == 0 else (lambda p: p[c - 7:c + 7, a])
            changed = np.flatnonzero(win(want[pl]).astype(np.int64) != win(planes[pl]))
            lo, hi = SPAN[label]
            assert all(lo <= k - 7 < hi for k in changed), (d, sharp, pl, a, c, wd, qn, dl, label, changed - 7)
            assert len(changed) or label == "not filtered" or not L, ("a filtered line changes", d, sharp, pl, a, c, wd, qn, dl, label)
            if label in ("hev", "normal"):
                written.setdefault((min(pl, 1), label), set()).update(win(want[pl])[7 + lo:7 + hi].tolist())
        if sharp == 0:
            for key in itertools.product((0, 1), ("hev", "normal")):
                assert {0, mx} <= written[key], "both pixel clips among the oracle's %s lines, plane type %d" % key[::-1]
        w, h = (ACROSS, ALONG) if d == 0 else (ALONG, ACROSS)
        pic = ctx.picture(w, h, api.LAYOUT_I420, bpc)
        try:
            run_and_compare(ctx, pic, planes, want, t, lvl, lut_e, lut_i, rng)
        finally:
            pic.free()


# ------------------------------------------------------------------ transform grids

def pow2_segments(n):
    out, x = [], 0
    while x < n:
        s = 64
        while s > n - x:
            s >>= 1
        out.append((x, s))
        x += s
    return out


def split_rect(rng, x, y, w, h, out):
    legal = max(w, h) <= 4 * min(w, h)
    stop = {64: 0.15, 32: 0.3, 16: 0.45, 8: 0.45, 4: 1.0}[max(w, h)]          # about a third of the luma edge units per filter width
    if legal and rng.random() < stop:
        out.append((x, y, w, h))
        return
    if w > h or (w == h and rng.random() < 0.5) or h == 4:
        if w == 4:
            out.append((x, y, w, h))
            return
        split_rect(rng, x, y, w // 2, h, out)
        split_rect(rng, x + w // 2, y, w // 2, h, out)
    else:
        split_rect(rng, x, y, w, h // 2, out)
        split_rect(rng, x, y + h // 2, w, h // 2, out)


def transform_grid(rng, pw, ph):
    """a plane cut into legal transform rectangles (4 .. 64, aspect up to 4): [(x, y, w, h)]"""
    out = []
    for (x, w), (y, h) in itertools.product(pow2_segments(pw), pow2_segments(ph)):
        split_rect(rng, x, y, w, h, out)
    assert all(max(w, h) <= 4 * min(w, h) and w in (4, 8, 16, 32, 64) and h in (4, 8, 16, 32, 64) for _, _, w, h in out)
    return out


def grid_edges(rects, pw, ph):
    """{(dir, position, unit along the edge): smaller transform size across the edge} for every interior edge unit"""
    ident = np.zeros((ph // 4, pw // 4), np.int64)
    size = np.zeros((2, ph // 4, pw // 4), np.int64)
    for k, (x, y, w, h) in enumerate(rects):
        ident[y // 4:(y + h) // 4, x // 4:(x + w) // 4] = k
        size[0, y // 4:(y + h) // 4, x // 4:(x + w) // 4] = w
        size[1, y // 4:(y + h) // 4, x // 4:(x + w) // 4] = h
    edges = {}
    for y4, x4 in itertools.product(range(ph // 4), range(pw // 4)):
        if x4 and ident[y4, x4] != ident[y4, x4 - 1]:
            edges[(0, x4, y4)] = int(min(size[0, y4, x4], size[0, y4, x4 - 1]))
        if y4 and ident[y4, x4] != ident[y4 - 1, x4]:
            edges[(1, y4, x4)] = int(min(size[1, y4, x4], size[1, y4 - 1, x4]))
    return edges, ident


def filter_width(pl, tx):
    return min(tx, 16) if pl == 0 else 4 if tx == 4 else 6


@pytest.mark.parametrize("bpc,layout", [(8, api.LAYOUT_I400), (8, api.LAYOUT_I420), (8, api.LAYOUT_I422), (8, api.LAYOUT_I444),
                                        (10, api.LAYOUT_I400), (10, api.LAYOUT_I420), (10, api.LAYOUT_I422), (10, api.LAYOUT_I444),
                                        (12, api.LAYOUT_I420)])
def test_edges_at_their_legal_spacing(ctx, bpc, layout):
    oracle = util.default_oracle()
    rng = np.random.default_rng(5200 + bpc + 16 * layout)
    w, h = 200, 136
    planes = synth.make_planes(rng, w, h, bpc, smooth=False, layout=layout)
    ss_hor, ss_ver = int(layout in (api.LAYOUT_I420, api.LAYOUT_I422)), int(layout == api.LAYOUT_I420)
    lvl = np.zeros((B4_ROWS, B4_STRIDE, 4), np.uint8)
    e, i = make_lut(int(rng.integers(0, 8)))
    tasks, widths = [], {}
    for pl in range(len(planes)):
        pw, ph = (w, h) if pl == 0 else (w >> ss_hor, h >> ss_ver)
        planes[pl][:, :] = structured_plane(rng, planes[pl].shape, bpc)
        rects = transform_grid(rng, pw, ph)
        edges, ident = grid_edges(rects, pw, ph)
        for comp in set(COMP[pl]):
            per_block = rng.integers(1, 64, size=len(rects))
            per_block[rng.random(len(rects)) < 0.15] = 0
            lvl[:ph // 4, :pw // 4, comp] = per_block[ident]
        sp = planes[pl].strides[0] // planes[pl].itemsize
        masks = {}
        for (d, pos, u), tx in edges.items():
            wd = filter_width(pl, tx)
            widths[(pl, d, pos, u)] = wd
            masks.setdefault((d, pos, u // 32), [0, 0, 0])[{4: 0, 8: 1, 6: 1, 16: 2}[wd]] |= 1 << (u % 32)
        for (d, pos, seg), vm in masks.items():
            x, y = (pos * 4, seg * 128) if d == 0 else (seg * 128, pos * 4)
            tasks.append((y * sp + x, (y // 4) * B4_STRIDE + x // 4, vm, pl, d, COMP[pl][d], 0))
    t = np.zeros(len(tasks), api.LF_TASK)
    for k, v in enumerate(tasks):
        t[k] = v
    # ---- coverage
    luma = [wd for (pl, d, pos, u), wd in widths.items() if pl == 0]
    for wd in (4, 8, 16):
        assert luma.count(wd) >= 0.15 * len(luma), "luma width %d: %d of %d edge units" % (wd, luma.count(wd), len(luma))
    pairs = {(min(pl, 1), d, wd) for (pl, d, pos, u), wd in widths.items()
             if widths.get((pl, d, pos + {4: 1, 8: 2, 6: 2, 16: 4}[wd], u)) == wd}
    want_pairs = {(0, d, wd) for d in (0, 1) for wd in (4, 8, 16)} | ({(1, d, wd) for d in (0, 1) for wd in (4, 6)} if layout else set())
    assert pairs == want_pairs, sorted(want_pairs - pairs)
    n_units = {bin(int(np.bitwise_or.reduce(t[k]["vmask"]))).count("1") for k in range(len(t)) if t[k]["plane"] == 0 and t[k]["dir"] == 0}
    assert 32 in n_units and {1, 2} & n_units, "34 units down a luma column: tasks of 32 + 2"
    want = synth.copy_planes(planes)
    oracle_lf(oracle, bpc, want, t, lvl, e, i)
    assert sum(int((want[pl] != planes[pl]).sum()) for pl in range(len(planes))) > 1000, "the case must actually filter something"
    pic = ctx.picture(w, h, layout, bpc)
    try:
        run_and_compare(ctx, pic, planes, want, t, lvl, e, i, rng)
    finally:
        pic.free()
