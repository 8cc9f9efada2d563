"""Intra prediction, ENUMERATED: every mode, angle delta, block shape and edge-availability flag against the oracle.

tests/test_ipred.py draws 16 random tasks per batch from smoothed noise and only asserts that all 14 modes came up.  This module walks
the space (reference: test_ipred.oracle_task = the reference's dav1d_prepare_intra_edges + its intra_pred entries; independent
192 x 192 cells with the block at (64, 64), as test_ipred.gen_batches) and asserts what it ran BEFORE it compares anything:

* test_every_mode_angle_shape_and_flag, on noise (full range, not smoothed), 8 / 10 / 12 bit.
  hip: directional modes 1 .. 8 x angle delta -3 .. 3 x the 19 shapes in 4 .. 64 x all 64 flags values; the five other mode values
  (DC — which the flags turn into DC / DC_TOP / DC_LEFT / DC_128 —, SMOOTH, SMOOTH_V, SMOOTH_H, PAETH) x shape x flags; the filter
  mode x its five filter indices x the 14 shapes up to 32 x flags.  The tile ends w4 / h4 and the visible sizes max_w / max_h step through the
  value sets of gen_batches: every (mode, shape) meets each value of each of the four, each w4 value with and without the top-right
  flag, each h4 value with and without the bottom-left flag, and every mode all 144 combinations.
  emu: every (mode, angle, shape) at least once and every (mode, flags) at least once.
* test_extremal_neighbourhoods: every (mode, angle, shape), all neighbours available, edge filter on, the smooth bit alternating, on
  cells of all 0, all bitdepth_max, 0 / bitdepth_max alternating along the top and left edges with period 1 and with period 2, and a
  single step at the corner (top row and corner bitdepth_max over a left column of 0, and the inverse).  hip and emu alike.

Cost, measured (wall time): the CPU suite (-m "not gpu") took 932 s with the libraries built before the sweep modules (1613 s from a clean tree) and
takes 1016 s with them; this module is 22 s of that (test_mc_sweep.py 61 s, test_ipred_sweep.py 22 s).  On the device neither module nor the -m gpu
total has been timed yet.  An emulator trap ends the pytest process: run this module in a
pytest call of its own first."""
import numpy as np
import pytest

import util
import test_ipred
from test_ipred import CELL
import synth_frames as synth
from dav1d_amd import api

SIZES = [4, 8, 16, 32, 64]
SHAPES = [(w, h) for w in SIZES for h in SIZES if w // 4 <= h <= w * 4]
FILTER_SHAPES = [s for s in SHAPES if max(s) <= 32]
DIRECTIONAL = list(range(1, 9))
OTHER = [0, 9, 10, 11, 12]
FILTER = 13
ANGLES = list(range(-3, 4))
PATTERNS = ["zero", "max", "alternating-1", "alternating-2", "step-top", "step-left"]


def mode_angle_shapes():
    """every legal (mode, angle delta or filter index, shape)"""
    out = [(m, a, s) for m in DIRECTIONAL for a in ANGLES for s in SHAPES]
    out += [(m, 0, s) for m in OTHER for s in SHAPES]
    out += [(FILTER, a, s) for a in range(5) for s in FILTER_SHAPES]
    return out


def tile_and_visible(flags, a, si, m):
    """indices of w4, h4, max_w, max_h in the value sets of test_ipred.gen_batches, stepped by the other parameters of the task (a: index
    of its angle, si: of its shape): the w4 choice runs through its four values on flags bits 0 and 3, so with the top-right bit (2) set
    and clear alike; the h4 choice on bits 1 and 2, so whatever the bottom-left bit (3) is"""
    b = [flags >> k & 1 for k in range(6)]
    wi = (b[0] + 2 * b[3] + b[4] + a + si) % 4
    hi = (b[1] + 2 * b[2] + b[5] + a + m) % 4
    return wi, hi, (flags // 4 + a + si) % 3, (flags + flags // 12 + a // 3 + m) % 3


def make_row(mode, angle, shape, flags):
    a = angle + 3 if mode in DIRECTIONAL else angle
    return (mode, angle, shape[0], shape[1], flags) + tile_and_visible(flags, a, SHAPES.index(shape), mode)


def enumerated_rows(full):
    """[(mode, angle, w, h, flags, w4 choice, h4 choice, max_w choice, max_h choice)]"""
    rows = []
    if full:
        for m, a, s in mode_angle_shapes():
            for fl in range(64):
                rows.append(make_row(m, a, s, fl))
        return rows
    per_mode = {}
    for m, a, s in mode_angle_shapes():
        k = per_mode[m] = per_mode.get(m, -1) + 1
        rows.append(make_row(m, a, s, (k * 27 + 3) % 64 if k < 64 else (k * 5) % 64))
    for m in OTHER:                 # 19 shapes are fewer than 64 flags values: the flags once more, the shape rotating
        for fl in range(64):
            rows.append(make_row(m, 0, SHAPES[(fl + m) % len(SHAPES)], fl))
    return rows


def assert_coverage(rows, full):
    mas = {(m, a, (w, h)) for m, a, w, h, *_ in rows}
    assert mas == set(mode_angle_shapes()), "every (mode, angle, shape)"
    assert {(m, fl) for m, _, _, _, fl, *_ in rows} == {(m, fl) for m in range(14) for fl in range(64)}, "every (mode, flags)"
    if not full:
        return
    assert {r[:5] for r in rows} == {(m, a, w, h, fl) for m, a, (w, h) in mode_angle_shapes() for fl in range(64)} and len(rows) == 64 * len(mas)
    by_mode, by_ms = {}, {}
    for m, a, w, h, fl, wi, hi, mwi, mhi in rows:
        by_mode.setdefault(m, set()).add((wi, hi, mwi, mhi))
        d = by_ms.setdefault((m, w, h), [set(), set(), set(), set()])
        d[0].add((wi, fl >> 2 & 1)); d[1].add((hi, fl >> 3 & 1)); d[2].add(mwi); d[3].add(mhi)
    assert all(len(v) == 144 for v in by_mode.values()), "every mode meets all combinations of w4, h4, max_w, max_h"
    for key, d in by_ms.items():
        assert len(d[0]) == 8 and len(d[1]) == 8 and len(d[2]) == 3 and len(d[3]) == 3, ("every (mode, shape) meets every value", key)


def tasks_of(rows, cells, sp):
    t = np.zeros(len(rows), api.IPRED_TASK)
    for k, ((m, a, w, h, fl, wi, hi, mwi, mhi), (cx, cy)) in enumerate(zip(rows, cells)):
        x, y = cx + 64, cy + 64
        t[k]["dst_off"] = y * sp + x
        t[k]["x4"], t[k]["y4"] = x // 4, y // 4
        t[k]["w4"] = x // 4 + [w // 4, w // 4 + 1, 2 * (w // 4), 40][wi]
        t[k]["h4"] = y // 4 + [h // 4, h // 4 + 1, 2 * (h // 4), 40][hi]
        t[k]["tw"], t[k]["th"], t[k]["mode"], t[k]["angle"], t[k]["flags"] = w // 4, h // 4, m, a, fl
        t[k]["max_w"] = [w, max(4, w // 2), 4 * 40][mwi]
        t[k]["max_h"] = [h, max(4, h // 2), 4 * 40][mhi]
    return t


def run_rows(ctx, oracle, bpc, pic, plane, rows, what):
    """rows in batches of one block per cell, on the picture as `plane` fills it; the picture and the oracle's copy carry on from batch
    to batch (a block only ever writes inside its own cell, and reads outside its own rectangle)"""
    W = pic.w
    cells = [(cx, cy) for cy in range(0, pic.h - CELL + 1, CELL) for cx in range(0, W - CELL + 1, CELL)]
    pic.upload(0, plane)
    want = synth.copy_planes([plane])
    sp = pic.stride_px(0)
    assert want[0].strides[0] == sp * plane.itemsize
    for lo in range(0, len(rows), len(cells)):
        part = rows[lo:lo + len(cells)]
        t = tasks_of(part, cells, sp)
        for k in range(len(t)):
            test_ipred.oracle_task(oracle, bpc, want, t[k], 0, None)
        ctx.ipred_batch(pic, t)
        got = pic.download(0)
        bad = np.argwhere(got != want[0])
        if len(bad):
            yy, xx = bad[0]
            k = (yy // CELL) * (W // CELL) + xx // CELL
            raise AssertionError("%s, %d bpc: (%d,%d) of the cell is %d, the oracle has %d (%d px differ); task (mode, angle, w, h, flags, "
                                 "w4 / h4 / max_w / max_h choice) = %s" % (what, bpc, xx % CELL, yy % CELL, got[yy, xx], want[0][yy, xx], len(bad),
                                                                           part[k] if k < len(part) else None))


def _picture(ctx, bpc, n_rows):
    side = 16 if ctx.backend != "emu" else 8
    pic = ctx.picture(side * CELL, side * CELL, api.LAYOUT_I400, bpc)
    plane = np.zeros((pic.padded_shape(0)[0], pic.stride_px(0)), pic.dtype)[:, :pic.padded_shape(0)[1]]
    return pic, plane


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_mode_angle_shape_and_flag(ctx, bpc):
    oracle = util.default_oracle()
    full = ctx.backend != "emu"
    rows = enumerated_rows(full)
    assert_coverage(rows, full)
    pic, plane = _picture(ctx, bpc, len(rows))
    rng = np.random.default_rng(2500 + bpc)
    plane[:] = rng.integers(0, 1 << bpc, size=plane.shape)
    run_rows(ctx, oracle, bpc, pic, plane, rows, "enumerated")
    pic.free()


def pattern_plane(plane, pattern, bdmax):
    yy, xx = np.mgrid[0:plane.shape[0], 0:plane.shape[1]]
    if pattern == "zero":
        v = np.zeros(plane.shape, bool)
    elif pattern == "max":
        v = np.ones(plane.shape, bool)
    elif pattern == "alternating-1":
        v = ((xx + yy) & 1) == 1
    elif pattern == "alternating-2":
        v = (((xx >> 1) + (yy >> 1)) & 1) == 1
    else:
        top = (yy % CELL) < 64                    # the rows above the block, the corner pixel included
        v = top if pattern == "step-top" else ~top
    plane[:] = np.where(v, bdmax, 0)


def extremal_rows():
    rows = []
    for k, (m, a, s) in enumerate(mode_angle_shapes()):
        rows.append((m, a, s[0], s[1], 15 | 16 | (32 if k & 1 else 0), 3, 3, 2, 2))
    return rows


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_extremal_neighbourhoods(ctx, bpc):
    oracle = util.default_oracle()
    rows = extremal_rows()
    assert {(m, a, (w, h)) for m, a, w, h, *_ in rows} == set(mode_angle_shapes()), "every (mode, angle, shape)"
    assert {(m, fl >> 5) for m, _, _, _, fl, *_ in rows} == {(m, b) for m in range(14) for b in (0, 1)} and all(r[4] & 31 == 31 for r in rows)
    pic, plane = _picture(ctx, bpc, len(rows))
    bdmax = (1 << bpc) - 1
    for pattern in PATTERNS:
        pattern_plane(plane, pattern, bdmax)
        # what the pattern promises about the neighbours of every block: top row y = 63, left column x = 63, corner (63, 63) of a cell
        top, left, corner = plane[63, 64:192], plane[64:192, 63], plane[63, 63]
        if pattern.startswith("alternating"):
            p = int(pattern[-1])
            for e in (top, left):
                assert set(np.unique(e)) == {0, bdmax} and (e[:-p] != e[p:]).all()
        elif pattern.startswith("step"):
            assert (top == corner).all() and (left == bdmax - corner).all() and corner == (bdmax if pattern == "step-top" else 0)
        else:
            assert (top == corner).all() and (left == corner).all() and corner == (bdmax if pattern == "max" else 0)
        run_rows(ctx, oracle, bpc, pic, plane, rows, pattern)
    pic.free()
