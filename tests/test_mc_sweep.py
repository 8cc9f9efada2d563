"""Motion compensation, ENUMERATED: every filter, every sub-pel phase and every block shape against the oracle.

tests/test_mc.py and tests/test_frame.py compare random samples; the kernels pick their code path from a small discrete space
(10 filter_2d x 16 mx x 16 my x 29 shapes x put / prep: packed v_dot2 tap pairs per (set, phase), the 4-tap sets for w <= 4 and
h <= 4, a span table per filter, the 8-row window of 4-row tiles), so this module walks that space instead of drawing from it.  What
each test ran is collected in a set FIRST and the set is asserted, so the coverage below is a checked fact:

* test_every_filter_phase_and_shape — ctx.mc_batch, put and prep, 8 / 10 / 12 bit, raster and tiled references, against
  test_mc._oracle_mc.  hip: the full product filter_2d x mx x my x shape.  emu: every (filter_2d, mx, my) at least once with the shape
  rotating through the shape list, and every (shape, filter_2d) at the phase classes (0,0), (mx,0), (0,my), (mx,my).  In both, a fixed
  5/16 of the tasks leave the picture (left, right, top, bottom, a corner), and every filter meets every side.
* test_extremal_reference_content — every (filter_2d, mx, my) on patches of all 0, all bitdepth_max and the two windows that drive
  output pixel (0, 0) to its largest and smallest sum (bitdepth_max exactly where the product of the horizontal and the vertical
  tap is positive / negative).  The tap signs are read off the ORACLE's response to a unit impulse, never off a table of the code
  under test.  Shapes 4x4, 8x8, 16x16, 32x8.  hip: the full product with the four patterns.  emu: every (filter_2d, mx, my) with both
  worst-case windows (shape rotating), and every (shape, filter_2d, pattern) at the four phase classes.  The oracle's put outputs of
  the worst-case windows must contain both 0 and bitdepth_max (asserted on the oracle alone).
* test_recon_lists_over_every_filter_and_phase — the production path: ctx.recon_list over square 4x4 .. 64x64 luma blocks of a 4:2:0
  picture with their chroma blocks and a residual each, against test_frame.oracle_frame; raster / tiled / tiled-native references,
  recon_fuse at its default and at 0.  Single-reference blocks take every (filter_2d, mx, my) (odd luma phases included), avg
  compounds every filter_2d with independent phases of their two references.  hip: the full product per luma block size; emu: every
  triple at least once over the blocks of the frame.  Which launch took the blocks is read from the counts of
  dav1d_hip_recon_list_run_timed: with the default mask every block of 4x4 .. 32x32 is in a paired launch, with recon_fuse = 0 none is.

Cost, measured (wall time): the CPU suite (-m "not gpu") took 932 s with the libraries built before the sweep modules (1613 s from a clean tree) and
takes 1016 s with them; this module is 61 s of that (test_mc_sweep.py 61 s, test_ipred_sweep.py 22 s).  On the device neither module nor the -m gpu
total has been timed yet.  An emulator trap ends the pytest process: run this module in a
pytest call of its own first."""
import ctypes as C
import itertools

import numpy as np
import pytest

import util
import test_mc
import test_frame
import synth_frames as synth
from dav1d_amd import api

SIZES = [2, 4, 8, 16, 32, 64, 128]
N_TRIPLES = 10 * 16 * 16
PHASE_CLASSES = [(0, 0), (1, 0), (0, 1), (1, 1)]          # (mx != 0, my != 0)
SIDES = ["left", "right", "top", "bottom", "corner"]


def legal_shapes(kind):
    """w, h in 2 .. 128, h within w / 4 .. 4 w; prep from w = 4 (reference tests/checkasm/mc.c:58-122)"""
    return [(w, h) for w in SIZES for h in SIZES if max(w // 4, 2) <= h <= min(4 * w, 128) and (kind == 0 or w >= 4)]


def position_class(f, mx, my, s):
    """0 .. 4: the window leaves the picture at SIDES[class]; 5 .. 15: interior.  As mx (or my) runs through its 16 values with the
    rest fixed, all 16 classes come up: every (filter, shape, my) meets every side."""
    return (13 * my + s + 5 * mx + 3 * f) % 16


def source_position(cls, k, w, h, vis_w, vis_h):
    """k: a running number that varies the choice inside a class"""
    ix = 4 + (k * 37) % (vis_w - w - 8)
    iy = 4 + (k * 53) % (vis_h - h - 8)
    left, right = [-w - 5, -3, -1, 1], [vis_w - w + 1, vis_w - 2, vis_w + 9, vis_w - w - 2]
    top, bottom = [-h - 5, -2, -1, 2], [vis_h - h + 2, vis_h - 1, vis_h + 20, vis_h - h - 1]
    if cls == 0:
        return left[k % 4], iy
    if cls == 1:
        return right[k % 4], iy
    if cls == 2:
        return ix, top[k % 4]
    if cls == 3:
        return ix, bottom[k % 4]
    if cls == 4:
        return (left, right)[k & 1][(k >> 2) % 4], (top, bottom)[(k >> 1) & 1][(k >> 3) % 4]
    return ix, iy


def enumerated_rows(kind, full, vis_w, vis_h):
    """[(filter_2d, mx, my, w, h, src_x, src_y, side or None)]"""
    shapes = legal_shapes(kind)
    picks = []
    if full:
        for f, mx, my in itertools.product(range(10), range(16), range(16)):
            picks += [(f, mx, my, s) for s in range(len(shapes))]
    else:
        for k, (f, mx, my) in enumerate(itertools.product(range(10), range(16), range(16))):
            picks.append((f, mx, my, (k + k // len(shapes)) % len(shapes)))
        for s in range(len(shapes)):
            for f in range(10):
                a, b = 1 + (3 * s + f) % 15, 1 + (5 * s + 7 * f) % 15          # the non-zero phases rotate too
                picks += [(f, a * cx, b * cy, s) for cx, cy in PHASE_CLASSES]
    rows = []
    for k, (f, mx, my, s) in enumerate(picks):
        w, h = shapes[s]
        cls = position_class(f, mx, my, s)
        sx, sy = source_position(cls, k, w, h, vis_w, vis_h)
        rows.append((f, mx, my, w, h, sx, sy, SIDES[cls] if cls < 5 else None))
    return rows


def assert_coverage(rows, kind, full):
    shapes = legal_shapes(kind)
    ran = {(f, mx, my, w, h, kind) for f, mx, my, w, h, _, _, _ in rows}
    if full:
        want = {(f, mx, my, w, h, kind) for f in range(10) for mx in range(16) for my in range(16) for w, h in shapes}
        assert ran == want, "%d of %d (filter, mx, my, shape) combinations" % (len(ran & want), len(want))
    else:
        triples = {(f, mx, my) for f, mx, my, _, _, _ in ran}
        assert len(triples) == N_TRIPLES, "every (filter_2d, mx, my)"
        by_triple_shape = {}
        for f, mx, my, w, h, _ in ran:
            by_triple_shape.setdefault((w, h), set()).add((f, mx, my))
        assert all(len(by_triple_shape.get(s, ())) >= 0.9 * N_TRIPLES / len(shapes) for s in shapes), "the shape rotates through the list"
        classes = {(w, h, f, mx != 0, my != 0) for f, mx, my, w, h, _ in ran}
        assert classes == {(w, h, f, bool(cx), bool(cy)) for w, h in shapes for f in range(10) for cx, cy in PHASE_CLASSES}, \
            "every (shape, filter_2d) at the four phase classes"
    # edge emulation: every filter leaves the picture on every side with the filter of that direction switched on
    met = {(f, side) for f, mx, my, _, _, _, _, side in rows if side and (mx if side in ("left", "right") else my if side in ("top", "bottom") else mx and my)}
    assert met == {(f, side) for f in range(10) for side in SIDES}
    n_edge = sum(1 for r in rows if r[7])
    assert 0.2 < n_edge / len(rows) < 0.45, "most tasks are interior, a fixed share is not"


def pack_batches(rows, DW, DH):
    """Put destinations packed on shelves of a DW x DH plane (rows sorted by shape so that a shelf holds one height); a new batch
    when the plane is full.  Returns [[(row, x, y, prep_off)]]."""
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][4], -rows[i][3]))
    batches, cur = [], []
    x = y = shelf = off = 0
    for i in order:
        w, h = rows[i][3], rows[i][4]
        if x + w > DW:
            x, y, shelf = 0, y + shelf, 0
        if y + h > DH:
            batches.append(cur)
            cur, x, y, shelf, off = [], 0, 0, 0, 0
        cur.append((rows[i], x, y, off))
        x += w
        off += w * h
        shelf = max(shelf, h)
    if cur:
        batches.append(cur)
    return batches


def run_and_compare(ctx, oracle, bpc, kind, rows, refplane, vis_w, vis_h, DW, DH, what):
    """rows through ctx.mc_batch, once with the reference read in raster order and once through its tiled twin; every task against
    test_mc._oracle_mc.  Returns the oracle's put blocks when kind == 0 (as (row, block) pairs)."""
    pd = util.pix_dtype(bpc)
    refs = {}
    for name in ("raster", "tiled"):
        r = ctx.picture(vis_w, vis_h, api.LAYOUT_I400, bpc)
        r.upload(0, refplane)
        if name == "tiled":
            r.retile()
            assert r.pic.twin_ok and r.pic.twin[0]
        refs[name] = r
    rng = np.random.default_rng(bpc + kind)
    dsts = {name: ctx.picture(DW, DH, api.LAYOUT_I400, bpc) for name in refs}
    dplane = rng.integers(0, 1 << bpc, size=dsts["raster"].padded_shape(0)).astype(pd)
    for d in dsts.values():
        d.upload(0, dplane)
    sp = dsts["raster"].stride_px(0)
    want_plane = dplane.copy()
    out = []
    for batch in pack_batches(rows, DW, DH):
        n = len(batch)
        t = np.zeros(n, api.MC_TASK)
        prep_sz = batch[-1][3] + batch[-1][0][3] * batch[-1][0][4]
        want_prep = np.zeros(prep_sz, np.int16)
        for i, ((f, mx, my, w, h, sx, sy, _), x, y, off) in enumerate(batch):
            t[i]["src_x"], t[i]["src_y"], t[i]["w"], t[i]["h"] = sx, sy, w, h
            t[i]["mx"], t[i]["my"], t[i]["filter_2d"], t[i]["kind"] = mx, my, f, kind
            if kind == 0:
                t[i]["dst_off"] = y * sp + x
                test_mc._oracle_mc(oracle, bpc, refplane, vis_w, vis_h, t[i], dst_block=want_plane[y:, x:])
            else:
                t[i]["dst_off"] = off
                test_mc._oracle_mc(oracle, bpc, refplane, vis_w, vis_h, t[i], tmp=want_prep[off:])
        if kind == 0:
            out += [(b[0], want_plane[b[2]:b[2] + b[0][4], b[1]:b[1] + b[0][3]].copy()) for b in batch]
        bx, by = np.array([b[1] for b in batch]), np.array([b[2] for b in batch])
        offs = np.array([b[3] for b in batch])
        for name, ref in refs.items():
            prep = ctx.buffer(max(prep_sz, 8) * 2)
            prep.zero()
            ctx.mc_batch(dsts[name], [ref], t, prep)
            got_plane = dsts[name].download(0)
            if kind == 0:
                bad = np.argwhere(got_plane != want_plane)
                if len(bad):
                    yy, xx = bad[0]
                    hit = np.flatnonzero((bx <= xx) & (xx < bx + t["w"]) & (by <= yy) & (yy < by + t["h"]))
                    raise AssertionError("%s, %d bpc put, %s references: (%d,%d) of the destination is %d, the oracle has %d; %d pixels differ; "
                                         "task (filter_2d, mx, my, w, h, src_x, src_y, side) = %s at (%d,%d)" %
                                         (what, bpc, name, xx, yy, got_plane[yy, xx], want_plane[yy, xx], len(bad),
                                          batch[hit[0]][0] if len(hit) else None, bx[hit[0]] if len(hit) else -1, by[hit[0]] if len(hit) else -1))
            else:
                got_prep = prep.download(np.int16, prep_sz)
                bad = np.flatnonzero(got_prep != want_prep)
                if len(bad):
                    i = int(np.searchsorted(offs, bad[0], side="right")) - 1
                    raise AssertionError("%s, %d bpc prep, %s references: element %d is %d, the oracle has %d; %d elements differ; "
                                         "task (filter_2d, mx, my, w, h, src_x, src_y, side) = %s, element %d of it" %
                                         (what, bpc, name, bad[0], got_prep[bad[0]], want_prep[bad[0]], len(bad), batch[i][0], bad[0] - offs[i]))
                assert np.array_equal(got_plane, dplane), "prep must not touch the destination picture"
            prep.free()
    for o in list(refs.values()) + list(dsts.values()):
        o.free()
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
@pytest.mark.parametrize("kind", [0, 1], ids=["put", "prep"])
def test_every_filter_phase_and_shape(ctx, bpc, kind):
    oracle = util.default_oracle()
    full = ctx.backend != "emu"
    vis_w, vis_h = 333, 277                       # odd on purpose; the allocation is padded to 384 x 384
    rows = enumerated_rows(kind, full, vis_w, vis_h)
    assert_coverage(rows, kind, full)
    rng = np.random.default_rng(4100 + bpc)
    probe = ctx.picture(vis_w, vis_h, api.LAYOUT_I400, bpc)
    refplane = rng.integers(0, 1 << bpc, size=probe.padded_shape(0)).astype(util.pix_dtype(bpc))      # the padding is NOT edge-replicated
    probe.free()
    D = 4096 if full else 2048
    run_and_compare(ctx, oracle, bpc, kind, rows, refplane, vis_w, vis_h, D, D, "enumerated")


# ------------------------------------------------------------------ extremal content

EXT_SHAPES = [(4, 4), (8, 8), (16, 16), (32, 8)]
PATTERNS = ["max", "zero", "worst+", "worst-"]
PATCH = 48                 # patch pitch in the reference picture: a multiple of the patterns' period that holds 8 + 32 + 7 columns


def oracle_tap_signs(oracle):
    """sign[filter_2d][direction 0 = horizontal / 1 = vertical][0 = small (<= 4) / 1 = large][phase] -> eight values in -1, 0, 1:
    the sign of what an impulse at tap position t adds to output pixel (0, 0) of the oracle's 8-bit mct."""
    out = np.zeros((10, 2, 2, 16, 8), np.int8)
    tmp = np.zeros(8 * 8, np.int16)
    for f in range(10):
        for d in range(2):
            for big in range(2):
                w, h = (8 if big else 4, 8) if d == 0 else (8, 8 if big else 4)
                for m in range(16):
                    for t in range(8):
                        src = np.zeros((24, 24), np.uint8)
                        if d == 0:
                            src[8, 8 + t - 3] = 255
                        else:
                            src[8 + t - 3, 8] = 255
                        oracle.call(8, "mct", f, 0, tmp.ctypes.data, src.ctypes.data + 8 * 24 + 8, 24, w, h, m if d == 0 else 0, 0 if d == 0 else m)
                        out[f, d, big, m, t] = np.sign(int(tmp[0]))
    return out


def extremal_rows(full):
    """[(filter_2d, mx, my, w, h, pattern)]"""
    rows = []
    if full:
        for f, mx, my in itertools.product(range(10), range(16), range(16)):
            rows += [(f, mx, my, w, h, p) for w, h in EXT_SHAPES for p in PATTERNS]
        return rows
    for k, (f, mx, my) in enumerate(itertools.product(range(10), range(16), range(16))):
        w, h = EXT_SHAPES[(k + k // 4 + k // 16) % 4]
        rows += [(f, mx, my, w, h, "worst+"), (f, mx, my, w, h, "worst-")]
    for s, (w, h) in enumerate(EXT_SHAPES):
        for f in range(10):
            for pi, p in enumerate(PATTERNS):
                a, b = 1 + (3 * s + f + pi) % 15, 1 + (5 * s + 7 * f + 2 * pi) % 15
                rows += [(f, a * cx, b * cy, w, h, p) for cx, cy in PHASE_CLASSES]
    return rows


def assert_extremal_coverage(rows, full):
    ran = set(rows)
    if full:
        assert ran == {(f, mx, my, w, h, p) for f in range(10) for mx in range(16) for my in range(16) for w, h in EXT_SHAPES for p in PATTERNS}
        return
    for p in ("worst+", "worst-"):
        assert len({r[:3] for r in ran if r[5] == p}) == N_TRIPLES, "every (filter_2d, mx, my) on " + p
    assert {(w, h) for _, _, _, w, h, _ in ran} == set(EXT_SHAPES)
    classes = {(w, h, f, p, mx != 0, my != 0) for f, mx, my, w, h, p in ran}
    assert classes == {(w, h, f, p, bool(cx), bool(cy)) for w, h in EXT_SHAPES for f in range(10) for p in PATTERNS for cx, cy in PHASE_CLASSES}


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_extremal_reference_content(ctx, bpc):
    oracle = util.default_oracle()
    full = ctx.backend != "emu"
    signs = oracle_tap_signs(oracle)
    assert (signs[:, :, :, 0, 3] == 1).all() and (signs[:, :, :, 0].sum(axis=-1) == 1).all(), "phase 0 is the unit tap"
    assert (signs[0, :, 1, 1:] < 0).any(axis=(1, 2)).all() and (signs[9] >= 0).all(), "the regular 8-tap set has negative taps, bilinear has none"
    ext = extremal_rows(full)
    assert_extremal_coverage(ext, full)
    bdmax = (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    side = min(64, int(np.ceil(np.sqrt(len(ext)))))       # patches along one side of a reference picture (at most 3072 x 3072)
    per_pic, vis = side * side, side * PATCH
    for kind in (0, 1):
        put_blocks = []
        sel = [r for r in ext if kind == 0 or r[3] >= 4]
        for lo in range(0, len(sel), per_pic):
            part = sel[lo:lo + per_pic]
            probe = ctx.picture(vis, vis, api.LAYOUT_I400, bpc)
            refplane = np.zeros(probe.padded_shape(0), pd)
            probe.free()
            rows = []
            for k, (f, mx, my, w, h, p) in enumerate(part):
                px, py = (k % side) * PATCH, (k // side) * PATCH
                if p == "max":
                    refplane[py:py + PATCH, px:px + PATCH] = bdmax
                elif p != "zero":
                    sh = signs[f, 0, int(w > 4), mx].astype(np.int32)
                    sv = signs[f, 1, int(h > 4), my].astype(np.int32)
                    prod = sv[:, None] * sh[None, :]
                    win = np.where(prod > 0 if p == "worst+" else prod < 0, bdmax, 0).astype(pd)
                    # the 8 x 8 window of output pixel (0, 0) starts 3 columns and 3 rows before the block; repeated over the patch
                    refplane[py:py + PATCH, px:px + PATCH] = np.tile(win, (PATCH // 8, PATCH // 8))
                # block origin at (8 + 3, 8 + 3) of its patch: its window starts on the pattern's period
                rows.append((f, mx, my, w, h, px + 11, py + 11, p))
            got = run_and_compare(ctx, oracle, bpc, kind, rows, refplane, vis, vis, 2048, 2048, "extremal content")
            put_blocks += [(r, b) for r, b in got if r[7] in ("worst+", "worst-")]
        if kind == 0:
            # not vacuous: the worst-case windows drive the oracle itself into both clips
            lo = [r for r, b in put_blocks if b[0, 0] == 0 and r[7] == "worst-"]
            hi = [r for r, b in put_blocks if b[0, 0] == bdmax and r[7] == "worst+"]
            assert lo and hi, "the oracle's put outputs hold no 0 / no bitdepth_max"
            sub = [r for r in lo + hi if r[1] and r[2]]
            assert sub, "... nor at a phase that filters in both directions"


# ------------------------------------------------------------------ the production path: recon lists

REGION = 64


def enumerated_frame(bpc, regions_per_size, cols, seed, compound=None, transforms=None):
    """An inter frame in the layout of synth_frames.make_frame (64x64 regions of one luma block size each, 4:2:0, one transform per
    block), with ENUMERATED filters and phases: the single-reference blocks of every (plane class, block size) step through a
    permutation of all (filter_2d, mx, my); every fourth block of luma 8x8 and up is an avg compound whose two references step through
    the phases independently.  regions_per_size: {luma block size: number of regions}.  compound: None (every compound is an avg), or
    a function (serial number of the compound in the frame, its filter_2d) -> (COMP_TASK kind, arg) that decides each one.
    transforms: None (DCT_DCT, coefficients and eob of synth_frames.gen_coefs), or a function (plane class, tx, number of blocks) ->
    (coefficient slabs [n, coefficients], eob [n], txtp [n]) that decides the residual of every block of a (plane class, size)."""
    rng = np.random.default_rng(seed)
    sizes = [s for s, n in regions_per_size.items() for _ in range(n)]
    rng.shuffle(sizes)
    assert len(sizes) % cols == 0
    w, h = cols * REGION, len(sizes) // cols * REGION
    geo = synth.plane_geometry(w, h, bpc, 1)
    n_refs = 3
    mc, comp, itx, coefs = [], [], [], []
    counters, starts = {}, {}
    cf_off = prep_off = 0
    blocks = {}                                   # (plane class, size) -> [(plane, x, y, is compound, luma block index)]
    for r, s in enumerate(sizes):
        gx, gy = (r % cols) * REGION, (r // cols) * REGION
        k = REGION // s
        for j in range(k * k):
            bx, by = gx + (j % k) * s, gy + (j // k) * s
            is_comp = s >= 8 and (len(blocks.get((0, s), ())) % 4) == 3
            blocks.setdefault((0, s), []).append((0, bx, by, is_comp))
            if s > 4:
                for pl in (1, 2):
                    blocks.setdefault((1, s // 2), []).append((pl, bx // 2, by // 2, is_comp))
            elif (bx & 4) and (by & 4):           # 4x4 luma: chroma once per 8x8, by its last 4x4
                for pl in (1, 2):
                    blocks.setdefault((1, 4), []).append((pl, (bx // 2) & ~3, (by // 2) & ~3, False))
    start = 0
    for key in sorted(blocks):
        starts[key] = start
        start += sum(1 for b in blocks[key] if not b[3])
    single_seen, comp_seen = set(), set()
    for key in sorted(blocks):
        cls, pw = key
        lst = blocks[key]
        n = len(lst)
        t = np.zeros(2 * n, api.MC_TASK)
        ct = np.zeros(n, api.COMP_TASK)
        nt = nc = 0
        cnt = ccnt = starts[key]
        for i, (pl, bx, by, is_comp) in enumerate(lst):
            dst_off = by * geo[pl][0] + bx
            for r in range(2 if is_comp else 1):
                # 1021 and 1777 are prime to 2560: each a permutation of the triples; the two references of a compound step through different ones
                tr = (cnt * 1021) % N_TRIPLES if not is_comp else ((ccnt * 1021 + 77) % N_TRIPLES, (ccnt * 1777 + (ccnt >> 8) * 53 + 911) % N_TRIPLES)[r]
                f, mx, my = ((i // 4) % 10 if is_comp else tr // 256), (tr >> 4) & 15, tr & 15       # one filter per block
                far = (i + r) % 11 == 0                                            # a share points out of the picture
                dx, dy = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
                if far:
                    dx, dy = dx * 24, dy * 24
                e = t[nt]
                e["src_x"], e["src_y"], e["w"], e["h"] = bx + dx, by + dy, pw, pw
                e["mx"], e["my"], e["filter_2d"], e["plane"], e["ref"] = mx, my, f, pl, (i + r * (1 + i % 2)) % n_refs
                if is_comp:
                    e["kind"], e["dst_off"] = 1, prep_off
                    if r == 0:
                        ct[nc]["dst_off"], ct[nc]["tmp1_off"], ct[nc]["w"], ct[nc]["h"], ct[nc]["plane"] = dst_off, prep_off, pw, pw, pl
                        if compound is not None:
                            ct[nc]["kind"], ct[nc]["arg"] = compound(sum(len(c) for c in comp) + nc, f)
                        first = (f, mx, my)
                    else:
                        ct[nc]["tmp2_off"] = prep_off
                        comp_seen.add((f, first[1:], (mx, my)))
                        nc += 1
                        ccnt += 1
                    prep_off += pw * pw
                else:
                    e["kind"], e["dst_off"] = 0, dst_off
                    single_seen.add((f, mx, my, pl, pw))
                    cnt += 1
                nt += 1
        mc.append(t[:nt])
        comp.append(ct[:nc])
        tx = synth.SQ_TX[pw]
        cf, eob, txtp = synth.gen_coefs(rng, tx, n, bpc) + (0,) if transforms is None else transforms(cls, tx, n)
        it = np.zeros(n, api.ITX_TASK)
        it["dst_off"] = [b[2] * geo[b[0]][0] + b[1] for b in lst]
        it["cf_off"] = cf_off + np.arange(n, dtype=np.int64) * cf.shape[1]
        it["eob"], it["tx"], it["txtp"] = eob, tx, txtp
        it["plane"] = [b[0] for b in lst]
        itx.append(it)
        coefs.append(cf.reshape(-1))
        cf_off += n * cf.shape[1]
    fr = synth.Frame()
    fr.w, fr.h, fr.bpc, fr.n_refs = w, h, bpc, n_refs
    fr.mc, fr.comp, fr.itx, fr.coef = np.concatenate(mc), np.concatenate(comp), np.concatenate(itx), np.concatenate(coefs)
    fr.prep_elems = max(prep_off, 8)
    fr.single_seen, fr.comp_seen = single_seen, comp_seen
    fr.blocks_by_size = {}
    for (cls, pw), lst in blocks.items():
        fr.blocks_by_size[pw] = fr.blocks_by_size.get(pw, 0) + len(lst)
    return fr


def assert_frame_coverage(fr, full):
    triples = {s[:3] for s in fr.single_seen}
    assert len(triples) == N_TRIPLES, "single-reference blocks over every (filter_2d, mx, my): %d" % len(triples)
    assert {(mx & 1, my & 1) for _, mx, my, pl, _ in fr.single_seen if pl == 0} == {(0, 0), (0, 1), (1, 0), (1, 1)}, "odd luma phases"
    assert {pw for _, _, _, pl, pw in fr.single_seen if pl == 0} == {4, 8, 16, 32, 64}
    assert {pw for _, _, _, pl, pw in fr.single_seen if pl} == {4, 8, 16, 32}
    if full:        # the block classes of the default paired launches, each over the full product
        for pw in (4, 8, 16, 32):
            assert len({s[:3] for s in fr.single_seen if s[3] == 0 and s[4] == pw}) == N_TRIPLES, "luma %dx%d over every triple" % (pw, pw)
        for pw in (4, 8, 16):
            assert len({s[:3] for s in fr.single_seen if s[3] and s[4] == pw}) == N_TRIPLES, "chroma %dx%d over every triple" % (pw, pw)
    assert {c[0] for c in fr.comp_seen} == set(range(10)), "avg compounds over every filter_2d"
    assert sum(1 for _, a, b in fr.comp_seen if a != b) > 0.9 * len(fr.comp_seen), "... with independent phases of the two references"
    assert len({c[1:] for c in fr.comp_seen}) >= min(len(fr.comp), N_TRIPLES) // 2, "... and many different phase pairs"


_frames = {}


def _frame_and_oracle(bpc, full):
    """the frame, its inputs and the oracle's pictures: once per bit depth, shared by the six runs"""
    key = (bpc, full)
    if key not in _frames:
        if full:        # 3072 x 2368: at least 2560 single-reference luma blocks of each size 4x4 .. 32x32
            fr = enumerated_frame(bpc, {64: 644, 32: 854, 16: 214, 8: 54, 4: 10}, 48, seed=600 + bpc)
        else:
            fr = enumerated_frame(bpc, {64: 5, 32: 5, 16: 4, 8: 5, 4: 5}, 8, seed=600 + bpc)
        rng = np.random.default_rng(61 + bpc)
        refs = [synth.make_planes(rng, fr.w, fr.h, bpc, smooth=(i == 1)) for i in range(fr.n_refs)]
        dst0 = synth.make_planes(rng, fr.w, fr.h, bpc, smooth=False)
        want, _, want_coef = test_frame.oracle_frame(util.default_oracle(), fr, dst0, refs)
        _frames[key] = (fr, refs, dst0, want, want_coef)
    return _frames[key]


@pytest.mark.parametrize("fuse", [None, 0], ids=["default-paired", "two-kernels"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_recon_lists_over_every_filter_and_phase(ctx, bpc, fuse, twin_refs):
    full = ctx.backend != "emu"
    fr, refs_h, dst0, want, want_coef = _frame_and_oracle(bpc, full)
    assert_frame_coverage(fr, full)
    if fuse is not None:
        ctx.set_option("recon_fuse", fuse)
    mask = ctx.get_option("recon_fuse") & 31
    assert mask == (15 if fuse is None else 0)
    got, _, got_coef = test_frame.hip_frame(ctx, fr, dst0, refs_h, recon=True)
    for pl in range(3):
        bad = np.argwhere(got[pl] != want[pl])
        if len(bad):
            yy, xx = bad[0]
            sp = got[pl].strides[0] // got[pl].itemsize
            m = fr.mc[fr.mc["plane"] == pl]
            raise AssertionError("plane %d differs at (%d,%d): %d, the oracle has %d (%d px); blocks there: %s" %
                                 (pl, xx, yy, got[pl][yy, xx], want[pl][yy, xx], len(bad), _blocks_at(fr, pl, xx, yy, sp)))
    assert np.array_equal(got_coef, want_coef)
    # which launches took the blocks
    if twin_refs != "native":
        counts = _launch_counts(ctx, fr, dst0, refs_h, want)
        paired = {4 << k: counts[k] for k in range(5)}
        expect = {pw: (n if mask >> synth.SQ_TX[pw] & 1 else 0) for pw, n in fr.blocks_by_size.items()}
        assert paired == expect, "blocks in the paired launches by size: %s, expected %s" % (paired, expect)
        if mask:
            assert sum(paired.values()) == len(fr.itx) - fr.blocks_by_size[64] and not any(counts[21:25]), "4x4 .. 32x32 all went through the paired launches"
        else:
            assert sum(counts[5:20]) > 0 and sum(counts[21:40]) == len(fr.itx)


def _blocks_at(fr, pl, xx, yy, sp):
    out = []
    for kind, lst in (("mc", fr.mc), ("comp", fr.comp)):
        if kind == "mc":
            lst = lst[lst["kind"] == 0]
        lst = lst[lst["plane"] == pl]
        x, y = lst["dst_off"] % sp, lst["dst_off"] // sp
        hit = lst[(x <= xx) & (xx < x + lst["w"]) & (y <= yy) & (yy < y + lst["h"])]
        for t in hit:
            if kind == "comp":
                srcs = fr.mc[(fr.mc["kind"] == 1) & np.isin(fr.mc["dst_off"], [t["tmp1_off"], t["tmp2_off"]])]
                out.append(("avg", int(t["w"]), [tuple(int(s[k]) for k in ("filter_2d", "mx", "my", "src_x", "src_y", "ref")) for s in srcs]))
            else:
                out.append(("put", int(t["w"])) + tuple(int(t[k]) for k in ("filter_2d", "mx", "my", "src_x", "src_y", "ref")))
    return out


def _launch_counts(ctx, fr, dst0, refs_h, want):
    """dav1d_hip_recon_list_run_timed on a fresh copy of the inputs: its pictures (they must be the oracle's too) and the number of
    blocks each of its 40 launches held ([0..4] paired by size, [5..19] prediction, [20] compound, [21..39] residual by transform)."""
    dst = ctx.picture(fr.w, fr.h, api.LAYOUT_I420, fr.bpc)
    refs = [ctx.picture(fr.w, fr.h, api.LAYOUT_I420, fr.bpc) for _ in refs_h]
    for pl in range(3):
        dst.upload(pl, dst0[pl])
        for r, rp in zip(refs, refs_h):
            r.upload(pl, rp[pl])
    prep = ctx.buffer(fr.prep_elems * 2)
    prep.zero()
    coef = ctx.buffer_from(fr.coef)
    rl = ctx.recon_list(dst, fr.mc, fr.comp, fr.itx)
    ms, counts = (C.c_float * 40)(), (C.c_size_t * 40)()
    arr = (api.Picture * len(refs))(*[r.pic for r in refs])
    rc = ctx.lib.dav1d_hip_recon_list_run_timed(ctx.h, rl.h, C.byref(dst.pic), arr, len(refs), prep.ptr, None, coef.ptr, ms, counts)
    assert rc == 0, rc
    for pl in range(3):
        assert np.array_equal(dst.download(pl), want[pl]), "timed run, plane %d" % pl
    rl.destroy()
    for o in [dst, prep, coef] + refs:
        o.free()
    return [int(v) for v in counts]
