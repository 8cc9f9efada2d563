"""The inverse transform, ENUMERATED: every (size, type, eob) of csrc/itx_body.h / csrc/itx.hip against the oracle, byte for byte.

tests/test_itx.py draws about one random eob per sub-size class and (size, type), as checkasm does.  The kernel does not read the
whole coefficient slab: the host derives from the eob how long a prefix can be non-zero (2-D classes and WHT: the generated table
av1_scan_prefix_end; H classes: eob + 1; V classes: everything), the kernel fetches and re-zeroes ceil(end * sizeof(coef) / 16)
16-byte pieces of it and zero-fills the rest in LDS.  A prefix one piece short drops the farthest coefficient, a wrong table entry
shows at one eob only, so this module lists every eob.  What the rows cover is collected in a set FIRST and the set is asserted;
every condition (`end`, the pieces, the blocks of a wave) is computed here from the scans (util.scans(), the oracle's tables) and
the formulas of the specification, never read from the code under test.

* test_scan_prefix_table_matches_the_scans -- host only: av1_scan_prefix_off / av1_scan_prefix_end parsed out of the header;
  every entry equals 1 + max(scan[0 .. eob]), the offsets are the running sums of min(w,32) * min(h,32).
* test_every_size_type_and_eob -- hip: all 19 sizes x every legal type x every eob (WHT_WHT: eob 1 .. 14, what test_itx.py
  draws), 20 750 blocks per bit depth.  emu: per (size, type) eob 0, 1, the last and both sides of the first and the last change of
  the piece count; for one type of each scan class per size both sides of EVERY change; every eob at 4x4.  Coefficients: a forward transform of a
  random residual (util.fwd_itx_coefs, the residual within a quarter of the pixel range so that the sum with a destination pixel
  of the middle half seldom clips), cut after the row's eob in the scan order of its class, with two positions forced to be
  non-zero: scan position eob and the position with the highest slab index among scan positions 0 .. eob.  Blocks sit on a picture
  of random pixels with a gap between them.  Asserted on the ORACLE alone, for every row: its block with the highest-index
  coefficient set to 0 differs from its block with it (so a dropped coefficient cannot pass).  Three runs: (a) dense in one list of
  at least 4096 tasks (the per-size kernels), (b) dense in lists of fewer than 4096 tasks that each hold every size
  (itx_multi_kernel), (c) packed (util.pack_coefs) through (a)'s route.  Pixels, everything outside the blocks and the coefficient
  arena (zeroed like the reference when dense, untouched when packed) are compared.
* test_blocks_that_share_a_wave -- BPW = 64 / max(min(h, 32), w) blocks share a wave.  For every size with BPW > 1 and k in
  {1, BPW - 1, BPW, BPW + 1, 2 BPW + 1}: lists of k blocks which, put together, hold dc-only, DCT_DCT with eob 1 and a full-eob
  block of every legal type; neighbours in a list differ in path, in dense / packed and in plane (0, 1, 2 of an I420 picture).  Each
  list runs alone (one launch for every size) and, together with one list of every other size, padded past 4096 tasks with blocks of
  another size (the per-size kernels: a size's blocks are still the list's alone).

* test_recon_routes_over_every_type_and_eob_class -- the fused prediction + residual launches of the inter lists (csrc/recon.hip)
  and the two-kernel route (recon_fuse default and 0; raster / tiled / tiled-native references): a 384 x 320 4:2:0 frame of
  test_mc_sweep.enumerated_frame whose transform blocks, luma 4x4 .. 64x64 and chroma 4x4 .. 32x32, step through every legal type of
  their size (H and V classes up to 16x16, IDTX at 32x32, WHT_WHT at 4x4) crossed with the eob classes {0, 1, both sides of the first
  and of the last change of the piece count, the last}, coefficients as above; dense and packed; against test_frame.oracle_frame; the
  blocks of each launch are asserted.  test_recon_residuals_onto_a_picture_in_its_twin_only runs the frame's predictions and its
  residuals as two tiled-native lists: the transform body then reads its destination through the tiled twin.

* test_intra_routes_over_every_size_and_type -- an intra pass in the manner of synth_frames.make_intra_pass (make_shape_pass below):
  64 x 64 regions, never two neighbours, each tiled by one of the 19 transform shapes in the 2:1 wavefront order, in luma and (where
  the shape fits the chroma region, else halved) in chroma, as many regions per shape as it takes for its blocks to hold every
  (legal type, eob class) and every legal prediction mode, in luma and in chroma: both asserted before anything runs.  Through every
  route of test_postchain.hip_intra (paired lists, prediction + residual lists, flow, sb) against test_postchain.oracle_intra.  No
  route refuses a shape: the lists take any legal (prediction size, transform) pair.

THE FORCED MAGNITUDE.  The forward transform of the tests scales an orthonormal transform by S = scale(w * h) * sqrt(w * h) / 2 (8
for most sizes, 4 at 32x32, 2 at 64x64; util._SCALE, tests/checkasm/itx.c:74-100), so a lone coefficient c comes back as a residual
of root-mean-square c / (S * sqrt(w * h)) over the block when both passes spread it, and of more where a pass is the identity (one
line, or one pixel for IDTX).  The forced values have magnitude M = ceil(scale(w * h) * w * h) = 2 * S * sqrt(w * h): a residual of 2
pixel LSB r.m.s., well above the roundings of the two passes, whatever the type and the bit depth (the pixel LSB does not depend on
it).  That is 64 at 4x4 .. 256 from 16x16 on.  WHT_WHT shifts its input right by 2 first: its M = 64 becomes 16, 4 LSB r.m.s. over
the 16 pixels.  At IDTX the forced coefficient alone makes its pixel (M / S <= 64): a destination pixel of the middle half of the
8-bit range cannot clip on it.  A coefficient the transform already made larger than M keeps its value.

Cost: DESIGN.md 11.  An emulator trap ends the pytest process: run this module in a pytest call of its own first."""
import math
import os
import re

import numpy as np
import pytest

import util
import synth_frames as synth
import test_frame
import test_mc_sweep
from dav1d_amd import api

GAP = 4               # pixels between two blocks
POOL = 4              # forward transforms per (size, type): row eob takes number eob % POOL
ONE_LAUNCH = 4096     # lists shorter than this run every size in one launch (include/dav1d_hip.h: dav1d_hip_itx_list_run)
PACKED = 1            # DAV1D_HIP_ITX_PACKED
N_COEF = [min(w, 32) * min(h, 32) for w, h in zip(util.TX_W, util.TX_H)]
assert "DAV1D_HIP_ITX_ONE_LAUNCH" not in os.environ, "the library reads its one-launch threshold from this variable: the runs below would swap routes"
WHT_EOBS = range(1, 15)       # what util.gen_itx_coefs gives test_itx.py for WHT_WHT (sub-size class 1 of a 4x4 block)


def tx_scale(tx):
    return util._SCALE[int(math.log2(util.TX_W[tx] * util.TX_H[tx])) - 4]


def forced_magnitude(tx):
    return int(math.ceil(tx_scale(tx) * util.TX_W[tx] * util.TX_H[tx]))


def scan_class(txtp):
    return "wht" if txtp == util.WHT_WHT else ("2d", "h", "v")[util.tx_class(txtp)]


def prefix_end(tx, txtp):
    """end[eob]: how much of the slab a block with that eob can have written -- 2-D and WHT: 1 + max(scan[0 .. eob]); H: eob + 1;
    V: the slab"""
    n = N_COEF[tx]
    if util.tx_class(txtp) == 2:
        return np.full(n, n, np.int64)
    return 1 + np.maximum.accumulate(util.scan_order(tx, txtp))


def pieces(end, bpc):
    return (end * np.dtype(util.coef_dtype(bpc)).itemsize + 15) >> 4


def blocks_per_wave(tx):
    return 64 // max(min(util.TX_H[tx], 32), util.TX_W[tx])


# ------------------------------------------------------------------ 0. the host table

def test_scan_prefix_table_matches_the_scans():
    src = open(os.path.join(util.ROOT, "dav1d_amd", "csrc", "av1_scan_prefix.h")).read()

    def table(name):
        m = re.search(r"%s\[(\d+)\]\s*=\s*\{([^}]*)\}" % name, src)
        assert m, name
        vals = [int(v) for v in m.group(2).replace("\n", " ").split(",") if v.strip()]
        assert len(vals) == int(m.group(1)), "%s: %d values for %s entries" % (name, len(vals), m.group(1))
        return np.array(vals, np.int64)

    off, end = table("av1_scan_prefix_off"), table("av1_scan_prefix_end")
    assert len(off) == 20 and np.array_equal(off, np.concatenate([[0], np.cumsum(N_COEF)])), "offsets are not the running sums of min(w,32) * min(h,32)"
    assert len(end) == off[19] == 7440
    scans = util.scans()
    for tx in range(19):
        assert len(scans[tx]) == N_COEF[tx] and sorted(scans[tx]) == list(range(N_COEF[tx])), "scan of %s is no permutation" % util.TX_NAMES[tx]
        want = 1 + np.maximum.accumulate(scans[tx].astype(np.int64))
        got = end[off[tx]:off[tx + 1]]
        bad = np.flatnonzero(got != want)
        assert not len(bad), "%s, eob %d: the table has %d, 1 + max(scan[0 .. eob]) is %d (%d entries differ)" % (
            util.TX_NAMES[tx], bad[0], got[bad[0]], want[bad[0]], len(bad))


# ------------------------------------------------------------------ blocks, placement, oracle, runs

class Block:
    def __init__(self, tx, txtp, eob, cf, plane=0, packed=False, tag=None):
        self.tx, self.txtp, self.eob, self.cf, self.plane, self.packed, self.tag = tx, txtp, eob, cf, plane, packed, tag
        self.w, self.h = util.TX_W[tx], util.TX_H[tx]

    def __repr__(self):
        return "%s %s eob %d plane %d %s at (%d,%d)%s" % (util.TX_NAMES[self.tx], util.TXTP_NAMES[self.txtp], self.eob, self.plane,
                                                         "packed" if self.packed else "dense", self.x, self.y, "" if self.tag is None else " [%s]" % (self.tag,))


_fwd_pool = {}


def fwd_pool(tx, txtp, bpc):
    key = (tx, txtp, bpc)
    if key not in _fwd_pool:
        rng = np.random.default_rng(990000 + (tx * 17 + txtp) * 3 + bpc)
        _fwd_pool[key] = [util.fwd_itx_coefs(rng, tx, txtp, bpc, amp=((1 << bpc) - 1) >> 2) for _ in range(POOL)]
    return _fwd_pool[key]


def make_coefs(tx, txtp, eob, bpc, order=None):
    """the slab of a row and the slab index of its farthest coefficient"""
    order = util.scan_order(tx, txtp) if order is None else order
    cf = fwd_pool(tx, txtp, bpc)[eob % POOL].copy()
    cf[order[eob + 1:]] = 0
    far = int(order[:eob + 1].max())
    m = forced_magnitude(tx)
    for pos in (int(order[eob]), far):
        if abs(cf[pos]) < m:
            cf[pos] = -m if cf[pos] < 0 else m
    cf_max = (1 << (15 if bpc == 8 else bpc + 7)) - 1          # what the entropy decoder can hand over, src/recon_tmpl.c:decode_coefs
    assert np.abs(cf).max() <= cf_max
    return cf.astype(util.coef_dtype(bpc)), far


def place(blocks, shapes):
    """shelves of one height per plane, GAP pixels apart; shapes[plane] = (rows, columns) available"""
    cur = {}
    for b in sorted(blocks, key=lambda b: (b.plane, -b.h, -b.w)):
        ph, pw = shapes[b.plane]
        x, y, shelf = cur.get(b.plane, (0, 0, 0))
        if x + b.w > pw:
            x, y, shelf = 0, y + shelf + GAP, 0
        assert y + b.h <= ph, "the picture is too small for the rows"
        b.x, b.y = x, y
        cur[b.plane] = (x + b.w + GAP, y, max(shelf, b.h))


def rows_needed(blocks, width):
    """luma rows a picture `width` wide needs for place() of one-plane blocks"""
    x = y = shelf = 0
    for b in sorted(blocks, key=lambda b: (-b.h, -b.w)):
        if x + b.w > width:
            x, y, shelf = 0, y + shelf + GAP, 0
        x, shelf = x + b.w + GAP, max(shelf, b.h)
    return y + shelf


def oracle_blocks(oracle, bpc, blocks, planes):
    for b in blocks:
        cf = b.cf.copy()
        oracle.call(bpc, "itxfm_add", b.tx, b.txtp, planes[b.plane][b.y:, b.x:].ctypes.data, planes[b.plane].strides[0], cf.ctypes.data, b.eob)
        assert not cf.any()          # the reference leaves its slab zeroed


def arena_of(blocks, bpc, extra=0):
    """(arena, what a run leaves of it, cf_off per block): dense slabs come back zeroed, packed values stay; every block starts on a
    16-byte boundary; `extra` zero coefficients at the end (the padding blocks' shared slab)"""
    parts, want, offs, off = [], [], [], 0
    for b in blocks:
        v = util.pack_coefs(b.tx, b.txtp, b.cf, b.eob) if b.packed else b.cf
        v = np.concatenate([v, np.zeros(-len(v) % 16, v.dtype)])
        parts.append(v)
        want.append(v if b.packed else np.zeros_like(v))
        offs.append(off)
        off += len(v)
    tail = [np.zeros(extra, util.coef_dtype(bpc))]
    return np.concatenate(parts + tail), np.concatenate(want + tail), offs


def tasks_of(pic, blocks, offs):
    t = np.zeros(len(blocks), api.ITX_TASK)
    for i, (b, off) in enumerate(zip(blocks, offs)):
        t[i] = (b.y * pic.stride_px(b.plane) + b.x, off, b.eob, b.tx, b.txtp, b.plane, PACKED if b.packed else 0, (0, 0))
    return t


def run_and_compare(ctx, pic, pre, want, blocks, lists, arena, want_arena, what):
    """pre -> the picture, every list of `lists` through ctx.itx_add_batch, then planes and arena against the oracle's"""
    for pl in range(pic.n_planes):
        pic.upload(pl, pre[pl])
    dcoef = ctx.buffer_from(arena)
    for t in lists:
        ctx.itx_add_batch(pic, t, dcoef)
    got_arena = dcoef.download(arena.dtype, len(arena))
    dcoef.free()
    for pl in range(pic.n_planes):
        got = pic.download(pl)
        bad = np.argwhere(got != want[pl])
        if len(bad):
            yy, xx = bad[0]
            hit = [b for b in blocks if b.plane == pl and b.x <= xx < b.x + b.w and b.y <= yy < b.y + b.h]
            raise AssertionError("%s, %d bpc: (%d,%d) of plane %d is %d, the oracle has %d (before the call: %d); %d pixels differ; block: %r" % (
                what, pic.bpc, xx, yy, pl, got[yy, xx], want[pl][yy, xx], pre[pl][yy, xx], len(bad), hit[0] if hit else "none: outside every block"))
    bad = np.flatnonzero(got_arena != want_arena)
    assert not len(bad), "%s, %d bpc: coefficient %d of the arena is %d after the run, expected %d (%d differ)" % (
        what, pic.bpc, bad[0], got_arena[bad[0]], want_arena[bad[0]], len(bad))


def random_planes_with_mid_blocks(rng, pic, blocks):
    """random pixels everywhere; inside the blocks the middle half of the range, so that a pixel clip cannot hide a residual"""
    bpc = pic.bpc
    pre = [rng.integers(0, 1 << bpc, size=pic.padded_shape(pl)).astype(pic.dtype) for pl in range(pic.n_planes)]
    for b in blocks:
        pre[b.plane][b.y:b.y + b.h, b.x:b.x + b.w] = rng.integers(1 << (bpc - 2), 3 << (bpc - 2), size=(b.h, b.w))
    return pre


def padding_tasks(pic, tx, cf_off, x0, y0):
    """ONE_LAUNCH dc-only blocks of size tx with a zero coefficient, tiling a region of plane 0 from (x0, y0): they change nothing,
    and all read the same zero slab"""
    w, h = util.TX_W[tx], util.TX_H[tx]
    t = np.zeros(ONE_LAUNCH, api.ITX_TASK)
    i = np.arange(ONE_LAUNCH)
    t["dst_off"] = (y0 + (i // 64) * h) * pic.stride_px(0) + x0 + (i % 64) * w
    t["cf_off"], t["tx"] = cf_off, tx
    return t


# ------------------------------------------------------------------ 1. every size, type and eob

def sweep_rows(full, bpc):
    rows = []
    for tx in range(19):
        n = N_COEF[tx]
        dense_class = set()
        for txtp in util.legal_txtps(tx):
            cls = scan_class(txtp)
            legal = WHT_EOBS if cls == "wht" else range(n)
            if full:
                eobs = set(legal)
            else:
                p = pieces(prefix_end(tx, txtp), bpc)
                ch = np.flatnonzero(p[1:] != p[:-1]) + 1                 # p changes between eob ch - 1 and eob ch
                if cls not in dense_class:                              # the first type of its class: every change
                    dense_class.add(cls)
                else:
                    ch = ch[[0, -1]] if len(ch) else ch
                eobs = {0, 1, n - 1} | {int(e) for e in ch} | {int(e) - 1 for e in ch}
                if tx == 0:                                             # 4x4: every eob (H classes: every residue of `end`)
                    eobs |= set(legal)
                eobs = {min(max(e, legal[0]), legal[-1]) for e in eobs}
            rows += [(tx, txtp, e) for e in sorted(eobs)]
    return rows


def assert_sweep_coverage(rows, full, bpc):
    have = set(rows)
    assert len(have) == len(rows)
    per16 = 16 // np.dtype(util.coef_dtype(bpc)).itemsize
    residues, classes = set(), set()
    for tx in range(19):
        n = N_COEF[tx]
        seen_class = set()
        for txtp in util.legal_txtps(tx):
            cls = scan_class(txtp)
            end = prefix_end(tx, txtp)
            lo, hi = (WHT_EOBS[0], WHT_EOBS[-1]) if cls == "wht" else (0, n - 1)
            mine = sorted(e for (t, tp, e) in have if (t, tp) == (tx, txtp))
            assert mine and lo <= mine[0] and mine[-1] <= hi
            classes.add(cls)
            residues |= {int(end[e]) % per16 for e in mine}
            if full:
                assert mine == list(range(lo, hi + 1)), "%s %s: not every eob" % (util.TX_NAMES[tx], util.TXTP_NAMES[txtp])
                continue
            p = pieces(end, bpc)
            ch = [int(e) for e in np.flatnonzero(p[1:] != p[:-1]) + 1 if lo < e <= hi]
            assert {lo, max(1, lo), hi} <= set(mine)
            if cls in seen_class:
                ch = ch[:1] + ch[-1:]
            seen_class.add(cls)
            for e in ch:
                assert e in mine and e - 1 in mine, "%s %s: the change of the piece count at eob %d is not met from both sides" % (
                    util.TX_NAMES[tx], util.TXTP_NAMES[txtp], e)
    if full:
        assert len(rows) == sum(len(WHT_EOBS) if tp == util.WHT_WHT else N_COEF[tx] for tx in range(19) for tp in util.legal_txtps(tx)) == 20750
    assert classes == {"2d", "h", "v", "wht"}
    assert residues == set(range(per16)), "residues of `end` modulo the %d coefficients of 16 bytes: %s" % (per16, sorted(residues))


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_size_type_and_eob(ctx, bpc):
    oracle = util.default_oracle()
    full = ctx.backend == "hip"
    rows = sweep_rows(full, bpc)
    assert_sweep_coverage(rows, full, bpc)

    rng = np.random.default_rng(8800 + bpc)
    orders = {}
    blocks, fars = [], []
    for tx, txtp, eob in rows:
        if (tx, txtp) not in orders:
            orders[tx, txtp] = util.scan_order(tx, txtp)
        cf, far = make_coefs(tx, txtp, eob, bpc, orders[tx, txtp])
        blocks.append(Block(tx, txtp, eob, cf))
        fars.append(far)
    width = 4096 if full else 2048
    rows_px = rows_needed(blocks, width)
    n_pad = max(0, ONE_LAUNCH - len(blocks))         # a thinned set shorter than the one-launch threshold is padded up to it
    pad_y = rows_px + GAP
    pic = ctx.picture(width, pad_y + (4 * ((n_pad + 63) // 64) if n_pad else 0), api.LAYOUT_I400, bpc)
    place(blocks, [pic.padded_shape(0)])
    pre = random_planes_with_mid_blocks(rng, pic, blocks)
    want = [pre[0].copy()]
    oracle_blocks(oracle, bpc, blocks, want)

    # on the oracle alone: without its farthest coefficient every block comes out different
    scratch = np.zeros((64, 64), pic.dtype)
    hidden = []
    for b, far in zip(blocks, fars):
        scratch[:b.h, :b.w] = pre[0][b.y:b.y + b.h, b.x:b.x + b.w]
        cf = b.cf.copy()
        assert cf[far] and not cf[far + 1:].any()
        cf[far] = 0
        oracle.call(bpc, "itxfm_add", b.tx, b.txtp, scratch.ctypes.data, scratch.strides[0], cf.ctypes.data, b.eob)
        if np.array_equal(scratch[:b.h, :b.w], want[0][b.y:b.y + b.h, b.x:b.x + b.w]):
            hidden.append(b)
    assert not hidden, "%d bpc: the farthest coefficient of %d rows does not show in the oracle's output, the first: %r" % (bpc, len(hidden), hidden[0])

    # (a) dense, one list: the per-size kernels
    arena, want_arena, offs = arena_of(blocks, bpc, extra=16)
    t = tasks_of(pic, blocks, offs)
    pad = padding_tasks(pic, 0, len(arena) - 16, 0, pad_y)[:n_pad]
    whole = np.concatenate([t, pad])
    assert len(whole) >= ONE_LAUNCH
    run_and_compare(ctx, pic, pre, want, blocks, [whole[rng.permutation(len(whole))]], arena, want_arena, "dense, one list")
    # (b) dense, lists below the one-launch threshold that each mix all sizes
    n_lists = len(t) // 2048 + 1
    perm = rng.permutation(len(t))
    lists = [t[perm[j::n_lists]] for j in range(n_lists)]
    assert all(len(l) < ONE_LAUNCH and set(l["tx"]) == set(range(19)) for l in lists)
    run_and_compare(ctx, pic, pre, want, blocks, lists, arena, want_arena, "dense, %d short lists" % n_lists)
    # (c) packed, through (a)'s route
    for b in blocks:
        b.packed = True
    arena, want_arena, offs = arena_of(blocks, bpc, extra=16)
    whole = np.concatenate([tasks_of(pic, blocks, offs), padding_tasks(pic, 0, len(arena) - 16, 0, pad_y)[:n_pad]])
    run_and_compare(ctx, pic, pre, want, blocks, [whole[rng.permutation(len(whole))]], arena, want_arena, "packed, one list")
    pic.free()


# ------------------------------------------------------------------ 2. blocks that share a wave

def wave_menu(tx):
    """the paths a block of this size can take: (txtp, eob)"""
    n = N_COEF[tx]
    return [(0, 0), (0, 1)] + [(tp, WHT_EOBS[-1] if tp == util.WHT_WHT else n - 1) for tp in util.legal_txtps(tx)]


def wave_lists(tx):
    """[(k, [(txtp, eob, plane, packed)])]: for every k, windows of k consecutive entries of the menu (cyclic) that cover it; along
    a list the plane steps 0, 1, 2 and dense / packed alternate"""
    bpw = blocks_per_wave(tx)
    menu = wave_menu(tx)
    out = []
    for k in sorted({1, bpw - 1, bpw, bpw + 1, 2 * bpw + 1} - {0}):
        for li, start in enumerate(range(0, len(menu), k)):
            items = []
            for j in range(k):
                txtp, eob = menu[(start + j) % len(menu)]
                items.append((txtp, eob, (j + li) % 3, bool((j + li) & 1)))
            out.append((k, items))
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_blocks_that_share_a_wave(ctx, bpc):
    oracle = util.default_oracle()
    rng = np.random.default_rng(8900 + bpc)
    sizes = [tx for tx in range(19) if blocks_per_wave(tx) > 1]
    assert [util.TX_NAMES[tx] for tx in range(19) if tx not in sizes] == ["64x64", "64x32", "64x16"]
    assert {util.TX_NAMES[tx]: blocks_per_wave(tx) for tx in (0, 1, 2, 3, 11)} == {"4x4": 16, "8x8": 8, "16x16": 4, "32x32": 2, "32x64": 2}
    # ---- what the lists hold, asserted before anything runs
    lists, covered = [], set()
    for tx in sizes:
        bpw = blocks_per_wave(tx)
        menu = set(wave_menu(tx))
        assert {(0, 0), (0, 1)} <= menu and {tp for tp, e in menu if e > 1} == set(util.legal_txtps(tx))
        for k, items in wave_lists(tx):
            lists.append((tx, k, items))
            covered.add((tx, k, frozenset(items)))
        for k in {1, bpw - 1, bpw, bpw + 1, 2 * bpw + 1} - {0}:
            mine = [items for (t, kk, items) in lists if (t, kk) == (tx, k)]
            assert mine and all(len(items) == k for items in mine)
            assert {(tp, e) for items in mine for (tp, e, pl, pk) in items} == menu, "%s, k %d: the lists leave out a path" % (util.TX_NAMES[tx], k)
            if k >= 2:     # every list mixes paths, wire formats and planes
                for items in mine:
                    assert len({(tp, e) for tp, e, pl, pk in items}) >= 2 and {pk for tp, e, pl, pk in items} == {False, True}
                    assert len({pl for tp, e, pl, pk in items}) == min(k, 3)
            else:
                assert {pk for items in mine for tp, e, pl, pk in items} == {False, True} and {pl for items in mine for tp, e, pl, pk in items} == {0, 1, 2}
        # a list of at most BPW blocks is one wave whatever its order: dc-only, eob 1 and full blocks meet in one where BPW allows
        if bpw >= 3:
            assert any(k <= bpw and {(0, 0), (0, 1)} <= {(tp, e) for tp, e, pl, pk in items} and any(e > 1 for tp, e, pl, pk in items) for (t, k, items) in lists if t == tx)
    assert len(covered) == len(lists) and {(tx, k) for tx, k, _ in covered} == {(tx, k) for tx in sizes for k in {1, blocks_per_wave(tx) - 1, blocks_per_wave(tx), blocks_per_wave(tx) + 1, 2 * blocks_per_wave(tx) + 1} - {0}}

    blocks, members = [], []
    for li, (tx, k, items) in enumerate(lists):
        mine = []
        for txtp, eob, plane, packed in items:
            cf, _ = make_coefs(tx, txtp, eob, bpc)
            blocks.append(Block(tx, txtp, eob, cf, plane, packed, tag="list %d, k %d" % (li, k)))
            mine.append(len(blocks) - 1)
        members.append(mine)
    pad_h = 8 * (ONE_LAUNCH // 64)
    pic = ctx.picture(1024, 1024 + pad_h, api.LAYOUT_I420, bpc)
    place(blocks, [(1024, 1024), (512, 512), (512, 512)])
    pre = random_planes_with_mid_blocks(rng, pic, blocks)
    want = [p.copy() for p in pre]
    oracle_blocks(oracle, bpc, blocks, want)
    assert all(not np.array_equal(want[b.plane][b.y:b.y + b.h, b.x:b.x + b.w], pre[b.plane][b.y:b.y + b.h, b.x:b.x + b.w]) for b in blocks)
    arena, want_arena, offs = arena_of(blocks, bpc, extra=64)
    t = tasks_of(pic, blocks, offs)
    alone = [t[m] for m in members]
    assert all(len(l) < ONE_LAUNCH for l in alone)
    run_and_compare(ctx, pic, pre, want, blocks, alone, arena, want_arena, "every list alone")
    # padded with 4096 blocks of another size: the list's own size runs in its per-size kernel, in the same waves.  One launch per
    # size, so a padded list takes one list of EVERY size (the padding is 4x4; the 4x4 lists are padded with 8x8 on their own)
    pads = {ptx: padding_tasks(pic, ptx, len(arena) - 64, 0, 1024) for ptx in (0, 1)}
    by_size = {tx: [m for (t_, k, items), m in zip(lists, members) if t_ == tx] for tx in sizes}
    padded = [np.concatenate([t[m], pads[1]]) for m in by_size[0]]
    for j in range(max(len(v) for tx, v in by_size.items() if tx)):
        padded.append(np.concatenate([t[v[j]] for tx, v in by_size.items() if tx and j < len(v)] + [pads[0]]))
    assert sorted(i for l in padded for i in l["cf_off"][:-ONE_LAUNCH]) == sorted(offs)
    assert all(len(l) > ONE_LAUNCH for l in padded)
    run_and_compare(ctx, pic, pre, want, blocks, padded, arena, want_arena, "every list padded past the one-launch threshold")
    pic.free()


# ------------------------------------------------------------------ 3. the fused routes of the inter lists

def eob_classes(tx, txtp, bpc):
    """eob 0, 1, both sides of the first and of the last change of the piece count, the last"""
    n = N_COEF[tx]
    p = pieces(prefix_end(tx, txtp), bpc)
    ch = np.flatnonzero(p[1:] != p[:-1]) + 1
    e = {0, 1, n - 1} | ({int(ch[0]) - 1, int(ch[0]), int(ch[-1]) - 1, int(ch[-1])} if len(ch) else set())
    legal = WHT_EOBS if txtp == util.WHT_WHT else range(n)
    return sorted({min(max(v, legal[0]), legal[-1]) for v in e})


def type_and_eob_combos(tx, bpc):
    """the type steps fastest: a few blocks already hold every type"""
    classes = {tp: eob_classes(tx, tp, bpc) for tp in util.legal_txtps(tx)}
    return [(tp, classes[tp][r]) for r in range(7) for tp in classes if r < len(classes[tp])]


def stepped_transforms(bpc, seen):
    """for test_mc_sweep.enumerated_frame: the blocks of a (plane class, size) step through every (legal type, eob class); chroma
    starts elsewhere in the cycle than luma.  seen collects (plane class, tx, txtp, eob)."""
    def decide(cls, tx, n):
        combos = type_and_eob_combos(tx, bpc)
        cf = np.empty((n, N_COEF[tx]), util.coef_dtype(bpc))
        eob, txtp = np.empty(n, np.int64), np.empty(n, np.int64)
        for i in range(n):
            txtp[i], eob[i] = combos[(i + 5 * cls) % len(combos)]
            cf[i], _ = make_coefs(tx, int(txtp[i]), int(eob[i]), bpc)
            seen.add((cls, tx, int(txtp[i]), int(eob[i])))
        return cf, eob, txtp
    return decide


_recon_frames = {}


def recon_frame_and_oracle(bpc):
    """a 384 x 320 frame of test_mc_sweep.enumerated_frame, its inputs and the oracle's pictures: once per bit depth"""
    if bpc not in _recon_frames:
        seen = set()
        fr = test_mc_sweep.enumerated_frame(bpc, {64: 7, 32: 5, 16: 8, 8: 5, 4: 5}, 6, seed=8700 + bpc, transforms=stepped_transforms(bpc, seen))
        rng = np.random.default_rng(87 + bpc)
        refs = [synth.make_planes(rng, fr.w, fr.h, bpc, smooth=(i == 1)) for i in range(fr.n_refs)]
        dst0 = synth.make_planes(rng, fr.w, fr.h, bpc, smooth=False)
        want, _, want_coef = test_frame.oracle_frame(util.default_oracle(), fr, dst0, refs)
        _recon_frames[bpc] = (fr, seen, refs, dst0, want, want_coef)
    return _recon_frames[bpc]


def assert_recon_coverage(seen, bpc):
    for tx in range(5):
        assert {(tp, e) for cls, t, tp, e in seen if t == tx} == set(type_and_eob_combos(tx, bpc)), "%s: not every (type, eob class)" % util.TX_NAMES[tx]
        for cls in (0, 1) if tx < 4 else (0,):
            assert {tp for c, t, tp, e in seen if (c, t) == (cls, tx)} == set(util.legal_txtps(tx)), "plane class %d, %s: not every type" % (cls, util.TX_NAMES[tx])
    assert not any(cls == 1 and t == 4 for cls, t, tp, e in seen)
    assert {scan_class(tp) for cls, t, tp, e in seen if t <= 2} == {"2d", "h", "v", "wht"} and (0, 3, 9) in {s[:3] for s in seen}      # H and V up to 16x16, IDTX at 32x32


def compare_frame(got, got_coef, want, want_coef, what):
    for pl in range(3):
        bad = np.argwhere(got[pl] != want[pl])
        if len(bad):
            raise AssertionError("%s: plane %d differs at (%d,%d): %d, the oracle has %d (%d px)" % (
                what, pl, bad[0][1], bad[0][0], got[pl][tuple(bad[0])], want[pl][tuple(bad[0])], len(bad)))
    assert np.array_equal(got_coef, want_coef), what + ": the coefficient arena is not zeroed like the reference's"


@pytest.mark.parametrize("fuse", [None, 0], ids=["default-paired", "two-kernels"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_recon_routes_over_every_type_and_eob_class(ctx, bpc, fuse, twin_refs):
    fr, seen, refs_h, dst0, want, want_coef = recon_frame_and_oracle(bpc)
    assert_recon_coverage(seen, bpc)
    if fuse is not None:
        ctx.set_option("recon_fuse", fuse)
    mask = ctx.get_option("recon_fuse") & 31
    assert mask == (15 if fuse is None else 0)
    for packed in (False, True):
        got, _, got_coef = test_frame.hip_frame(ctx, fr, dst0, refs_h, recon=True, packed=packed)
        compare_frame(got, got_coef, want, want_coef, "packed" if packed else "dense")
    if twin_refs != "native":          # which launches took the blocks
        counts = test_mc_sweep._launch_counts(ctx, fr, dst0, refs_h, want)
        paired = {4 << k: counts[k] for k in range(5)}
        expect = {pw: (n if mask >> synth.SQ_TX[pw] & 1 else 0) for pw, n in fr.blocks_by_size.items()}
        assert paired == expect, "blocks in the paired launches by size: %s, expected %s" % (paired, expect)
        if mask:
            assert sum(paired.values()) == len(fr.itx) - fr.blocks_by_size[64] and not any(counts[21:25])
        else:
            assert sum(counts[5:20]) > 0 and sum(counts[21:40]) == len(fr.itx)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_recon_residuals_onto_a_picture_in_its_twin_only(ctx, bpc):
    """the same frame in two lists run tiled-native: predictions first, which leave the picture in its twin ONLY, then a list of
    residuals alone, whose transform body reads the destination through the tiled twin (`tsrc` of itx_body)"""
    fr, seen, refs_h, dst0, want, want_coef = recon_frame_and_oracle(bpc)
    assert_recon_coverage(seen, bpc)
    refs = []
    for rp in refs_h:
        r = ctx.picture(fr.w, fr.h, api.LAYOUT_I420, bpc)
        for pl in range(3):
            r.upload(pl, rp[pl])
        r.retile()
        refs.append(r)
    dst = ctx.picture(fr.w, fr.h, api.LAYOUT_I420, bpc)
    for pl in range(3):
        dst.upload(pl, dst0[pl])
    prep = ctx.buffer(fr.prep_elems * 2)
    prep.zero()
    coef = ctx.buffer_from(fr.coef)
    none = np.zeros(0, api.ITX_TASK)
    pred = ctx.recon_list(dst, fr.mc, fr.comp, none)
    pred.run_tiled(dst, refs, prep, coef)
    assert dst.pic.twin_ok == api.TWIN_ONLY
    res = ctx.recon_list(dst, np.zeros(0, api.MC_TASK), np.zeros(0, api.COMP_TASK), fr.itx)
    res.run_tiled(dst, refs, prep, coef)
    assert dst.pic.twin_ok == api.TWIN_ONLY
    got = [dst.download(pl) for pl in range(3)]
    compare_frame(got, coef.download(fr.coef.dtype, len(fr.coef)), want, want_coef, "residuals onto the twin")
    pred.destroy(); res.destroy()
    for o in refs + [dst, prep, coef]:
        o.free()


# ------------------------------------------------------------------ 4. the intra routes

INTRA_ROUTES = {"paired": dict(paired=True), "two-lists": dict(paired=False), "flow": dict(paired=False, flow=True), "sb": dict(paired=False, sb=True)}


def shape_modes(tx):
    """the prediction modes legal for a block of the shape: filter intra stops at 32 x 32"""
    return list(range(14)) if max(util.TX_W[tx], util.TX_H[tx]) <= 32 else list(range(13))


def chroma_shape(t):
    """the transform shape of the chroma planes of a region whose luma is tiled by shape t: t itself where it fits 32 x 32, else halved"""
    if max(util.TX_W[t], util.TX_H[t]) <= 32:
        return t
    return [i for i in range(19) if (util.TX_W[i], util.TX_H[i]) == (util.TX_W[t] // 2, util.TX_H[t] // 2)][0]


def regions_per_shape(bpc):
    """so many 64 x 64 regions per shape that its luma blocks, and the chroma blocks of a shape that fits the chroma region, hold
    every (type, eob class) and every legal mode"""
    out = []
    for t in range(19):
        need = max(len(type_and_eob_combos(t, bpc)), len(shape_modes(t)))
        per = (64 // util.TX_W[t]) * (64 // util.TX_H[t])
        if chroma_shape(t) == t:
            per = min(per, 2 * (32 // util.TX_W[t]) * (32 // util.TX_H[t]))
        out.append(-(-need // per))
    return out


def make_shape_pass(bpc, seed, seen):
    """An intra pass in the manner of synth_frames.make_intra_pass on a 4:2:0 picture ten cells of 128 x 128 wide: one 64 x 64
    luma region per cell, so never two neighbours; regions_per_shape() of them per transform shape, each tiled by its shape in all
    three planes (chroma: chroma_shape), one transform per predicted block.  Block (i, j) of a region's grid goes into wave
    j + 2 i.  The top-right neighbours a block of height h reads are the h pixels after its own width: below the region's top row
    they lie in earlier waves only when h <= w, so a taller block has no top-right edge there; the bottom-left edge exists only left
    of the region.  Along the blocks of a (plane class, shape), whatever their region, the transform steps through
    type_and_eob_combos and the mode through the modes legal for the shape.  seen collects (plane class, tx, txtp, eob, mode)."""
    regions = [t for t, n in enumerate(regions_per_shape(bpc)) for _ in range(n)]
    cols = 10
    w, h = cols * 128, -(-len(regions) // cols) * 128
    geo = synth.plane_geometry(w, h, bpc, 1)
    waves, coef_parts, cf_off = {}, [], 0
    count = {}                      # (plane class, tx) -> blocks so far
    for r, t in enumerate(regions):
        gx, gy = (r % cols) * 128 + 64, (r // cols) * 128 + 64
        for pl in range(3):
            ss = 1 if pl else 0
            tx = chroma_shape(t) if pl else t
            bw, bh = util.TX_W[tx], util.TX_H[tx]
            kc, kr = (64 >> ss) // bw, (64 >> ss) // bh
            pwid, phei = w >> ss, h >> ss
            combos, modes = type_and_eob_combos(tx, bpc), shape_modes(tx)
            for irow in range(kr):
                for jcol in range(kc):
                    n = count.get((ss, tx), 0)
                    count[ss, tx] = n + 1
                    bx, by = (gx >> ss) + jcol * bw, (gy >> ss) + irow * bh
                    pt = np.zeros(1, api.IPRED_TASK)[0]
                    pt["dst_off"] = by * geo[pl][0] + bx
                    pt["x4"], pt["y4"], pt["w4"], pt["h4"] = bx // 4, by // 4, pwid // 4, phei // 4
                    pt["tw"], pt["th"] = bw // 4, bh // 4
                    mode = modes[n % len(modes)]
                    pt["mode"] = mode
                    pt["angle"] = (n // 3) % 7 - 3 if 1 <= mode <= 8 else (n // 3) % 5 if mode == 13 else 0
                    top_right = irow == 0 or (jcol + 1 < kc and bh <= bw)
                    pt["flags"] = 1 + 2 + top_right * 4 + (jcol == 0 and irow + 1 < kr) * 8 + 16 + (n & 1) * 32
                    pt["plane"], pt["kind"] = pl, 0
                    pt["max_w"], pt["max_h"] = pwid - bx, phei - by
                    txtp, eob = combos[n % len(combos)]
                    cf, _ = make_coefs(tx, txtp, eob, bpc)
                    it = np.zeros(1, api.ITX_TASK)[0]
                    it["dst_off"], it["cf_off"], it["eob"], it["tx"], it["txtp"], it["plane"] = pt["dst_off"], cf_off, eob, tx, txtp, pl
                    coef_parts.append(cf)
                    cf_off += len(cf)
                    seen.add((ss, tx, txtp, eob, mode))
                    a, b = waves.setdefault(jcol + 2 * irow, ([], []))
                    a.append(pt); b.append(it)
    p = synth.IntraPass()
    p.batches = [(np.array(waves[d][0], api.IPRED_TASK), np.array(waves[d][1], api.ITX_TASK)) for d in sorted(waves)]
    p.coef = np.concatenate(coef_parts)
    p.w, p.h = w, h
    return p


def assert_shape_pass_coverage(seen, bpc):
    """luma: all 19 shapes; chroma: the 14 shapes that fit its 32 x 32 region.  Each with EVERY (legal type, eob class) of
    type_and_eob_combos -- eob 0, 1, both sides of the first and of the last piece change, the last -- and every legal mode."""
    fits = [tx for tx in range(19) if chroma_shape(tx) == tx]
    assert len(fits) == 14 and {tx for cls, tx, tp, e, m in seen if cls == 1} == set(fits) and {tx for cls, tx, tp, e, m in seen if cls == 0} == set(range(19))
    for cls, shapes in ((0, range(19)), (1, fits)):
        for tx in shapes:
            mine = [s for s in seen if s[:2] == (cls, tx)]
            assert {(tp, e) for _, _, tp, e, m in mine} == set(type_and_eob_combos(tx, bpc)), "plane class %d, %s: not every (type, eob class)" % (cls, util.TX_NAMES[tx])
            assert {tp for _, _, tp, e, m in mine if e == N_COEF[tx] - 1} == set(util.legal_txtps(tx)) - {util.WHT_WHT}, "plane class %d, %s: not every type with a full block" % (cls, util.TX_NAMES[tx])
            assert {m for _, _, tp, e, m in mine} == set(shape_modes(tx)), "plane class %d, %s: not every mode" % (cls, util.TX_NAMES[tx])


_shape_passes = {}


@pytest.mark.parametrize("route", list(INTRA_ROUTES))
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_intra_routes_over_every_size_and_type(ctx, bpc, route):
    import test_postchain
    if bpc not in _shape_passes:
        seen = set()
        ip = make_shape_pass(bpc, 8600 + bpc, seen)
        rng = np.random.default_rng(86 + bpc)
        planes = synth.make_planes(rng, ip.w, ip.h, bpc, smooth=True)
        want = synth.copy_planes(planes)
        test_postchain.oracle_intra(util.default_oracle(), ip, want, ip.w, ip.h, bpc)
        _shape_passes[bpc] = (ip, seen, planes, want)
    ip, seen, planes, want = _shape_passes[bpc]
    assert_shape_pass_coverage(seen, bpc)
    pic = ctx.picture(ip.w, ip.h, api.LAYOUT_I420, bpc)
    for pl in range(3):
        pic.upload(pl, planes[pl])
    test_postchain.hip_intra(ctx, ip, pic, **INTRA_ROUTES[route])
    for pl in range(3):
        got = pic.download(pl)
        bad = np.argwhere(got != want[pl])
        if len(bad):
            yy, xx = bad[0]
            raise AssertionError("%s, %d bpc: plane %d differs at (%d,%d): %d, the oracle has %d (%d px)" % (route, bpc, pl, xx, yy, got[yy, xx], want[pl][yy, xx], len(bad)))
    pic.free()
