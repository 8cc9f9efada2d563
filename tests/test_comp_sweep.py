"""Compound prediction and blending, ENUMERATED: avg / w_avg / mask / w_mask / blend / blend_v / blend_h (csrc/comp.hip) and the fused
w_avg tile kind of the inter lists (MCT_WAVG, csrc/mc_body.h) against the oracle, byte for byte.

tests/test_mc.py::test_compound_matches_reference and tests/test_mcx.py::test_blend_matches_reference draw shapes, weights and masks
from a seed on an I400 picture; this module lists them, on planes 0, 1 and 2 of I400, I420 and I422 pictures whose pixels are random
before the call (a write outside a block shows).  What the rows cover is collected in a set FIRST and the set is asserted; every
condition is computed from the specification's arithmetic (src/mc_tmpl.c:628-794, restated here), never read from the code under test.

* test_every_kind_shape_and_argument — ctx.comp_batch.  The 24 legal compound shapes; hip: w_avg weight 1 .. 15 x shape, emu: every
  weight and every shape.  Both: mask with a constant mask of every value 0 .. 64 (rotating over the shapes) and a random mask per shape,
  w_mask ss 0 / 1 / 2 x sign 0 / 1 x shape, avg per shape; blend on its 10 shapes, blend_v and blend_h on their 34, blend masks holding
  every value 0 .. 64; the part of a blend_v / blend_h block outside (3 w / 4) x h resp. w x (3 h / 4) keeps its pixels.  Every kind on
  every (layout, plane).  Preps in the range mct produces.
* test_w_mask_thresholds_and_roundings — constructed prep pairs: |tmp1 - tmp2| at every threshold of m = 38 .. 64 and one LSB either
  side, both signs, near the bottom, the middle and the top of int16.  m >= 55 (the imin(..., 64) included) needs pairs OUTSIDE what
  prep makes from pixels (|diff| <= 4080 at 8 bit gives m <= 53; 16368 at 10 bit and 16380 at 12 bit give m <= 54): that is intended,
  w_mask_c is defined for any int16 pair.  Quads and pairs whose m values give every residue of the 4:2:0 sum mod 4 and of the 4:2:2 sum mod 2, each at sign 0 and 1.
* test_extremal_predictions — blocks of the smallest and the largest value the ORACLE's mct gives on the worst-case windows of
  test_mc_sweep (maximised over filters, phases and both tap sets), and of the int16 corners, in all pairings, against 0 and as
  checkerboards, through every compound kind; blends of pixel 0 / bitdepth_max pairings at every mask value.
* test_fused_weighted_compounds_in_lists — the production route: ctx.recon_list over a 4:2:0 frame of test_mc_sweep.enumerated_frame
  whose compounds are w_avg with every weight 1 .. 15 at every filter_2d (some stay avg, so that the waves of the paired launches mix
  all three kinds), raster / tiled / tiled-native references, recon_fuse at its default and at 0, against test_frame.oracle_frame; the
  number of fused compounds and the blocks of each paired launch are asserted.  One more run shares PREP blocks between compounds (that
  defeats fusing: the two-step route must give the oracle's pictures too), and one has worst-case windows in both references at
  weights 1 and 15.

Cost: DESIGN.md 11.  An emulator trap ends the pytest process: run this module in a pytest call of its own first."""
import numpy as np
import pytest

import util
import test_mc_sweep
import test_frame
import synth_frames as synth
from dav1d_amd import api

AVG, WAVG, MASK, WMASK, BLEND, BLEND_V, BLEND_H = range(7)
KIND_NAMES = ["avg", "w_avg", "mask", "w_mask", "blend", "blend_v", "blend_h"]
LAYOUT_PLANES = [(api.LAYOUT_I400, 0), (api.LAYOUT_I420, 0), (api.LAYOUT_I420, 1), (api.LAYOUT_I420, 2),
                 (api.LAYOUT_I422, 0), (api.LAYOUT_I422, 1), (api.LAYOUT_I422, 2)]
SIZES = [2, 4, 8, 16, 32, 64, 128]
COMP_SHAPES = [(w, h) for w in SIZES[1:] for h in SIZES[1:] if max(w // 4, 4) <= h <= min(4 * w, 128)]       # tests/checkasm/mc.c:297-299
BLEND_SHAPES = [(w, h) for w in (4, 8, 16, 32) for h in (4, 8, 16, 32) if max(w // 2, 4) <= h <= min(2 * w, 32)]           # :456-458
BLEND_V_SHAPES = [(w, h) for w in (2, 4, 8, 16, 32) for h in SIZES if h <= (64 if w == 2 else 128)]                        # :496-498
BLEND_H_SHAPES = [(w, h) for w in SIZES for h in (2, 4, 8, 16, 32) if h >= (4 if w == 128 else 2)]                         # :535-537
assert (len(COMP_SHAPES), len(BLEND_SHAPES), len(BLEND_V_SHAPES), len(BLEND_H_SHAPES)) == (24, 10, 34, 34)
GAP = 4                    # pixels between two blocks of a destination plane
PIC_W, PIC_H = 1536, 1024  # multiples of 128: the allocation has no padding of its own


def inter_bits(bpc):
    return 4 if bpc == 8 else 14 - bpc


def prep_bias(bpc):
    return 0 if bpc == 8 else 8192


class Item:
    """one comp task: a / b = the two int16 predictions (a = the pixels of `tmp` for the blends), m = the mask read (mask, blend),
    fill = what the destination block holds before the call (None: the picture's random pixels)"""

    def __init__(self, kind, w, h, lp, a, b=None, m=None, arg=0, ss=0, fill=None, tag=None):
        self.kind, self.w, self.h, self.lp, self.a, self.b, self.m, self.arg, self.ss, self.fill, self.tag = kind, w, h, lp, a, b, m, arg, ss, fill, tag

    def __repr__(self):
        layout, pl = LAYOUT_PLANES[self.lp]
        return "%s %dx%d arg %d ss %d on plane %d of layout %d at (%d,%d)%s" % (KIND_NAMES[self.kind], self.w, self.h, self.arg, self.ss, pl, layout,
                                                                                self.x, self.y, " [%s]" % (self.tag,) if self.tag is not None else "")


def blend_extent(it):
    return ((it.w * 3) >> 2 if it.kind == BLEND_V else it.w), ((it.h * 3) >> 2 if it.kind == BLEND_H else it.h)


def run_items(ctx, oracle, bpc, items, seed, what, check=None):
    """items through the oracle's DSP entries on host planes, check(outs) on the oracle's outputs alone ([(block, w_mask output or
    None)]), then through ctx.comp_batch (compounds and blends in a call each per picture: their arenas differ in type) and compared."""
    pd = util.pix_dtype(bpc)
    rng = np.random.default_rng(seed)
    pics, pre = {}, {}
    for layout in sorted({LAYOUT_PLANES[it.lp][0] for it in items}):
        pics[layout] = ctx.picture(PIC_W, PIC_H, layout, bpc)
        pre[layout] = [rng.integers(0, 1 << bpc, size=pics[layout].padded_shape(pl)).astype(pd) for pl in range(pics[layout].n_planes)]
    cur = {}
    for i in sorted(range(len(items)), key=lambda i: (items[i].lp, -items[i].h, -items[i].w)):         # shelves of one height
        it = items[i]
        layout, pl = LAYOUT_PLANES[it.lp]
        ph, pw = pre[layout][pl].shape
        x, y, shelf = cur.get(it.lp, (0, 0, 0))
        if x + it.w > pw:
            x, y, shelf = 0, y + shelf + GAP, 0
        assert y + it.h <= ph, "the destination picture is too small for the rows"
        it.x, it.y = x, y
        cur[it.lp] = (x + it.w + GAP, y, max(shelf, it.h))
        if it.fill is not None:
            pre[layout][pl][y:y + it.h, x:x + it.w] = it.fill
    want = {layout: [p.copy() for p in planes] for layout, planes in pre.items()}
    outs = []
    for it in items:
        layout, pl = LAYOUT_PLANES[it.lp]
        plane = want[layout][pl]
        d, ds, w, h = plane[it.y:, it.x:].ctypes.data, plane.strides[0], it.w, it.h
        mo = None
        if it.kind == AVG:
            oracle.call(bpc, "avg", 0, 0, d, ds, it.a, it.b, w, h)
        elif it.kind == WAVG:
            oracle.call(bpc, "w_avg", 0, 0, d, ds, it.a, it.b, w, h, it.arg)
        elif it.kind == MASK:
            oracle.call(bpc, "mask", 0, 0, d, ds, it.a, it.b, w, h, it.m)
        elif it.kind == WMASK:
            mo = np.zeros(w * h, np.uint8)
            oracle.call(bpc, "w_mask", it.ss, 0, d, ds, it.a, it.b, w, h, mo, it.arg)
        elif it.kind == BLEND:
            oracle.call(bpc, "blend", 0, 0, d, ds, it.a, w, h, it.m)
        else:
            oracle.call(bpc, "blend_v" if it.kind == BLEND_V else "blend_h", 0, 0, d, ds, it.a, w, h)
        outs.append((plane[it.y:it.y + h, it.x:it.x + w].copy(), mo))
    if check is not None:
        check(outs)
    for layout, pic in pics.items():
        for pl in range(pic.n_planes):
            pic.upload(pl, pre[layout][pl])
        mine = [(i, it) for i, it in enumerate(items) if LAYOUT_PLANES[it.lp][0] == layout]
        for blends in (False, True):
            group = [(i, it) for i, it in mine if (it.kind >= BLEND) == blends]
            if not group:
                continue
            tasks = np.zeros(len(group), api.COMP_TASK)
            parts, masks = [], []
            off = moff = 0
            for k, (i, it) in enumerate(group):
                n = it.w * it.h
                pl = LAYOUT_PLANES[it.lp][1]
                assert it.a.dtype == (pd if blends else np.int16) and it.a.size == n
                tasks[k] = (it.y * pic.stride_px(pl) + it.x, off, 0 if blends else off + n, moff, it.w, it.h, it.kind, pl, it.arg, it.ss, 0)
                parts += [it.a.ravel()] if blends else [it.a.ravel(), it.b.ravel()]
                masks.append(np.zeros(n, np.uint8) if it.m is None else it.m.ravel())
                it.moff = moff
                off += n if blends else 2 * n
                moff += n
            arena, dmask = ctx.buffer_from(np.concatenate(parts)), ctx.buffer_from(np.concatenate(masks))
            ctx.comp_batch(pic, tasks, arena, dmask)
            got_mask = dmask.download(np.uint8, moff)
            for k, (i, it) in enumerate(group):
                n = it.w * it.h
                if it.kind == WMASK:         # only the sub-sampled part of a w_mask output is defined
                    n = (it.w >> (1 if it.ss else 0)) * (it.h >> (1 if it.ss == 2 else 0))
                w_ = outs[i][1][:n] if it.kind == WMASK else masks[k]
                bad = np.flatnonzero(got_mask[it.moff:it.moff + n] != w_[:n])
                assert not len(bad), "%s, %d bpc: mask element %d of %r is %d, the oracle has %d (%d differ)" % (
                    what, bpc, bad[0], it, got_mask[it.moff + bad[0]], w_[bad[0]], len(bad))
            arena.free(); dmask.free()
        for pl in range(pic.n_planes):
            got = pic.download(pl)
            bad = np.argwhere(got != want[layout][pl])
            if len(bad):
                yy, xx = bad[0]
                hit = [it for i, it in mine if LAYOUT_PLANES[it.lp][1] == pl and it.x <= xx < it.x + it.w and it.y <= yy < it.y + it.h]
                raise AssertionError("%s, %d bpc: (%d,%d) of plane %d, layout %d is %d, the oracle has %d (before the call: %d); %d pixels differ; task: %r" % (
                    what, bpc, xx, yy, pl, layout, got[yy, xx], want[layout][pl][yy, xx], pre[layout][pl][yy, xx], len(bad), hit[0] if hit else "none: outside every block"))
            for i, it in mine:               # blend_v / blend_h leave the last quarter of the block alone
                if it.kind in (BLEND_V, BLEND_H) and LAYOUT_PLANES[it.lp][1] == pl:
                    ww, hh = blend_extent(it)
                    keep = np.ones((it.h, it.w), bool)
                    keep[:hh, :ww] = False
                    blk = slice(it.y, it.y + it.h), slice(it.x, it.x + it.w)
                    assert np.array_equal(got[blk][keep], pre[layout][pl][blk][keep]), "%s: %r wrote outside %d x %d" % (what, it, ww, hh)
        pic.free()
    return outs


def mct_range_preps(rng, bpc, n):
    """the values prep produces from pixels, src/mc_tmpl.c:41-48"""
    return ((rng.integers(0, 1 << bpc, size=n) << inter_bits(bpc)) - prep_bias(bpc)).astype(np.int16)


# ------------------------------------------------------------------ 1. every kind, shape and argument

def compound_rows(full):
    """[(kind, w, h, arg, ss, constant mask value or None)]"""
    rows = []
    if full:
        rows += [(WAVG, w, h, wt, 0, None) for wt in range(1, 16) for w, h in COMP_SHAPES]
    else:
        rows += [(WAVG, w, h, 1 + s % 15, 0, None) for s, (w, h) in enumerate(COMP_SHAPES)]
    rows += [(MASK,) + COMP_SHAPES[m % len(COMP_SHAPES)] + (0, 0, m) for m in range(65)]
    rows += [(MASK, w, h, 0, 0, None) for w, h in COMP_SHAPES]
    rows += [(WMASK, w, h, sign, ss, None) for ss in range(3) for sign in range(2) for w, h in COMP_SHAPES]
    rows += [(AVG, w, h, 0, 0, None) for w, h in COMP_SHAPES]
    return rows


def blend_rows():
    return [(BLEND, w, h, 0, 0, None) for w, h in BLEND_SHAPES] + [(BLEND_V, w, h, 0, 0, None) for w, h in BLEND_V_SHAPES] + \
           [(BLEND_H, w, h, 0, 0, None) for w, h in BLEND_H_SHAPES]


def assert_row_coverage(rows, full):
    ran = set(rows)
    weights = {(r[3], r[1], r[2]) for r in ran if r[0] == WAVG}
    assert {wt for wt, _, _ in weights} == set(range(1, 16)), "every w_avg weight"
    if full:
        assert weights == {(wt, w, h) for wt in range(1, 16) for w, h in COMP_SHAPES}, "w_avg: weight x shape"
    assert {(r[0], r[1], r[2]) for r in ran if r[0] <= WMASK} == {(k, w, h) for k in range(4) for w, h in COMP_SHAPES}, "every (kind, shape)"
    assert {(r[4], r[3], r[1], r[2]) for r in ran if r[0] == WMASK} == {(ss, sg, w, h) for ss in range(3) for sg in range(2) for w, h in COMP_SHAPES}, \
        "w_mask: ss x sign x shape"
    assert {r[5] for r in ran if r[0] == MASK and r[5] is not None} == set(range(65)), "a constant mask of every value"
    assert {(r[1], r[2]) for r in ran if r[0] == MASK and r[5] is not None} == set(COMP_SHAPES), "... over every shape"
    assert {(r[1], r[2]) for r in ran if r[0] == MASK and r[5] is None} == set(COMP_SHAPES), "a random mask on every shape"
    for kind, shapes in ((BLEND, BLEND_SHAPES), (BLEND_V, BLEND_V_SHAPES), (BLEND_H, BLEND_H_SHAPES)):
        assert {(r[1], r[2]) for r in ran if r[0] == kind} == set(shapes), KIND_NAMES[kind]
    # the widths and heights at which 3/4 of the side is odd or 1 (src/mc_tmpl.c:700, 715)
    assert (2, 2) in BLEND_V_SHAPES and (2, 2) in BLEND_H_SHAPES and (2 * 3) >> 2 == 1


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_kind_shape_and_argument(ctx, bpc):
    oracle = util.default_oracle()
    full = ctx.backend != "emu"
    rows = compound_rows(full) + blend_rows()
    assert_row_coverage(rows, full)
    rng = np.random.default_rng(7100 + bpc)
    pd = util.pix_dtype(bpc)
    items, blend_mask_values = [], set()
    for k, (kind, w, h, arg, ss, cm) in enumerate(rows):
        n = w * h
        lp = k % len(LAYOUT_PLANES)
        if kind <= WMASK:
            m = None
            if kind == MASK:
                m = np.full(n, cm, np.uint8) if cm is not None else rng.integers(0, 65, size=n).astype(np.uint8)
            items.append(Item(kind, w, h, lp, mct_range_preps(rng, bpc, n), mct_range_preps(rng, bpc, n), m, arg, ss))
        else:
            m = None
            if kind == BLEND:               # a ramp through 0 .. 64 from a start that moves, mixed with random values
                m = np.where(rng.integers(0, 2, size=n) == 1, (np.arange(n) * 7 + 13 * k) % 65, rng.integers(0, 65, size=n)).astype(np.uint8)
                blend_mask_values |= set(m.tolist())
            items.append(Item(kind, w, h, lp, rng.integers(0, 1 << bpc, size=n).astype(pd), None, m))
    assert blend_mask_values == set(range(65)), "blend masks hold every value 0 .. 64"
    assert {(it.kind, it.lp) for it in items} == {(k, lp) for k in range(7) for lp in range(len(LAYOUT_PLANES))}, "every kind on every (layout, plane)"
    run_items(ctx, oracle, bpc, items, 7200 + bpc, "every kind, shape and argument")


# ------------------------------------------------------------------ 2. w_mask thresholds and roundings

def w_mask_shift(bpc):
    mask_sh = bpc + inter_bits(bpc) - 4
    return mask_sh, 1 << (mask_sh - 5)


def spec_m(t1, t2, bpc):
    """src/mc_tmpl.c:741-742, restated"""
    mask_sh, mask_rnd = w_mask_shift(bpc)
    return np.minimum(38 + ((np.abs(t1.astype(np.int64) - t2.astype(np.int64)) + mask_rnd) >> mask_sh), 64)


def pair_with_diff(ad, negative, base):
    """(tmp1, tmp2) with |tmp1 - tmp2| == ad; base -1 / 0 / 1: the smaller of the two at the bottom of int16, the two around 0, the
    larger at the top"""
    lo = {-1: -32768, 0: -(ad // 2), 1: 32767 - ad}[base]
    return (lo, lo + ad) if negative else (lo + ad, lo)


def threshold_block(bpc, rng):
    """a 32 x 32 block: the threshold pairs, then quads for the sub-sampled roundings, then preps as made from random pixels"""
    mask_sh, mask_rnd = w_mask_shift(bpc)
    W = 32
    t1, t2 = (mct_range_preps(rng, bpc, W * W).reshape(W, W) for _ in range(2))       # m <= 54: only the constructed pairs go further
    pairs, seen = [], set()
    for k in range(27):
        for d in (-1, 0, 1):
            ad = (k << mask_sh) - mask_rnd + d
            if ad < 0:
                continue
            for negative in (False, True):
                for base in (-1, 0, 1):
                    pairs.append(pair_with_diff(ad, negative, base))
                    seen.add((k, d, negative, base))
    for ad in ((27 << mask_sh) - mask_rnd, 40 << mask_sh, 65535):            # past the clamp, up to the largest difference of two int16
        pairs += [pair_with_diff(ad, negative, -1) for negative in (False, True)]
    assert seen >= {(k, d, ng, b) for k in range(1, 27) for d in (-1, 0, 1) for ng in (False, True) for b in (-1, 0, 1)} and (0, 0, False, 0) not in seen
    assert max(abs(a - b) for a, b in pairs) == 65535 and all(-32768 <= v <= 32767 for p in pairs for v in p)
    rows = (len(pairs) + W - 1) // W
    flat1, flat2 = t1[:rows].reshape(-1), t2[:rows].reshape(-1)
    flat1[:len(pairs)], flat2[:len(pairs)] = [p[0] for p in pairs], [p[1] for p in pairs]
    # quads (m, .., m + 1, ..) with r values of m + 1: the 4:2:0 sum is r mod 4, their rows are the 4:2:2 pairs (m, m), (m, m + 1), (m + 1, m + 1)
    qi = 0
    for k0 in (0, 13, 25):
        for r in range(4):
            for j, e in enumerate([0] * (4 - r) + [1] * r):
                ad = max(((k0 + e) << mask_sh) - mask_rnd, 0)
                a, b = pair_with_diff(ad, bool((qi + j) & 1), (-1, 0, 1)[qi % 3])
                t1[rows + (rows & 1) + (j >> 1), 2 * qi + (j & 1)], t2[rows + (rows & 1) + (j >> 1), 2 * qi + (j & 1)] = a, b
            qi += 1
    assert rows + (rows & 1) + 2 <= W and 2 * qi <= W
    return t1, t2


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_w_mask_thresholds_and_roundings(ctx, bpc):
    """The rows with m >= 55 (m == 64 and its clamp among them) are int16 pairs that mct cannot produce; the reference is defined for
    them (65535 * 64 fits an int) and so are the kernels."""
    oracle = util.default_oracle()
    rng = np.random.default_rng(7300 + bpc)
    t1, t2 = threshold_block(bpc, rng)
    W = t1.shape[0]
    m = spec_m(t1, t2, bpc)
    assert set(m.ravel().tolist()) == set(range(38, 65)), "the pairs give every m 38 .. 64 by the specification's arithmetic"
    mask_sh, mask_rnd = w_mask_shift(bpc)
    assert (np.abs(t1.astype(np.int64) - t2) + mask_rnd >= 27 << mask_sh).any(), "... and some would give m > 64 without the clamp"
    quads = m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]
    assert set((quads % 4).ravel().tolist()) == {0, 1, 2, 3}, "4:2:0: every residue of the sum, at sign 0 and at sign 1 (a task each)"
    assert set(((m[:, 0::2] + m[:, 1::2]) % 2).ravel().tolist()) == {0, 1}, "4:2:2: both residues"
    from_pixels = np.array([0, (1 << bpc) - 1]) * (1 << inter_bits(bpc)) - prep_bias(bpc)
    assert spec_m(from_pixels[1:], from_pixels[:1], bpc)[0] == (53 if bpc == 8 else 54), "preps made from pixels stop at m == 53 / 54"
    items = [Item(WMASK, W, W, (3 * ss + sign) % len(LAYOUT_PLANES), t1.ravel(), t2.ravel(), None, sign, ss, tag="ss %d sign %d" % (ss, sign))
             for ss in range(3) for sign in range(2)]
    bdmax = (1 << bpc) - 1

    def check(outs):
        by = {(it.ss, it.arg): o for it, o in zip(items, outs)}
        for sign in range(2):
            assert set(by[0, sign][1].tolist()) == set(range(38, 65)), "the oracle's 4:4:4 masks hold every value 38 .. 64"
            assert np.array_equal(by[0, sign][1].reshape(W, W), m), "... the ones the restated arithmetic gives"
        assert (by[1, 0][1][:W * W // 2] != by[1, 1][1][:W * W // 2]).any(), "the oracle's 4:2:2 masks of sign 0 and 1 differ"
        assert (by[2, 0][1][:W * W // 4] != by[2, 1][1][:W * W // 4]).any(), "the oracle's 4:2:0 masks of sign 0 and 1 differ"
        for blk, _ in outs:
            assert blk.min() == 0 and blk.max() == bdmax, "the oracle's pixels hold both clips"

    run_items(ctx, oracle, bpc, items, 7400 + bpc, "w_mask thresholds", check)


# ------------------------------------------------------------------ 3. extremal predictions

_tap_signs = []
_mct_range = {}


def tap_signs(oracle):
    if not _tap_signs:
        _tap_signs.append(test_mc_sweep.oracle_tap_signs(oracle))
    return _tap_signs[0]


def oracle_mct_range(oracle, bpc):
    """(smallest, largest) value of the oracle's mct over the worst-case windows of every (filter_2d, mx, my) and both tap sets"""
    if bpc not in _mct_range:
        signs = tap_signs(oracle)
        bdmax = (1 << bpc) - 1
        pd = util.pix_dtype(bpc)
        lo, hi = 1 << 20, -(1 << 20)
        tmp = np.zeros(8 * 8, np.int16)
        src = np.zeros((24, 24), pd)
        for f in range(10):
            for bw, bh in ((0, 0), (0, 1), (1, 0), (1, 1)):
                for mx in range(16):
                    sh = signs[f, 0, bw, mx].astype(np.int32)
                    for my in range(16):
                        prod = signs[f, 1, bh, my].astype(np.int32)[:, None] * sh[None, :]
                        for positive in (True, False):
                            src[5:13, 5:13] = np.where(prod > 0 if positive else prod < 0, bdmax, 0)
                            oracle.call(bpc, "mct", f, 0, tmp.ctypes.data, src.ctypes.data + (8 * 24 + 8) * src.itemsize, src.strides[0],
                                        8 if bw else 4, 8 if bh else 4, mx, my)
                            lo, hi = min(lo, int(tmp[0])), max(hi, int(tmp[0]))
        _mct_range[bpc] = (lo, hi)
    return _mct_range[bpc]


def extremal_fills(lo, hi, w, h):
    """[(name, tmp1, tmp2)]"""
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.where((yy + xx) & 1, hi, lo)
    const = lambda v: np.full((h, w), v)
    out = [("%d|%d" % (a, b), const(a), const(b)) for a in (lo, hi) for b in (lo, hi)]
    out += [("%d|0" % v, const(v), const(0)) for v in (lo, hi)] + [("0|%d" % v, const(0), const(v)) for v in (lo, hi)]
    out += [("checker|checker", checker, checker), ("checker|inverse", checker, lo + hi - checker)]
    return [(n, a.astype(np.int16).ravel(), b.astype(np.int16).ravel()) for n, a, b in out]


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_extremal_predictions(ctx, bpc):
    oracle = util.default_oracle()
    bdmax = (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    lo, hi = oracle_mct_range(oracle, bpc)
    # more than the pixel range on either side: the sharp filters overshoot
    assert lo < -prep_bias(bpc) and hi > (bdmax << inter_bits(bpc)) - prep_bias(bpc), (lo, hi)
    variants = [(AVG, 0, 0, None)] + [(WAVG, wt, 0, None) for wt in (1, 8, 15)] + [(MASK, 0, 0, m) for m in (0, 1, 32, 63, 64)] + \
               [(WMASK, sign, ss, None) for ss in range(3) for sign in range(2)]
    shapes = [(8, 8), (4, 16), (16, 4)]
    items = []
    for rng_name, (a, b) in (("mct", (lo, hi)), ("int16", (-32768, 32767))):
        for vi, (kind, arg, ss, cm) in enumerate(variants):
            for fi in range(10):
                w, h = shapes[(vi + fi) % 3]
                name, t1, t2 = extremal_fills(a, b, w, h)[fi]
                items.append(Item(kind, w, h, len(items) % len(LAYOUT_PLANES), t1, t2, None if cm is None else np.full(w * h, cm, np.uint8), arg, ss,
                                  tag="%s %s" % (rng_name, name)))
    assert len({(it.kind, it.arg, it.ss, it.tag, None if it.m is None else int(it.m[0])) for it in items}) == 2 * 15 * 10
    n_comp = len(items)
    for m in range(65):
        for d in (0, bdmax):
            for t in (0, bdmax):
                items.append(Item(BLEND, 4, 4, len(items) % len(LAYOUT_PLANES), np.full(16, t, pd), None, np.full(16, m, np.uint8), fill=d, tag="dst %d tmp %d m %d" % (d, t, m)))
    for kind, (w, h) in [(k, s) for k in (BLEND_V, BLEND_H) for s in ((2, 2), (8, 8), (32, 16))]:
        for d in (0, bdmax):
            for t in (0, bdmax):
                items.append(Item(kind, w, h, len(items) % len(LAYOUT_PLANES), np.full(w * h, t, pd), None, None, fill=d, tag="dst %d tmp %d" % (d, t)))

    def check(outs):
        for part, what in ((outs[:n_comp], "compound"), (outs[n_comp:], "blend")):
            assert min(b.min() for b, _ in part) == 0 and max(b.max() for b, _ in part) == bdmax, "the oracle's %s outputs hold both clips" % what
        # both clips by clipping, not by hitting the end exactly: avg_c (src/mc_tmpl.c:628-640) of (max, max) is above bitdepth_max, of (min, min) below 0
        avg = lambda v: (2 * v + (1 << inter_bits(bpc)) + 2 * prep_bias(bpc)) >> (inter_bits(bpc) + 1)
        assert avg(hi) > bdmax and avg(lo) < 0, (avg(lo), avg(hi))

    run_items(ctx, oracle, bpc, items, 7500 + bpc, "extremal predictions", check)


# ------------------------------------------------------------------ 4. fused w_avg in the lists (the production route)

FUSED_REGIONS = {64: 8, 32: 8, 16: 8, 8: 8}        # 512 x 256: 170 luma compounds and their chroma blocks


def weighted(per_filter):
    """the `compound` argument of test_mc_sweep.enumerated_frame: per filter_2d, weights 1 .. 15 in turn and then one avg"""
    def pick(serial, f):
        c = per_filter.get(f, 0)
        per_filter[f] = c + 1
        return (WAVG, 1 + c % 16) if c % 16 < 15 else (AVG, 0)
    return pick


_fused = {}


def _fused_frame(bpc):
    if bpc not in _fused:
        fr = test_mc_sweep.enumerated_frame(bpc, FUSED_REGIONS, 8, seed=700 + bpc, compound=weighted({}))
        rng = np.random.default_rng(71 + bpc)
        refs = [synth.make_planes(rng, fr.w, fr.h, bpc, smooth=(i == 1)) for i in range(fr.n_refs)]
        dst0 = synth.make_planes(rng, fr.w, fr.h, bpc, smooth=False)
        want, _, want_coef = test_frame.oracle_frame(util.default_oracle(), fr, dst0, refs)
        _fused[bpc] = (fr, refs, dst0, want, want_coef)
    return _fused[bpc]


def assert_weighted_coverage(fr):
    comp, mc = fr.comp, fr.mc
    prep = {int(t["dst_off"]): t for t in mc[mc["kind"] == 1]}
    pairs, sizes, outside = set(), set(), 0
    for c in comp[comp["kind"] == WAVG]:
        a, b = prep[int(c["tmp1_off"])], prep[int(c["tmp2_off"])]
        assert a["filter_2d"] == b["filter_2d"]
        pairs.add((int(c["arg"]), int(a["filter_2d"])))
        sizes.add((int(c["plane"]) > 0, int(c["w"])))
        for t in (a, b):
            pw, ph = (fr.w, fr.h) if t["plane"] == 0 else (fr.w // 2, fr.h // 2)
            outside += int(t["src_x"] < 3 or t["src_y"] < 3 or t["src_x"] + t["w"] + 4 > pw or t["src_y"] + t["h"] + 4 > ph)
    assert pairs == {(wt, f) for wt in range(1, 16) for f in range(10)}, "every weight 1 .. 15 meets every filter_2d: %d of 150" % len(pairs)
    assert sizes == {(False, s) for s in (8, 16, 32, 64)} | {(True, s) for s in (4, 8, 16, 32)}, "w_avg on every luma and chroma size"
    n_w = int((comp["kind"] == WAVG).sum())
    assert 0.05 * n_w < outside < n_w, "a share of the sources leaves the picture"
    assert 0 < int((comp["kind"] == AVG).sum()) < n_w / 8, "some compounds stay avg"
    assert set(comp["kind"].tolist()) == {AVG, WAVG}
    assert sum(1 for _, a, b in fr.comp_seen if a != b) > 0.9 * len(fr.comp_seen), "independent phases of the two references"


def _compare_frame(fr, got, want, got_coef, want_coef, what):
    for pl in range(3):
        bad = np.argwhere(got[pl] != want[pl])
        if len(bad):
            yy, xx = bad[0]
            sp = got[pl].strides[0] // got[pl].itemsize
            hit = []
            lst = fr.comp[fr.comp["plane"] == pl]
            x, y = lst["dst_off"] % sp, lst["dst_off"] // sp
            for c in lst[(x <= xx) & (xx < x + lst["w"]) & (y <= yy) & (yy < y + lst["h"])]:
                srcs = fr.mc[(fr.mc["kind"] == 1) & np.isin(fr.mc["dst_off"], [c["tmp1_off"], c["tmp2_off"]])]
                hit.append((KIND_NAMES[int(c["kind"])], "weight %d" % c["arg"], "%dx%d" % (c["w"], c["h"]),
                            [tuple(int(s[k]) for k in ("filter_2d", "mx", "my", "src_x", "src_y", "ref")) for s in srcs]))
            raise AssertionError("%s: plane %d differs at (%d,%d): %d, the oracle has %d (%d px); compounds there: %s; other blocks: %s" % (
                what, pl, xx, yy, got[pl][yy, xx], want[pl][yy, xx], len(bad), hit, test_mc_sweep._blocks_at(fr, pl, xx, yy, sp) if not hit else "-"))
    assert np.array_equal(got_coef, want_coef), what + ": coefficients"


@pytest.mark.parametrize("fuse", [None, 0], ids=["default-paired", "two-kernels"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_fused_weighted_compounds_in_lists(ctx, bpc, fuse, twin_refs):
    fr, refs_h, dst0, want, want_coef = _fused_frame(bpc)
    assert_weighted_coverage(fr)
    if fuse is not None:
        ctx.set_option("recon_fuse", fuse)
    mask = ctx.get_option("recon_fuse") & 31
    assert mask == (15 if fuse is None else 0)
    il = ctx.inter_list(fr.mc, fr.comp)
    n_fused = il.n_fused
    il.destroy()
    assert n_fused == len(fr.comp), "every avg and w_avg compound is fused with its two predictions: %d of %d" % (n_fused, len(fr.comp))
    got, _, got_coef = test_frame.hip_frame(ctx, fr, dst0, refs_h, recon=True)
    _compare_frame(fr, got, want, got_coef, want_coef, "weighted compounds")
    if twin_refs != "native":
        counts = test_mc_sweep._launch_counts(ctx, fr, dst0, refs_h, want)
        paired = {4 << k: counts[k] for k in range(5)}
        expect = {pw: (n if mask >> synth.SQ_TX[pw] & 1 else 0) for pw, n in fr.blocks_by_size.items()}
        expect.setdefault(64, 0)
        assert paired == expect, "blocks in the paired launches by size: %s, expected %s" % (paired, expect)
        if mask:
            assert sum(paired.values()) == len(fr.itx) - fr.blocks_by_size[64] and not any(counts[21:25]), "4x4 .. 32x32 all went through the paired launches"
        else:
            assert sum(counts[5:20]) > 0 and sum(counts[21:40]) == len(fr.itx)


def shared_prep_variant(fr):
    """a copy of the frame in which, of every four w_avg compounds of one plane and size, the second reads the first one's first PREP
    block instead of its own: two readers of one block, so neither compound can be fused.  Returns (frame, compounds un-fused)."""
    import copy
    out = copy.copy(fr)
    out.comp = fr.comp.copy()
    groups = {}
    for i, c in enumerate(out.comp):
        if c["kind"] == WAVG:
            groups.setdefault((int(c["plane"]), int(c["w"])), []).append(i)
    n = 0
    for idx in groups.values():
        for g in range(0, len(idx) - 1, 4):
            out.comp[idx[g + 1]]["tmp1_off"] = out.comp[idx[g]]["tmp1_off"]
            n += 2
    return out, n


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_fused_weighted_compounds_in_lists_shared_prep(ctx, bpc):
    """(the extra run of test_fused_weighted_compounds_in_lists) compounds whose PREP block has a second reader go the two-step route"""
    fr0, refs_h, dst0, _, _ = _fused_frame(bpc)
    fr, n_shared = shared_prep_variant(fr0)
    n_w = int((fr.comp["kind"] == WAVG).sum())
    assert 0.4 * n_w <= n_shared <= 0.5 * n_w + 8, "every second w_avg compound shares a PREP block with another one"
    il = ctx.inter_list(fr.mc, fr.comp)
    n_fused = il.n_fused
    il.destroy()
    assert n_fused == len(fr.comp) - n_shared, "fused: %d, expected %d - %d" % (n_fused, len(fr.comp), n_shared)
    want, _, want_coef = test_frame.oracle_frame(util.default_oracle(), fr, dst0, refs_h)
    got, _, got_coef = test_frame.hip_frame(ctx, fr, dst0, refs_h, recon=True)
    _compare_frame(fr, got, want, got_coef, want_coef, "compounds that share a PREP block")


EXT_TRIPLES = [(0, 8, 8), (2, 3, 13), (1, 15, 1), (5, 7, 0), (6, 0, 9), (9, 8, 8), (4, 4, 12), (8, 11, 5)]      # (filter_2d, mx, my)


def extremal_frame(bpc, signs):
    """128 x 128, 4:2:0: 16x16 luma blocks with their 8x8 chroma blocks, each a w_avg compound of weight 1 or 15 whose two references
    hold, over the block's own area, the worst-case window of the block's (filter_2d, mx, my) with the period of the window (8): the
    output pixels at multiples of 8 see exactly that window in both references.  Residuals are zero."""
    w = h = 128
    geo = synth.plane_geometry(w, h, bpc, 1)
    bdmax = (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    refs = [synth.make_planes(np.random.default_rng(0), w, h, bpc, smooth=False) for _ in range(2)]      # (views with the device's row stride)
    for planes in refs:
        for p in planes:
            p[:] = 0
    mc, comp, itx = [], [], []
    prep_off = cf_off = 0
    n = 0
    for pl, s in ((0, 16), (1, 8), (2, 8)):
        pw = w if pl == 0 else w // 2
        for by in range(0, pw, s):
            for bx in range(0, pw, s):
                f, mx, my = EXT_TRIPLES[n % len(EXT_TRIPLES)]
                positive = bool((n // len(EXT_TRIPLES)) & 1)
                prod = signs[f, 1, 1, my].astype(np.int32)[:, None] * signs[f, 0, 1, mx].astype(np.int32)[None, :]
                win = np.where(prod > 0 if positive else prod < 0, bdmax, 0).astype(pd)
                # the window of output pixel (0, 0) starts 3 columns and rows before the block: roll the tiling by 3 (s is a multiple of 8)
                tile = np.roll(np.tile(win, (s // 8, s // 8)), (3, 3), axis=(0, 1))
                ct = np.zeros(1, api.COMP_TASK)[0]
                ct["dst_off"], ct["w"], ct["h"], ct["plane"], ct["kind"], ct["arg"] = by * geo[pl][0] + bx, s, s, pl, WAVG, (1, 15)[(n // 3) & 1]
                for r in range(2):
                    refs[r][pl][by:by + s, bx:bx + s] = tile
                    e = np.zeros(1, api.MC_TASK)[0]
                    e["src_x"], e["src_y"], e["w"], e["h"], e["mx"], e["my"], e["filter_2d"] = bx, by, s, s, mx, my, f
                    e["plane"], e["ref"], e["kind"], e["dst_off"] = pl, r, 1, prep_off
                    ct["tmp1_off" if r == 0 else "tmp2_off"] = prep_off
                    prep_off += s * s
                    mc.append(e)
                comp.append(ct)
                it = np.zeros(1, api.ITX_TASK)[0]
                it["dst_off"], it["cf_off"], it["eob"], it["tx"], it["plane"] = ct["dst_off"], cf_off, 0, synth.SQ_TX[s], pl
                itx.append(it)
                cf_off += s * s
                n += 1
    fr = synth.Frame()
    fr.w, fr.h, fr.bpc, fr.n_refs = w, h, bpc, 2
    fr.mc, fr.comp, fr.itx = np.array(mc, api.MC_TASK), np.array(comp, api.COMP_TASK), np.array(itx, api.ITX_TASK)
    fr.coef = np.zeros(cf_off, util.coef_dtype(bpc))
    fr.prep_elems = prep_off
    return fr, refs


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_fused_weighted_compounds_on_extremal_content(ctx, bpc, twin_refs):
    """(the extremal part of test_fused_weighted_compounds_in_lists) the two mad_i24 of the fused w_avg at the ends of what mct gives"""
    oracle = util.default_oracle()
    fr, refs_h = extremal_frame(bpc, tap_signs(oracle))
    bdmax = (1 << bpc) - 1
    assert set(fr.comp["arg"].tolist()) == {1, 15} and {(int(t["filter_2d"]), int(t["mx"]), int(t["my"])) for t in fr.mc} == set(EXT_TRIPLES)
    rng = np.random.default_rng(77 + bpc)
    dst0 = synth.make_planes(rng, fr.w, fr.h, bpc, smooth=False)
    want, _, want_coef = test_frame.oracle_frame(oracle, fr, dst0, refs_h)
    for pl in range(3):
        vis = want[pl][:fr.h >> (pl > 0), :fr.w >> (pl > 0)]
        assert vis.min() == 0 and vis.max() == bdmax, "the oracle's plane %d holds both clips" % pl
    il = ctx.inter_list(fr.mc, fr.comp)
    n_fused = il.n_fused
    il.destroy()
    assert n_fused == len(fr.comp)
    got, _, got_coef = test_frame.hip_frame(ctx, fr, dst0, refs_h, recon=True)
    _compare_frame(fr, got, want, got_coef, want_coef, "worst-case windows at weights 1 and 15")
