"""Loop restoration, ENUMERATED: every edge combination, stripe height, width class, parameter set and extreme against the oracle.

tests/test_lr.py compares random samples (14 stripes per bit depth on one 4:0:0 plane).  The kernels choose their rows and columns from a
small discrete space -- 16 edge combinations, the `use_bottom` rules (Wiener h >= 4 with rows above, else h >= 6; 5x5 / mix additionally
only for even h; 3x3 h >= 3), the width against the 64 (62) columns of a wave, the clamp of the rows below to the plane's last row -- and
their packed arithmetic has ends (the two Wiener clamps, z = 0 and z >= 255, the 12-bit product next to 2^32).  This module walks that
space.  All pictures are 4:2:0 with tasks on planes 0, 1 and 2 (own strides and heights); stripes do not overlap, keep x >= 4 and two
rows above them.  What each test ran is collected in a set FIRST and the set is asserted, so the coverage below is a checked fact:

* test_wiener_every_edge_height_and_width_class -- edges 0 .. 15 x h in {1 .. 8, 63, 64} x w in {1 .. 4, 61 .. 67, 127 .. 129, 383, 384} x
  7- / 5-tap on noise.  hip: the full product per plane type (luma, chroma).  emu: every (edges, h, taps) and every (edges, w) per plane
  type.  Both: per plane type and tap count one stripe with y + h == plane height - 1 and one with y + h == plane height - 2, with
  HAVE_BOTTOM; for the first the oracle's two rows below are the plane's last row twice.
* test_wiener_extremal_taps_and_content -- taps at the corners of test_lr.wiener_params' ranges (f0 in {-5, 10}, 0 for 5-tap; f1 in
  {-23, 8}; f2 in {-17, 46}; horizontal and vertical corners independent: 64 + 16 filters) x content all 0, all bitdepth_max and the six
  windows with bitdepth_max exactly where the horizontal tap, the vertical tap or their product is positive / negative.  The same on
  hip and emu.  The oracle's outputs of the window cases hold both 0 and bitdepth_max (asserted on the oracle alone).
* test_sgr_every_set_edge_and_height -- 16 parameter sets (5x5, 3x3, mix) x edges 0 .. 15 x h in {1 .. 8, 63, 64}, widths rotating through
  {1, 2, 3, 60 .. 64, 70, 384}, laid out as rows of equal y and h with different sets and edges side by side (gaps 0, 0, 3, 17): the
  units of a row share waves.  hip: the full product per plane type.  emu: every (set, edges) and every (type, edges, h) per plane
  type.  Bottom-of-plane stripes as above for all three types.
* test_sgr_extremal_content_and_weights -- 16 sets x weights at the corners w0 in {-96, 31}, w1' in {-32, 95} (stored 128 - w0 - w1') x
  content all 0, all max, checkerboard 0 / max, a single max pixel in 0 and the inverse, half-plane steps (vertical, horizontal).  A
  numpy restatement of p and z (labels only) shows z == 0 and z >= 255 for 3x3 and for 5x5 at every bit depth; at 12 bit the all-max
  5x5 case ((x * sum) * one_by_x within 0.4 % of 2^32) is present.  The same on hip and emu.

An emulator trap ends the pytest process: run this module in a pytest call of its own first.  Cost: DESIGN.md 11."""
import itertools
import struct

import numpy as np
import pytest

import util
import golden_cases
import synth_frames as synth
from test_lr import wiener_params
from dav1d_amd import api

HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 8, 63, 64]
WIENER_WIDTHS = [1, 2, 3, 4, 61, 62, 63, 64, 65, 66, 67, 127, 128, 129, 383, 384]
SGR_WIDTHS = [1, 2, 3, 60, 61, 62, 63, 64, 70, 384]
SGR_GAPS = [0, 0, 3, 17]
PIC_W, PIC_H = 1016, 510          # chroma 508 x 255: odd height, widths that are no multiple of a wave
HAVE_BOTTOM = 8


def sgr_type(set_idx):
    s0, s1 = golden_cases.SGR_PARAMS[set_idx]
    return 2 + (1 if not s0 else 0 if not s1 else 2)          # 2: 5x5, 3: 3x3, 4: mix (enum Dav1dHipLrType)


SETS_OF_TYPE = {t: [s for s in range(16) if sgr_type(s) == t] for t in (2, 3, 4)}


def plane_size(pl):
    return (PIC_W, PIC_H) if pl == 0 else ((PIC_W + 1) >> 1, (PIC_H + 1) >> 1)


# ------------------------------------------------------------------ rows (pure functions)

def wiener_geometry_rows(full):
    """[(ptype, edges, h, w, taps)], ptype 0 luma / 1 chroma"""
    rows = []
    for ptype in (0, 1):
        if full:
            rows += [(ptype, e, h, w, t) for e, h, w, t in itertools.product(range(16), HEIGHTS, WIENER_WIDTHS, (7, 5))]
        else:
            for e in range(16):
                for k, (h, t) in enumerate(itertools.product(HEIGHTS, (7, 5))):          # 20 per edges: all 16 widths come up
                    rows.append((ptype, e, h, WIENER_WIDTHS[(k + 3 * e + ptype) % 16], t))
    return rows


def sgr_geometry_rows(full):
    """[(ptype, set, edges, h, w)]"""
    rows = []
    for ptype in (0, 1):
        k = 0
        if full:
            for h, s, e in itertools.product(HEIGHTS, range(16), range(16)):
                rows.append((ptype, (s + e) % 16, e, h, SGR_WIDTHS[k % 10]))          # neighbours differ in set AND edges
                k += 1
        else:
            for hi, h in enumerate(HEIGHTS):
                for e in range(16):
                    for typ in (4, 2, 3):
                        sets = SETS_OF_TYPE[typ]
                        rows.append((ptype, sets[hi % len(sets)], e, h, SGR_WIDTHS[k % 10]))          # 10 heights: every set of the type
                        k += 1
    return rows


def pack(items, gaps=(8,), vgap=2):
    """items: [(plane, w, h, payload)] -> batches [[(plane, x, y, w, h, payload)]]: per plane shelves of ONE height (units of a shelf
    share y and h), x >= 4, two rows above every stripe and both rows below it inside the plane; a new batch when a plane is full."""
    per_plane = {0: [[]], 1: [[]], 2: [[]]}
    state = {}
    for n, (pl, w, h, payload) in enumerate(items):
        PW, PH = plane_size(pl)
        x, y, sh = state.get(pl, (4, 2, h))
        if sh != h or x + w + 4 > PW:
            x, y, sh = 4, y + sh + vgap, h
        if y + h + 2 > PH:
            per_plane[pl].append([])
            x, y = 4, 2
        per_plane[pl][-1].append((pl, x, y, w, h, payload))
        state[pl] = (x + w + gaps[n % len(gaps)], y, sh)
    out = []
    for b in itertools.zip_longest(per_plane[0], per_plane[1], per_plane[2], fillvalue=[]):
        if b[0] or b[1] or b[2]:
            out.append(b[0] + b[1] + b[2])
    return out


def bottom_of_plane(payloads):
    """one batch: per plane and payload a stripe that ends one row and one that ends two rows above the plane's last row"""
    out = []
    for pl in range(3):
        PW, PH = plane_size(pl)
        x = 4
        for payload in payloads:
            for k, h in ((1, 8), (2, 6)):
                out.append((pl, x, PH - k - h, 67, h, payload))
                x += 67 + 8
        assert x <= PW
    return out


def wiener_filter(corner_h, corner_v, bpc):
    """taps (f0, f1, f2) per direction -> LooprestorationParams.filter as lr_stripe builds it (src/lr_apply_tmpl.c:55-66)"""
    f = np.zeros((2, 8), np.int16)
    for d, (f0, f1, f2) in enumerate((corner_h, corner_v)):
        f[d, 0] = f[d, 6] = f0
        f[d, 1] = f[d, 5] = f1
        f[d, 2] = f[d, 4] = f2
    f[0, 3] = -(f[0, 0] + f[0, 1] + f[0, 2]) * 2 + (128 if bpc > 8 else 0)
    f[1, 3] = 128 - (f[1, 0] + f[1, 1] + f[1, 2]) * 2
    return f


def sgr_filter(set_idx, w0, w1p):
    s0, s1 = golden_cases.SGR_PARAMS[set_idx]
    f = np.zeros((2, 8), np.int16)
    f[0, :4] = (s0, s1, w0, 128 - w0 - w1p)
    return f


# ------------------------------------------------------------------ the comparison

def noise_planes(rng, bpc):
    return synth.make_planes(rng, PIC_W, PIC_H, bpc, smooth=False, layout=api.LAYOUT_I420)


def oracle_stripe(oracle, bpc, work, sp, lp, pl, x, y, w, h, typ, edges, filt):
    """one looprestorationfilter_fn call as lr_stripe() issues it, in place in `work` (== sp on entry); returns the filtered block"""
    PH = plane_size(pl)[1]
    stride_px = work.strides[0] // work.itemsize
    bps = work.itemsize
    left = np.ascontiguousarray(sp[y:y + h, x - 4:x])
    L = np.zeros((8, stride_px), sp.dtype)
    L[0, :lp.shape[1]], L[1, :lp.shape[1]] = lp[y - 2], lp[y - 1]
    # backup_lpf stores the plane's last row twice where it is the first of the two rows below (src/lf_apply_tmpl.c:77-97)
    L[6, :lp.shape[1]], L[7, :lp.shape[1]] = lp[min(y + h, PH - 1)], lp[min(y + h + 1, PH - 1)]
    dst = work.ctypes.data + (y * stride_px + x) * bps
    if typ < 2:
        oracle.call(bpc, "wiener", typ, 0, dst, work.strides[0], left, L.ctypes.data + x * bps, w, h, np.ascontiguousarray(filt), edges)
    else:
        s0, s1, w0, w1 = (int(v) for v in filt[0][:4])
        params = np.frombuffer(struct.pack("<IIhh", s0, s1, w0, w1) + b"\0" * 20, np.uint8).copy()
        oracle.call(bpc, "sgr", typ - 2, 0, dst, work.strides[0], left, L.ctypes.data + x * bps, w, h, params, edges)
    out = work[y:y + h, x:x + w].copy()
    work[y:y + h, x:x + w] = sp[y:y + h, x:x + w]
    return out


def run_batches(ctx, bpc, rng, batches, planes_of):
    """batches: [[(plane, x, y, w, h, (type, edges, filter, ...))]]; planes_of(b) -> (src planes, lpf planes) of batch b (the same objects
    again: not uploaded again).  Every plane of dst is compared whole: stripes hold the oracle's pixels, the rest its fill.  Returns the
    oracle's blocks per batch."""
    oracle = util.default_oracle()
    src, lpf, dst = (ctx.picture(PIC_W, PIC_H, api.LAYOUT_I420, bpc) for _ in range(3))
    fill = noise_planes(rng, bpc)
    up_s = up_l = work = None
    blocks = []
    try:
        for b, batch in enumerate(batches):
            sp, lp = planes_of(b)
            if sp is not up_s:
                for pl in range(3):
                    src.upload(pl, sp[pl])
                up_s, work = sp, synth.copy_planes(sp)
            if lp is not up_l:
                for pl in range(3):
                    lpf.upload(pl, lp[pl])
                up_l = lp
            want = synth.copy_planes(fill)
            t = np.zeros(len(batch), api.LR_TASK)
            outs = []
            for i, (pl, x, y, w, h, payload) in enumerate(batch):
                typ, edges, filt = payload[:3]
                assert x >= 4 and y >= 2 and x + w + 4 <= sp[pl].shape[1] and y + h < plane_size(pl)[1]
                assert (want[pl][y:y + h, x:x + w] == fill[pl][y:y + h, x:x + w]).all(), "stripes do not overlap"
                t[i] = (x, y, w, h, pl, edges, typ, 0, filt)
                blk = oracle_stripe(oracle, bpc, work[pl], sp[pl], lp[pl], pl, x, y, w, h, typ, edges, filt)
                want[pl][y:y + h, x:x + w] = blk
                outs.append(blk)
            blocks.append(outs)
            for pl in range(3):
                dst.upload(pl, fill[pl])
            ctx.lr_batch(dst, src, lpf, t)
            for pl in range(3):
                got = dst.download(pl)
                bad = np.argwhere(got != want[pl])
                if len(bad):
                    yy, xx = bad[0]
                    hit = [(v[:5], v[5][:2], np.asarray(v[5][2]).tolist()) for v in batch
                           if v[0] == pl and v[1] <= xx < v[1] + v[3] and v[2] <= yy < v[2] + v[4]]
                    raise AssertionError("batch %d plane %d differs at (%d,%d): got %d want %d (%d px); (plane, x, y, w, h), (type, edges), filter: %s"
                                         % (b, pl, xx, yy, got[yy, xx], want[pl][yy, xx], len(bad), hit[:1] or "outside every stripe"))
    finally:
        for o in (src, lpf, dst):
            o.free()
    return blocks


def plane_rotation(ptype, k):
    """chroma tasks alternate between planes 1 and 2 by the parity of k's bit count: neither plane keeps one residue of any counter"""
    return 0 if ptype == 0 else 1 + (bin(k).count("1") & 1)


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_wiener_every_edge_height_and_width_class(ctx, bpc):
    full = ctx.backend == "hip"
    rng = np.random.default_rng(4100 + bpc)
    rows = wiener_geometry_rows(full)
    items = []
    for k, (ptype, e, h, w, taps) in enumerate(rows):
        typ = 0 if taps == 7 else 1
        items.append((plane_rotation(ptype, k), w, h, (typ, e, wiener_params(rng, bpc, taps == 5))))
    batches = pack(items)
    bottom = bottom_of_plane([(typ, 15, wiener_params(rng, bpc, typ == 1)) for typ in (0, 1)])
    batches.append(bottom)
    # ---- coverage, from what is handed to the kernel
    ran = {(min(pl, 1), v[1], h, w, 7 - 2 * v[0]) for b in batches[:-1] for pl, x, y, w, h, v in b}
    for ptype in (0, 1):
        if full:
            assert {r[1:] for r in ran if r[0] == ptype} == set(itertools.product(range(16), HEIGHTS, WIENER_WIDTHS, (7, 5)))
        else:
            assert {(e, h, t) for p, e, h, w, t in ran if p == ptype} == set(itertools.product(range(16), HEIGHTS, (7, 5)))
            assert {(e, w) for p, e, h, w, t in ran if p == ptype} == set(itertools.product(range(16), WIENER_WIDTHS))
    assert {pl for b in batches for pl, *_ in b} == {0, 1, 2}
    ends = {(min(pl, 1), v[0], plane_size(pl)[1] - (y + h)) for pl, x, y, w, h, v in bottom if v[1] & HAVE_BOTTOM}
    assert ends == set(itertools.product((0, 1), (0, 1), (1, 2))), "both plane types, both tap counts: one and two rows left below"
    sp, lp = noise_planes(rng, bpc), noise_planes(rng, bpc)
    run_batches(ctx, bpc, rng, batches, lambda b: (sp, lp))


WIENER_PATTERNS = ["zero", "max", "h+", "h-", "v+", "v-", "hv+", "hv-"]
UNIT = 8          # the extremal cases are 8 x 8 stripes with a 7 x 7 window around pixel (3, 3)


def effective_taps(filt, bpc):
    """the 7 weights each direction applies to the pixels: the centre tap carries the implicit 128 (8 bit adds pixel * 128 beside the
    stored taps, the stored high-bit-depth centre tap holds it: src/looprestoration_tmpl.c wiener_filter_h)"""
    eh = [int(v) for v in filt[0][:7]]
    ev = [int(v) for v in filt[1][:7]]
    if bpc == 8:
        eh[3] += 128
    return eh, ev


def wiener_window(pattern, filt, bpc):
    """(UNIT + 8) x (UNIT + 8) content around a stripe (4 pixels of surround each side)"""
    mx = (1 << bpc) - 1
    n = UNIT + 8
    if pattern in ("zero", "max"):
        return np.full((n, n), mx if pattern == "max" else 0, np.int64)
    eh, ev = effective_taps(filt, bpc)
    sign = 1 if pattern[-1] == "+" else -1
    a = np.zeros((n, n), np.int64)
    for r in range(7):
        for c in range(7):
            p = eh[c] if pattern[:-1] == "h" else ev[r] if pattern[:-1] == "v" else eh[c] * ev[r]
            if p * sign > 0:
                a[4 + r, 4 + c] = mx          # stripe pixel (3, 3) sits at (7, 7): tap (r, c) reads (4 + r, 4 + c)
    if pattern[:-1] == "h":
        a[:, :] = a[7:8, :]
    if pattern[:-1] == "v":
        a[:, :] = a[:, 7:8]
    return a


def paint_batches(batches, bpc, window_of):
    """per batch src planes (== lpf planes) of zeros with window_of(payload) painted around every stripe"""
    out = []
    for batch in batches:
        planes = synth.copy_planes(synth.make_planes(np.random.default_rng(0), PIC_W, PIC_H, bpc, smooth=False, layout=api.LAYOUT_I420))
        for p in planes:
            p[:, :] = 0
        for pl, x, y, w, h, payload in batch:
            win = window_of(payload)
            assert win.shape == (h + 8, w + 8)
            planes[pl][y - 2:y + h + 2, x - 4:x + w + 4] = win[2:-2]          # two rows above and below, four columns each side
        out.append(planes)
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_wiener_extremal_taps_and_content(ctx, bpc):
    rng = np.random.default_rng(4200 + bpc)
    corners7 = list(itertools.product((-5, 10), (-23, 8), (-17, 46)))
    corners5 = list(itertools.product((0,), (-23, 8), (-17, 46)))
    filters = [(0, ch, cv) for ch in corners7 for cv in corners7] + [(1, ch, cv) for ch in corners5 for cv in corners5]
    items = []
    for k, ((typ, ch, cv), pattern) in enumerate(itertools.product(filters, WIENER_PATTERNS)):
        items.append((k % 3, UNIT, UNIT, (typ, 15, wiener_filter(ch, cv, bpc), pattern, ch, cv)))
    batches = pack(items, vgap=6)
    ran = {(v[0], v[4], v[5], v[3]) for b in batches for pl, x, y, w, h, v in b}
    assert ran == {(typ, ch, cv, p) for typ, ch, cv in filters for p in WIENER_PATTERNS} and len(filters) == 64 + 16
    assert {pl for b in batches for pl, *_ in b} == {0, 1, 2}
    painted = paint_batches(batches, bpc, lambda v: wiener_window(v[3], v[2], bpc))
    blocks = run_batches(ctx, bpc, rng, batches, lambda b: (painted[b], painted[b]))
    seen = set()
    for batch, outs in zip(batches, blocks):
        for (pl, x, y, w, h, v), blk in zip(batch, outs):
            if v[3] not in ("zero", "max"):
                seen |= set(np.unique(blk).tolist()) & {0, (1 << bpc) - 1}
    assert seen == {0, (1 << bpc) - 1}, "the windows drive the oracle's output to both ends"


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_sgr_every_set_edge_and_height(ctx, bpc):
    full = ctx.backend == "hip"
    rng = np.random.default_rng(4300 + bpc)
    rows = sgr_geometry_rows(full)
    items = []
    for k, (ptype, s, e, h, w) in enumerate(rows):
        w0, w1p = int(rng.integers(-96, 32)), int(rng.integers(-32, 96))
        items.append((plane_rotation(ptype, k), w, h, (sgr_type(s), e, sgr_filter(s, w0, w1p), s)))
    batches = pack(items, SGR_GAPS)
    bottom = bottom_of_plane([(sgr_type(s), 15, sgr_filter(s, -20, 60), s) for s in (0, 10, 14)])
    batches.append(bottom)
    ran = {(min(pl, 1), v[3], v[1], h, v[0]) for b in batches[:-1] for pl, x, y, w, h, v in b}
    for ptype in (0, 1):
        if full:
            assert {r[1:4] for r in ran if r[0] == ptype} == set(itertools.product(range(16), range(16), HEIGHTS))
        else:
            assert {(s, e) for p, s, e, h, t in ran if p == ptype} == set(itertools.product(range(16), range(16)))
            assert {(t, e, h) for p, s, e, h, t in ran if p == ptype} == set(itertools.product((2, 3, 4), range(16), HEIGHTS))
    assert {w for b in batches[:-1] for pl, x, y, w, h, v in b} == set(SGR_WIDTHS)
    assert {pl for b in batches for pl, *_ in b} == {0, 1, 2}
    # rows of equal y and h hold different sets and edges side by side, some without a gap
    shelves = {}
    for bi, b in enumerate(batches[:-1]):
        for pl, x, y, w, h, v in b:
            shelves.setdefault((bi, pl, y), []).append((x, w, h, v[3], v[1], v[0]))
    mixed = [s for s in shelves.values() if len({u[2] for u in s}) == 1 and len({u[3] for u in s}) > 1 and len({u[4] for u in s}) > 1]
    assert len(mixed) >= 0.5 * len(shelves) and any(len({u[5] for u in s}) == 3 for s in mixed)
    assert any(a[0] + a[1] == b_[0] for s in mixed for a, b_ in zip(sorted(s), sorted(s)[1:])), "adjacent units"
    ends = {(min(pl, 1), v[0], plane_size(pl)[1] - (y + h)) for pl, x, y, w, h, v in bottom if v[1] & HAVE_BOTTOM}
    assert ends == set(itertools.product((0, 1), (2, 3, 4), (1, 2)))
    sp, lp = noise_planes(rng, bpc), noise_planes(rng, bpc)
    # flat and nearly flat areas beside the noise: the whole x_by_x range (as tests/test_lr.py does)
    for p in sp:
        p[:, p.shape[1] // 3:p.shape[1] // 2] = p[0, 0]
        q = p[:, p.shape[1] // 2:2 * p.shape[1] // 3]
        q[:, :] = (1 << (bpc - 1)) + (q >> (bpc - 2))
    run_batches(ctx, bpc, rng, batches, lambda b: (sp, lp))


SGR_PATTERNS = ["zero", "max", "checker", "pixel", "hole", "step_v", "step_h"]
SGR_W, SGR_H = 12, 8


def sgr_window(pattern, bpc):
    mx = (1 << bpc) - 1
    a = np.zeros((SGR_H + 8, SGR_W + 8), np.int64)
    if pattern == "max":
        a[:, :] = mx
    elif pattern == "checker":
        a[::2, ::2] = mx
        a[1::2, 1::2] = mx
    elif pattern in ("pixel", "hole"):
        a[4 + SGR_H // 2, 4 + SGR_W // 2] = mx
        if pattern == "hole":
            a = mx - a
    elif pattern == "step_v":
        a[:, 4 + SGR_W // 2:] = mx
    elif pattern == "step_h":
        a[4 + SGR_H // 2:, :] = mx
    return a


def sgr_z(win, bpc, n, s):
    """z of sgr_calc_row_ab (src/looprestoration_tmpl.c:505-523) at every box position inside the window -- labels only"""
    r = 1 if n == 9 else 2
    k = 2 * r + 1
    v = np.lib.stride_tricks.sliding_window_view(win.astype(np.int64), (k, k))
    a = (v * v).sum((2, 3)) + ((1 << (2 * (bpc - 8))) >> 1) >> (2 * (bpc - 8))
    b = v.sum((2, 3)) + ((1 << (bpc - 8)) >> 1) >> (bpc - 8)
    p = np.maximum(a * n - b * b, 0)
    return (((p * s) & 0xffffffff) + (1 << 19)) >> 20


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_sgr_extremal_content_and_weights(ctx, bpc):
    rng = np.random.default_rng(4400 + bpc)
    weights = list(itertools.product((-96, 31), (-32, 95)))
    items = []
    for k, (s, (w0, w1p), pattern) in enumerate(itertools.product(range(16), weights, SGR_PATTERNS)):
        items.append((k % 3, SGR_W, SGR_H, (sgr_type(s), 15, sgr_filter(s, w0, w1p), s, (w0, w1p), pattern)))
    batches = pack(items, vgap=6)
    ran = {(v[3], v[4], v[5]) for b in batches for pl, x, y, w, h, v in b}
    assert ran == set(itertools.product(range(16), weights, SGR_PATTERNS))
    assert {pl for b in batches for pl, *_ in b} == {0, 1, 2}
    zs = {9: set(), 25: set()}
    for s, pattern in itertools.product(range(16), SGR_PATTERNS):
        s0, s1 = golden_cases.SGR_PARAMS[s]
        for n, strength in ((25, s0), (9, s1)):
            if strength:
                z = sgr_z(sgr_window(pattern, bpc), bpc, n, strength)
                zs[n] |= ({"z == 0"} if (z == 0).any() else set()) | ({"z >= 255"} if (z >= 255).any() else set())
    assert zs[9] == zs[25] == {"z == 0", "z >= 255"}
    # all max under a 5x5 box: x = x_by_x[0], sum = 25 * bitdepth_max -- at 12 bit (x * sum) * one_by_x is the product closest to 2^32
    assert any(v[0] in (2, 4) and v[5] == "max" for b in batches for pl, x, y, w, h, v in b)
    painted = paint_batches(batches, bpc, lambda v: sgr_window(v[5], bpc))
    run_batches(ctx, bpc, rng, batches, lambda b: (painted[b], painted[b]))
