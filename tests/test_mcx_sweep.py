"""Warped and scaled motion compensation and super-resolution resize, ENUMERATED: csrc/mcx.hip against the oracle, byte for byte.

tests/test_mcx.py draws positions, phases, steps and warp parameters from a seed on an I400 picture with one reference; this module
lists them, on planes 0, 1 and 2 of I420 pictures with three references of different content.  What the rows cover is collected in a
set FIRST and the set is asserted; every condition (which filter row or phase an output pixel reads, which side a window leaves on) is
computed here from the specification's arithmetic (src/mc_tmpl.c:189-357, 799-866, 918-944 and src/recon_tmpl.c:990-1047, 1115-1174,
restated), never read from the code under test.  The oracle side calls emu_edge wherever the reference driver does
(test_mcx._oracle_warp, _oracle_mc_scaled); the kernels clamp coordinates instead.

* test_warp_every_filter_row — with abcd == 0 one task reads one row of the 193-row warp filter table in each pass: every row in the
  horizontal pass with the vertical row rotating and the converse (hip: also the product over every eighth row), then tasks with
  non-zero abcd of both signs whose rows run into both ends of the table; every (pass, row) for put and for prep; block origins off
  every side, a corner and more than 15 pixels outside (the whole 15x15 window is replicated edge).
* test_warp_extremal_content — rows 0, 64, 192 and the rows with the largest positive / negative tap sums (from the ORACLE's impulse
  response) on all 0, all max, a checkerboard and the two worst-case windows.
* test_scaled_every_filter_phase_and_step — put, prep and PUT_TMP.  hip: filter_2d x fxi x fyi x the four tap-set classes at step 1024
  (put, prep); emu, and PUT_TMP on both: every (filter_2d, fxi, fyi) once on small shapes.  Both: every (filter_2d, set class) at the four phase classes, the
  step classes {1, below 1024, 1024, between, 2048} per axis against every filter_2d and set class, every legal shape, the 128-wide and
  128-high blocks at step 2048, 5/16 of the windows off the picture (every filter on every side, some entirely outside).  PUT_TMP pixels
  are compared in the arena, the destination stays untouched, and some of them feed blend_h / blend_v as in obmc().
* test_scaled_extremal_content — all 0, all max and test_mc_sweep's worst-case windows of the task's phase pair at step 1024.
* test_resize_every_denominator_and_row — w_den 9 .. 16 x source widths 16, 17, 255, 512 and one output wider than 256; all 64 filter
  rows; both clamps of the source column.

Cost: DESIGN.md 11.  An emulator trap ends the pytest process: run this module in a pytest call of its own first."""
import itertools

import numpy as np
import pytest

import util
import test_mc_sweep
from test_mcx import _oracle_warp, _oracle_mc_scaled
from dav1d_amd import api

PUT, PREP, PUT_TMP = 0, 1, 2
KINDS = ["put", "prep", "put_tmp"]
SIDES = test_mc_sweep.SIDES + ["far"]
BLEND_V_KIND, BLEND_H_KIND = 5, 6          # enum Dav1dHipCompKind


def make_refs(ctx, bpc, vis_w, vis_h, seed, fill=None):
    """three I420 references of different (random) content: (device pictures, host planes [ref][plane], visible (w, h) per plane)"""
    rng = np.random.default_rng(seed)
    pd = util.pix_dtype(bpc)
    pics, planes = [], []
    for r in range(3):
        p = ctx.picture(vis_w, vis_h, api.LAYOUT_I420, bpc)
        a = [rng.integers(0, 1 << bpc, size=p.padded_shape(pl)).astype(pd) for pl in range(3)]       # the padding is NOT edge-replicated
        if fill is not None:
            fill(r, a)
        for pl in range(3):
            p.upload(pl, a[pl])
        pics.append(p)
        planes.append(a)
    dims = [(int(pics[0].pic.p[pl].w), int(pics[0].pic.p[pl].h)) for pl in range(3)]
    assert dims[1] == ((vis_w + 1) >> 1, (vis_h + 1) >> 1)
    return pics, planes, dims


def make_dst(ctx, bpc, w, h, seed):
    rng = np.random.default_rng(seed)
    dst = ctx.picture(w, h, api.LAYOUT_I420, bpc)
    pre = [rng.integers(0, 1 << bpc, size=dst.padded_shape(pl)).astype(util.pix_dtype(bpc)) for pl in range(3)]
    for pl in range(3):
        dst.upload(pl, pre[pl])
    return dst, pre


def sides_left(left, top, right, bottom, pw, ph):
    """which sides the source rectangle [left - 3, right + 4) x [top - 3, bottom + 4) leaves the plane on, as the drivers test it"""
    s = set()
    if left < 3:
        s.add("left")
    if right + 4 > pw:
        s.add("right")
    if top < 3:
        s.add("top")
    if bottom + 4 > ph:
        s.add("bottom")
    if len(s & {"left", "right"}) and len(s & {"top", "bottom"}):
        s.add("corner")
    if right + 4 <= 0 or left - 3 >= pw or bottom + 4 <= 0 or top - 3 >= ph:
        s.add("far")
    return s


def edge_position(cls, k, ww, wh, pw, ph):
    """the origin of a ww x wh source window: cls 0 .. 5 = off the plane at SIDES[cls], else inside; k varies the choice"""
    ix, iy = 4 + (k * 37) % (pw - ww - 8), 4 + (k * 53) % (ph - wh - 8)
    left, right = [-ww - 5, -3, -1, 1], [pw - ww + 1, pw - 2, pw + 9, pw - ww - 2]
    top, bottom = [-wh - 5, -2, -1, 2], [ph - wh + 2, ph - 1, ph + 20, ph - wh - 1]
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
    if cls == 5:
        return [(-ww - 24, iy), (pw + 20, iy), (ix, -wh - 24), (ix, ph + 20), (-ww - 21, ph + 23)][k % 5]
    return ix, iy


# ------------------------------------------------------------------ warp

WARP_LO, WARP_HI = -64 * 1024 - 512, 128 * 1024 + 511        # 64 + ((t + 512) >> 10) is within 0 .. 192 for t in this range
WARP_VIS = (121, 91)


def warp_rows_of(mx, my, abcd):
    """the filter rows the two passes of one task read, src/mc_tmpl.c:808-832: (15 x 8 horizontal, 8 x 8 vertical)"""
    y15, x8 = np.mgrid[0:15, 0:8]
    y8, x8b = np.mgrid[0:8, 0:8]
    return 64 + ((mx + y15 * abcd[1] + x8 * abcd[0] + 512) >> 10), 64 + ((my + y8 * abcd[3] + x8b * abcd[2] + 512) >> 10)


def row_param(r):
    return (r - 64) << 10


def warp_rows(full):
    """[(kind, mx, my, abcd)]"""
    rows = []
    for kind in (PUT, PREP):
        for r in range(193):
            rows.append((kind, row_param(r), row_param((r * 7 + 3 + kind) % 193), (0, 0, 0, 0)))
            rows.append((kind, row_param((r * 11 + 5 + kind) % 193), row_param(r), (0, 0, 0, 0)))
        if full:
            rows += [(kind, row_param(a), row_param(b), (0, 0, 0, 0)) for a in range(0, 193, 8) for b in range(0, 193, 8)]
        # rows that vary inside the block: both signs of every component, the first and the last row of the table reached exactly
        mags = [(0x155, 0x2a3, 0x1c1, 0x333), (0x7ff, 0x400, 0x3ff, 0x7ff), (37, 1900, 2047, 5), (0x1000, 0x800, 0xfff, 0x1001)]
        for n, (sg, mg, where) in enumerate(itertools.product(itertools.product((1, -1), repeat=4), mags, ("low", "high", "mid"))):
            abcd = tuple(s * m for s, m in zip(sg, mg))
            hx = [y * abcd[1] + x * abcd[0] for y in (0, 14) for x in (0, 7)]
            hy = [y * abcd[3] + x * abcd[2] for y in (0, 7) for x in (0, 7)]
            pick = lambda off: WARP_LO - min(off) if where == "low" else WARP_HI - max(off) if where == "high" else (WARP_LO + WARP_HI) // 2 - off[n % 4]
            rows.append((kind, pick(hx), pick(hy), abcd))
    return rows


def assert_warp_coverage(rows, full):
    reached, whole = {}, {}
    signs = set()
    for kind, mx, my, abcd in rows:
        rh, rv = warp_rows_of(mx, my, abcd)
        assert 0 <= rh.min() and rh.max() <= 192 and 0 <= rv.min() and rv.max() <= 192, "row outside the table: %s" % ((kind, mx, my, abcd),)
        # the vertical pass of output row y reads mid rows y .. y + 7: all 15 horizontal rows are used by some output pixel
        reached.setdefault(kind, set()).update((0, int(r)) for r in rh.ravel())
        reached[kind].update((1, int(r)) for r in rv.ravel())
        if not any(abcd):
            whole.setdefault(kind, set()).update([(0, int(rh[0, 0])), (1, int(rv[0, 0]))])
        else:
            signs.update((c, v > 0) for c, v in enumerate(abcd))
            assert len(set(rh.ravel().tolist())) > 1 and len(set(rv.ravel().tolist())) > 1, "the rows vary inside the block"
    for kind in (PUT, PREP):
        assert reached[kind] == {(p, r) for p in range(2) for r in range(193)}, "%s: %d of 386 (pass, row)" % (KINDS[kind], len(reached[kind]))
        assert whole[kind] == reached[kind], "%s: ... each of them by a task that reads it for a whole pass (abcd == 0)" % KINDS[kind]
    assert signs == {(c, s) for c in range(4) for s in (False, True)}, "both signs of a, b, c and d"
    if full:
        assert {(k, mx, my) for k, mx, my, abcd in rows if not any(abcd)} >= {(k, row_param(a), row_param(b)) for k in (PUT, PREP) for a in range(0, 193, 8)
                                                                            for b in range(0, 193, 8)}


def run_warp(ctx, oracle, bpc, tasks, labels, ref_pics, ref_planes, dims, what, want_clips=False):
    """tasks (WARP_TASK without offsets): put blocks on a grid of pitch 12 in their plane of an I420 picture, prep blocks in an arena
    with row stride 8 or 24; oracle first, then ctx.warp_batch.  Returns the oracle's put blocks."""
    dst, pre = make_dst(ctx, bpc, 768, 512, 40 + bpc)
    want = [p.copy() for p in pre]
    n_put = [0, 0, 0]
    off = 0
    where = []
    for i, t in enumerate(tasks):
        pl = int(t["plane"])
        pw, ph = dims[pl]
        if t["kind"] == PUT:
            per_row = want[pl].shape[1] // 12
            x, y = (n_put[pl] % per_row) * 12, (n_put[pl] // per_row) * 12
            assert y + 8 <= want[pl].shape[0], "the destination picture is too small"
            n_put[pl] += 1
            t["dst_off"] = y * dst.stride_px(pl) + x
            where.append((x, y))
        else:
            t["tmp_stride"] = (8, 24)[i & 1]
            t["dst_off"] = off
            where.append(off)
            off += 8 * int(t["tmp_stride"])
    want_prep = np.zeros(max(off, 8), np.int16)
    put_blocks = []
    for i, t in enumerate(tasks):
        pl = int(t["plane"])
        plane = ref_planes[int(t["ref"])][pl]
        if t["kind"] == PUT:
            x, y = where[i]
            _oracle_warp(oracle, bpc, plane, dims[pl][0], dims[pl][1], t, dst_block=want[pl][y:, x:])
            put_blocks.append((i, want[pl][y:y + 8, x:x + 8].copy()))
        else:
            _oracle_warp(oracle, bpc, plane, dims[pl][0], dims[pl][1], t, tmp=want_prep[where[i]:])
    if want_clips:
        bdmax = (1 << bpc) - 1
        assert min(b.min() for _, b in put_blocks) == 0 and max(b.max() for _, b in put_blocks) == bdmax, "the oracle's put outputs hold both clips"
    prep = ctx.buffer(len(want_prep) * 2)
    prep.zero()
    ctx.warp_batch(dst, ref_pics, tasks, prep)
    for pl in range(3):
        got = dst.download(pl)
        bad = np.argwhere(got != want[pl])
        if len(bad):
            yy, xx = bad[0]
            hit = [i for i, t in enumerate(tasks) if t["kind"] == PUT and t["plane"] == pl and where[i][0] <= xx < where[i][0] + 8 and where[i][1] <= yy < where[i][1] + 8]
            raise AssertionError("%s, %d bpc warp put: (%d,%d) of plane %d is %d, the oracle has %d (before the call: %d); %d pixels differ; task %s %s" % (
                what, bpc, xx, yy, pl, got[yy, xx], want[pl][yy, xx], pre[pl][yy, xx], len(bad),
                tuple(tasks[hit[0]]) if hit else "none: outside every block", labels[hit[0]] if hit else ""))
    got_prep = prep.download(np.int16, len(want_prep))
    bad = np.flatnonzero(got_prep != want_prep)
    if len(bad):
        hit = [i for i, t in enumerate(tasks) if t["kind"] == PREP and where[i] <= bad[0] < where[i] + 8 * int(t["tmp_stride"])]
        raise AssertionError("%s, %d bpc warp prep: element %d is %d, the oracle has %d; %d differ; task %s %s" % (
            what, bpc, bad[0], got_prep[bad[0]], want_prep[bad[0]], len(bad), tuple(tasks[hit[0]]) if hit else "none", labels[hit[0]] if hit else ""))
    dst.free(); prep.free()
    return put_blocks


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_warp_every_filter_row(ctx, bpc):
    oracle = util.default_oracle()
    full = ctx.backend != "emu"
    rows = warp_rows(full)
    assert_warp_coverage(rows, full)
    ref_pics, ref_planes, dims = make_refs(ctx, bpc, WARP_VIS[0], WARP_VIS[1], 4300 + bpc)
    tasks = np.zeros(len(rows), api.WARP_TASK)
    labels, met, combos, deep = [], set(), set(), set()
    for k, (kind, mx, my, abcd) in enumerate(rows):
        pl, ref = k % 3, (k // 3 + k // 7) % 3
        pw, ph = dims[pl]
        cls = (k * 5 + kind) % 16
        sx, sy = edge_position(cls, k // 16, 8, 8, pw, ph)
        left = sides_left(sx, sy, sx + 8, sy + 8, pw, ph)        # the driver's test: dx < 3 || dx + 8 + 4 > w || ...
        if cls < 6:
            assert SIDES[cls] in left, (SIDES[cls], sx, sy)
        if sx + 11 < -15 or sx - 3 > pw + 15 or sy + 11 < -15 or sy - 3 > ph + 15:
            deep.add(kind)
        met.update((kind, s) for s in left)
        combos.add((kind, pl, ref))
        tasks[k] = (0, sx, sy, mx, my, abcd, 8, kind, pl, ref, (0, 0, 0))
        labels.append("(%s)" % ", ".join(sorted(left)) if left else "(inside)")
    assert met == {(kind, s) for kind in (PUT, PREP) for s in SIDES}, "every side, a corner and a far origin meet put and prep"
    assert combos == {(kind, pl, r) for kind in (PUT, PREP) for pl in range(3) for r in range(3)}, "every (kind, plane, ref)"
    assert deep == {PUT, PREP}, "origins more than 15 pixels outside: the whole 15 x 15 window is replicated edge"
    run_warp(ctx, oracle, bpc, tasks, labels, ref_pics, ref_planes, dims, "every filter row")
    for p in ref_pics:
        p.free()


_warp_response = []


def oracle_warp_response(oracle):
    """resp[pass][row][t]: what a source pixel of 255 at tap position t adds to output (0, 0) of the oracle's 8-bit warp8x8t, the other
    pass at row 64 (the zero offset: two positive taps, nearly all weight on one; the signs and the order of the sums are what is used)"""
    if not _warp_response:
        resp = np.zeros((2, 193, 8), np.int32)
        tmp = np.zeros(64, np.int16)
        abcd = np.zeros(4, np.int16)
        for p in range(2):
            for r in range(193):
                for t in range(8):
                    src = np.zeros((24, 24), np.uint8)
                    if p == 0:
                        src[8, 8 + t - 3] = 255
                    else:
                        src[8 + t - 3, 8] = 255
                    oracle.call(8, "warp8x8t", 0, 0, tmp.ctypes.data, 8, src.ctypes.data + 8 * 24 + 8, 24, abcd, row_param(r if p == 0 else 64), row_param(r if p == 1 else 64))
                    resp[p, r, t] = tmp[0]
        _warp_response.append(resp)
    return _warp_response[0]


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_warp_extremal_content(ctx, bpc):
    oracle = util.default_oracle()
    resp = oracle_warp_response(oracle)
    assert (np.sign(resp[:, 64]) == [0, 0, 0, 1, 1, 0, 0, 0]).all(), "row 64, the zero offset, has two taps, both positive"
    pos, neg = np.where(resp > 0, resp, 0).sum(axis=2), np.where(resp < 0, resp, 0).sum(axis=2)
    assert (neg < 0).any(axis=1).all(), "the table has negative taps"
    subset = sorted({0, 64, 192, 32, 150, int(pos[0].argmax()), int(neg[0].argmin()), int(pos[1].argmax()), int(neg[1].argmin())})
    patterns = ["zero", "max", "checker", "worst+", "worst-"]
    combos = [(a, b, p) for a in subset for b in subset for p in patterns]
    bdmax = (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    side = int(np.ceil(np.sqrt(len(combos))))
    PITCH = 24                       # a patch: the 15 x 15 window of a block at (8, 8) of it, patterns of period 8 and 2

    def fill(r, planes):
        if r:
            return
        for k, (a, b, p) in enumerate(combos):
            py, px = (k // side) * PITCH, (k % side) * PITCH
            if p == "checker":
                yy, xx = np.mgrid[0:PITCH, 0:PITCH]
                patch = np.where((yy + xx) & 1, bdmax, 0)
            elif p in ("zero", "max"):
                patch = np.full((PITCH, PITCH), bdmax if p == "max" else 0)
            else:
                prod = np.sign(resp[1, b])[:, None] * np.sign(resp[0, a])[None, :]
                win = np.where(prod > 0 if p == "worst+" else prod < 0, bdmax, 0)
                # the 8 x 8 window of output pixel (0, 0) of a block at (8, 8) starts at (5, 5)
                patch = np.roll(np.tile(win, (3, 3)), (5, 5), axis=(0, 1))
            planes[0][py:py + PITCH, px:px + PITCH] = patch.astype(pd)

    ref_pics, ref_planes, dims = make_refs(ctx, bpc, side * PITCH, side * PITCH, 4400 + bpc, fill)
    tasks = np.zeros(2 * len(combos), api.WARP_TASK)
    labels = []
    for k, (a, b, p) in enumerate(combos):
        for kind in (PUT, PREP):
            tasks[2 * k + kind] = (0, (k % side) * PITCH + 8, (k // side) * PITCH + 8, row_param(a), row_param(b), (0, 0, 0, 0), 8, kind, 0, 0, (0, 0, 0))
            labels.append("rows (%d, %d) on %s" % (a, b, p))
    blocks = run_warp(ctx, oracle, bpc, tasks, labels, ref_pics, ref_planes, dims, "extremal content", want_clips=True)
    worst = {labels[i]: blk for i, blk in blocks if "worst" in labels[i]}
    assert any(b[0, 0] == 0 for l, b in worst.items() if l.endswith("-")) and any(b[0, 0] == bdmax for l, b in worst.items() if l.endswith("+")), \
        "the worst-case windows drive the oracle into both clips"
    for p in ref_pics:
        p.free()


# ------------------------------------------------------------------ scaled

SC_VIS = (639, 557)
STEP_CLASSES = ["1", "below", "1024", "between", "2048"]
STEPS = {"1": [1], "below": [512, 700, 1023, 37], "1024": [1024], "between": [1025, 1500, 2047], "2048": [2048]}
PHASE_OFFSETS = [0, 63, 64, 1023, 500, 333, 960, 127]
SMALL_AREA = 128


def step_class(d):
    return "1" if d == 1 else "below" if d < 1024 else "1024" if d == 1024 else "between" if d < 2048 else "2048"


def scaled_shapes(kind):
    return test_mc_sweep.legal_shapes(1 if kind == PREP else 0)


def scaled_rows(kind, full):
    """[(filter_2d, mx, my, w, h, dx, dy)] (w, h at 3, 4 as test_mc_sweep.pack_batches reads them)"""
    shapes = scaled_shapes(kind)
    by_class = {(cw, ch): [s for s in shapes if (s[0] > 4) == cw and (s[1] > 4) == ch] for cw in (False, True) for ch in (False, True)}
    small = [s for s in shapes if s[0] * s[1] <= SMALL_AREA]
    rows = []
    n = 0
    if full and kind != PUT_TMP:
        for f, fx, fy, (cw, ch) in itertools.product(range(10), range(16), range(16), by_class):
            w, h = by_class[cw, ch][n % len(by_class[cw, ch])]
            rows.append((f, fx * 64 + PHASE_OFFSETS[n % 8] % 64, fy * 64 + PHASE_OFFSETS[(n // 8) % 8] % 64, w, h, 1024, 1024))
            n += 1
    else:
        for f, fx, fy in itertools.product(range(10), range(16), range(16)):
            w, h = small[n % len(small)]
            rows.append((f, fx * 64 + PHASE_OFFSETS[n % 8] % 64, fy * 64 + PHASE_OFFSETS[(n // 8) % 8] % 64, w, h, 1024, 1024))
            n += 1
    for f in range(10):                       # every (filter_2d, set class) at the four phase classes
        for (cw, ch), lst in by_class.items():
            for px, py in test_mc_sweep.PHASE_CLASSES:
                w, h = [s for s in lst if s[0] * s[1] <= 1024][n % len([s for s in lst if s[0] * s[1] <= 1024])]
                rows.append((f, px * (64 + (n * 83) % 960), py * (64 + (n * 131) % 960), w, h, 1024, 1024))
                n += 1
    for axis in range(2):                     # the step classes per axis: every filter_2d and both set classes of that axis
        for c, f, big in itertools.product(STEP_CLASSES, range(10), (False, True)):
            lst = [s for s in shapes if (s[axis] > 4) == big and s[0] * s[1] <= 2048]
            w, h = lst[n % len(lst)]
            d = STEPS[c][n % len(STEPS[c])]
            other = STEPS[STEP_CLASSES[(n // 3) % 5]][(n // 7) % len(STEPS[STEP_CLASSES[(n // 3) % 5]])]
            mx, my = PHASE_OFFSETS[n % 8], PHASE_OFFSETS[(n // 2 + 3) % 8]
            rows.append((f, mx, my, w, h) + ((d, other) if axis == 0 else (other, d)))
            n += 1
    for s, (w, h) in enumerate(shapes):       # every legal shape; the widest source windows: 128 at step 2048
        rows.append((s % 10, PHASE_OFFSETS[s % 8], PHASE_OFFSETS[(s + 5) % 8], w, h, 2048 if w == 128 or s % 3 == 0 else 1024, 2048 if h == 128 or s % 4 == 0 else 900))
    return rows


def scaled_phases(mx, w, dx):
    return set((((mx + np.arange(w) * dx) & 0x3ff) >> 6).tolist())


def assert_scaled_coverage(rows, kind, full):
    shapes = scaled_shapes(kind)
    hx, hy, steps_x, steps_y, triples, classes = set(), set(), set(), set(), set(), set()
    for f, mx, my, w, h, dx, dy in rows:
        assert 0 <= mx <= 1023 and 0 <= my <= 1023 and 1 <= dx <= 2048 and 1 <= dy <= 2048
        fxs, fys = scaled_phases(mx, w, dx), scaled_phases(my, h, dy)
        hx.update((f, w > 4, p) for p in fxs)
        hy.update((f, h > 4, p) for p in fys)
        steps_x.add((step_class(dx), f, w > 4))
        steps_y.add((step_class(dy), f, h > 4))
        if dx == 1024 and dy == 1024:
            fx, fy = fxs.pop(), fys.pop()
            triples.add((f, fx, fy, w > 4, h > 4))
            classes.add((f, w > 4, h > 4, fx != 0, fy != 0))
    both = (False, True)
    assert hx == {(f, b, p) for f in range(10) for b in both for p in range(16)}, "every (filter_2d, w > 4, fxi), fxi == 0 included: %d of 320" % len(hx)
    assert hy == {(f, b, p) for f in range(10) for b in both for p in range(16)}, "every (filter_2d, h > 4, fyi), fyi == 0 included: %d of 320" % len(hy)
    assert steps_x == {(c, f, b) for c in STEP_CLASSES for f in range(10) for b in both}, "every horizontal step class x filter_2d x set class"
    assert steps_y == {(c, f, b) for c in STEP_CLASSES for f in range(10) for b in both}, "every vertical step class x filter_2d x set class"
    assert classes == {(f, a, b, c, d) for f in range(10) for a in both for b in both for c in both for d in both}, "every (filter_2d, set class) at the four phase classes"
    assert {(r[3], r[4]) for r in rows} == set(shapes), "every legal shape"
    assert {(r[3], r[5]) for r in rows} >= {(128, 2048)} and {(r[4], r[6]) for r in rows} >= {(128, 2048)}, "the widest source windows"
    assert {r[1] for r in rows} >= {0, 63, 64, 1023} and {r[2] for r in rows} >= {0, 63, 64, 1023}
    assert {t[:3] for t in triples} == set(itertools.product(range(10), range(16), range(16))), "every (filter_2d, fxi, fyi)"
    if full and kind != PUT_TMP:
        assert triples == {t + c for t in itertools.product(range(10), range(16), range(16)) for c in itertools.product(both, both)}, \
            "filter_2d x fxi x fyi x the four set classes"


def place_scaled(rows, dims):
    """(plane, ref, src_x, src_y, sides it leaves on) per row: 5/16 .. 6/16 of the windows leave the plane"""
    out = []
    for k, (f, mx, my, w, h, dx, dy) in enumerate(rows):
        pl, ref = (0, 1, 2, 0)[(k + k // 4) % 4], (k // 2 + f) % 3
        pw, ph = dims[pl]
        ww, wh = ((mx + (w - 1) * dx) >> 10) + 1, ((my + (h - 1) * dy) >> 10) + 1
        cls = (7 * k + 3 * f + k // 16) % 16
        sx, sy = edge_position(cls, k // 16 + f, ww, wh, pw, ph)
        left = sides_left(sx, sy, sx + ww, sy + wh, pw, ph)
        assert (cls < 6) == bool(left) and (cls >= 6 or SIDES[cls] in left), (cls, left, sx, sy, ww, wh)
        out.append((pl, ref, sx, sy, left))
    return out


def assert_scaled_edges(rows, placed):
    n_edge = sum(1 for p in placed if p[4])
    assert 0.2 < n_edge / len(rows) < 0.45, "most windows are inside the plane, a fixed share is not: %d of %d" % (n_edge, len(rows))
    met = {(r[0], s) for r, p in zip(rows, placed) for s in p[4]}
    assert met == {(f, s) for f in range(10) for s in SIDES}, "every filter_2d leaves the plane on every side, at a corner and entirely"
    assert {(p[0], p[1]) for p in placed} == {(pl, r) for pl in range(3) for r in range(3)}, "every (plane, ref)"


def run_scaled(ctx, oracle, bpc, kind, rows, placed, ref_pics, ref_planes, dims, D, what, blends=0):
    """rows through ctx.mc_scaled_batch, every task against test_mcx._oracle_mc_scaled; put blocks packed on shelves of their plane of
    an I420 picture (a new batch when a plane is full).  blends: that many PUT_TMP blocks then go through blend_h / blend_v
    (ctx.comp_batch) onto the destination, as obmc() does.  Returns the oracle's (row index, block) pairs of put and PUT_TMP."""
    pd = util.pix_dtype(bpc)
    dst, pre = make_dst(ctx, bpc, D, D, 60 + bpc + kind)
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][4], -rows[i][3]))
    batches, cur, cursors, off = [], [], {}, 0
    for i in order:
        w, h = rows[i][3], rows[i][4]
        pl = placed[i][0]
        x = y = 0
        if kind == PUT:
            ph, pw = pre[pl].shape
            x, y, shelf = cursors.get(pl, (0, 0, 0))
            if x + w > pw:
                x, y, shelf = 0, y + shelf + 2, 0
            if y + h > ph:
                batches.append(cur)
                cur, cursors, off = [], {}, 0
                x, y, shelf = 0, 0, 0
            cursors[pl] = (x + w + 2, y, max(shelf, h))
        cur.append((i, x, y, off))
        off += w * h
    batches.append(cur)
    out = []
    for batch in batches:
        want = [p.copy() for p in pre]
        n_el = batch[-1][3] + rows[batch[-1][0]][3] * rows[batch[-1][0]][4]
        want_arena = np.zeros(max(n_el, 8), pd if kind == PUT_TMP else np.int16)
        t = np.zeros(len(batch), api.MC_SCALED_TASK)
        for k, (i, x, y, off) in enumerate(batch):
            f, mx, my, w, h, dx, dy = rows[i]
            pl, ref, sx, sy, _ = placed[i]
            t[k] = (y * dst.stride_px(pl) + x if kind == PUT else off, sx, sy, mx, my, dx, dy, w, h, f, kind, pl, ref, (0, 0))
            plane = ref_planes[ref][pl]
            if kind == PUT:
                _oracle_mc_scaled(oracle, bpc, plane, dims[pl][0], dims[pl][1], t[k], dst_block=want[pl][y:, x:])
                out.append((i, want[pl][y:y + h, x:x + w].copy()))
            elif kind == PREP:
                _oracle_mc_scaled(oracle, bpc, plane, dims[pl][0], dims[pl][1], t[k], tmp=want_arena[off:])
            else:
                _oracle_mc_scaled(oracle, bpc, plane, dims[pl][0], dims[pl][1], t[k], dst_block=want_arena[off:off + w * h].reshape(h, w))
                out.append((i, want_arena[off:off + w * h].reshape(h, w).copy()))
        for pl in range(3):
            dst.upload(pl, pre[pl])
        arena = ctx.buffer(len(want_arena) * want_arena.itemsize)
        arena.zero()
        ctx.mc_scaled_batch(dst, ref_pics, t, arena)
        name = lambda k: "(filter_2d, mx, my, w, h, dx, dy) = %s, (plane, ref, src_x, src_y, sides) = %s" % (rows[batch[k][0]], placed[batch[k][0]])
        for pl in range(3):
            got = dst.download(pl)
            bad = np.argwhere(got != want[pl])
            if len(bad):
                yy, xx = bad[0]
                hit = [k for k, (i, x, y, off) in enumerate(batch) if kind == PUT and placed[i][0] == pl and x <= xx < x + rows[i][3] and y <= yy < y + rows[i][4]]
                raise AssertionError("%s, %d bpc scaled %s: (%d,%d) of plane %d is %d, the oracle has %d (before the call: %d); %d pixels differ; task %s" % (
                    what, bpc, KINDS[kind], xx, yy, pl, got[yy, xx], want[pl][yy, xx], pre[pl][yy, xx], len(bad), name(hit[0]) if hit else "none: outside every block"))
        if kind != PUT:
            got_arena = arena.download(want_arena.dtype, len(want_arena))
            bad = np.flatnonzero(got_arena != want_arena)
            if len(bad):
                k = int(np.searchsorted([b[3] for b in batch], bad[0], side="right")) - 1
                raise AssertionError("%s, %d bpc scaled %s: element %d of the arena is %d, the oracle has %d; %d differ; task %s, element %d of it" % (
                    what, bpc, KINDS[kind], bad[0], got_arena[bad[0]], want_arena[bad[0]], len(bad), name(k), bad[0] - batch[k][3]))
        if blends:
            # obmc(): the predictions in the arena onto the destination, blend_h for the first half, blend_v for the second
            legal = lambda w, h: w <= 32 and h <= 32          # within the shapes of both (tests/checkasm/mc.c:496-498, 535-537)
            picks = []
            for k, (i, x, y, off) in enumerate(batch):
                bk = BLEND_H_KIND if len(picks) < blends // 2 else BLEND_V_KIND
                if len(picks) < blends and legal(rows[i][3], rows[i][4]):
                    picks.append((k, bk))
            assert len(picks) == blends and {bk for _, bk in picks} == {BLEND_H_KIND, BLEND_V_KIND}
            ct = np.zeros(len(picks), api.COMP_TASK)
            by = 0
            for j, (k, bk) in enumerate(picks):
                i, _, _, off = batch[k]
                w, h, pl = rows[i][3], rows[i][4], placed[i][0]
                ct[j] = (by * dst.stride_px(pl) + 8, off, 0, 0, w, h, bk, pl, 0, 0, 0)              # one below the other
                blk = want[pl][by:, 8:]
                oracle.call(bpc, "blend_h" if bk == BLEND_H_KIND else "blend_v", 0, 0, blk.ctypes.data, want[pl].strides[0], want_arena[off:off + w * h], w, h)
                by += h + 4
                assert by < want[2].shape[0]
            ctx.comp_batch(dst, ct, arena, None)
            for pl in range(3):
                assert np.array_equal(dst.download(pl), want[pl]), "%s, %d bpc: blend_h / blend_v of scaled PUT_TMP predictions, plane %d" % (what, bpc, pl)
        arena.free()
    dst.free()
    return out


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_scaled_every_filter_phase_and_step(ctx, bpc):
    oracle = util.default_oracle()
    full = ctx.backend != "emu"
    ref_pics, ref_planes, dims = make_refs(ctx, bpc, SC_VIS[0], SC_VIS[1], 4500 + bpc)
    for kind in (PUT, PREP, PUT_TMP):
        rows = scaled_rows(kind, full)
        assert_scaled_coverage(rows, kind, full)
        placed = place_scaled(rows, dims)
        assert_scaled_edges(rows, placed)
        run_scaled(ctx, oracle, bpc, kind, rows, placed, ref_pics, ref_planes, dims, 2048 if full else 1024, "every phase and step", blends=12 if kind == PUT_TMP else 0)
    for p in ref_pics:
        p.free()


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_scaled_extremal_content(ctx, bpc):
    oracle = util.default_oracle()
    if not _signs:
        _signs.append(test_mc_sweep.oracle_tap_signs(oracle))
    signs = _signs[0]
    bdmax = (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    PATCH = test_mc_sweep.PATCH
    triples = list(itertools.product(range(10), range(16), range(16)))
    all_combos = []
    for k, (f, fx, fy) in enumerate(triples):
        all_combos += [(f, fx, fy) + test_mc_sweep.EXT_SHAPES[(k + k // 4 + k // 16) % 4] + (p,) for p in ("worst+", "worst-")]
    for s, (w, h) in enumerate(test_mc_sweep.EXT_SHAPES):
        for f in range(10):
            all_combos += [(f, (3 * s + f) % 16, (5 * s + 7 * f) % 16, w, h, p) for p in test_mc_sweep.PATTERNS]
    assert {c[:3] for c in all_combos if c[5] == "worst+"} == set(triples) == {c[:3] for c in all_combos if c[5] == "worst-"}
    assert {(c[3], c[4], c[5]) for c in all_combos} == {s + (p,) for s in test_mc_sweep.EXT_SHAPES for p in test_mc_sweep.PATTERNS}
    side = 32                        # patches along one side of a reference picture (1536 x 1536)
    lo, hi = [], []
    for c0 in range(0, len(all_combos), side * side):
        combos = all_combos[c0:c0 + side * side]

        def fill(r, planes):
            for k, (f, fx, fy, w, h, p) in enumerate(combos):
                py, px = (k // side) * PATCH, (k % side) * PATCH
                if p in ("zero", "max"):
                    planes[0][py:py + PATCH, px:px + PATCH] = bdmax if p == "max" else 0
                else:
                    prod = signs[f, 1, int(h > 4), fy].astype(np.int32)[:, None] * signs[f, 0, int(w > 4), fx].astype(np.int32)[None, :]
                    win = np.where(prod > 0 if p == "worst+" else prod < 0, bdmax, 0).astype(pd)
                    planes[0][py:py + PATCH, px:px + PATCH] = np.tile(win, (PATCH // 8, PATCH // 8))

        ref_pics, ref_planes, dims = make_refs(ctx, bpc, side * PATCH, side * PATCH, 4600 + bpc, fill)
        rows = [(f, fx * 64 + (k * 29) % 64, fy * 64 + (k * 13) % 64, w, h, 1024, 1024) for k, (f, fx, fy, w, h, p) in enumerate(combos)]
        # block origin at (8 + 3, 8 + 3) of its patch: the window of output (0, 0) starts on the pattern's period
        placed = [(0, k % 3, (k % side) * PATCH + 11, (k // side) * PATCH + 11, set()) for k in range(len(combos))]
        for kind in (PUT, PREP):
            blocks = run_scaled(ctx, oracle, bpc, kind, rows, placed, ref_pics, ref_planes, dims, 1024, "extremal content")
            if kind == PUT:
                lo += [i for i, b in blocks if combos[i][5] == "worst-" and b[0, 0] == 0 and combos[i][1] and combos[i][2]]
                hi += [i for i, b in blocks if combos[i][5] == "worst+" and b[0, 0] == bdmax and combos[i][1] and combos[i][2]]
        for p in ref_pics:
            p.free()
    assert lo and hi, "the oracle's put outputs hold both clips at phases that filter in both directions"


_signs = []


# ------------------------------------------------------------------ resize

def upscale_params(src_w, dst_w):
    """reference src/decode.c:3321-3325 (C division truncates toward zero)"""
    dx = ((src_w << 14) + (dst_w >> 1)) // dst_w
    err = dst_w * dx - (src_w << 14)
    num = -((dst_w - src_w) << 13) + (dst_w >> 1)
    q = abs(num) // dst_w * (1 if num >= 0 else -1)
    e2 = abs(err) // 2 * (1 if err >= 0 else -1)
    return dx, (q + 128 - e2) & 0x3fff


def resize_taps(dst_w, dx, mx0):
    """(filter row, first source column before the clamp) per output column, src/mc_tmpl.c:925-940 restated"""
    rows, cols = [], []
    mx, src_x = mx0, -1
    for _ in range(dst_w):
        rows.append(mx >> 8)
        cols.append(src_x - 3)
        mx += dx
        src_x += mx >> 14
        mx &= 0x3fff
    return np.array(rows), np.array(cols)


@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_resize_every_denominator_and_row(ctx, bpc):
    oracle = util.default_oracle()
    bdmax = (1 << bpc) - 1
    pd = util.pix_dtype(bpc)
    rng = np.random.default_rng(4700 + bpc)
    cases = [(d, sw) for d in range(9, 17) for sw in (16, 17, 255, 512)]
    assert (16, 255) in cases and 16 * 255 >> 3 > 256 and 9 * 255 >> 3 > 256, "a second block column of the 256-wide grid"
    seen_rows, clamps, dens = set(), set(), set()
    H = 8
    for k, (w_den, src_w) in enumerate(cases):
        dst_w = w_den * src_w >> 3
        dx, mx0 = upscale_params(src_w, dst_w)
        rows, first = resize_taps(dst_w, dx, mx0)
        seen_rows |= set(rows.tolist())
        if (first < 0).any():
            clamps.add("left")
        if (first + 7 > src_w - 1).any():
            clamps.add("right")
        dens.add(w_den)
        pl = k % 3
        src = ctx.picture(src_w << (pl > 0), H << (pl > 0), api.LAYOUT_I420, bpc)
        dst = ctx.picture(dst_w << (pl > 0), H << (pl > 0), api.LAYOUT_I420, bpc)
        splanes = [rng.integers(0, 1 << bpc, size=src.padded_shape(p)).astype(pd) for p in range(3)]
        content = ("random", "zero", "max", "alternating")[(k + k // 4) % 4]
        if content != "random":
            xx = np.arange(splanes[pl].shape[1])
            splanes[pl][:] = {"zero": 0 * xx, "max": 0 * xx + bdmax, "alternating": np.where(xx & 1, bdmax, 0)}[content][None, :]
        dplanes = [rng.integers(0, 1 << bpc, size=dst.padded_shape(p)).astype(pd) for p in range(3)]
        for p in range(3):
            src.upload(p, splanes[p])
            dst.upload(p, dplanes[p])
        want = [p.copy() for p in dplanes]
        y0, h = ((0, H), (1, H - 3))[k & 1]
        oracle.call(bpc, "resize", 0, 0, want[pl][y0:].ctypes.data, want[pl].strides[0], splanes[pl][y0:].ctypes.data, splanes[pl].strides[0], dst_w, h, src_w, dx, mx0)
        ctx.resize(dst, src, pl, dst_w, y0, h, src_w, dx, mx0)
        for p in range(3):
            got = dst.download(p)
            bad = np.argwhere(got != want[p])
            assert not len(bad), "resize w_den %d, %d -> %d (dx %d, mx0 %d), plane %d, rows %d .. %d, %s content: plane %d differs at %s (%d px)" % (
                w_den, src_w, dst_w, dx, mx0, pl, y0, y0 + h, content, p, bad[0][::-1], len(bad))
        src.free(); dst.free()
    assert seen_rows == set(range(64)), "all 64 filter rows: %d" % len(seen_rows)
    assert clamps == {"left", "right"} and dens == set(range(9, 17))
