"""The bookkeeping of the paired prediction + residual waves (recon.hip: mc_body.h, itx_body.h) against the oracle, on the smallest
picture at which it can go wrong: 72x40 4:2:0 (not a multiple of 64, an odd count of 8x8 tiles; the allocator's strides — 128 luma,
64 chroma pixels — are padded and differ between the planes), every block of one size class paired with its transform block.

What a wave works out besides pixels, and where these lists take it:

  * the hand-off of the tile records and of the reference table through LDS: 150 / 75 / 27 / 9 blocks of 4x4 / 8x8 / 16x16 / 32x32 leave a
    partial last wave in every class, the 8x8 waves make two prediction calls (the table is staged by the first), n_refs = 1 and 3 with
    a different reference per tile of a wave, one of the references of ANOTHER size than the picture the list was made for;
  * the window gather: source columns at every offset 0 .. 7 inside an 8-pixel piece (both parities), every filter pair of the
    reference's Filter2d including bilinear, every phase including 0 in either direction — the spans of the taps decide which rows and
    pieces of a window are fetched — and blocks on all four edges whose motion vectors reach outside by 1 .. 8 pixels, from rounds that
    shift the displacement by one each: windows inside the picture, across its edge, and exactly on the boundary between the two paths;
  * the combine and the store to the LDS tile: PUT, AVG and WAVG tiles in one list (the list's order puts them into the same waves
    at the seams of its groups and into waves of one kind elsewhere);
  * the transform: dc-only and full blocks, every 2-D transform kind the size has, uniform and mixed waves alike;
  * the way out: luma, U and V blocks in one wave, narrow stores (raster planes), wide stores next to the twin and into the twin only,
    from raster and from tiled references.

Everything is compared bit for bit: the three padded planes, the twin where one is written, the coefficient arena."""
import ctypes as C

import numpy as np
import pytest

import util
from dav1d_amd import api
from dav1d_amd._lib import ITX_TASK, MC_TASK, COMP_TASK
import synth_frames as synth
from test_frame import RP, planes_struct, read_twin

W, H = 72, 40
ODD_REF = (104, 56)         # the size of the reference that is not the picture's
SIZES = {"4x4": 4, "8x8": 8, "16x16": 16, "32x32": 32}
ROUNDS = 3
_cases = {}


def _blocks(s):
    """(x, y, plane) of every block of size s whose origin lies inside the visible plane (the last column and row of blocks reach into
    the padding, as the reference's do), luma first; 4x4: the blocks of the four corners, to keep the emulated run short"""
    out = []
    for pl in range(3):
        pw, ph = (W, H) if pl == 0 else (W // 2, H // 2)
        xs, ys = list(range(0, pw, s)), list(range(0, ph, s))
        if s == 4:
            xs, ys = sorted(set(xs[:5] + xs[-5:])), sorted(set(ys[:3] + ys[-3:]))
        out += [(x, y, pl) for y in ys for x in xs]
    return out[:-1] if s == 32 else out          # (32x32: nine blocks, two to a wave)


def _oracle(frame, dst0, refs_h, ref_sizes):
    """oracle_frame of test_frame.py with a size per reference"""
    rl = util.replay_lib()
    entry = C.cast(util.default_oracle()._entry, C.c_void_p)
    dst = synth.copy_planes(dst0)
    drp = planes_struct(dst, frame.w, frame.h)
    refs = (RP * len(refs_h))(*[planes_struct(r, rw, rh) for r, (rw, rh) in zip(refs_h, ref_sizes)])
    prep = np.zeros(frame.prep_elems, np.int16)
    coef = frame.coef.copy()
    mask = np.zeros(16, np.uint8)
    assert rl.dav1d_replay_mc(entry, frame.bpc, C.byref(drp), refs, frame.mc.ctypes.data, len(frame.mc), prep.ctypes.data) == 0
    assert rl.dav1d_replay_comp(entry, frame.bpc, C.byref(drp), frame.comp.ctypes.data, len(frame.comp), prep.ctypes.data, mask.ctypes.data) == 0
    assert rl.dav1d_replay_itx(entry, frame.bpc, C.byref(drp), frame.itx.ctypes.data, len(frame.itx), coef.ctypes.data) == 0
    return dst, coef


def make_case(s, bpc, n_refs, rnd):
    """(frame, dst planes, reference planes and sizes, the oracle's planes and coefficient arena) of one round, made once"""
    key = (s, bpc, n_refs, rnd)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(1500 + 97 * s + bpc + 7 * n_refs + rnd)
    geo = synth.plane_geometry(W, H, bpc, 1)
    blocks = _blocks(s)
    n = len(blocks)
    tx = synth.SQ_TX[s]
    full, _ = synth.gen_coefs(rng, tx, n, bpc, eob_class_p=(0.0, 0.0, 1.0))
    ncoef = full.shape[1]
    kinds = list(range(10)) if s <= 16 else [0, 9]          # 2-D classes (DCT_DCT .. ) and, at 32x32, the identity
    mc, comp, itx = [], [], []
    coef = np.zeros((n, ncoef), full.dtype)
    prep_off = n_pred = 0
    used = dict.fromkeys("lrtb", 0)

    def reach(side):
        used[side] += 1
        return 1 + (used[side] - 1 + 3 * rnd) % 8

    for i, (x, y, pl) in enumerate(blocks):
        j = i + rnd
        pw, ph = (W, H) if pl == 0 else (W // 2, H // 2)
        off = y * geo[pl][0] + x
        two = j % 4 in (1, 3)
        preds = []
        for r in range(2 if two else 1):
            k = j + 5 * r
            # displacements: the columns walk through all eight offsets of a piece; a block on an edge reaches outside by 1 .. 8 pixels
            dx, dy = k % 8 - 3, (k // 8) % 8 - 3
            on_x = [sd for sd, on in (("l", x == 0), ("r", x + s >= pw)) if on]
            on_y = [sd for sd, on in (("t", y == 0), ("b", y + s >= ph)) if on]
            if on_x:
                sd = on_x[k % len(on_x)]
                dx = -reach(sd) if sd == "l" else pw - x - s + reach(sd)
            if on_y:
                sd = on_y[k % len(on_y)]
                dy = -reach(sd) if sd == "t" else ph - y - s + reach(sd)
            t = np.zeros((), MC_TASK)
            t["src_x"], t["src_y"], t["w"], t["h"] = x + dx, y + dy, s, s
            # phases and filter pairs by the running number of the prediction, continued from round to round (13: the fewest a round has)
            q = n_pred + 13 * rnd
            n_pred += 1
            t["mx"], t["my"] = q % 16, (5 * q + 3) % 16
            t["filter_2d"], t["plane"], t["ref"] = q % 10, pl, (j + r) % n_refs
            if two:
                t["kind"], t["dst_off"] = 1, prep_off
                prep_off += s * s
            else:
                t["kind"], t["dst_off"] = 0, off
            preds.append(t)
        mc += preds
        if two:
            c = np.zeros((), COMP_TASK)
            c["dst_off"], c["tmp1_off"], c["tmp2_off"] = off, preds[0]["dst_off"], preds[1]["dst_off"]
            c["w"] = c["h"] = s
            c["kind"], c["arg"], c["plane"] = (0, 0, pl) if j % 4 == 1 else (1, 1 + j % 15, pl)
            comp.append(c)
        it = np.zeros((), ITX_TASK)
        it["dst_off"], it["cf_off"], it["tx"], it["plane"] = off, i * ncoef, tx, pl
        if j % 3 == 0:                                    # dc-only
            coef[i, 0] = full[i, 0]
            it["eob"], it["txtp"] = 0, 0
        else:
            coef[i] = full[i]
            it["eob"], it["txtp"] = ncoef - 1, kinds[j % len(kinds)]
        itx.append(it)
    f = synth.Frame()
    f.w, f.h, f.bpc, f.n_refs = W, H, bpc, n_refs
    f.mc, f.itx = np.array(mc, MC_TASK), np.array(itx, ITX_TASK)
    f.comp = np.array(comp, COMP_TASK) if comp else np.zeros(0, COMP_TASK)
    f.coef = coef.reshape(-1).copy()
    f.prep_elems = max(prep_off, 8)
    ref_sizes = [ODD_REF if n_refs == 3 and r == 2 else (W, H) for r in range(n_refs)]
    refs = [synth.make_planes(rng, rw, rh, bpc) for rw, rh in ref_sizes]
    dst0 = synth.make_planes(rng, W, H, bpc, smooth=False)
    want, want_coef = _oracle(f, dst0, refs, ref_sizes)
    _cases[key] = (f, dst0, refs, ref_sizes, want, want_coef)
    return _cases[key]


def test_the_lists_hold_what_they_are_for():
    """the generator above, checked once: every column offset and parity, filter pair and phase, kind of tile and of transform, edge and reach"""
    for s in SIZES.values():
        offs, filt, mx, my, reach, kinds, txk, planes = set(), set(), set(), set(), set(), set(), set(), set()
        for rnd in range(ROUNDS):
            f = make_case(s, 10, 3, rnd)[0]
            for t in f.mc:
                pw, ph = (W, H) if t["plane"] == 0 else (W // 2, H // 2)
                offs.add((int(t["src_x"]) - 3) & 7)
                filt.add(int(t["filter_2d"])); mx.add(int(t["mx"])); my.add(int(t["my"]))
                reach.add(("l", -int(t["src_x"]))); reach.add(("t", -int(t["src_y"])))
                reach.add(("r", int(t["src_x"]) + s - pw)); reach.add(("b", int(t["src_y"]) + s - ph))
            kinds |= {("put",)} | {("avg",) if c["kind"] == 0 else ("wavg",) for c in f.comp}
            txk |= {(int(t["txtp"]), int(t["eob"]) == 0) for t in f.itx}
            planes |= {int(t["plane"]) for t in f.itx}
        assert offs == set(range(8)) and filt == set(range(10)) and mx == set(range(16)) and my == set(range(16)), s
        for side in "ltrb":
            assert {d for e, d in reach if e == side} >= set(range(1, 9)), (s, side)
        assert kinds == {("put",), ("avg",), ("wavg",)} and planes == {0, 1, 2}, s
        assert {k for k, dc in txk if not dc} == (set(range(10)) if s <= 16 else {0, 9}) and (0, True) in txk, s


FORMS = ["raster-refs", "tiled-refs", "raster+twin", "twin-only"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_refs", [1, 3])
@pytest.mark.parametrize("bpc", [10, 8])
@pytest.mark.parametrize("size", list(SIZES))
def test_paired_waves_against_the_oracle(ctx, size, bpc, n_refs, form):
    s = SIZES[size]
    ctx.set_option("recon_fuse", 15)
    ctx.set_option("recon_coop_below", 0)            # one wave per group: the form the step runs (the cooperative one: test_write_out_planes.py)
    for rnd in range(ROUNDS):
        frame, dst0, refs_h, ref_sizes, want, want_coef = make_case(s, bpc, n_refs, rnd)
        refs = []
        for rp, (rw, rh) in zip(refs_h, ref_sizes):
            r = ctx.picture(rw, rh, api.LAYOUT_I420, bpc)
            for pl in range(3):
                r.upload(pl, rp[pl])
            if form != "raster-refs":
                r.retile()
            refs.append(r)
        prep = ctx.buffer(frame.prep_elems * 2)
        prep.zero()
        dst = ctx.picture(W, H, api.LAYOUT_I420, bpc)
        for pl in range(3):
            dst.upload(pl, dst0[pl])
        coef = ctx.buffer_from(frame.coef)
        rl = ctx.recon_list(dst, frame.mc, frame.comp, frame.itx)
        try:
            twin = None
            if form in ("raster-refs", "tiled-refs"):
                rl.run(dst, refs, prep, coef)
            elif form == "raster+twin":
                rl.run_twin(dst, refs, prep, coef)
                assert dst.pic.twin_ok == 1
                twin = [read_twin(ctx, dst, pl) for pl in range(3)]
            else:
                rl.run_tiled(dst, refs, prep, coef)
                assert dst.pic.twin_ok == api.TWIN_ONLY, "the launches did not write the twin themselves"
            got = [dst.download(pl) for pl in range(3)]
            got_coef = coef.download(frame.coef.dtype, len(frame.coef))
        finally:
            rl.destroy()
            for o in refs + [prep, dst, coef]:
                o.free()
        covered = [np.zeros(want[pl].shape, bool) for pl in range(3)]
        for t in frame.itx:
            sp = synth.plane_geometry(W, H, bpc, 1)[t["plane"]][0]
            y, x = divmod(int(t["dst_off"]), sp)
            covered[t["plane"]][y:y + s, x:x + s] = True
        for pl in range(3):
            bad = np.argwhere(got[pl] != want[pl])
            assert not len(bad), "round %d: plane %d differs at %s (%d px)" % (rnd, pl, bad[0], len(bad))
            if twin is not None:
                # (run_twin leaves in the twin what the list writes)
                th, tw = min(twin[pl].shape[0], want[pl].shape[0]), want[pl].shape[1]
                bad = np.argwhere((twin[pl][:th, :tw] != want[pl][:th]) & covered[pl][:th])
                assert not len(bad), "round %d: twin of plane %d differs at %s (%d px)" % (rnd, pl, bad[0], len(bad))
        assert np.array_equal(got_coef, want_coef), "round %d: coefficient slabs" % rnd
