"""The shapes at which tile_write_out (itx_body.h) can pick a wrong plane or position for a piece, against the oracle.

The paired kernels pack 16 / 8 / 4 / 2 blocks of 4x4 / 8x8 / 16x16 / 32x32 pixels into a wave and store them in rounds of 64 row pieces;
each piece's stride, plane pointer and twin pointer are picked by the plane of ITS block (one scalar plane per round for 32x32 blocks,
two for 16x16 ones, a lane's own for the small sizes).  A picture of 2 x 2 blocks whose recon list holds three luma blocks and the U
and the V block puts luma and chroma blocks side by side in one wave and leaves a partial last wave:

    16x16 (32x32 picture):  waves (L, L, L, U) (V)       two planes in one round, a last wave of one block
    32x32 (64x64 picture):  waves (L, L) (L, U) (V)      two planes in a wave, a last wave of one block
    8x8, 4x4 (16x16, 8x8):  one wave holds all five      three planes among the lanes of one round

(every block reads the same reference with even source columns and the same transform path: the list's orderings keep L, L, L, U, V).
Each runs at 8 and 10 bits, into the three states a picture can be left in (raster planes, raster + twin, twin only), with 1 and 3
references — the reference table a small-tile wave copies to LDS has n_refs entries, and the blocks read the LAST one — as one wave
per group and in the cooperative form, and with one block whose window crosses the picture's corner (the edge-emulation loads).
Pixels, twins and zeroed coefficient slabs are compared."""
import numpy as np
import pytest

import util
from dav1d_amd import api
from dav1d_amd._lib import ITX_TASK, MC_TASK, COMP_TASK
import synth_frames as synth
from test_frame import oracle_frame, read_twin

SIZES = {"4x4": 4, "8x8": 8, "16x16": 16, "32x32": 32}
_cases = {}


def make_case(s, bpc, n_refs):
    """(frame, dst planes, reference planes, the oracle's planes and coefficient arena), made once per shape"""
    key = (s, bpc, n_refs)
    if key in _cases:
        return _cases[key]
    w = h = 2 * s
    geo = synth.plane_geometry(w, h, bpc, 1)
    rng = np.random.default_rng(1400 + s + bpc + n_refs)
    # (x, y, plane): three luma blocks, then the chroma blocks (each covers its whole s x s plane)
    blocks = [(0, 0, 0), (s, 0, 0), (0, s, 0), (0, 0, 1), (0, 0, 2)]
    n = len(blocks)
    tx = synth.SQ_TX[s]
    mc = np.zeros(n, MC_TASK)
    itx = np.zeros(n, ITX_TASK)
    cf, _ = synth.gen_coefs(rng, tx, n, bpc, eob_class_p=(0.0, 0.0, 1.0))      # full blocks, DCT_DCT: one transform path
    eob = np.full(n, cf.shape[1] - 1)
    for i, (x, y, pl) in enumerate(blocks):
        off = y * geo[pl][0] + x
        # the first block's window hangs over the picture's top-left corner; the others stay inside where the size allows (even columns)
        sx, sy = (x - 6, y - 4) if i == 0 else (x + 2, y + 1)
        mc[i] = (off, sx, sy, s, s, 4 if pl == 0 else 6, 10, 0, 0, pl, n_refs - 1, 0)
        itx[i]["dst_off"], itx[i]["cf_off"], itx[i]["eob"] = off, i * cf.shape[1], eob[i]
        itx[i]["tx"], itx[i]["txtp"], itx[i]["plane"] = tx, 0, pl
    f = synth.Frame()
    f.w, f.h, f.bpc, f.n_refs = w, h, bpc, n_refs
    f.mc, f.comp, f.itx, f.coef = mc, np.zeros(0, COMP_TASK), itx, cf.reshape(-1).copy()
    f.prep_elems = 8
    refs = [synth.make_planes(rng, w, h, bpc) for _ in range(n_refs)]
    dst0 = synth.make_planes(rng, w, h, bpc, smooth=False)
    want, _, want_coef = oracle_frame(util.default_oracle(), f, dst0, refs)
    assert not want_coef.any()
    _cases[key] = (f, dst0, refs, want, want_coef)
    return _cases[key]


@pytest.mark.parametrize("state", ["raster", "raster+twin", "twin-only"])
@pytest.mark.parametrize("n_refs", [1, 3])
@pytest.mark.parametrize("bpc", [8, 10])
@pytest.mark.parametrize("size", list(SIZES))
def test_blocks_of_three_planes_in_one_wave(ctx, size, bpc, n_refs, state):
    s = SIZES[size]
    frame, dst0, refs_h, want, want_coef = make_case(s, bpc, n_refs)
    w, h = frame.w, frame.h
    ctx.set_option("recon_fuse", 15)
    refs = []
    for rp in refs_h:
        r = ctx.picture(w, h, api.LAYOUT_I420, bpc)
        for pl in range(3):
            r.upload(pl, rp[pl])
        r.retile()                     # the launches only write a twin themselves when they read their references through twins
        refs.append(r)
    prep = ctx.buffer(frame.prep_elems * 2)
    prep.zero()
    try:
        for form, coop_below in (("one wave per group", 0), ("cooperative", 4096)):
            ctx.set_option("recon_coop_below", coop_below)
            dst = ctx.picture(w, h, api.LAYOUT_I420, bpc)
            for pl in range(3):
                dst.upload(pl, dst0[pl])
            coef = ctx.buffer_from(frame.coef)
            rl = ctx.recon_list(dst, frame.mc, frame.comp, frame.itx)
            if state == "raster":
                rl.run(dst, refs, prep, coef)
            elif state == "raster+twin":
                rl.run_twin(dst, refs, prep, coef)
                assert dst.pic.twin_ok == 1
                twin = [read_twin(ctx, dst, pl) for pl in range(3)]
            else:
                rl.run_tiled(dst, refs, prep, coef)
                assert dst.pic.twin_ok == api.TWIN_ONLY
                raw = np.zeros((dst.padded_shape(0)[0], dst.stride_px(0)), dst.dtype)
                ctx.sync()
                assert ctx.lib.dav1d_hip_download(ctx.h, raw.ctypes.data, dst.pic.p[0].data, raw.nbytes) == 0
                assert np.array_equal(raw[:, :dst0[0].shape[1]], dst0[0]), (form, "the raster planes were written")
            got = [dst.download(pl) for pl in range(3)]
            got_coef = coef.download(frame.coef.dtype, len(frame.coef))
            rl.destroy()
            dst.free()
            coef.free()
            for pl in range(3):
                bad = np.argwhere(got[pl] != want[pl])
                assert not len(bad), "%s: plane %d differs at %s (%d px)" % (form, pl, bad[0], len(bad))
                if state == "raster+twin":
                    # (run_twin leaves in the twin what the list writes: the fourth luma block, which no task covers, is not compared)
                    vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
                    diff = twin[pl][:vh, :vw] != want[pl][:vh, :vw]
                    if pl == 0:
                        diff[s:, s:] = False
                    bad = np.argwhere(diff)
                    assert not len(bad), "%s: twin of plane %d differs at %s (%d px)" % (form, pl, bad[0], len(bad))
            assert np.array_equal(got_coef, want_coef), (form, "coefficient slabs")
    finally:
        for o in refs + [prep]:
            o.free()
