"""The tone part of a colour handle through the sized calls: dav1d_hip_surface_export_rgb_colour_reduced,
dav1d_hip_surface_export_rgb_linear_reduced and their batches.  tests/test_surface_tone.py holds the restatement of step 1b (`tone`), the full-size
call, the helper and the refusals.

The oracles are the ones the two families have, with `tone` put between the light and the matrix: for the code-value family the light is
lin[test_surface_rgb.rgb_values(test_surface_reduced.reduced_planes(...))], for the linear-light family it is test_surface_linear.light_of(sums(...));
steps 2 to 4 are test_surface_linear.after_light either way.  Every comparison is exact, padding included; a batch is compared with its single calls
byte for byte.  Every case with `ctx` runs on the emulated build and, under -m gpu, on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import util
import test_surface_colour as tc
import test_surface_linear as ln
import test_surface_reduced as rd
import test_surface_tone as tn
from dav1d_amd import api
from test_surface import Dest
from test_surface_rgb_scaled import even_crop, same_bytes
from util import make_source

EINVAL = 22
I400, I420, I422, I444 = api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
F32, F16 = api.SAMPLE_F32, api.SAMPLE_F16
f32 = np.float32

# a handful of test_surface_reduced.GEOMS: over 8:1 with chroma under it; 9:1; a crop whose 4:2:0 chroma window starts at 7 mod 8; 20:1 across
# while down goes up; exactly 8:1 across; more outputs across than a cell holds
GEOMS = [rd.GEOMS[k] for k in (0, 1, 6, 8, 10, 11)]
CASES = tc.CASES          # (bpc, layout, raster / twin-only)
COMBOS = tc.COMBOS        # (stage, format, sample, normalisation, chroma_pos): 144
FAMILIES = ("colour_reduced", "linear_reduced")


_deal_rng = np.random.default_rng(42008)
DEAL = {family: _deal_rng.permutation(len(COMBOS)) for family in FAMILIES}


def combo_of(case, gi, family):
    """24 cases x 6 geometries = 144 = len(COMBOS): a fixed permutation per family, so that every family meets every combination exactly once (a
    multiplier as in test_surface_colour_reduced.combo_of leaves a geometry without any stage that has a matrix: the seed is one under which every
    geometry and every depth, layout and state meets every value of every option — test_the_cases_meet_every_combination)"""
    return COMBOS[DEAL[family][case * len(GEOMS) + gi]]


def want_colour_reduced(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tables, tone_part, scale=None, bias=None, planes=None):
    lin, m, enc = tables
    planes = planes if planes is not None else rd.reduced_planes(vis, layout, dw, dh, crop)
    l = tn.light(planes, layout, bpc, pos, lin)
    return ln.after_light(tn.tone(l, *tone_part) if tone_part is not None else l, sample, fmt, m, enc, scale, bias)


def want_linear_reduced(vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tables, tone_part, scale=None, bias=None):
    lin, m, enc = tables
    q, e = ln.q_of(lin)
    l = ln.light_of(ln.sums(vis, layout, bpc, dw, dh, crop, pos, q), e)
    return ln.after_light(tn.tone(l, *tone_part) if tone_part is not None else l, sample, fmt, m, enc, scale, bias)


WANT = {"colour_reduced": want_colour_reduced, "linear_reduced": want_linear_reduced}


def single(pic, family):
    return pic.export_rgb_colour_reduced if family == "colour_reduced" else pic.export_rgb_linear_reduced


def batch(ctx, family):
    return ctx.export_rgb_colour_reduced_batch if family == "colour_reduced" else ctx.export_rgb_linear_reduced_batch


def check(ctx, pic, family, colour, want, dw, dh, fmt, sample, crop=None, pos=0, scale=None, bias=None, rows=(0, 1 << 30), what="", **kw):
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        single(pic, family)(d.surface, colour, crop, pos, scale, bias, rows[0], rows[1])
        d.check(want, rows=None if rows == (0, 1 << 30) else [rows] * len(want),
                what="toned %s %s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d chroma_pos %d" % (family, what, pic.w, pic.h, dw, dh, crop, pic.bpc,
                                                                                                              pic.layout, fmt, sample, pos))
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 1. random tables against numpy

def test_the_cases_meet_every_combination():
    assert len(COMBOS) == 144 and len(CASES) * len(GEOMS) == 144
    for family in FAMILIES:
        met = {}
        for case in range(len(CASES)):
            for gi in range(len(GEOMS)):
                met.setdefault(combo_of(case, gi, family), []).append((CASES[case], gi))
        assert set(met) == set(COMBOS) and all(len(v) == 1 for v in met.values()), family
        for index in range(5):          # every geometry and every depth, layout and state meets every value of every option
            values = {c[index] for c in COMBOS}
            for gi in range(len(GEOMS)):
                assert {combo_of(case, gi, family)[index] for case in range(len(CASES))} == values, (family, index, gi)
            for part in range(3):
                for v in {c[part] for c in CASES}:
                    assert {combo_of(case, gi, family)[index] for case in range(len(CASES)) if CASES[case][part] == v for gi in range(len(GEOMS))} == values, (family, index, part, v)
    assert all(combo_of(case, gi, FAMILIES[0]) != combo_of(case, gi, FAMILIES[1]) for case in range(len(CASES)) for gi in range(len(GEOMS)))


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%dbit-l%d-%s" % c for c in CASES])
def test_random_tables(ctx, case):
    bpc, layout, state = CASES[case]
    rng = np.random.default_rng(42000 + case)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    handles = {st: tn.toned(ctx, *tc.tables_of(st, lin, m, enc), tone_part=tp, bpc=bpc) for st in tc.STAGES}
    pics = {}
    try:
        for gi, ((w, h), crop, (dw, dh)) in enumerate(GEOMS):
            if (w, h) not in pics:
                pics[w, h] = make_source(ctx, np.random.default_rng(42100 + 100 * bpc + 10 * layout + w), w, h, layout, bpc, state, extremes=True)
            pic, vis = pics[w, h]
            crop = even_crop(crop, layout) if crop else None
            for family in FAMILIES:
                st, fmt, sample, norm, pos = combo_of(case, gi, family)
                scale = [f32(v) for v in rng.uniform(0.5, 2, 3)] if norm else None
                bias = [f32(v) for v in rng.uniform(-1, 1, 3)] if norm else None
                want = WANT[family](vis, layout, bpc, dw, dh, crop, fmt, sample, pos, tc.tables_of(st, lin, m, enc), tp, scale, bias)
                check(ctx, pic, family, handles[st], want, dw, dh, fmt, sample, crop, pos, scale, bias, what="%s %s norm %d" % (state, st, norm))
            assert pic.pic.twin_ok == (api.TWIN_ONLY if state == "twin-only" else 0)
    finally:
        ctx.sync()
        for pic, _ in pics.values():
            pic.free()
        for hd in handles.values():
            ctx.colour_destroy(hd)


# ------------------------------------------------------------------------------------------------ the batches are their single calls

SRC = (168, 60)
ITEMS = [(None, (18, 6)), (None, (90, 33)), ((20, 10, 32, 44), (56, 5)), ((10, 6, 99, 41), (99, 41)), ((0, 0, 128, 60), (1, 1))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("bpc,layout", [(10, I420), (12, I444)], ids=["10bit-420", "12bit-444"])
def test_a_toned_batch_is_its_single_calls(ctx, bpc, layout, family):
    """items over 8:1, under it, up across with 8.8:1 down, at d == s and to 1 x 1, from a raster and a twin-only picture of two layouts in one batch: every item
    against numpy and against the bytes of its single call"""
    rng = np.random.default_rng(42200 + 10 * bpc + layout)
    tables = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    colour = tn.toned(ctx, *tables, tone_part=tp, bpc=bpc)
    a = make_source(ctx, rng, SRC[0], SRC[1], layout, bpc, "raster", extremes=True)
    b = make_source(ctx, rng, SRC[0], SRC[1], I420 if layout == I444 else I444, bpc, "twin-only")
    try:
        items = [((a, b)[k & 1],) + ITEMS[k] for k in range(len(ITEMS))]
        for fmt, sample, pos, norm in ((P, F32, 2, False), (K4, F16, 1, True)):
            scale, bias = ([f32(2), f32(0.5), f32(1)], [f32(-1), f32(0.25), f32(0)]) if norm else (None, None)
            dests = [Dest(ctx, size[0], size[1], src[0].layout, bpc, fmt, sample) for src, _, size in items]
            crops = [even_crop(crop, src[0].layout) if crop else None for src, crop, _ in items]
            batch(ctx, family)([d.surface for d in dests], [src[0] for src, _, _ in items], colour, [c or (0, 0) + SRC for c in crops], pos, scale, bias)
            for k, ((src, _, (dw, dh)), crop, d) in enumerate(zip(items, crops, dests)):
                d.check(WANT[family](src[1], src[0].layout, bpc, dw, dh, crop, fmt, sample, pos, tables, tp, scale, bias), what="toned %s batch, item %d" % (family, k))
                one = Dest(ctx, dw, dh, src[0].layout, bpc, fmt, sample)
                single(src[0], family)(one.surface, colour, crop, pos, scale, bias)
                same_bytes(one, d)
                one.free()
                d.free()
        assert a[0].pic.twin_ok == 0 and b[0].pic.twin_ok == api.TWIN_ONLY
    finally:
        ctx.sync()
        a[0].free()
        b[0].free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 2. exact anchors, in both families

@pytest.mark.parametrize("family", FAMILIES)
def test_anchors(ctx, family):
    """a gain of ones writes the bytes of the un-toned handle; k = 0 with gain[0] = 2 those of an un-toned handle whose lin is doubled (in the
    linear-light family q is the same table under an exponent one higher, so l doubles exactly); a toned and an un-toned handle alternate back to
    back, six exports with no sync in between, and each writes its own bytes"""
    (w, h), bpc, layout = (170, 62), 10, I420
    rng = np.random.default_rng(42300)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    two = np.full(tn.ENC_N, 0x4200, np.uint16)
    two[0] = 0x4000
    hs = {"plain": ctx.colour(lin, m, enc, bpc=bpc), "ones": tn.toned(ctx, lin, m, enc, (tp[0], tn.ONES), bpc), "doubled": ctx.colour((lin * f32(2)).astype(f32), m, enc, bpc=bpc),
          "two": tn.toned(ctx, lin, m, enc, ([0, 0, 0], two), bpc), "toned": tn.toned(ctx, lin, m, enc, tp, bpc)}
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    geoms = [((14, 14, 150, 40), (7, 3)), (None, (96, 34)), ((8, 4, 24, 24), (40, 40))]
    try:
        for crop, (dw, dh) in geoms:
            for x, y in (("plain", "ones"), ("doubled", "two")):
                a, b = Dest(ctx, dw, dh, layout, bpc, K4, F16), Dest(ctx, dw, dh, layout, bpc, K4, F16)
                single(pic, family)(a.surface, hs[x], crop, 1)
                single(pic, family)(b.surface, hs[y], crop, 1)
                same_bytes(a, b)
                a.free()
                b.free()
        dests = [Dest(ctx, dw, dh, layout, bpc, P, F32) for _, (dw, dh) in geoms + geoms]
        ctx.sync()
        for k, (crop, _) in enumerate(geoms + geoms):          # no sync in between
            single(pic, family)(dests[k].surface, hs["toned" if k & 1 else "plain"], crop, 2)
        ctx.sync()
        for k, (crop, (dw, dh)) in enumerate(geoms + geoms):
            dests[k].check(WANT[family](vis, layout, bpc, dw, dh, crop, P, F32, 2, (lin, m, enc), tp if k & 1 else None), what="%s export %d of six" % (family, k))
            dests[k].free()
    finally:
        pic.free()
        for hd in hs.values():
            ctx.colour_destroy(hd)


# ------------------------------------------------------------------------------------------------ 4. workgroups that loop, 5. bands

def test_workgroups_that_loop(ctx):
    """the export kernel of the code-value family behind its item table: 1030 x 130 at its own size, colour_cells 2, 3 and 64"""
    w, h, layout, bpc = 1030, 130, I420, 10
    rng = np.random.default_rng(42400)
    tables = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    colour = tn.toned(ctx, *tables, tone_part=tp, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        want = tn.expect(vis, layout, bpc, K4, F16, 1, *tables, tone_part=tp)          # d == s: Q is the picture
        for cells in (2, 3, 64):
            ctx.set_option("colour_cells", cells)
            check(ctx, pic, "colour_reduced", colour, want, w, h, K4, F16, None, 1, what="colour_cells %d" % cells)
    finally:
        ctx.set_option("colour_cells", 0)
        ctx.sync()
        pic.free()
        ctx.colour_destroy(colour)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pos", [1, 2])
def test_bands_sentinels_and_the_source(ctx, pos, family):
    (w, h), crop, (dw, dh), bpc, layout = (200, 330), None, (21, 35), 10, I420
    rng = np.random.default_rng(42500 + pos)
    tables = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    colour = tn.toned(ctx, *tables, tone_part=tp, bpc=bpc)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        twin = util.twin_bytes(ctx, pic)
        want = WANT[family](vis, layout, bpc, dw, dh, crop, K4, F16, pos, tables, tp)
        whole = Dest(ctx, dw, dh, layout, bpc, K4, F16)
        for r0 in range(0, dh, 6):
            r1 = min(r0 + 6, dh)
            check(ctx, pic, family, colour, want, dw, dh, K4, F16, crop, pos, rows=(r0, r1), what="band [%d, %d)" % (r0, r1))
            single(pic, family)(whole.surface, colour, crop, pos, row0=r0, row1=r1 if r1 < dh else 1 << 30)
        whole.check(want, what="the union of the bands")
        whole.free()
        assert pic.pic.twin_ok == api.TWIN_ONLY and np.array_equal(util.twin_bytes(ctx, pic), twin)
    finally:
        pic.free()
        ctx.colour_destroy(colour)


# ------------------------------------------------------------------------------------------------ 6. the linear path's table

@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_the_light_table_of_a_toned_handle(ctx, bpc):
    """q and e do not know the tone part; a toned handle whose lin has a negative entry is created, serves the other calls, and is refused by the
    linear-light calls exactly as an un-toned one"""
    rng = np.random.default_rng(42600 + bpc)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    plain, toned = ctx.colour(lin, m, enc, bpc=bpc), tn.toned(ctx, lin, m, enc, tp, bpc)
    qa, ea = ctx.colour_light_table(plain, bpc)
    qb, eb = ctx.colour_light_table(toned, bpc)
    wq, we = ln.q_of(lin)
    assert ea == eb == we and np.array_equal(qa, qb) and np.array_equal(qb, wq)
    ctx.colour_destroy(plain)
    ctx.colour_destroy(toned)
    neg = lin.copy()
    neg[7] = -neg[7]
    h = tn.toned(ctx, neg, tone_part=tp, bpc=bpc)
    pic, vis = make_source(ctx, rng, 64, 32, I444, bpc, "raster")
    d, e = Dest(ctx, 8, 4, I444, bpc, P, F32), Dest(ctx, 64, 32, I444, bpc, P, F32)
    try:
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            ctx.colour_light_table(h, bpc)
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            pic.export_rgb_linear_reduced(d.surface, h)
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            ctx.export_rgb_linear_reduced_batch([d.surface], [pic], h)
        d.check(None, what="a refused export")
        pic.export_rgb_colour(e.surface, h)
        e.check(tn.expect(vis, I444, bpc, P, F32, 0, neg, tone_part=tp), what="a lin with a negative entry through export_rgb_colour")
        pic.export_rgb_colour_reduced(d.surface, h)
        d.check(want_colour_reduced(vis, I444, bpc, 8, 4, None, P, F32, 0, (neg, None, None), tp), what="... and through export_rgb_colour_reduced")
    finally:
        d.free()
        e.free()
        pic.free()
        ctx.colour_destroy(h)


# ------------------------------------------------------------------------------------------------ 10. the tensor functions

def _torch_child():
    """(a process of its own, for the reason tests/test_surface.py gives)"""
    import torch
    w, h, bpc, layout = 520, 180, 10, I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(42700)
    lin, m, enc, has_matrix, has_enc, k, gain, has_gain = api.colour_tables_toned(tctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)          # PQ / BT.2020 to sRGB / BT.709
    assert has_matrix and has_enc and has_gain
    tables, tp = (lin, m.reshape(9), enc), (k, gain)
    colour = tctx.colour_for(bpc, 16, 9, 13, 1, 203.0, 1000.0, luminance=True)
    crops = [None, (20, 10, 64, 90), (14, 14, 33, 21), (0, 0, 512, 160)]
    rects = [c if c is not None else (0, 0, w, h) for c in crops]
    srcs = [make_source(tctx, rng, w, h, layout, bpc, state, extremes=True) for state in ("twin-only", "raster", "twin-only", "retiled")]
    pics = [s[0] for s in srcs]

    def bits(t):
        return t.cpu().numpy().view(np.uint16)
    for linear_light, want_of in ((False, want_colour_reduced), (True, want_linear_reduced)):
        t = torch.full((4, 3, 24, 40), 7.0, dtype=torch.float16, device="cuda")
        api.export_colour_batch_to_tensor(pics, t, colour, crops=rects, chroma_pos=api.CHROMA_VERTICAL, linear_light=linear_light)
        tctx.sync()
        for i, (pic, vis) in enumerate(srcs):
            want = want_of(vis, layout, bpc, 40, 24, crops[i], P, F16, 1, tables, tp)
            assert all(np.array_equal(bits(t[i, c]), want[c].view(np.uint16)) for c in range(3)), "(4, 3, 24, 40) item %d, linear_light %s" % (i, linear_light)
        assert 0.0 <= float(t.float().min()) and float(t.float().max()) <= 1.0, "sRGB code values in [0, 1]"
        for crop in (None, (0, 0, 512, 160)):
            t = torch.full((24, 40, 4), 7.0, dtype=torch.float16, device="cuda")
            api.export_colour_to_tensor(pics[0], t, colour, crop=crop, chroma_pos=api.CHROMA_VERTICAL, linear_light=linear_light)
            tctx.sync()
            want = want_of(srcs[0][1], layout, bpc, 40, 24, crop, K4, F16, 1, tables, tp)[0]
            assert np.array_equal(bits(t).reshape(24, 40 * 4), want.view(np.uint16)), "HWC float16 tensor, crop %s, linear_light %s" % (crop, linear_light)
    assert [p.pic.twin_ok for p in pics] == [api.TWIN_ONLY, 0, api.TWIN_ONLY, 1]
    tctx.sync()
    for pic, _ in srcs:
        pic.free()
    tctx.colour_destroy(colour)
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_colour_to_tensor_with_a_toned_handle():
    """export_colour_batch_to_tensor into (4, 3, 24, 40) float16 and export_colour_to_tensor into (24, 40, 4) float16 with the handle of
    colour_for(luminance=True), on code values and in linear light"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
