"""dav1d_hip_colour_update_tone (dav1d_amd/csrc/surface_stats.hip): the tone part of a LIVE colour handle replaced in stream order.
Exports enqueued before the call use the old part, exports enqueued after it the new one, with no sync in between — byte for byte what fresh handles
of those parts write, through every family that takes a handle.  Every case with `ctx` runs on the emulated build and, under -m gpu, on the device."""
import ctypes as C

import numpy as np
import pytest

import util
import test_surface_colour as tc
import test_surface_scaled as tsc
import test_surface_tone as tn
import test_surface_tone_sized as tz
from dav1d_amd import api
from dav1d_amd._lib import ColourTone
from test_surface import Dest

EINVAL, EXDEV = 22, 18
I420 = api.LAYOUT_I420
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
F32, F16 = api.SAMPLE_F32, api.SAMPLE_F16
ENC_N = tc.ENC_N
f32 = np.float32
FAMILIES = ("full", "colour_reduced", "linear_reduced")


def export(pic, family, surface, colour, pos):
    if family == "full":
        pic.export_rgb_colour(surface, colour, pos)
    else:
        tz.single(pic, family)(surface, colour, None, pos)


@pytest.mark.parametrize("family", FAMILIES)
def test_three_exports_alternate_between_two_tone_parts(ctx, family):
    """part A (the handle's own), update to B, update back to A: three exports and two updates with no sync, each export against the bytes a FRESH
    handle of its part writes and against numpy; the caller's gain is overwritten as soon as the update returns"""
    w, h, bpc, layout = 131, 19, 10, I420
    dw, dh = (w, h) if family == "full" else (40, 11)
    rng = np.random.default_rng(52000 + FAMILIES.index(family))
    lin, m, enc = tc.random_tables(rng, bpc)
    parts = [tn.random_tone(rng), tn.random_tone(rng)]
    live = ctx.colour(lin, m, enc, bpc=bpc, tone=parts[0])
    fresh = [ctx.colour(lin, m, enc, bpc=bpc, tone=tp) for tp in parts]
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    configs = [(K4, F16, 1), (P, F32, 2), (K3, F16, 0)]
    got = [Dest(ctx, dw, dh, layout, bpc, fmt, sample) for fmt, sample, _ in configs]
    ref = [Dest(ctx, dw, dh, layout, bpc, fmt, sample) for fmt, sample, _ in configs]
    try:
        for j, (fmt, sample, pos) in enumerate(configs):
            export(pic, family, ref[j].surface, fresh[j & 1], pos)
        ctx.sync()
        before = tsc._live(ctx), int(ctx.lib.dav1d_hip_light_stats_alive())
        for j, (fmt, sample, pos) in enumerate(configs):          # no sync in between
            if j:
                k, gain = np.array(parts[j & 1][0]), np.array(parts[j & 1][1])
                ctx.colour_update_tone(live, (k, gain))
                gain[:] = 0x7BFF          # the caller's arrays are the caller's again
                k[:] = 0
            export(pic, family, got[j].surface, live, pos)
        ctx.sync()
        assert (tsc._live(ctx), int(ctx.lib.dav1d_hip_light_stats_alive())) == before
        for j, (fmt, sample, pos) in enumerate(configs):
            tz.same_bytes(got[j], ref[j])
            tp = parts[j & 1]
            if family == "full":
                want = tn.expect(vis, layout, bpc, fmt, sample, pos, lin, m, enc, tp)
            else:
                want = tz.WANT[family](vis, layout, bpc, dw, dh, None, fmt, sample, pos, (lin, m, enc), tp)
            got[j].check(want, what="%s, export %d of three" % (family, j))
        if family == "linear_reduced":          # the light table in fixed point is what it was
            qa, ea = ctx.colour_light_table(live, bpc)
            qb, eb = ctx.colour_light_table(fresh[0], bpc)
            assert ea == eb and np.array_equal(qa, qb)
    finally:
        for d in got + ref:
            d.free()
        pic.free()
        for hd in [live] + fresh:
            ctx.colour_destroy(hd)


def test_more_updates_than_the_staging_ring_has_slots(ctx):
    """six updates back to back with one export behind each: the ring's slots come round again"""
    w, h, bpc, layout = 67, 19, 8, I420
    rng = np.random.default_rng(52100)
    lin, m, enc = tc.random_tables(rng, bpc)
    parts = [tn.random_tone(rng) for _ in range(6)]
    live = ctx.colour(lin, m, enc, bpc=bpc, tone=tn.random_tone(rng))
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "raster")
    got = [Dest(ctx, w, h, layout, bpc, K4, F16) for _ in parts]
    try:
        for d, tp in zip(got, parts):
            ctx.colour_update_tone(live, tp)
            pic.export_rgb_colour(d.surface, live, 1)
        for j, (d, tp) in enumerate(zip(got, parts)):
            d.check(tn.expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, tp), what="update %d of six" % j)
    finally:
        for d in got:
            d.free()
        pic.free()
        ctx.colour_destroy(live)


def test_python_update_with_a_gain_that_has_to_be_copied(ctx):
    """Context.colour_update_tone with gain as a list, an int32 array, a strided view and a float16 array: each is copied to contiguous uint16 inside the
    call, and the copy has to live until the library has staged it — the bytes are those of the contiguous uint16 array"""
    w, h, bpc, layout = 67, 19, 10, I420
    rng = np.random.default_rng(52400)
    lin, m, enc = tc.random_tables(rng, bpc)
    live = ctx.colour(lin, m, enc, bpc=bpc, tone=tn.random_tone(rng))
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")
    try:
        for name in ("list", "int32", "strided", "float16", "k as a list"):
            k, gain = tn.random_tone(rng)
            want = tn.expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, (k, gain))
            if name == "list":
                given = (k, [int(v) for v in gain])
            elif name == "int32":
                given = (k, gain.astype(np.int32))
            elif name == "strided":
                wide = np.full(2 * ENC_N, 0x7C00, np.uint16)          # (what lies between the entries would be refused)
                wide[::2] = gain
                given = (k, wide[::2])
                assert not given[1].flags["C_CONTIGUOUS"]
            elif name == "float16":
                given = (k, gain.view(np.float16)[::1])
            else:
                given = ([float(v) for v in k], gain)
            for _ in range(3):          # (what a freed copy holds depends on the allocator: several goes)
                ctx.colour_update_tone(live, given)
                tc.export_and_check(ctx, pic, live, want, K4, F16, "update_tone with gain as %s" % name, pos=1)
    finally:
        ctx.sync()
        pic.free()
        ctx.colour_destroy(live)


def _raw(ctx, h, k, gain, c=True, t=True):
    keep = np.ascontiguousarray(gain, np.uint16) if gain is not None else None
    tone = ColourTone(k=(C.c_float * 3)(*[float(v) for v in k]))
    if keep is not None:
        tone.gain = keep.ctypes.data_as(C.POINTER(C.c_uint16))
    return ctx.lib.dav1d_hip_colour_update_tone(ctx.h if c else None, h, C.byref(tone) if t else None)


def test_refusals_change_nothing(ctx):
    w, h, bpc, layout = 67, 19, 10, I420
    rng = np.random.default_rng(52200)
    lin, m, enc = tc.random_tables(rng, bpc)
    tp = tn.random_tone(rng)
    k, gain = tn.random_tone(rng)
    toned, plain = ctx.colour(lin, m, enc, bpc=bpc, tone=tp), ctx.colour(lin, m, enc, bpc=bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only")

    def poked(a, i, v):
        b = np.array(a)
        b[i] = v
        return b
    try:
        before = tsc._live(ctx)
        assert _raw(ctx, toned, k, gain, c=False) == -EINVAL and _raw(ctx, None, k, gain) == -EINVAL and _raw(ctx, toned, k, gain, t=False) == -EINVAL
        assert _raw(ctx, plain, k, gain) == -EINVAL, "a handle without a tone part has no room for a gain"
        with pytest.raises(api.HipError, match="errno %d" % EINVAL):
            ctx.colour_update_tone(plain, (k, gain))
        assert _raw(ctx, toned, k, None) == -EINVAL
        for bad in (np.nan, np.inf, -np.inf):
            for i in range(3):
                assert _raw(ctx, toned, poked(k, i, bad), gain) == -EINVAL
        for bad in (0x7C00, 0xFC00, 0x7E00, 0xFFFF):
            assert _raw(ctx, toned, k, poked(gain, 0, bad)) == -EINVAL and _raw(ctx, toned, k, poked(gain, ENC_N - 1, bad)) == -EINVAL
        with pytest.raises(ValueError):
            ctx.colour_update_tone(toned, (k, gain[:100]))
        assert tsc._live(ctx) == before
        # neither handle has changed
        tc.export_and_check(ctx, pic, toned, tn.expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, tp), K4, F16, "the toned handle after refused updates", pos=1)
        tc.export_and_check(ctx, pic, plain, tc.expect(vis, layout, bpc, K4, F16, 1, lin, m, enc), K4, F16, "the un-toned handle after a refused update", pos=1)
        # the largest finite halves of either sign and any finite k are taken
        ok = (np.array([-3e38, 0.0, -0.0], f32), poked(poked(gain, 7, 0x7BFF), 8, 0xFBFF))
        assert _raw(ctx, toned, *ok) == 0
        tc.export_and_check(ctx, pic, toned, tn.expect(vis, layout, bpc, K4, F16, 1, lin, m, enc, ok), K4, F16, "after an update", pos=1)
    finally:
        ctx.sync()
        pic.free()
        ctx.colour_destroy(toned)
        ctx.colour_destroy(plain)


def test_a_handle_of_another_device_is_refused():
    """-EXDEV on the emulator's two devices (tests/conftest.py), behind the other refusals"""
    ctx = util.make_context("emu")
    assert ctx.lib.dav1d_hip_device_count() >= 2
    other = api.Context(1, lib_path=ctx.lib_path)
    try:
        rng = np.random.default_rng(52300)
        k, gain = tn.random_tone(rng)
        foreign = other.colour(*tc.random_tables(rng, 10), bpc=10, tone=tn.random_tone(rng))
        ctx.lib.dav1d_hip_context_use(ctx.h)
        assert _raw(ctx, foreign, k, gain) == -EXDEV
        assert _raw(ctx, foreign, [np.nan, 0, 0], gain) == -EINVAL and _raw(ctx, foreign, k, None) == -EINVAL
        ctx.lib.dav1d_hip_context_use(other.h)
        assert _raw(other, foreign, k, gain) == 0
        other.colour_destroy(foreign)
    finally:
        other.close()
        ctx.lib.dav1d_hip_context_use(ctx.h)
        ctx.close()
