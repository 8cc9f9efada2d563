"""Tensor-ready RGB: dav1d_hip_surface_export_rgb (dav1d_amd/csrc/surface_rgb.hip) against numpy.

Sited chroma (chroma_pos 0 / 1 / 2), packed RGB / RGBA next to the planes, binary16 next to float32, a per-channel normalisation.  The rules of
include/dav1d_hip.h are restated here in numpy (nothing is imported from the product but its constants and bindings); every destination is filled
with 0xA5 first and compared byte for byte, padding included.  Every case runs on the emulated build and, under -m gpu, on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import util
import test_filmgrain
import test_surface as ts
from dav1d_amd import api
from dav1d_amd._lib import RgbParams
from util import put_in_state

EINVAL, ENOTSUP = 22, 95
LAYOUTS = [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444]
SIZES = [(8, 2), (9, 3), (130, 18), (131, 19)]      # chroma 65x9 and 66x10 at 4:2:0: two cells across, two down, odd edges
P, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
N, M, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32, api.SAMPLE_F16


# ------------------------------------------------------------------------------------------------ the rules, restated

def subsampling(layout):
    return (1 if layout in (api.LAYOUT_I420, api.LAYOUT_I422) else 0), (1 if layout == api.LAYOUT_I420 else 0)


def vertical_taps(y, ss_v, pos):
    """[(chroma row, weight)] of luma row y, weights summing to 4 (rows not yet clamped)"""
    if not ss_v:
        return [(y, 4)]
    k = y >> 1
    if pos == 0:
        return [(k, 4)]
    if pos == 1:
        return [(k, 3), (k + 1, 1)] if y & 1 else [(k - 1, 1), (k, 3)]
    return [(k, 2), (k + 1, 2)] if y & 1 else [(k, 4)]


def horizontal_taps(x, ss_h, pos):
    if not ss_h:
        return [(x, 2)]
    k = x >> 1
    if pos == 0 or not x & 1:
        return [(k, 2)]
    return [(k, 1), (k + 1, 1)]


def upsample(plane, w, h, ss_h, ss_v, pos):
    ch, cw = plane.shape
    c = plane.astype(np.int64)
    rows = [[(min(max(r, 0), ch - 1), wt) for r, wt in vertical_taps(y, ss_v, pos)] for y in range(h)]
    cols = [[(min(max(q, 0), cw - 1), wt) for q, wt in horizontal_taps(x, ss_h, pos)] for x in range(w)]
    # at most two taps per axis: as index / weight arrays, the second tap with weight 0 where there is one only
    def arrays(taps):
        i0 = np.array([t[0][0] for t in taps]); w0 = np.array([t[0][1] for t in taps])
        i1 = np.array([t[-1][0] for t in taps]); w1 = np.array([t[-1][1] if len(t) > 1 else 0 for t in taps])
        return i0, w0, i1, w1
    r0, wr0, r1, wr1 = arrays(rows)
    c0, wc0, c1, wc1 = arrays(cols)
    acc = 0
    for ri, rw in ((r0, wr0), (r1, wr1)):
        for ci, cwt in ((c0, wc0), (c1, wc1)):
            acc = acc + rw[:, None] * cwt[None, :] * c[ri[:, None], ci[None, :]]
    out = (acc + 4) >> 3
    assert out.min() >= 0 and out.max() <= c.max()
    return out


def rgb_values(vis, layout, bpc, matrix, full_range, pos):
    """R, G, B as integers in [0, max] (int64 arrays of luma size)"""
    d, mx = bpc, (1 << bpc) - 1
    Y = vis[0].astype(np.int64)
    h, w = Y.shape
    if layout == api.LAYOUT_I400:
        U = V = np.full((h, w), 1 << (d - 1), np.int64)
    else:
        ss_h, ss_v = subsampling(layout)
        U, V = upsample(vis[1], w, h, ss_h, ss_v, pos), upsample(vis[2], w, h, ss_h, ss_v, pos)
    if matrix == 0:
        return V, Y, U
    cy, crv, cbu, cgu, cgv = ts.rgb_coefficients(matrix, full_range, d)
    y = Y - (0 if full_range else 16 << (d - 8))
    cb, cr = U - (1 << (d - 1)), V - (1 << (d - 1))
    R = np.clip((cy * y + crv * cr + 8192) >> 14, 0, mx)
    G = np.clip((cy * y - cgu * cb - cgv * cr + 8192) >> 14, 0, mx)
    B = np.clip((cy * y + cbu * cb + 8192) >> 14, 0, mx)
    return R, G, B


def samples(values, bpc, sample, scale=None, bias=None):
    """the three planes in the sample type, and the opaque alpha"""
    mx = (1 << bpc) - 1
    if sample == N:
        dt = np.uint8 if bpc == 8 else np.uint16
        return [v.astype(dt) for v in values], dt(mx)
    if sample == M:
        return [(v.astype(np.uint16) << (16 - bpc)).astype(np.uint16) for v in values], np.uint16(mx << (16 - bpc))
    out = []
    for k, v in enumerate(values):
        if scale is None:
            f = v.astype(np.float32) * np.float32(1.0 / mx)
        else:
            f = (v.astype(np.float32) * np.float32(scale[k])).astype(np.float32) + np.float32(bias[k])
        assert f.dtype == np.float32
        out.append(f if sample == F32 else f.astype(np.float16))
    return out, (np.float32(1.0) if sample == F32 else np.float16(1.0))


def arrange(planes, alpha, fmt):
    """what the surface's planes hold: three planes, or one of interleaved samples"""
    if fmt == P:
        return planes
    n = 3 if fmt == K3 else 4
    h, w = planes[0].shape
    out = np.empty((h, w * n), planes[0].dtype)
    for k in range(3):
        out[:, k::n] = planes[k]
    if n == 4:
        out[:, 3::n] = alpha
    return [out]


def expect(vis, layout, bpc, fmt, sample, pos, matrix=1, full_range=0, scale=None, bias=None):
    planes, alpha = samples(rgb_values(vis, layout, bpc, matrix, full_range, pos), bpc, sample, scale, bias)
    return arrange(planes, alpha, fmt)


def make_picture(ctx, w, h, layout, bpc, state, fill):
    """a device picture whose padded planes are fill(plane index, padded shape)"""
    pic = ctx.picture(w, h, layout, bpc)
    planes = [fill(pl, pic.padded_shape(pl)).astype(pic.dtype) for pl in range(pic.n_planes)]
    for pl in range(pic.n_planes):
        pic.upload(pl, planes[pl])
    put_in_state(ctx, pic, state)
    return pic, [planes[pl][:pic.pic.p[pl].h, :pic.pic.p[pl].w] for pl in range(pic.n_planes)]


def export_and_check(ctx, pic, want, fmt, sample, what, pos=0, scale=None, bias=None, rows=(0, 1 << 30), **kw):
    d = ts.Dest(ctx, pic.w, pic.h, pic.layout, pic.bpc, fmt, sample, **kw)
    try:
        pic.export_rgb(d.surface, pos, scale, bias, rows[0], rows[1])
        d.check(want, what=what)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------------ 1. upsampling

def test_tap_weights_restated():
    for pos in (0, 1, 2):
        for y in range(6):
            assert sum(wt for _, wt in vertical_taps(y, 1, pos)) == 4 and sum(wt for _, wt in vertical_taps(y, 0, pos)) == 4
            assert sum(wt for _, wt in horizontal_taps(y, 1, pos)) == 2 and sum(wt for _, wt in horizontal_taps(y, 0, pos)) == 2
    ramp = np.arange(40, dtype=np.uint16).reshape(5, 8) * 8
    assert np.array_equal(upsample(ramp, 16, 10, 1, 1, 0), ramp[np.arange(10)[:, None] >> 1, np.arange(16)[None, :] >> 1])


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["i400", "i420", "i422", "i444"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_upsampling(ctx, bpc, layout, state):
    for w, h in SIZES:
        rng = np.random.default_rng(9000 + 100 * bpc + 10 * layout + w)
        pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, state)
        try:
            replicated = ts.expect_rgb(vis, layout, bpc, 1, 0)
            for pos in (0, 1, 2):
                want = expect(vis, layout, bpc, P, N, pos)
                if pos == 0 or layout in (api.LAYOUT_I400, api.LAYOUT_I444):
                    assert all(np.array_equal(a, b) for a, b in zip(want, replicated)), "replication is today's rule"
                elif min(w, h) > 8:
                    assert any(not np.array_equal(a, b) for a, b in zip(want, replicated))
                export_and_check(ctx, pic, want, P, N, "%dx%d %d bpc layout %d %s chroma_pos %d" % (w, h, bpc, layout, state, pos), pos=pos)
            assert pic.pic.twin_ok == (api.TWIN_ONLY if state == "twin-only" else 0)
        finally:
            pic.free()


@pytest.mark.parametrize("layout", [api.LAYOUT_I420, api.LAYOUT_I422], ids=["i420", "i422"])
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_upsampling_of_extremal_content(ctx, bpc, layout):
    mx = (1 << bpc) - 1
    fills = {
        "zero": lambda pl, s: np.zeros(s, np.int64),
        "max": lambda pl, s: np.full(s, mx, np.int64),
        "columns": lambda pl, s: np.broadcast_to((np.arange(s[1])[None, :] & 1) * mx, s),
        "rows": lambda pl, s: np.broadcast_to((np.arange(s[0])[:, None] & 1) * mx, s),
    }
    for w, h in ((131, 19), (130, 18)):
        for name, fill in fills.items():
            pic, vis = make_picture(ctx, w, h, layout, bpc, "twin-only", fill)
            try:
                for pos in (1, 2):
                    for full in (0, 1):
                        export_and_check(ctx, pic, expect(vis, layout, bpc, P, N, pos, 9, full), P, N,
                                         "%s %dx%d %d bpc layout %d chroma_pos %d full %d" % (name, w, h, bpc, layout, pos, full), pos=pos, matrix=9, full_range=full)
            finally:
                pic.free()


def test_colocated_chroma_constant_per_row_is_replication_on_even_rows(ctx):
    """a check with a formula of its own: chroma_pos 2 puts chroma row k on luma row 2k, and a row of one value has nothing to interpolate across"""
    w, h, bpc, layout = 131, 19, 10, api.LAYOUT_I420
    rng = np.random.default_rng(9100)
    row_values = rng.integers(0, 1 << bpc, size=(3, 256))

    def fill(pl, s):
        return rng.integers(0, 1 << bpc, size=s) if pl == 0 else np.broadcast_to(row_values[pl, :s[0], None], s)
    pic, vis = make_picture(ctx, w, h, layout, bpc, "raster", fill)
    s = ctx.surface(w, h, layout, bpc, P, N)
    try:
        pic.export_rgb(s, api.CHROMA_COLOCATED)
        got = s.download()
        want = ts.expect_rgb(vis, layout, bpc, 1, 0)
        for k in range(3):
            assert np.array_equal(got[k][0::2], want[k][0::2])
        assert any(not np.array_equal(got[k][1::2], want[k][1::2]) for k in range(3))
    finally:
        s.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 2. equivalence with the export that exists

@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("bpc,layout", [(8, api.LAYOUT_I420), (10, api.LAYOUT_I420), (12, api.LAYOUT_I422), (10, api.LAYOUT_I444), (10, api.LAYOUT_I400)])
def test_null_params_equal_the_plain_export(ctx, bpc, layout, state):
    for w, h in ((131, 19), (9, 3)):
        rng = np.random.default_rng(9200 + bpc + layout)
        pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, state, extremes=w > 100)
        try:
            for sample in (N, M, F32):
                if sample == M and bpc == 8:
                    continue
                a = ts.Dest(ctx, w, h, layout, bpc, P, sample, matrix=5)
                b = ts.Dest(ctx, w, h, layout, bpc, P, sample, matrix=5)
                pic.export(a.surface)
                assert ctx.lib.dav1d_hip_surface_export_rgb(ctx.h, C.byref(b.surface.desc), C.byref(pic.pic), None, 0, 1 << 30) == 0
                ctx.sync()
                for k, (x, y) in enumerate(zip(a.bufs, b.bufs)):
                    size = a.shapes[k][0] * a.strides[k]
                    assert np.array_equal(x.download(np.uint8)[a.lead[k]:a.lead[k] + size], y.download(np.uint8)[b.lead[k]:b.lead[k] + size])
                b.check(ts.expect_rgb(vis, layout, bpc, 5, 0, sample), what="NULL params, sample %d" % sample)
                a.check(ts.expect_rgb(vis, layout, bpc, 5, 0, sample), what="plain export, sample %d" % sample)
                a.free()
                b.free()
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 3. packed formats

@pytest.mark.parametrize("fmt", [K3, K4], ids=["rgb", "rgba"])
@pytest.mark.parametrize("bpc", [8, 10])
def test_packed_formats(ctx, bpc, fmt):
    n = 3 if fmt == K3 else 4
    for (w, h), layout, state in (((131, 19), api.LAYOUT_I420, "twin-only"), ((130, 18), api.LAYOUT_I422, "raster"), ((9, 3), api.LAYOUT_I444, "raster")):
        rng = np.random.default_rng(9300 + bpc + w)
        pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, state)
        try:
            for sample in (N, M, F32, F16):
                if sample == M and bpc == 8:
                    continue
                planar = expect(vis, layout, bpc, P, sample, 1)
                want = expect(vis, layout, bpc, fmt, sample, 1)
                for k in range(3):
                    assert np.array_equal(np.ascontiguousarray(want[0][:, k::n]).view(np.uint8), planar[k].view(np.uint8)), "the planar result, interleaved"
                if n == 4:
                    mx = (1 << bpc) - 1
                    alpha = {N: mx, M: mx << (16 - bpc) if bpc > 8 else None, F32: 1.0, F16: 1.0}[sample]
                    assert (want[0][:, 3::4] == alpha).all()
                export_and_check(ctx, pic, want, fmt, sample, "%dx%d %d bpc format %d sample %d" % (w, h, bpc, fmt, sample), pos=1)
        finally:
            pic.free()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-sample-off"])
@pytest.mark.parametrize("pad", [0, 2, 14, 64])
@pytest.mark.parametrize("bpc", [8, 10])
def test_packed_strides_and_overwrites(ctx, bpc, pad, offset):
    """tight rows, rows padded by 2, 14 and 64 bytes, a base one sample past a 256-byte boundary: vector stores and the narrow path, whole units
    and the last partial unit of a row; every byte outside the visible samples keeps the sentinel"""
    rng = np.random.default_rng(9400 + bpc + pad)
    for w, h in ((131, 19), (130, 18), (8, 2)):
        pic, vis = util.make_source(ctx, rng, w, h, api.LAYOUT_I420, bpc, "twin-only")
        try:
            for fmt in (K3, K4, P):
                for sample in (N, F16, F32):
                    es = 4 if sample == F32 else 2 if (bpc > 8 or sample == F16) else 1
                    if pad % es:
                        continue          # not a stride of this sample type: test_refusals
                    export_and_check(ctx, pic, expect(vis, api.LAYOUT_I420, bpc, fmt, sample, 2), fmt, sample,
                                     "%dx%d %d bpc format %d sample %d pad %d offset %d" % (w, h, bpc, fmt, sample, pad, offset), pos=2, pad=pad, offset=offset * es)
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 4. binary16 and normalisation

def _f16_driver(tmp_path_factory):
    """dv::f32_to_f16_bits of dav1d_amd/csrc/common.h, the integer form of the emulated build, behind a C function"""
    d = tmp_path_factory.mktemp("f16")
    src, so = os.path.join(d, "f16.cpp"), os.path.join(d, "f16.so")
    with open(src, "w") as f:
        f.write('#include "common.h"\nextern "C" void f16_of(const float *in, uint16_t *out, int n) { for (int i = 0; i < n; i++) out[i] = dv::f32_to_f16_bits(in[i]); }\n')
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I" + os.path.join(util.ROOT, "tests", "emu"), "-I" + os.path.join(util.ROOT, "dav1d_amd", "csrc"),
                    src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.f16_of.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    return lib


def test_f32_to_f16_bits_over_every_binary16_neighbourhood(tmp_path_factory):
    lib = _f16_driver(tmp_path_factory)
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    bits = halves.view(np.uint32)
    # every binary16 value, its float32 neighbours, and the float32 midpoints between neighbouring binary16 values with their neighbours (the ties)
    mid = ((bits.astype(np.uint64) + np.roll(bits, -1).astype(np.uint64)) // 2).astype(np.uint32)
    sub = ((np.arange(1025) + 0.5) * 2.0 ** -24).astype(np.float32).view(np.uint32)      # the ties between subnormals, exact in float32
    sub = np.concatenate([sub, sub | 0x80000000])
    cand = np.concatenate([bits, bits + 1, bits - 1, mid, mid + 1, mid - 1, sub, sub + 1, sub - 1]).astype(np.uint32)
    x = cand.view(np.float32)
    got = np.zeros(len(x), np.uint16)
    lib.f16_of(x.ctypes.data, got.ctypes.data, len(x))
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7c00) == 0x7c00).all() and ((got[nan] & 0x3ff) != 0).all() and np.array_equal(got[nan] >> 15, (cand[nan] >> 31).astype(np.uint16))
    assert (~nan).sum() > 6 * 63000


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@pytest.mark.parametrize("bpc", [8, 10])
def test_f16_and_normalisation(ctx, bpc):
    w, h, layout = 131, 19, api.LAYOUT_I420
    mx = (1 << bpc) - 1
    rng = np.random.default_rng(9500 + bpc)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    imagenet = ([np.float32(1.0 / (mx * s)) for s in IMAGENET_STD], [np.float32(-m / s) for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)])
    # R: multiples of 2^-25 around 0 — negative values, binary16 subnormals (units of 2^-24), every odd multiple a tie; G: subnormals that are exact;
    # B: an ordinary pair with a negative bias
    odd = ([np.float32(2.0 ** -25), np.float32(2.0 ** -24), np.float32(1e-3)], [np.float32(-5 * 2.0 ** -25), np.float32(-3 * 2.0 ** -24), np.float32(-0.3)])
    vals = rgb_values(vis, layout, bpc, 1, 0, 1)
    r = (vals[0] - 5).astype(np.float64) * 2.0 ** -25
    assert (r < 0).any() and ((r > 0) & (r < 2.0 ** -14)).any() and (((vals[0] - 5) & 1) == 1).any(), "negative values, subnormals and ties are in the expectation"
    half = samples(vals, bpc, F16, *odd)[0][0]
    ties = ((vals[0] - 5) & 3)
    assert (half[ties == 1].view(np.uint16) & 1 == 0).all() and (half[ties == 3].view(np.uint16) & 1 == 0).all(), "ties went to even"
    try:
        for fmt in (P, K3, K4):
            for sample in (F32, F16):
                export_and_check(ctx, pic, expect(vis, layout, bpc, fmt, sample, 1), fmt, sample, "%d bpc format %d sample %d, not normalised" % (bpc, fmt, sample), pos=1)
                for name, (scale, bias) in (("imagenet", imagenet), ("subnormals and ties", odd)):
                    export_and_check(ctx, pic, expect(vis, layout, bpc, fmt, sample, 1, scale=scale, bias=bias), fmt, sample,
                                     "%d bpc format %d sample %d, %s" % (bpc, fmt, sample, name), pos=1, scale=scale, bias=bias)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. bands

def chroma_rows_read(r0, r1, ch, ss_v, pos):
    out = set()
    for y in range(r0, r1):
        out |= {min(max(r, 0), ch - 1) for r, wt in vertical_taps(y, ss_v, pos) if wt}
    return out


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_bands(ctx, pos, state):
    w, h, bpc, layout = 200, 40, 10, api.LAYOUT_I420
    rng = np.random.default_rng(9600 + pos)
    pic, vis = util.make_source(ctx, rng, w, h, layout, bpc, state)
    try:
        for fmt, sample in ((P, N), (K4, F16)):
            want = expect(vis, layout, bpc, fmt, sample, pos)
            for band in (2, 6, 16):
                d = ts.Dest(ctx, w, h, layout, bpc, fmt, sample)
                for r0 in range(0, h, band):
                    pic.export_rgb(d.surface, pos, row0=r0, row1=min(r0 + band, h))
                d.check(want, what="bands of %d rows, chroma_pos %d format %d" % (band, pos, fmt))
                d.free()
            # one band alone leaves every other row at the sentinel
            d = ts.Dest(ctx, w, h, layout, bpc, fmt, sample)
            pic.export_rgb(d.surface, pos, row0=16, row1=22)
            d.check(want, rows=[(16, 22)] * len(want), what="band [16, 22)")
            d.free()
    finally:
        pic.free()


@pytest.mark.parametrize("layout", [api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444], ids=["i420", "i422", "i444"])
def test_rows_needed(ctx, layout):
    bpc = 10
    for w, h in ((200, 40), (131, 19)):
        pic = ctx.picture(w, h, layout, bpc)
        s = ctx.surface(w, h, layout, bpc, K3, F16)
        ss_v = subsampling(layout)[1]
        ch = (h + ss_v) >> ss_v
        try:
            for pos in (0, 1, 2):
                for band in (2, 6, 16):
                    for r0 in range(0, h, band):
                        r1 = min(r0 + band, h)
                        read = chroma_rows_read(0, r1, ch, ss_v, pos)
                        brute = max(r1, min(h, (max(read) + 1) << ss_v))
                        assert pic.rgb_rows_needed(s, pos, r1) == brute, (w, h, pos, r1)
                        assert brute == (min(h, r1 + 2) if ss_v and pos else min(h, r1))
                        # ... and the band itself reads no chroma row that needs more than that
                        assert min(h, (max(chroma_rows_read(r0, r1, ch, ss_v, pos)) + 1) << ss_v) <= brute
                assert pic.rgb_rows_needed(s, pos, 1 << 30) == h
        finally:
            s.free()
            pic.free()


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refusals(ctx):
    w, h = 131, 19
    rng = np.random.default_rng(9700)
    pics = {}
    for bpc, layout in ((10, api.LAYOUT_I420), (8, api.LAYOUT_I420), (10, api.LAYOUT_I444)):
        pics[bpc, layout] = util.make_source(ctx, rng, w, h, layout, bpc, "raster")[0]

    def refused(code, bpc, layout, fmt, sample, change=None, rows=(0, 1 << 30), params=None, shape_as=None, **kw):
        pic = pics[bpc, layout]
        d = ts.Dest(ctx, w, h, layout, bpc, shape_as[0] if shape_as else fmt, shape_as[1] if shape_as else sample, **kw)
        d.surface.desc.format, d.surface.desc.sample = fmt, sample
        if change:
            change(d.surface.desc)
        p = C.byref(params) if params is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_rgb(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), p, rows[0], rows[1])
        assert rc == -code, (rc, code)
        if rows[0] == 0:
            assert ctx.lib.dav1d_hip_surface_rgb_rows_needed(C.byref(d.surface.desc), C.byref(pic.pic), p, rows[1]) == -code
        d.check(None, what="a refused export")
        d.free()

    def setter(name, value):
        return lambda desc: setattr(desc, name, value)

    def stride(k, delta):
        def f(desc):
            desc.stride[k] = desc.stride[k] + delta
        return f

    def null_plane(k):
        def f(desc):
            desc.data[k] = None
        return f
    I420, I444 = api.LAYOUT_I420, api.LAYOUT_I444
    try:
        for fmt in (api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, 5, -1):          # not an RGB format
            refused(EINVAL, 10, I420, fmt, N, shape_as=(P, N))
        for sample in (4, -1):
            refused(EINVAL, 10, I420, K3, sample, shape_as=(K3, N))
        for fmt in (P, K3, K4):
            refused(EINVAL, 8, I420, fmt, M, shape_as=(fmt, F16))                # MSB16 at 8 bpc
            for sample in (N, M):                                               # normalisation is for float samples
                refused(EINVAL, 10, I420, fmt, sample, params=RgbParams(1, 1, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)))
            for pos in (-1, 3):
                refused(EINVAL, 10, I420, fmt, F16, params=RgbParams(pos, 0))
            refused(EINVAL, 10, I420, fmt, N, setter("w", w + 1))
            refused(EINVAL, 10, I420, fmt, N, setter("h", h - 1))
            refused(EINVAL, 10, I420, fmt, N, null_plane(0))
            refused(EINVAL, 10, I420, fmt, F16, stride(0, -2))                    # below the row's bytes
            refused(EINVAL, 10, I420, fmt, F32, stride(0, +2), pad=4)             # not a multiple of the sample size
            refused(EINVAL, 10, I420, fmt, N, matrix=0)                           # identity needs 4:4:4
            refused(EINVAL, 10, I420, fmt, N, rows=(1, 18))                       # odd row0
            refused(EINVAL, 10, I420, fmt, N, rows=(0, 3))                        # odd row1 that is not the picture's end
            for m in (2, 4, 8, 14, -1):
                refused(ENOTSUP, 10, I420, fmt, N, matrix=m)
        refused(EINVAL, 10, I420, P, N, null_plane(2))
        assert ctx.lib.dav1d_hip_surface_export_rgb(None, None, None, None, 0, 2) == -EINVAL
        # ... and the same surfaces are accepted when nothing is wrong with them (a packed surface has one plane: data[1], data[2] are not looked at)
        for (bpc, layout), pic in pics.items():
            for fmt in (P, K3, K4):
                d = ts.Dest(ctx, w, h, layout, bpc, fmt, F16, matrix=0 if layout == I444 else 6)
                pic.export_rgb(d.surface, 2)
                ctx.sync()
                d.free()
    finally:
        for p in pics.values():
            p.free()


def test_the_existing_entry_points_still_refuse_the_new_codes(ctx):
    w, h, bpc, layout = 64, 32, 10, api.LAYOUT_I420
    rng = np.random.default_rng(9800)
    pic = util.make_source(ctx, rng, w, h, layout, bpc, "raster")[0]
    grain = ctx.fg_prepare(test_filmgrain.random_fg(rng, bpc, 0), bpc, layout)
    try:
        for fmt, sample in ((K3, N), (K4, N), (P, F16), (K4, F16)):
            d = ts.Dest(ctx, w, h, layout, bpc, fmt, sample)
            desc, p = C.byref(d.surface.desc), C.byref(pic.pic)
            assert ctx.lib.dav1d_hip_surface_export(ctx.h, desc, p, 0, h) == -EINVAL
            assert ctx.lib.dav1d_hip_surface_export_grain(ctx.h, desc, p, grain, 0, 0, h) == -EINVAL
            assert ctx.lib.dav1d_hip_surface_export_scaled(ctx.h, desc, p, None, 0, h) == -EINVAL
            assert ctx.lib.dav1d_hip_surface_scaled_rows_needed(desc, p, None, h) == -EINVAL
            d.check(None, what="a refused export")
            d.free()
    finally:
        ctx.sync()
        ctx.fg_grain_destroy(grain)
        pic.free()


# ------------------------------------------------------------------------------------------------ 7. torch (GPU only)

def _torch_child():
    """(a process of its own, for the reason tests/test_surface.py gives)"""
    import torch
    w, h, bpc, layout = 130, 18, 10, api.LAYOUT_I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(9900)
    pic, vis = util.make_source(tctx, rng, w, h, layout, bpc, "twin-only", extremes=True)
    mx = (1 << bpc) - 1
    scale, bias = [1.0 / (mx * s) for s in IMAGENET_STD], [-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]
    for n, fmt in ((3, K3), (4, K4)):
        t = torch.full((h, w, n), 7.0, dtype=torch.float16, device="cuda")
        api.export_to_tensor(pic, t, matrix=1, full_range=0, chroma_pos=api.CHROMA_VERTICAL, scale=scale, bias=bias)
        tctx.sync()
        got = t.cpu().numpy().reshape(h, w * n)
        want = expect(vis, layout, bpc, fmt, F16, 1, scale=[np.float32(v) for v in scale], bias=[np.float32(v) for v in bias])[0]
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), "HWC float16 tensor, %d channels" % n
    t = torch.empty((3, h, w), dtype=torch.float16, device="cuda")
    api.export_to_tensor(pic, t, chroma_pos=api.CHROMA_COLOCATED)
    tctx.sync()
    want = expect(vis, layout, bpc, P, F16, 2)
    assert all(np.array_equal(t[k].cpu().numpy().view(np.uint16), want[k].view(np.uint16)) for k in range(3)), "CHW float16 tensor"
    assert pic.pic.twin_ok == api.TWIN_ONLY
    pic.free()
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_to_tensor_hwc_float16():
    """export_to_tensor into HWC float16 tensors (3 and 4 channels, ImageNet normalisation, chroma_pos 1) and a CHW float16 tensor equals the
    numpy expectation, with the context opened on torch's current stream"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ 8. the glue's call sequence, object accounting

@pytest.mark.parametrize("bpc,layout", [(10, api.LAYOUT_I420), (8, api.LAYOUT_I444)], ids=["10bit-420", "8bit-444"])
def test_grain_then_rgb_export_leaves_no_object(ctx, bpc, layout):
    """The library calls of dav1d_hip_glue_output_rgb with grain, in its order (the function itself needs a decoder around it): dav1d_hip_fg_prepare,
    dav1d_hip_picture_alloc, dav1d_hip_fg_apply_prepared into the temporary picture, dav1d_hip_surface_export_rgb from that, dav1d_hip_sync, the
    frees.  The surface holds the RGB of the grained planes; dav1d_hip_live_objects is what it was."""
    def live():
        out = (C.c_longlong * 4)()
        assert ctx.lib.dav1d_hip_live_objects(out) == 0
        return list(out)
    w, h = 130, 18
    rng = np.random.default_rng(9950 + bpc)
    is_id = int(layout == api.LAYOUT_I444)
    data = test_filmgrain.random_fg(rng, bpc, 2 if is_id else 0)
    src, vis = util.make_source(ctx, rng, w, h, layout, bpc, "raster")
    d = ts.Dest(ctx, w, h, layout, bpc, K4, F16, matrix=0 if is_id else 1)
    before = live()
    try:
        grain = ctx.fg_prepare(data, bpc, layout)
        tmp = ctx.picture(w, h, layout, bpc)
        ctx.fg_apply_prepared(tmp, src, grain, is_id)
        tmp.export_rgb(d.surface, api.CHROMA_VERTICAL)
        ctx.sync()
        grained = [tmp.download(pl)[:tmp.pic.p[pl].h, :tmp.pic.p[pl].w] for pl in range(3)]
        tmp.free()
        ctx.fg_grain_destroy(grain)
        assert live() == before
        assert any(not np.array_equal(a, b) for a, b in zip(grained, vis)), "the grain set changes nothing"
        d.check(expect(grained, layout, bpc, K4, F16, 1, matrix=0 if is_id else 1), what="grain, then RGBA float16")
    finally:
        d.free()
        src.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
