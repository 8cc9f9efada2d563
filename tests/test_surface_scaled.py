"""Scale and crop in the device surface export: dav1d_hip_surface_export_scaled / dav1d_hip_surface_scaled_rows_needed
(dav1d_amd/csrc/surface_scale.hip) against numpy.

The call must write byte for byte what dav1d_hip_surface_export writes from a picture whose planes are the scaled planes.  The scaled planes
never come from the library: `axis_weights` / `scale_plane` restate the definition of include/dav1d_hip.h with Python integers
and int64 (asserting that the weights of every output sum to 4096 over at most 9 taps and that the horizontal sum stays below 2^32); the surface
is the numpy restatement of tests/test_surface.py (expect_yuv / expect_rgb) of those planes.  The defining properties (1:1 is the plain export,
2:1 is the rounded mean of four, constants stay, a crop at ratio 1 is a slice) are checked against formulas that share no code with that oracle.
Every comparison is exact; every destination is filled with 0xA5 first and compared byte by byte, padding included (test_surface.Dest).

Sources are 190x102, 333x77 and 64x64.  GEOMS names what each destination size is for.

Thinned on the emulator (the device runs the full product):
  * test_every_geometry: one of the seven geometries per (bpc, layout, state), rotating;
  * test_constants: two geometries per value instead of seven;
  * test_rgb: one matrix per (layout, range, state), rotating, and one geometry instead of three.
The emulator has no clock: test_export_is_asynchronous_and_timed asks for a positive device time on the device only.
Unaligned destinations: the byte offsets 0, 2, 6 and row paddings 0, 2, 10 are those of 2-byte samples; a float surface takes them in the same
number of half samples (0, 4, 12 and 0, 4, 20), a surface's stride being a multiple of its sample size by definition."""
import ctypes as C
import functools

import numpy as np
import pytest

import util
from dav1d_amd import api
from test_surface import Dest, expect_rgb, expect_yuv
from util import STATES, make_source

EINVAL, ENOTSUP = 22, 95
LAYOUTS = [api.LAYOUT_I400, api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444]
LAYOUT_IDS = ["i400", "i420", "i422", "i444"]
P, S, R = api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, api.SURFACE_RGB_PLANAR
N, M, F = api.SAMPLE_NATIVE, api.SAMPLE_MSB16, api.SAMPLE_F32
GEOMS = [((190, 102), (95, 51)),        # the exact half
         ((190, 102), (47, 13)),        # an odd ratio, odd sizes
         ((333, 77), (64, 33)),         # ... with a destination of exactly one 64-sample run
         ((333, 77), (42, 10)),         # the 9-tap end of the range
         ((190, 102), (24, 13)),
         ((190, 102), (189, 101)),      # almost 1:1: another phase in every column
         ((64, 64), (32, 32))]


def ss_of(layout):
    return int(layout in (api.LAYOUT_I420, api.LAYOUT_I422)), int(layout == api.LAYOUT_I420)


# ------------------------------------------------------------------------------------------------ the oracle (numpy, Python integers)

@functools.lru_cache(None)
def axis_weights(s, d):
    """per output of an axis (s source samples to d): (first tap, weights), from the definition"""
    assert 1 <= d <= s <= 8 * d
    out = []
    for o in range(d):
        a, b = o * s, (o + 1) * s
        i0, i1 = a // d, (b + d - 1) // d - 1
        prev, ws = 0, []
        for k in range(i0, i1 + 1):
            q = ((min(b, (k + 1) * d) - a) * 4096 + s // 2) // s
            ws.append(q - prev)
            prev = q
        assert sum(ws) == 4096 and len(ws) <= 9 and min(ws) >= 0 and i1 < s, (s, d, o, ws)
        out.append((i0, tuple(ws)))
    return out


def scale_plane(plane, dw, dh):
    sh, sw = plane.shape
    p = plane.astype(np.int64)
    t = np.empty((dh, sw), np.int64)
    for j, (i0, ws) in enumerate(axis_weights(sh, dh)):
        t[j] = (sum(w * p[i0 + k] for k, w in enumerate(ws)) + 8) >> 4
    assert t.max() < 1 << 20
    out = np.empty((dh, dw), np.int64)
    for o, (i0, ws) in enumerate(axis_weights(sw, dw)):
        acc = sum(w * t[:, i0 + k] for k, w in enumerate(ws)) + (1 << 19)
        assert acc.max() < 1 << 32
        out[:, o] = acc >> 20
    return out.astype(plane.dtype)


def windows(vis, layout, crop):
    x0, y0, w, h = crop
    out = []
    for pl, v in enumerate(vis):
        ssh, ssv = ss_of(layout) if pl else (0, 0)
        out.append(v[y0 >> ssv:(y0 >> ssv) + ((h + ssv) >> ssv), x0 >> ssh:(x0 >> ssh) + ((w + ssh) >> ssh)])
    return out


def scaled_planes(vis, layout, dw, dh, crop=None):
    crop = crop or (0, 0, vis[0].shape[1], vis[0].shape[0])
    out = []
    for pl, win in enumerate(windows(vis, layout, crop)):
        ssh, ssv = ss_of(layout) if pl else (0, 0)
        out.append(scale_plane(win, (dw + ssh) >> ssh, (dh + ssv) >> ssv))
    return out


def want_of(planes, layout, bpc, fmt, sample, matrix=1, full_range=0):
    if fmt == R:
        return expect_rgb(planes, layout, bpc, matrix, full_range, sample)
    return expect_yuv(planes, bpc, fmt, sample)


def check_scaled(ctx, pic, vis, dw, dh, fmt, sample, crop=None, matrix=1, full_range=0, planes=None, what="", **kw):
    planes = planes if planes is not None else scaled_planes(vis, pic.layout, dw, dh, crop)
    d = Dest(ctx, dw, dh, pic.layout, pic.bpc, fmt, sample, matrix=matrix, full_range=full_range, **kw)
    try:
        pic.export_scaled(d.surface, crop)
        d.check(want_of(planes, pic.layout, pic.bpc, fmt, sample, matrix, full_range),
                what="%s %dx%d -> %dx%d crop %s %d bpc layout %d format %d sample %d matrix %d" % (what, pic.w, pic.h, dw, dh, crop, pic.bpc, pic.layout, fmt, sample, matrix))
    finally:
        d.free()


def source_from(ctx, padded, w, h, layout, bpc, state):
    """a device picture in `state` from padded planes of the test's own"""
    pic = ctx.picture(w, h, layout, bpc)
    for pl in range(pic.n_planes):
        pic.upload(pl, padded[pl])
    util.put_in_state(ctx, pic, state)
    return pic, [padded[pl][:pic.pic.p[pl].h, :pic.pic.p[pl].w] for pl in range(pic.n_planes)]


def test_weights_of_every_axis_used():
    """4096 in sum, at most 9 taps, never negative, for every (s, d) the cases below use (asserted inside axis_weights); 9 taps are reached"""
    most = 0
    for (w, h), (dw, dh) in GEOMS:
        for s, d in ((w, dw), (h, dh), ((w + 1) >> 1, (dw + 1) >> 1), ((h + 1) >> 1, (dh + 1) >> 1)):
            most = max(most, max(len(ws) for _, ws in axis_weights(s, d)))
    assert most == 9
    assert all(ws == (4096,) and i0 == o for o, (i0, ws) in enumerate(axis_weights(77, 77)))
    assert all(ws == (2048, 2048) and i0 == 2 * o for o, (i0, ws) in enumerate(axis_weights(64, 32)))


# ------------------------------------------------------------------------------------------------ 1. every geometry

@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("bpc", [8, 10, 12])
def test_every_geometry(ctx, bpc, layout, state):
    """planar and semi-planar, native samples; a twin-only source has 0x5A in every raster byte and must stay twin-only"""
    k = bpc // 2 + 2 * layout + 3 * STATES.index(state)
    for (w, h), (dw, dh) in GEOMS if ctx.backend != "emu" else [GEOMS[k % len(GEOMS)]]:
        pic, vis = make_source(ctx, np.random.default_rng(11000 + 100 * bpc + 10 * layout + w + dw), w, h, layout, bpc, state)
        try:
            before = pic.pic.twin_ok
            assert before == {"raster": 0, "retiled": 1, "twin-only": api.TWIN_ONLY}[state]
            planes = scaled_planes(vis, layout, dw, dh)
            for fmt in (P, S):
                check_scaled(ctx, pic, vis, dw, dh, fmt, N, planes=planes, what=state)
                assert pic.pic.twin_ok == before
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 2. defining properties

@pytest.mark.parametrize("layout", [api.LAYOUT_I420, api.LAYOUT_I444], ids=["i420", "i444"])
@pytest.mark.parametrize("state", ["raster", "twin-only"])
def test_same_size_is_the_plain_export(ctx, state, layout):
    """dw x dh == w x h with a NULL crop: the bytes of dav1d_hip_surface_export, library against library, padding included"""
    w, h, bpc = 190, 102, 10
    pic, _ = make_source(ctx, np.random.default_rng(11100 + layout), w, h, layout, bpc, state, extremes=True)
    try:
        for fmt in (P, S, R):
            for sample in (N, M, F):
                a, b = Dest(ctx, w, h, layout, bpc, fmt, sample, pad=2 * 4), Dest(ctx, w, h, layout, bpc, fmt, sample, pad=2 * 4)
                pic.export(a.surface)
                pic.export_scaled(b.surface)
                ctx.sync()
                for k, (x, y) in enumerate(zip(a.bufs, b.bufs)):
                    gx, gy = x.download(np.uint8), y.download(np.uint8)
                    n = min(len(gx) - a.lead[k], len(gy) - b.lead[k])
                    assert (gx != 0xA5).any() and np.array_equal(gx[a.lead[k]:a.lead[k] + n], gy[b.lead[k]:b.lead[k] + n]), (fmt, sample, k)
                    assert (gy[:b.lead[k]] == 0xA5).all() and (gy[b.lead[k] + n:] == 0xA5).all()
                a.free()
                b.free()
    finally:
        pic.free()


@pytest.mark.parametrize("w,h,layout,bpc,state", [(64, 64, api.LAYOUT_I420, 10, "twin-only"), (190, 102, api.LAYOUT_I444, 8, "raster"),
                                                  (190, 102, api.LAYOUT_I400, 12, "retiled")], ids=["64-i420", "190-i444", "190-i400"])
def test_exact_half_is_the_rounded_mean_of_four(ctx, w, h, layout, bpc, state):
    pic, vis = make_source(ctx, np.random.default_rng(11200 + w), w, h, layout, bpc, state, extremes=True)
    try:
        planes = []
        for v in vis:
            assert v.shape[0] % 2 == 0 and v.shape[1] % 2 == 0
            a = v.astype(np.int32)
            planes.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(v.dtype))
        for fmt in (P, S):
            check_scaled(ctx, pic, vis, w // 2, h // 2, fmt, N, planes=planes, what="2:1")
    finally:
        pic.free()


@pytest.mark.parametrize("value", ["zero", "max", "middle"])
def test_constants(ctx, value):
    """a constant picture gives that constant at every size of test_every_geometry"""
    bpc, layout = 10, api.LAYOUT_I420
    v = {"zero": 0, "max": (1 << bpc) - 1, "middle": 613}[value]
    k = ["zero", "max", "middle"].index(value)
    for (w, h), (dw, dh) in GEOMS if ctx.backend != "emu" else [GEOMS[(2 * k) % 7], GEOMS[(2 * k + 3) % 7]]:
        pic = ctx.picture(w, h, layout, bpc)
        try:
            for pl in range(3):
                pic.upload(pl, np.full(pic.padded_shape(pl), v, np.uint16))
            util.put_in_state(ctx, pic, "twin-only")
            ssh, ssv = ss_of(layout)
            planes = [np.full((dh, dw), v, np.uint16)] + [np.full(((dh + ssv) >> ssv, (dw + ssh) >> ssh), v, np.uint16)] * 2
            check_scaled(ctx, pic, None, dw, dh, P, N, planes=planes, what="constant %d" % v)
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 3. crop

CROPS = [((10, 6, 133, 71), (60, 33)),          # starts and ends inside 8x8 tiles and 64-sample cells
         ((64, 8, 126, 94), (63, 47)),
         ((189, 0, 1, 102), (1, 51)),           # the last column alone
         ((0, 101, 190, 1), (95, 1)),           # the last row alone
         ((10, 6, 133, 71), (133, 71)),         # ratio 1: a cropped copy
         ((2, 2, 37, 23), (19, 12))]            # odd w and h: odd chroma windows


@pytest.mark.parametrize("layout", [api.LAYOUT_I420, api.LAYOUT_I422, api.LAYOUT_I444], ids=["i420", "i422", "i444"])
@pytest.mark.parametrize("state", ["raster", "twin-only"])
def test_crop(ctx, state, layout):
    w, h, bpc = 190, 102, 10
    pic, vis = make_source(ctx, np.random.default_rng(11300 + layout), w, h, layout, bpc, state)
    ssh, ssv = ss_of(layout)
    try:
        for crop, (dw, dh) in CROPS:
            if (ssh and crop[0] & 1) or (ssv and crop[1] & 1):
                crop = (crop[0] - (crop[0] & ssh), crop[1] - (crop[1] & ssv), crop[2], crop[3])
            planes = None
            if (dw, dh) == crop[2:]:          # against the numpy slice, not the oracle
                planes = [np.ascontiguousarray(p) for p in windows(vis, layout, crop)]
                assert planes[1].shape == ((dh + ssv) >> ssv, (dw + ssh) >> ssh)
            for fmt in (P, S, R):
                check_scaled(ctx, pic, vis, dw, dh, fmt, N, crop=crop, planes=planes, what="crop " + state)
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 4. RGB

RGB_GEOMS = [GEOMS[0], GEOMS[2], GEOMS[4]]


@pytest.mark.parametrize("state", ["raster", "twin-only"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("full_range", [0, 1], ids=["limited", "full"])
def test_rgb(ctx, full_range, layout, state):
    """expect_rgb of the oracle's scaled planes: the existing formula, chroma replication and table"""
    matrices = [1, 5, 9] + ([0] if layout == api.LAYOUT_I444 else [])
    k = full_range + layout + 2 * STATES.index(state)
    geoms = RGB_GEOMS
    if ctx.backend == "emu":
        matrices, geoms = [matrices[k % len(matrices)]], [RGB_GEOMS[k % 3]]
    bpc = (8, 10, 12)[k % 3]
    for (w, h), (dw, dh) in geoms:
        pic, vis = make_source(ctx, np.random.default_rng(11400 + k + w), w, h, layout, bpc, state, extremes=True)
        try:
            planes = scaled_planes(vis, layout, dw, dh)
            for matrix in matrices:
                check_scaled(ctx, pic, vis, dw, dh, R, N, matrix=matrix, full_range=full_range, planes=planes, what="RGB " + state)
        finally:
            pic.free()


@pytest.mark.parametrize("sample", [M, F], ids=["msb16", "f32"])
def test_rgb_sample_types(ctx, sample):
    (w, h), (dw, dh) = GEOMS[1]
    pic, vis = make_source(ctx, np.random.default_rng(11450), w, h, api.LAYOUT_I420, 10, "twin-only", extremes=True)
    try:
        check_scaled(ctx, pic, vis, dw, dh, R, sample, what="RGB sample")
        check_scaled(ctx, pic, vis, dw, dh, S, sample, what="semi-planar sample")
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 5. bands

def dest_rows(fmt, n_planes, dh, r0, r1, ssv):
    dch = (dh + ssv) >> ssv
    if fmt == R:
        return [(r0, r1)] * 3
    return [(r0, r1)] + [(r0 >> ssv, dch if r1 >= dh else r1 >> ssv)] * (n_planes - 1)


@pytest.mark.parametrize("band", [2, 6, 16])
@pytest.mark.parametrize("fmt", [P, S, R], ids=["planar", "semiplanar", "rgb"])
def test_bands(ctx, fmt, band):
    """destination bands: each alone leaves every other row at the sentinel, their union equals the one call"""
    (w, h), (dw, dh), bpc, layout = (190, 102), (47, 33), 10, api.LAYOUT_I420
    pic, vis = make_source(ctx, np.random.default_rng(11500), w, h, layout, bpc, "twin-only")
    want = want_of(scaled_planes(vis, layout, dw, dh), layout, bpc, fmt, N)
    try:
        whole = Dest(ctx, dw, dh, layout, bpc, fmt, N)
        for r0 in range(0, dh, band):
            r1 = min(r0 + band, dh)
            d = Dest(ctx, dw, dh, layout, bpc, fmt, N)
            pic.export_scaled(d.surface, None, r0, r1)
            d.check(want, rows=dest_rows(fmt, len(want), dh, r0, r1, 1), what="band [%d, %d)" % (r0, r1))
            d.free()
            pic.export_scaled(whole.surface, None, r0, r1 if r1 < dh else 1 << 30)
        whole.check(want, what="the union of the bands")
        whole.free()
    finally:
        pic.free()


@pytest.mark.parametrize("fmt", [S, R], ids=["semiplanar", "rgb"])
@pytest.mark.parametrize("crop,size", [(None, (47, 33)), ((10, 6, 133, 71), (60, 33)), (None, (95, 51))], ids=["odd-ratio", "crop", "half"])
def test_rows_needed_is_safe_and_tight(ctx, fmt, crop, size):
    """For every band end r1: a copy of the source whose luma rows at and below scaled_rows_needed(r1), and the chroma rows under them, hold other
    values gives the same rows [0, r1); with one row fewer than the helper says at least one band of the sweep changes."""
    (w, h), (dw, dh), bpc, layout = (190, 102), size, 10, api.LAYOUT_I420
    rng = np.random.default_rng(11600)
    pic, vis = make_source(ctx, rng, w, h, layout, bpc, "raster")
    padded = [v.base for v in vis]
    want = want_of(scaled_planes(vis, layout, dw, dh, crop), layout, bpc, fmt, N)
    surface = Dest(ctx, dw, dh, layout, bpc, fmt, N)
    tight = False
    try:
        last = 0
        for r1 in list(range(6, dh, 6)) + [dh]:
            need = pic.scaled_rows_needed(surface.surface, crop, r1)
            assert last <= need <= h
            last = need
            y0, ch = (crop[1], crop[3]) if crop else (0, h)
            assert need == min(h, max(y0 + -(-r1 * ch // dh),
                                      2 * ((y0 >> 1) + -(-(((dh + 1) >> 1) if r1 >= dh else r1 >> 1) * ((ch + 1) >> 1) // ((dh + 1) >> 1)))))
            for rows, same in ((need, True), (need - 1, False)):
                other = [p.copy() for p in padded]
                other[0][rows:] ^= 0x155
                for pl in (1, 2):
                    other[pl][(rows + 1) >> 1:] ^= 0x155
                pic2, _ = source_from(ctx, other, w, h, layout, bpc, "twin-only")
                d = Dest(ctx, dw, dh, layout, bpc, fmt, N)
                pic2.export_scaled(d.surface, crop, 0, r1)
                if same:
                    d.check(want, rows=dest_rows(fmt, len(want), dh, 0, r1, 1), what="rows below %d changed, band [0, %d)" % (rows, r1))
                else:
                    try:
                        d.check(want, rows=dest_rows(fmt, len(want), dh, 0, r1, 1))
                    except AssertionError:
                        tight = True
                d.free()
                pic2.free()
        assert tight, "one source row fewer never changed a band: the helper is not tight"
    finally:
        surface.free()
        pic.free()


# ------------------------------------------------------------------------------------------------ 6. unaligned destinations

@pytest.mark.parametrize("pad", [0, 2, 10])
@pytest.mark.parametrize("offset", [0, 2, 6])
def test_unaligned_destinations(ctx, offset, pad):
    """the scalar store path, whole units and the partial last unit (47 = 5 * 8 + 7 samples, chroma 24 = 3 * 8)"""
    (w, h), (dw, dh), bpc, layout = (190, 102), (47, 13), 10, api.LAYOUT_I420
    pic, vis = make_source(ctx, np.random.default_rng(11700), w, h, layout, bpc, "twin-only")
    planes = scaled_planes(vis, layout, dw, dh)
    try:
        for fmt, sample in ((P, N), (S, N), (S, F), (R, N)):
            k = 2 if sample == F else 1          # (in half samples of the surface: see the module's docstring)
            check_scaled(ctx, pic, vis, dw, dh, fmt, sample, planes=planes, pad=pad * k, offset=offset * k, what="offset %d pad %d" % (offset, pad))
    finally:
        pic.free()


# ------------------------------------------------------------------------------------------------ 7. the source is left alone

def _live(ctx):
    out = (C.c_longlong * 4)()
    assert ctx.lib.dav1d_hip_live_objects(out) == 0
    return list(out)


def _raster_bytes(ctx, pic):
    out = np.zeros(pic.pic.alloc_size, np.uint8)
    ctx.sync()
    assert ctx.lib.dav1d_hip_download(ctx.h, out.ctypes.data, pic.pic.alloc, pic.pic.alloc_size) == 0
    return out


@pytest.mark.parametrize("fmt", [S, R], ids=["semiplanar", "rgb"])
def test_source_untouched(ctx, fmt):
    (w, h), (dw, dh), bpc, layout = (190, 102), (47, 13), 10, api.LAYOUT_I420
    for state in ("twin-only", "raster"):
        pic, vis = make_source(ctx, np.random.default_rng(11800), w, h, layout, bpc, state)
        try:
            raster = _raster_bytes(ctx, pic)
            twin = util.twin_bytes(ctx, pic) if state == "twin-only" else None
            ptrs, ok, live = [pic.pic.twin[pl] for pl in range(3)], pic.pic.twin_ok, _live(ctx)
            if state == "twin-only":
                assert (raster == 0x5A).all()
            check_scaled(ctx, pic, vis, dw, dh, fmt, N, crop=(10, 6, 133, 71), what=state)
            assert _live(ctx) == live, "the call allocated an object"
            assert pic.pic.twin_ok == ok and [pic.pic.twin[pl] for pl in range(3)] == ptrs
            assert np.array_equal(_raster_bytes(ctx, pic), raster)
            if twin is not None:
                assert np.array_equal(util.twin_bytes(ctx, pic), twin)
        finally:
            pic.free()


# ------------------------------------------------------------------------------------------------ 8. errors

def test_errors(ctx):
    w, h, bpc = 190, 102, 10
    rng = np.random.default_rng(11900)
    pics = {key: make_source(ctx, rng, w, h, key[1], key[0], "raster")[0]
            for key in ((10, api.LAYOUT_I420), (8, api.LAYOUT_I420), (10, api.LAYOUT_I422), (10, api.LAYOUT_I444))}

    def refused(code, fmt=P, sample=N, size=(95, 51), crop=None, rows=(0, 1 << 30), change=None, key=(10, api.LAYOUT_I420), helper=True, **kw):
        pic = pics[key]
        d = Dest(ctx, size[0], size[1], key[1], key[0], fmt, N if (sample == M and key[0] == 8) else sample, **kw)
        d.surface.desc.sample = sample
        if change:
            change(d.surface.desc)
        rect = api.SurfaceRect(*crop) if crop is not None else None
        rc = ctx.lib.dav1d_hip_surface_export_scaled(ctx.h, C.byref(d.surface.desc), C.byref(pic.pic), C.byref(rect) if rect else None, rows[0], rows[1])
        assert rc == -code, (rc, code, crop, size, rows)
        d.check(None, what="a refused export")
        if helper:          # the helper refuses what the export refuses (it sees drow1 only)
            assert ctx.lib.dav1d_hip_surface_scaled_rows_needed(C.byref(d.surface.desc), C.byref(pic.pic), C.byref(rect) if rect else None, rows[1]) == -code
        d.free()

    def null_plane(k):
        def f(desc):
            desc.data[k] = None
        return f

    def stride(k, delta):
        def f(desc):
            desc.stride[k] += delta
        return f
    try:
        # what the plain export refuses, with its code (the size rule excepted: 95x51 is accepted at the end)
        for fmt, k in ((P, 0), (P, 2), (S, 1), (R, 1)):
            refused(EINVAL, fmt, change=null_plane(k))
        refused(EINVAL, P, change=stride(0, -2))
        refused(EINVAL, S, change=stride(1, -2))
        refused(EINVAL, P, change=stride(0, +1), pad=2)
        refused(EINVAL, P, M, key=(8, api.LAYOUT_I420))
        refused(EINVAL, R, matrix=0)
        refused(ENOTSUP, R, matrix=4)
        refused(EINVAL, P, change=lambda d: setattr(d, "w", 0))
        refused(EINVAL, P, change=lambda d: setattr(d, "format", 3))
        # odd band rows
        refused(EINVAL, P, rows=(1, 32), helper=False)
        refused(EINVAL, R, rows=(0, 33))
        # the crop
        refused(EINVAL, crop=(100, 0, 100, 51), size=(50, 51))          # beyond the right edge
        refused(EINVAL, crop=(0, 60, 95, 51))                           # beyond the bottom
        refused(EINVAL, crop=(-2, 0, 95, 51))
        refused(EINVAL, crop=(0, -2, 95, 51))
        refused(EINVAL, crop=(0, 0, 0, 51))                             # empty
        refused(EINVAL, crop=(0, 0, 95, 0))
        refused(EINVAL, crop=(1, 0, 95, 51))                            # odd x0 at 4:2:0
        refused(EINVAL, crop=(0, 1, 95, 51))                            # odd y0 at 4:2:0
        refused(EINVAL, crop=(1, 0, 95, 51), key=(10, api.LAYOUT_I422))
        # ratios that are not built
        refused(ENOTSUP, size=(191, 102))
        refused(ENOTSUP, size=(190, 103))
        refused(ENOTSUP, size=(23, 51))                                 # 190 > 8 * 23
        refused(ENOTSUP, size=(95, 12))                                 # 102 > 8 * 12
        refused(ENOTSUP, crop=(0, 0, 94, 51), size=(95, 51))            # larger than the crop
        # ... and what is accepted: the same surfaces with nothing wrong, odd origins where the layout does not subsample the axis
        for key, crop, size in (((10, api.LAYOUT_I420), None, (95, 51)), ((10, api.LAYOUT_I422), (0, 1, 95, 51), (95, 51)),
                                ((10, api.LAYOUT_I444), (1, 1, 95, 51), (24, 13)), ((8, api.LAYOUT_I420), (0, 0, 184, 96), (23, 12))):
            d = Dest(ctx, size[0], size[1], key[1], key[0], R, N)
            pics[key].export_scaled(d.surface, crop)
            assert pics[key].scaled_rows_needed(d.surface, crop, 1 << 30) == (crop[1] + crop[3] if crop else h)
            ctx.sync()
            d.free()
    finally:
        for p in pics.values():
            p.free()


# ------------------------------------------------------------------------------------------------ 9. Python

def test_export_is_asynchronous_and_timed(ctx):
    """Context.surface + DevicePicture.export_scaled: the call returns with the work enqueued (nothing waits before download's sync), a device
    time from the context's two events, nothing left behind"""
    before = _live(ctx)
    pic, vis = make_source(ctx, np.random.default_rng(12000), 64, 64, api.LAYOUT_I420, 10, "retiled")
    s = ctx.surface(32, 32, api.LAYOUT_I420, 10, S, M)
    s.fill(0xA5)
    pic.export_scaled(s)
    got = s.download()
    ms = ctx.last_kernel_ms()
    assert ms > 0.0 if ctx.backend == "hip" else ms >= 0.0
    want = want_of(scaled_planes(vis, api.LAYOUT_I420, 32, 32), api.LAYOUT_I420, 10, S, M)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    s.free()
    pic.free()
    assert _live(ctx) == before


def _torch_child():
    """(a process of its own: torch brings its own HIP runtime, see tests/test_surface.py)"""
    import torch
    w, h, bpc, layout = 190, 102, 10, api.LAYOUT_I420
    tctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    pic, vis = make_source(tctx, np.random.default_rng(12100), w, h, layout, bpc, "twin-only", extremes=True)
    for crop in (None, (10, 6, 133, 71)):
        t = torch.empty((3, 54, 96), dtype=torch.float32, device="cuda")
        api.export_to_tensor(pic, t, matrix=1, full_range=0, crop=crop, resize=True)
        tctx.sync()
        got, want = t.cpu().numpy(), expect_rgb(scaled_planes(vis, layout, 96, 54, crop), layout, bpc, 1, 0, F)
        for k in range(3):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), "RGB float tensor, crop %s, plane %d" % (crop, k)
    t = torch.empty((3, 54, 96), dtype=torch.float32, device="cuda")
    for kw in ({}, {"crop": (0, 0, 96, 54)}):
        try:
            api.export_to_tensor(pic, t, **kw)
        except ValueError:
            pass
        else:
            raise AssertionError("a mismatched tensor was accepted without resize=True")
    assert pic.pic.twin_ok == api.TWIN_ONLY
    pic.free()
    tctx.close()
    print("torch-child ok")


@pytest.mark.gpu
def test_export_to_tensor_resized():
    """export_to_tensor(resize=True) into a float CHW RGB tensor of 96x54 from a 190x102 picture, again with crop=; the defaults still raise
    ValueError on a tensor of another size"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "torch-child"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torch-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["torch-child"]:
        _torch_child()
