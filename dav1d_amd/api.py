"""Thin object layer over the C ABI for Python callers (tests, bench.py, smoke()).

It only moves numpy arrays / device pointers in and out of the C entry points of
include/dav1d_hip.h; all reconstruction work happens in the HIP library.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FilmGrainData  # noqa: F401
from ._lib import ITX_TASK, MC_TASK, COMP_TASK, CDEF_TASK, LF_TASK, IPRED_TASK, LR_TASK, WARP_TASK, MC_SCALED_TASK, Picture, HostPicture  # noqa: F401  (re-exported)
from ._lib import Surface as SurfaceDesc
from ._lib import SurfaceRect, RgbParams, ColourDesc, ColourTone, LightStatsData, COLOUR_ENC_N

LAYOUT_I400, LAYOUT_I420, LAYOUT_I422, LAYOUT_I444 = 0, 1, 2, 3
SURFACE_PLANAR, SURFACE_SEMIPLANAR, SURFACE_RGB_PLANAR, SURFACE_RGB_PACKED, SURFACE_RGBA_PACKED = 0, 1, 2, 3, 4      # enum Dav1dHipSurfaceFormat
SAMPLE_NATIVE, SAMPLE_MSB16, SAMPLE_F32, SAMPLE_F16 = 0, 1, 2, 3      # enum Dav1dHipSurfaceSample
CHROMA_REPLICATE, CHROMA_VERTICAL, CHROMA_COLOCATED = 0, 1, 2         # Dav1dHipRgbParams.chroma_pos
RESIZE_BILINEAR = 0                                                   # enum Dav1dHipResizeFilter
_INTERP = {"bilinear": RESIZE_BILINEAR, "area": RESIZE_BILINEAR}      # export_to_tensor / export_batch_to_tensor: interp= ("area": the reduced calls, an
                                                                      # axis that goes up is interpolated linearly there as well)


def _filter_of(interp):
    if interp not in _INTERP:
        raise ValueError("interp= is None or one of %s" % sorted(_INTERP))
    return _INTERP[interp]


class HipError(RuntimeError):
    pass


def _chk(rc, what):
    if rc:
        why = ""
        if rc in (-5, -12, -38):          # -EIO / -ENOMEM / -ENOSYS: a HIP call was behind it
            try:
                why = " (HIP: %s)" % _lib.load().dav1d_hip_last_hip_error(None).decode()
            except Exception:           # noqa: BLE001
                pass
        raise HipError("%s failed: errno %d%s" % (what, -rc, why))


class DeviceBuffer:
    """A device allocation made through dav1d_hip_malloc."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_malloc(ctx.h, C.byref(p), self.nbytes), "malloc")
        self.ptr = p.value

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        assert offset + a.nbytes <= self.nbytes
        _chk(self.ctx.lib.dav1d_hip_upload(self.ctx.h, self.ptr + offset, a.ctypes.data, a.nbytes), "upload")

    def download(self, dtype, count=None, offset=0):
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dt)
        _chk(self.ctx.lib.dav1d_hip_download(self.ctx.h, out.ctypes.data, self.ptr + offset, out.nbytes), "download")
        return out

    def zero(self):
        _chk(self.ctx.lib.dav1d_hip_memset(self.ctx.h, self.ptr, 0, self.nbytes), "memset")

    def free(self):
        if self.ptr:
            self.ctx.lib.dav1d_hip_free(self.ctx.h, self.ptr)
            self.ptr = None


TWIN_ONLY = 2          # Dav1dHipPicture.twin_ok: the picture lives in its tiled twin, the raster planes are stale


class DevicePicture:
    def __init__(self, ctx, w, h, layout, bpc):
        self.ctx = ctx
        self.pic = Picture()
        _chk(ctx.lib.dav1d_hip_picture_alloc(ctx.h, C.byref(self.pic), w, h, layout, bpc), "picture_alloc")
        self.w, self.h, self.layout, self.bpc = w, h, layout, bpc
        self.dtype = np.uint8 if bpc == 8 else np.uint16

    @property
    def n_planes(self):
        return 1 if self.layout == LAYOUT_I400 else 3

    def padded_shape(self, plane):
        ss_ver = 1 if plane and self.layout == LAYOUT_I420 else 0
        ss_hor = 1 if plane and self.layout != LAYOUT_I444 else 0
        return (((self.h + 127) & ~127) >> ss_ver, ((self.w + 127) & ~127) >> ss_hor)

    def stride_px(self, plane):
        return self.pic.p[plane].stride // np.dtype(self.dtype).itemsize

    def upload(self, plane, arr):
        """arr: 2-D array of the PADDED plane shape (rows x cols)."""
        a = np.asarray(arr, dtype=self.dtype)
        if a.strides[1] != a.itemsize:
            a = np.ascontiguousarray(a)
        assert a.shape == self.padded_shape(plane), (a.shape, self.padded_shape(plane))
        _chk(self.ctx.lib.dav1d_hip_plane_upload(self.ctx.h, C.byref(self.pic), plane, a.ctypes.data,
                                                 a.strides[0], 1), "plane_upload")
        # the raster planes changed behind the tiled twin's back (Dav1dHipPicture.twin_ok is the caller's to keep)
        self.pic.twin_ok = 0
        if getattr(self.ctx, "auto_retile", False) and plane == self.n_planes - 1:
            self.retile()

    def untile(self):
        """dav1d_hip_picture_untile: a picture that lives in its twin gets its raster planes back (no-op otherwise)."""
        _chk(self.ctx.lib.dav1d_hip_picture_untile(self.ctx.h, C.byref(self.pic)), "picture_untile")

    def retile(self, overlapped=False):
        """(Re)build the tiled twin from the raster planes: motion compensation then reads this picture through it.  overlapped: on a
        side stream, next to whatever is enqueued afterwards (dav1d_hip_picture_retile_overlapped)."""
        fn = self.ctx.lib.dav1d_hip_picture_retile_overlapped if overlapped else self.ctx.lib.dav1d_hip_picture_retile
        _chk(fn(self.ctx.h, C.byref(self.pic)), "picture_retile")

    def download(self, plane):
        """Padded plane as a (rows x cols) view of a host array with the DEVICE row stride, so that
        the same pixel offsets address host and device copies."""
        rows, cols = self.padded_shape(plane)
        out = np.zeros((rows, self.stride_px(plane)), self.dtype)[:, :cols]
        _chk(self.ctx.lib.dav1d_hip_plane_download(self.ctx.h, C.byref(self.pic), plane, out.ctypes.data,
                                                   out.strides[0], 1), "plane_download")
        return out

    def export(self, surface, row0=0, row1=1 << 30, grain=None, is_id=0):
        """dav1d_hip_surface_export: luma rows [row0, row1) of this picture into a device surface of the caller, on the context's stream
        (asynchronous; a picture that lives in its twin only is read through the twin and stays there).  `grain` (a handle of
        Context.fg_prepare): film grain is applied in the same pass (dav1d_hip_surface_export_grain); the picture itself is not changed."""
        if grain is not None:
            _chk(self.ctx.lib.dav1d_hip_surface_export_grain(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), grain, is_id, row0, row1),
                 "surface_export_grain")
            return
        _chk(self.ctx.lib.dav1d_hip_surface_export(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), row0, row1), "surface_export")

    @staticmethod
    def _rect(crop):
        return None if crop is None else C.byref(SurfaceRect(*[int(v) for v in crop]))

    def export_scaled(self, surface, crop=None, row0=0, row1=1 << 30):
        """dav1d_hip_surface_export_scaled: the rectangle crop = (x0, y0, w, h) of this picture (None: all of it), scaled down to the surface's
        own size by the area scaler of include/dav1d_hip.h, into DESTINATION luma rows [row0, row1) of the surface.  Asynchronous like export."""
        _chk(self.ctx.lib.dav1d_hip_surface_export_scaled(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), self._rect(crop), row0, row1),
             "surface_export_scaled")

    def scaled_rows_needed(self, surface, crop, row1):
        """dav1d_hip_surface_scaled_rows_needed: the source luma rows, from the top, that destination rows [0, row1) of export_scaled read"""
        n = self.ctx.lib.dav1d_hip_surface_scaled_rows_needed(C.byref(surface.desc), C.byref(self.pic), self._rect(crop), row1)
        _chk(min(n, 0), "surface_scaled_rows_needed")
        return n

    @staticmethod
    def _rgb_params(chroma_pos, scale, bias):
        if scale is None and bias is None:
            return RgbParams(int(chroma_pos), 0)
        p = RgbParams(int(chroma_pos), 1)
        for k in range(3):
            p.scale[k] = 1.0 if scale is None else scale[k]
            p.bias[k] = 0.0 if bias is None else bias[k]
        return p

    def export_rgb(self, surface, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30):
        """dav1d_hip_surface_export_rgb: luma rows [row0, row1) as RGB into a planar or packed (RGB / RGBA) surface, any sample type, chroma
        upsampled at its site (chroma_pos: CHROMA_REPLICATE, CHROMA_VERTICAL, CHROMA_COLOCATED).  `scale` / `bias` (three floats each, R, G, B;
        float samples only) normalise: out = v * scale[c] + bias[c].  Asynchronous like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), C.byref(p), row0, row1), "surface_export_rgb")

    def export_rgb_colour(self, surface, colour, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30):
        """dav1d_hip_surface_export_rgb_colour: export_rgb followed in the same pass by the tables of `colour` (Context.colour / Context.colour_for):
        linearise, 3x3 matrix, re-encode.  Float surfaces only (F32, F16); without `scale` / `bias` the sample is the tables' value itself (no 1 / max
        factor).  rgb_rows_needed serves this call as it is.  Asynchronous like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb_colour(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), C.byref(p), colour, row0, row1),
             "surface_export_rgb_colour")

    def rgb_rows_needed(self, surface, chroma_pos, row1):
        """dav1d_hip_surface_rgb_rows_needed: the luma rows, from the top, that rows [0, row1) of export_rgb read"""
        p = self._rgb_params(chroma_pos, None, None)
        n = self.ctx.lib.dav1d_hip_surface_rgb_rows_needed(C.byref(surface.desc), C.byref(self.pic), C.byref(p), row1)
        _chk(min(n, 0), "surface_rgb_rows_needed")
        return n

    def export_rgb_scaled(self, surface, crop=None, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30):
        """dav1d_hip_surface_export_rgb_scaled: export_scaled and export_rgb in one pass — the rectangle `crop` (None: all of the picture) scaled
        down to the surface's size, as RGB planes or packed RGB / RGBA of any sample type, the scaled chroma upsampled at `chroma_pos`, normalised
        by `scale` / `bias`; DESTINATION luma rows [row0, row1).  Asynchronous like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb_scaled(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), row0, row1),
             "surface_export_rgb_scaled")

    def rgb_scaled_rows_needed(self, surface, crop, chroma_pos, row1):
        """dav1d_hip_surface_rgb_scaled_rows_needed: the source luma rows, from the top, that destination rows [0, row1) of export_rgb_scaled read"""
        p = self._rgb_params(chroma_pos, None, None)
        n = self.ctx.lib.dav1d_hip_surface_rgb_scaled_rows_needed(C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), row1)
        _chk(min(n, 0), "surface_rgb_scaled_rows_needed")
        return n

    def export_rgb_resized(self, surface, crop=None, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_resized: export_rgb_scaled to ANY size — an axis of the rectangle `crop` that is shorter than the surface's
        is interpolated up (RESIZE_BILINEAR: linear, half-sample centres), one that is longer goes down through the area scaler as before, every
        plane and axis on its own.  Everything else as in export_rgb_scaled.  Asynchronous like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb_resized(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), int(filter),
                                                               row0, row1), "surface_export_rgb_resized")

    def rgb_resized_rows_needed(self, surface, crop, chroma_pos, row1, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_rgb_resized_rows_needed: the source luma rows, from the top, that destination rows [0, row1) of export_rgb_resized read"""
        p = self._rgb_params(chroma_pos, None, None)
        n = self.ctx.lib.dav1d_hip_surface_rgb_resized_rows_needed(C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), int(filter), row1)
        _chk(min(n, 0), "surface_rgb_resized_rows_needed")
        return n

    def export_rgb_reduced(self, surface, crop=None, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_reduced: export_rgb_resized whose axes may go down by any ratio up to 256:1 (thumbnails, network inputs from
        8K pictures): the area rule at every ratio, `filter` for an axis that goes up.  Up to 8:1 on every axis the bytes are export_rgb_resized's.
        Asynchronous like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb_reduced(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), int(filter),
                                                               row0, row1), "surface_export_rgb_reduced")

    def rgb_reduced_rows_needed(self, surface, crop, chroma_pos, row1, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_rgb_reduced_rows_needed: the source luma rows, from the top, that destination rows [0, row1) of export_rgb_reduced read"""
        p = self._rgb_params(chroma_pos, None, None)
        n = self.ctx.lib.dav1d_hip_surface_rgb_reduced_rows_needed(C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), int(filter), row1)
        _chk(min(n, 0), "surface_rgb_reduced_rows_needed")
        return n

    def export_rgb_colour_reduced(self, surface, colour, crop=None, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_colour_reduced: export_rgb_reduced followed by the tables of `colour` (Context.colour / Context.colour_for) as in
        export_rgb_colour — the rectangle `crop` at the surface's size, any ratio up to 256:1 down and any size up, linearised, gamut-mapped and
        re-encoded.  Float surfaces only (F32, F16); the colour stage runs on the resampled code values.  rgb_reduced_rows_needed serves this call as
        it is.  Asynchronous like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb_colour_reduced(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), colour,
                                                                      int(filter), row0, row1), "surface_export_rgb_colour_reduced")

    def export_rgb_linear_reduced(self, surface, colour, crop=None, chroma_pos=0, scale=None, bias=None, row0=0, row1=1 << 30, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_linear_reduced: export_rgb_colour_reduced that scales in LINEAR LIGHT — the rectangle `crop` is converted to
        RGB and linearised at its own size (sited chroma at source resolution), the light is averaged with the weights of export_rgb_reduced, and the
        matrix, enc and normalisation of `colour` follow.  Float surfaces only; a handle whose lin has a negative entry is refused.  Asynchronous
        like export."""
        p = self._rgb_params(chroma_pos, scale, bias)
        _chk(self.ctx.lib.dav1d_hip_surface_export_rgb_linear_reduced(self.ctx.h, C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), colour,
                                                                      int(filter), row0, row1), "surface_export_rgb_linear_reduced")

    def rgb_linear_rows_needed(self, surface, crop, chroma_pos, row1, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_rgb_linear_rows_needed: the source luma rows, from the top, that destination rows [0, row1) of export_rgb_linear_reduced read"""
        p = self._rgb_params(chroma_pos, None, None)
        n = self.ctx.lib.dav1d_hip_surface_rgb_linear_rows_needed(C.byref(surface.desc), C.byref(self.pic), self._rect(crop), C.byref(p), int(filter), row1)
        _chk(min(n, 0), "surface_rgb_linear_rows_needed")
        return n

    @classmethod
    def view(cls, ctx, pic, w, h, layout, bpc):
        """A non-owning wrapper around a Picture descriptor (e.g. the frame-owned output of FrameInFlight.end())."""
        self = cls.__new__(cls)
        self.ctx, self.pic = ctx, pic
        self.w, self.h, self.layout, self.bpc = w, h, layout, bpc
        self.dtype = np.uint8 if bpc == 8 else np.uint16
        self.borrowed = True
        return self

    def free(self):
        if not getattr(self, "borrowed", False):
            self.ctx.lib.dav1d_hip_picture_free(self.ctx.h, C.byref(self.pic))


def surface_planes(w, h, layout, bpc, fmt, sample):
    """[(rows, samples per row)] of the planes of a surface, and the numpy dtype of its samples (include/dav1d_hip.h, Dav1dHipSurface)."""
    dt = np.dtype(np.float32 if sample == SAMPLE_F32 else np.float16 if sample == SAMPLE_F16 else np.uint16 if sample == SAMPLE_MSB16 or bpc > 8 else np.uint8)
    if fmt == SURFACE_RGB_PLANAR:
        return [(h, w)] * 3, dt
    if fmt in (SURFACE_RGB_PACKED, SURFACE_RGBA_PACKED):
        return [(h, (3 if fmt == SURFACE_RGB_PACKED else 4) * w)], dt
    if layout == LAYOUT_I400:
        return [(h, w)], dt
    cw = (w + 1) >> 1 if layout != LAYOUT_I444 else w
    ch = (h + 1) >> 1 if layout == LAYOUT_I420 else h
    if fmt == SURFACE_SEMIPLANAR:
        return [(h, w), (ch, 2 * cw)], dt
    return [(h, w), (ch, cw), (ch, cw)], dt


class Surface:
    """A Dav1dHipSurface: device memory a picture is exported into (DevicePicture.export).  Context.surface() makes one that owns its
    buffers; Surface.wrap() describes memory of somebody else (a torch tensor, an encoder's input) and frees nothing."""

    def __init__(self, ctx, w, h, layout, bpc, fmt, sample, matrix=1, full_range=0, strides=None):
        self.ctx = ctx
        self.shapes, self.dtype = surface_planes(w, h, layout, bpc, fmt, sample)
        self.strides = list(strides) if strides is not None else [cols * self.dtype.itemsize for _, cols in self.shapes]
        assert len(self.strides) == len(self.shapes)
        self.bufs = [ctx.buffer(max(rows * st, 16)) for (rows, _), st in zip(self.shapes, self.strides)]
        self._describe([b.ptr for b in self.bufs], w, h, fmt, sample, matrix, full_range)

    def _describe(self, ptrs, w, h, fmt, sample, matrix, full_range):
        self.desc = SurfaceDesc()
        for k, p in enumerate(ptrs):
            self.desc.data[k] = p
            self.desc.stride[k] = self.strides[k]
        self.desc.format, self.desc.sample, self.desc.w, self.desc.h = fmt, sample, w, h
        self.desc.matrix, self.desc.full_range = matrix, full_range

    @classmethod
    def wrap(cls, ctx, ptrs, strides, w, h, layout, bpc, fmt, sample, matrix=1, full_range=0):
        """Foreign device memory: ptrs / strides (bytes) per plane of the format."""
        self = cls.__new__(cls)
        self.ctx, self.bufs = ctx, None
        self.shapes, self.dtype = surface_planes(w, h, layout, bpc, fmt, sample)
        self.strides = list(strides)
        self._describe(list(ptrs), w, h, fmt, sample, matrix, full_range)
        return self

    def fill(self, byte):
        for b in self.bufs:
            _chk(self.ctx.lib.dav1d_hip_memset(self.ctx.h, b.ptr, byte, b.nbytes), "memset")

    def raw(self, k):
        """every byte of plane k's buffer as (rows, stride) uint8 (waits for the context's stream)"""
        rows = self.shapes[k][0]
        return self.bufs[k].download(np.uint8, rows * self.strides[k]).reshape(rows, self.strides[k])

    def download(self):
        """numpy arrays of the visible size, one per plane of the format"""
        out = []
        for k, (rows, cols) in enumerate(self.shapes):
            out.append(np.ascontiguousarray(self.raw(k)[:, :cols * self.dtype.itemsize]).view(self.dtype))
        return out

    def free(self):
        for b in self.bufs or []:
            b.free()
        self.bufs = None


def colour_tables(lib, bpc, trc_in, pri_in, trc_out=8, pri_out=1, white_nits=203.0, peak_nits=1000.0):
    """dav1d_hip_colour_tables (host arithmetic, no device): lin (float32), m (3 x 3 float32), enc (uint16 bit patterns), has_matrix, has_enc"""
    lin, m, enc = np.zeros(1 << bpc if bpc in (8, 10, 12) else 1, np.float32), np.zeros(9, np.float32), np.zeros(COLOUR_ENC_N, np.uint16)
    has_matrix, has_enc = C.c_int(0), C.c_int(0)
    _chk(lib.dav1d_hip_colour_tables(bpc, trc_in, pri_in, trc_out, pri_out, white_nits, peak_nits, lin.ctypes.data, m.ctypes.data, C.byref(has_matrix),
                                     enc.ctypes.data, C.byref(has_enc)), "colour_tables")
    return lin, m.reshape(3, 3), enc, bool(has_matrix.value), bool(has_enc.value)


def colour_tables_toned(lib, bpc, trc_in, pri_in, trc_out=8, pri_out=1, white_nits=203.0, peak_nits=1000.0):
    """dav1d_hip_colour_tables_toned (host arithmetic, no device): the tables of colour_tables with the tone curve taken out of enc and put into a gain
    on the pixel's luminance, and the HLG OOTF — lin, m, enc, has_matrix, has_enc, k (3 float32), gain (uint16 bit patterns), has_gain"""
    lin, m, enc = np.zeros(1 << bpc if bpc in (8, 10, 12) else 1, np.float32), np.zeros(9, np.float32), np.zeros(COLOUR_ENC_N, np.uint16)
    k, gain = np.zeros(3, np.float32), np.zeros(COLOUR_ENC_N, np.uint16)
    has_matrix, has_enc, has_gain = C.c_int(0), C.c_int(0), C.c_int(0)
    _chk(lib.dav1d_hip_colour_tables_toned(bpc, trc_in, pri_in, trc_out, pri_out, white_nits, peak_nits, lin.ctypes.data, m.ctypes.data, C.byref(has_matrix),
                                           enc.ctypes.data, C.byref(has_enc), k.ctypes.data, gain.ctypes.data, C.byref(has_gain)), "colour_tables_toned")
    return lin, m.reshape(3, 3), enc, bool(has_matrix.value), bool(has_enc.value), k, gain, bool(has_gain.value)


def export_to_tensor(pic, tensor, chroma=None, sample=None, matrix=1, full_range=0, row0=0, row1=1 << 30, grain=None, is_id=0, crop=None, resize=False,
                     chroma_pos=None, scale=None, bias=None, colour=None, interp=None):
    """Fills torch tensors on the picture's device through tensor.data_ptr(): `tensor` of shape (3, h, w) gets R, G, B planes; with
    `chroma` of shape (ceil(h / 2), 2 * ceil(w / 2)) given, `tensor` (h, w) gets luma and `chroma` the interleaved U, V of a 4:2:0
    picture (NV12 / P010 family).  The sample type follows the dtype (float32: F32; else `sample`, native by default).  The context should
    have been opened on the stream the tensors are used on (api.Context(stream=torch.cuda.current_stream().cuda_stream)).  `grain` / `is_id`:
    as in DevicePicture.export.  `resize=True`: the tensors' shape gives the output size, and `crop` = (x0, y0, w, h) (None: the whole picture)
    the rectangle that is scaled to it (DevicePicture.export_scaled; rows are then destination rows, and there is no grain).
    A tensor of shape (h, w, 3) or (h, w, 4) gets packed RGB / RGBA, and torch.float16 gets binary16 samples: both go through
    DevicePicture.export_rgb, as does any RGB tensor when `chroma_pos`, `scale` or `bias` is given (see there; no grain then).  With `resize=True`
    these go through DevicePicture.export_rgb_scaled; the output size of a packed tensor is its shape[0] x shape[1] (a shape that reads both ways, (3, n, 3) or (3, n, 4), raises ValueError with these options).
    `colour` (a handle of Context.colour / Context.colour_for): float RGB tensors go through DevicePicture.export_rgb_colour; not together with
    `grain`, `crop` or `resize`.
    `interp="bilinear"` (with `resize=True`; RGB tensors only, no `grain`, no `colour`): the output may be LARGER than the crop on either axis; the
    call goes through DevicePicture.export_rgb_resized.  `interp="area"`: through DevicePicture.export_rgb_reduced, which also serves an output up to
    256 times SMALLER than the crop on either axis (an axis that goes up is interpolated linearly).  `interp=None` keeps the routes above, which
    refuse such sizes."""
    import torch
    if interp is not None:
        flt = _filter_of(interp)
        if not resize:
            raise ValueError("interp= needs resize=True")
        if grain is not None or colour is not None or chroma is not None:
            raise ValueError("interp= goes through export_rgb_resized: RGB tensors only, no grain, no colour")
    if colour is not None and (grain is not None or crop is not None or resize):
        raise ValueError("colour= goes through export_rgb_colour: no grain, no crop, no resize")
    if crop is not None and not resize:
        raise ValueError("crop= needs resize=True")
    if resize and grain is not None:
        raise ValueError("the scaled export applies no film grain")
    hwc = resize and chroma is None and tensor.dim() == 3 and int(tensor.shape[2]) in (3, 4)
    if hwc and int(tensor.shape[0]) == 3:          # (3, n, 3) or (3, n, 4): planes of width 3 / 4, or a packed picture of height 3
        if tensor.dtype == torch.float16 or chroma_pos is not None or scale is not None or bias is not None:
            raise ValueError("a tensor of shape %s can be read as (3, h, w) and as (h, w, 3 or 4): not accepted with resize=True" % (tuple(tensor.shape),))
        hwc = False                                # what worked before these options: planes
    w, h = (int(tensor.shape[1]), int(tensor.shape[0])) if hwc else (int(tensor.shape[-1]), int(tensor.shape[-2])) if resize else (pic.w, pic.h)
    ts = [tensor] if chroma is None else [tensor, chroma]
    for t in ts:
        if not t.is_cuda or t.stride(-1) != 1:
            raise ValueError("export_to_tensor needs device tensors with unit stride along a row")
    if sample is None:
        sample = SAMPLE_F32 if tensor.dtype == torch.float32 else SAMPLE_F16 if tensor.dtype == torch.float16 else SAMPLE_NATIVE
    es = tensor.element_size()
    packed = chroma is None and tensor.dim() == 3 and tuple(tensor.shape[:2]) == (h, w) and int(tensor.shape[2]) in (3, 4)
    rgbx = packed or sample == SAMPLE_F16 or chroma_pos is not None or scale is not None or bias is not None or colour is not None
    if rgbx and (chroma is not None or grain is not None):
        raise ValueError("packed RGB, float16, chroma_pos, scale and bias go through export_rgb / export_rgb_scaled: RGB tensors only, no grain")
    if packed:
        if tensor.stride(1) != int(tensor.shape[2]):
            raise ValueError("a packed RGB tensor has its channels next to each other")
        fmt = SURFACE_RGB_PACKED if int(tensor.shape[2]) == 3 else SURFACE_RGBA_PACKED
        ptrs = [tensor.data_ptr()]
        strides = [tensor.stride(0) * es]
    elif chroma is None:
        if tuple(tensor.shape) != (3, h, w):
            raise ValueError("an RGB tensor has shape (3, h, w), (h, w, 3) or (h, w, 4)")
        fmt = SURFACE_RGB_PLANAR
        ptrs = [tensor[k].data_ptr() for k in range(3)]
        strides = [tensor.stride(1) * es] * 3
    else:
        if tuple(tensor.shape) != (h, w) or chroma.dtype != tensor.dtype:
            raise ValueError("a semi-planar pair has shapes (h, w) and (ceil(h / 2), 2 * ceil(w / 2)) and one dtype")
        fmt = SURFACE_SEMIPLANAR
        ptrs = [tensor.data_ptr(), chroma.data_ptr()]
        strides = [tensor.stride(0) * es, chroma.stride(0) * es]
    s = Surface.wrap(pic.ctx, ptrs, strides, w, h, pic.layout, pic.bpc, fmt, sample, matrix, full_range)
    if s.dtype.itemsize != es or (not packed and [tuple(t.shape[-2:]) for t in ts] != s.shapes[:len(ts)]):
        raise ValueError("tensor shapes / dtype do not fit the surface: %s %s" % (s.shapes, s.dtype))
    if interp == "area":
        pic.export_rgb_reduced(s, crop, chroma_pos or 0, scale, bias, row0, row1, flt)
        return s
    if interp is not None:
        pic.export_rgb_resized(s, crop, chroma_pos or 0, scale, bias, row0, row1, flt)
        return s
    if rgbx and resize:
        pic.export_rgb_scaled(s, crop, chroma_pos or 0, scale, bias, row0, row1)
        return s
    if colour is not None:
        pic.export_rgb_colour(s, colour, chroma_pos or 0, scale, bias, row0, row1)
        return s
    if rgbx:
        pic.export_rgb(s, chroma_pos or 0, scale, bias, row0, row1)
        return s
    if resize:
        pic.export_scaled(s, crop, row0, row1)
        return s
    pic.export(s, row0, row1, grain=grain, is_id=is_id)
    return s


def export_batch_to_tensor(pics, tensor, crops=None, matrix=1, full_range=0, sample=None, chroma_pos=None, scale=None, bias=None, interp=None):
    """Fills one torch tensor with N pictures (or N regions: pictures may repeat) through Context.export_rgb_scaled_batch, one launch for all of them:
    `tensor` of shape (N, 3, h, w) gets R, G, B planes, (N, h, w, 3) / (N, h, w, 4) gets packed RGB / RGBA; h x w is the output size of every item and
    crops[k] = (x0, y0, w, h) (`crops` None: the whole picture) the rectangle of pics[k] that is scaled to it.  The dtype picks the sample as in
    export_to_tensor (float32: F32, float16: F16, else `sample`, native by default).  Item k is written through tensor[k]: any batch stride is fine
    (a view such as big[::2]), rows need unit stride.  ValueError for what export_to_tensor raises, for len(pics) != N, and for a shape
    (N, 3, n, 3) or (N, 3, n, 4), which reads both ways.  `interp="bilinear"`: through Context.export_rgb_resized_batch, h x w may then be larger than
    a crop on either axis (None: such an item makes the batch raise, as before).  `interp="area"`: through Context.export_rgb_reduced_batch, h x w may
    also be up to 256 times smaller than a crop.  Returns the surfaces."""
    flt = None if interp is None else _filter_of(interp)
    if tensor.dim() != 4:
        raise ValueError("a batch tensor has shape (N, 3, h, w), (N, h, w, 3) or (N, h, w, 4)")
    shape = tuple(int(v) for v in tensor.shape)
    n = shape[0]
    if len(pics) != n or (crops is not None and len(crops) != n):
        raise ValueError("a tensor of shape %s takes %d pictures, and %d crops if any" % (shape, n, n))
    chw, hwc = shape[1] == 3, shape[3] in (3, 4)
    if chw and hwc:
        raise ValueError("a tensor of shape %s can be read as (N, 3, h, w) and as (N, h, w, 3 or 4): not accepted" % (shape,))
    if not chw and not hwc:
        raise ValueError("a batch tensor has shape (N, 3, h, w), (N, h, w, 3) or (N, h, w, 4)")
    if not tensor.is_cuda:
        raise ValueError("export_batch_to_tensor needs a device tensor")
    if tensor.stride(-1) != 1:
        raise ValueError("export_batch_to_tensor needs unit stride along a row")
    if hwc and tensor.stride(2) != shape[3]:
        raise ValueError("a packed RGB tensor has its channels next to each other")
    if sample is None:
        import torch
        sample = SAMPLE_F32 if tensor.dtype == torch.float32 else SAMPLE_F16 if tensor.dtype == torch.float16 else SAMPLE_NATIVE
    es = tensor.element_size()
    h, w = (shape[1], shape[2]) if hwc else (shape[2], shape[3])
    fmt = SURFACE_RGB_PLANAR if chw else SURFACE_RGB_PACKED if shape[3] == 3 else SURFACE_RGBA_PACKED
    surfaces = []
    for k, pic in enumerate(pics):
        t = tensor[k]
        ptrs, strides = ([t.data_ptr()], [t.stride(0) * es]) if hwc else ([t[c].data_ptr() for c in range(3)], [t.stride(1) * es] * 3)
        s = Surface.wrap(pic.ctx, ptrs, strides, w, h, pic.layout, pic.bpc, fmt, sample, matrix, full_range)
        if s.dtype.itemsize != es:
            raise ValueError("tensor dtype does not fit the surface of item %d: %s" % (k, s.dtype))
        surfaces.append(s)
    if n and interp == "area":
        pics[0].ctx.export_rgb_reduced_batch(surfaces, pics, crops, chroma_pos or 0, scale, bias, flt)
    elif n and flt is not None:
        pics[0].ctx.export_rgb_resized_batch(surfaces, pics, crops, chroma_pos or 0, scale, bias, flt)
    elif n:
        pics[0].ctx.export_rgb_scaled_batch(surfaces, pics, crops, chroma_pos or 0, scale, bias)
    return surfaces


def _colour_sample(tensor):
    import torch
    if tensor.dtype not in (torch.float32, torch.float16):
        raise ValueError("the colour-managed export writes float32 or float16 tensors")
    return SAMPLE_F32 if tensor.dtype == torch.float32 else SAMPLE_F16


def export_colour_to_tensor(pic, tensor, colour, crop=None, matrix=1, full_range=0, chroma_pos=None, scale=None, bias=None, linear_light=False):
    """Fills a float32 / float16 torch tensor with the rectangle `crop` = (x0, y0, w, h) of the picture (None: all of it) at the TENSOR's size, through
    the tables of `colour` (Context.colour / Context.colour_for): DevicePicture.export_rgb_colour_reduced.  Shape (3, h, w) gets R, G, B planes,
    (h, w, 3) / (h, w, 4) packed RGB / RGBA; h x w may be up to 256 times smaller than the crop on either axis, or larger.  Shape and stride rules are
    export_to_tensor's: a device tensor, unit stride along a row, the channels of a packed tensor next to each other, and a shape that reads both
    ways, (3, n, 3) or (3, n, 4), raises ValueError.  `linear_light=True` scales in linear light: DevicePicture.export_rgb_linear_reduced.
    Returns the surface."""
    if colour is None:
        raise ValueError("export_colour_to_tensor needs a colour handle")
    if tensor.dim() != 3:
        raise ValueError("an RGB tensor has shape (3, h, w), (h, w, 3) or (h, w, 4)")
    shape = tuple(int(v) for v in tensor.shape)
    chw, hwc = shape[0] == 3, shape[2] in (3, 4)
    if chw and hwc:
        raise ValueError("a tensor of shape %s can be read as (3, h, w) and as (h, w, 3 or 4): not accepted" % (shape,))
    if not chw and not hwc:
        raise ValueError("an RGB tensor has shape (3, h, w), (h, w, 3) or (h, w, 4)")
    if not tensor.is_cuda or tensor.stride(-1) != 1:
        raise ValueError("export_colour_to_tensor needs a device tensor with unit stride along a row")
    es = tensor.element_size()
    if hwc:
        if tensor.stride(1) != shape[2]:
            raise ValueError("a packed RGB tensor has its channels next to each other")
        h, w = shape[0], shape[1]
        fmt, ptrs, strides = (SURFACE_RGB_PACKED if shape[2] == 3 else SURFACE_RGBA_PACKED), [tensor.data_ptr()], [tensor.stride(0) * es]
    else:
        h, w = shape[1], shape[2]
        fmt, ptrs, strides = SURFACE_RGB_PLANAR, [tensor[k].data_ptr() for k in range(3)], [tensor.stride(1) * es] * 3
    s = Surface.wrap(pic.ctx, ptrs, strides, w, h, pic.layout, pic.bpc, fmt, _colour_sample(tensor), matrix, full_range)
    (pic.export_rgb_linear_reduced if linear_light else pic.export_rgb_colour_reduced)(s, colour, crop, chroma_pos or 0, scale, bias)
    return s


def export_colour_batch_to_tensor(pics, tensor, colour, crops=None, matrix=1, full_range=0, chroma_pos=None, scale=None, bias=None, linear_light=False):
    """Fills one float32 / float16 torch tensor with N pictures (or N regions: pictures may repeat) through Context.export_rgb_colour_reduced_batch:
    `tensor` of shape (N, 3, h, w) gets R, G, B planes, (N, h, w, 3) / (N, h, w, 4) packed RGB / RGBA; crops[k] = (x0, y0, w, h) (`crops` None: the
    whole picture) is the rectangle of pics[k] that goes to h x w, at any ratio up to 256:1 down and any size up, through the tables of `colour`.
    Shape and stride rules are export_batch_to_tensor's.  `linear_light=True` scales in linear light: Context.export_rgb_linear_reduced_batch.
    Returns the surfaces."""
    if colour is None:
        raise ValueError("export_colour_batch_to_tensor needs a colour handle")
    if tensor.dim() != 4:
        raise ValueError("a batch tensor has shape (N, 3, h, w), (N, h, w, 3) or (N, h, w, 4)")
    shape = tuple(int(v) for v in tensor.shape)
    n = shape[0]
    if len(pics) != n or (crops is not None and len(crops) != n):
        raise ValueError("a tensor of shape %s takes %d pictures, and %d crops if any" % (shape, n, n))
    chw, hwc = shape[1] == 3, shape[3] in (3, 4)
    if chw and hwc:
        raise ValueError("a tensor of shape %s can be read as (N, 3, h, w) and as (N, h, w, 3 or 4): not accepted" % (shape,))
    if not chw and not hwc:
        raise ValueError("a batch tensor has shape (N, 3, h, w), (N, h, w, 3) or (N, h, w, 4)")
    if not tensor.is_cuda:
        raise ValueError("export_colour_batch_to_tensor needs a device tensor")
    if tensor.stride(-1) != 1:
        raise ValueError("export_colour_batch_to_tensor needs unit stride along a row")
    if hwc and tensor.stride(2) != shape[3]:
        raise ValueError("a packed RGB tensor has its channels next to each other")
    sample = _colour_sample(tensor)
    es = tensor.element_size()
    h, w = (shape[1], shape[2]) if hwc else (shape[2], shape[3])
    fmt = SURFACE_RGB_PLANAR if chw else SURFACE_RGB_PACKED if shape[3] == 3 else SURFACE_RGBA_PACKED
    surfaces = []
    for k, pic in enumerate(pics):
        t = tensor[k]
        ptrs, strides = ([t.data_ptr()], [t.stride(0) * es]) if hwc else ([t[c].data_ptr() for c in range(3)], [t.stride(1) * es] * 3)
        surfaces.append(Surface.wrap(pic.ctx, ptrs, strides, w, h, pic.layout, pic.bpc, fmt, sample, matrix, full_range))
    if n:
        ctx = pics[0].ctx
        (ctx.export_rgb_linear_reduced_batch if linear_light else ctx.export_rgb_colour_reduced_batch)(surfaces, pics, colour, crops, chroma_pos or 0, scale, bias)
    return surfaces


class _List:
    def __init__(self, ctx, kind, tasks, dtype):
        self.ctx, self.kind = ctx, kind
        t = np.ascontiguousarray(tasks, dtype=dtype)
        self.n = len(t)
        self.h = C.c_void_p()
        _chk(getattr(ctx.lib, "dav1d_hip_%s_list_create" % kind)(ctx.h, C.byref(self.h), t.ctypes.data, len(t)),
             kind + "_list_create")

    def destroy(self):
        if self.h:
            getattr(self.ctx.lib, "dav1d_hip_%s_list_destroy" % self.kind)(self.ctx.h, self.h)
            self.h = None


class _InterList:
    def __init__(self, ctx, mc_tasks, comp_tasks):
        self.ctx = ctx
        m = np.ascontiguousarray(mc_tasks, dtype=MC_TASK)
        k = np.ascontiguousarray(comp_tasks, dtype=COMP_TASK)
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_inter_list_create(ctx.h, C.byref(self.h), m.ctypes.data, len(m), k.ctypes.data, len(k)),
             "inter_list_create")
        self.n_fused = int(ctx.lib.dav1d_hip_inter_list_fused(self.h))

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_inter_list_destroy(self.ctx.h, self.h)
            self.h = None


class _ReconList:
    """dav1d_hip_recon_list_*: predictions + residuals of a frame, pipelined per tile shape / transform size."""

    def __init__(self, ctx, geometry, mc_tasks, comp_tasks, itx_tasks):
        self.ctx = ctx
        m = np.ascontiguousarray(mc_tasks, dtype=MC_TASK)
        k = np.ascontiguousarray(comp_tasks, dtype=COMP_TASK)
        t = np.ascontiguousarray(itx_tasks, dtype=ITX_TASK)
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_recon_list_create(ctx.h, C.byref(self.h), C.byref(geometry.pic), m.ctypes.data, len(m),
                                                 k.ctypes.data, len(k), t.ctypes.data, len(t)), "recon_list_create")

    def run(self, dst, refs, prep, coef, mask=None):
        if getattr(self.ctx, "tiled_native", False):       # (tests: every recon list of the context leaves its picture in the twin only)
            return self.run_tiled(dst, refs, prep, coef, mask)
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        p = None if prep is None else (prep.ptr if hasattr(prep, "ptr") else prep)
        m = None if mask is None else (mask.ptr if hasattr(mask, "ptr") else mask)
        _chk(self.ctx.lib.dav1d_hip_recon_list_run(self.ctx.h, self.h, C.byref(dst.pic), arr, len(refs), p, m,
                                                   coef.ptr if hasattr(coef, "ptr") else coef), "recon_list_run")

    def run_tiled(self, dst, refs, prep, coef, mask=None):
        """dav1d_hip_recon_list_run_tiled: the picture lives in its tiled twin only afterwards (dst.pic.twin_ok == TWIN_ONLY when every
        launch could write tiles; 1 after the raster + retile fallback).  download() / the fetch calls un-tile on the way out."""
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        p = None if prep is None else (prep.ptr if hasattr(prep, "ptr") else prep)
        m = None if mask is None else (mask.ptr if hasattr(mask, "ptr") else mask)
        _chk(self.ctx.lib.dav1d_hip_recon_list_run_tiled(self.ctx.h, self.h, C.byref(dst.pic), arr, len(refs), p, m,
                                                         coef.ptr if hasattr(coef, "ptr") else coef), "recon_list_run_tiled")

    def run_twin(self, dst, refs, prep, coef, mask=None):
        """dav1d_hip_recon_list_run_twin: the frame's pixels also end up in dst's tiled twin (written by the launches themselves when
        they can, by a retile pass otherwise); dst.pic.twin_ok is set."""
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        p = None if prep is None else (prep.ptr if hasattr(prep, "ptr") else prep)
        m = None if mask is None else (mask.ptr if hasattr(mask, "ptr") else mask)
        _chk(self.ctx.lib.dav1d_hip_recon_list_run_twin(self.ctx.h, self.h, C.byref(dst.pic), arr, len(refs), p, m,
                                                        coef.ptr if hasattr(coef, "ptr") else coef), "recon_list_run_twin")

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_recon_list_destroy(self.ctx.h, self.h)
            self.h = None


def _tone_of(tone):
    """(k, gain) as a ColourTone, and the array it points into (to be kept alive for the call)"""
    k, gain = tone
    k = np.asarray(k, dtype=np.float32).reshape(-1)
    if k.size != 3:
        raise ValueError("tone is (k, gain) with three coefficients k")
    gain = np.ascontiguousarray(gain)
    gain = np.ascontiguousarray(gain.view(np.uint16) if gain.dtype == np.float16 else gain, dtype=np.uint16)
    if gain.size != COLOUR_ENC_N:
        raise ValueError("gain has COLOUR_ENC_N entries")
    return ColourTone(k=(C.c_float * 3)(*[float(v) for v in k]), gain=gain.ctypes.data_as(C.POINTER(C.c_uint16))), gain


class LightStats:
    """Per-picture light statistics on the device (dav1d_hip_light_stats_*, include/dav1d_hip.h): a histogram of luminance over the index of a toned
    handle's gain, with the pixels above 1.0, the pixels at or below 0 and the largest light.  add() accumulates without waiting; read() waits."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_light_stats_create(ctx.h, C.byref(self.h)), "light_stats_create")
        self._data = None

    def reset(self):
        _chk(self.ctx.lib.dav1d_hip_light_stats_reset(self.ctx.h, self.h), "light_stats_reset")
        self._data = None

    def add(self, pic, colour, k, crop=None, matrix=1, full_range=0, chroma_pos=0, row0=0, row1=1 << 30):
        """dav1d_hip_picture_light_stats: counts luma rows [row0, row1) of the rectangle crop = (x0, y0, w, h) of `pic` (None: all of it), its codes
        linearised by the handle `colour`, its luminance weighed by the three coefficients k."""
        k = np.asarray(k, dtype=np.float32).reshape(-1)
        if k.size != 3:
            raise ValueError("k has three coefficients")
        _chk(self.ctx.lib.dav1d_hip_picture_light_stats(self.ctx.h, self.h, C.byref(pic.pic), DevicePicture._rect(crop), matrix, full_range, chroma_pos, colour,
                                                        (C.c_float * 3)(*[float(v) for v in k]), row0, row1), "picture_light_stats")
        self._data = None

    def _read(self):
        if self._data is None:
            d = LightStatsData()
            _chk(self.ctx.lib.dav1d_hip_light_stats_read(self.ctx.h, self.h, C.byref(d)), "light_stats_read")
            self._data = d
        return self._data

    def read(self):
        """dav1d_hip_light_stats_read: {"n", "n_above", "n_nonpos" (ints), "max_light" (float32), "hist" (uint64 array of COLOUR_ENC_N)}.  Waits."""
        d = self._read()
        return {"n": int(d.n), "n_above": int(d.n_above), "n_nonpos": int(d.n_nonpos), "max_light": np.float32(d.max_light),
                "hist": np.ctypeslib.as_array(d.hist).astype(np.uint64)}

    def rank(self, fraction):
        """the bin that holds the pixel of rank max(1, ceil(fraction * n)) counted from the darkest (dav1d_hip_light_stats_rank); 0.999: the 99.9th percentile"""
        d = self._read()
        h = C.c_int(-1)
        _chk(self.ctx.lib.dav1d_hip_light_stats_rank(C.byref(d), max(1, int(np.ceil(fraction * int(d.n)))), C.byref(h)), "light_stats_rank")
        return h.value

    def mean(self):
        """dav1d_hip_light_stats_mean: the mean of the bins' values, in the unit of the index"""
        return float(self.ctx.lib.dav1d_hip_light_stats_mean(C.byref(self._read())))

    def free(self):
        if self.h:
            _chk(self.ctx.lib.dav1d_hip_light_stats_destroy(self.ctx.h, self.h), "light_stats_destroy")
            self.h = C.c_void_p()


class Context:
    """dav1d_hip_open() wrapper.  `stream` is a raw hipStream_t (int) or None."""

    def __init__(self, device=0, stream=None, lib_path=None):
        self.lib = _lib.load(lib_path)
        self.device, self.lib_path = device, lib_path
        h = C.c_void_p()
        rc = self.lib.dav1d_hip_open(C.byref(h), device, stream)
        if rc:
            raise HipError("dav1d_hip_open(device=%d) failed: errno %d (no usable MI355X device; there is no "
                           "CPU fallback)" % (device, -rc))
        self.h = h

    def close(self):
        if self.h:
            self.lib.dav1d_hip_close(self.h)
            self.h = None

    def get_option(self, name):
        """dav1d_hip_get_option: a counter or knob of this context (see include/dav1d_hip.h)"""
        v = C.c_long()
        _chk(self.lib.dav1d_hip_get_option(self.h, name.encode(), C.byref(v)), "get_option(%s)" % name)
        return v.value

    def set_option(self, name, value):
        """dav1d_hip_set_option: a tuning knob of this context (see include/dav1d_hip.h)"""
        _chk(self.lib.dav1d_hip_set_option(self.h, name.encode(), int(value)), "set_option(%s)" % name)

    def sync(self):
        _chk(self.lib.dav1d_hip_sync(self.h), "sync")

    def buffer(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def buffer_from(self, arr):
        a = np.ascontiguousarray(arr)
        b = DeviceBuffer(self, max(a.nbytes, 16))
        if a.nbytes:
            b.upload(a)
        return b

    def picture(self, w, h, layout, bpc):
        return DevicePicture(self, w, h, layout, bpc)

    def surface(self, w, h, layout, bpc, format, sample, matrix=1, full_range=0, strides=None):
        """A device output surface that owns its buffers (dav1d_hip_malloc); strides in bytes per plane, tight rows by default."""
        return Surface(self, w, h, layout, bpc, format, sample, matrix, full_range, strides)

    def graph_begin(self):
        """Start recording the list runs issued on this context (dav1d_hip_graph_begin)."""
        _chk(self.lib.dav1d_hip_graph_begin(self.h), "graph_begin")

    def graph_end(self):
        g = C.c_void_p()
        _chk(self.lib.dav1d_hip_graph_end(self.h, C.byref(g)), "graph_end")
        return g

    def graph_launch(self, g):
        _chk(self.lib.dav1d_hip_graph_launch(self.h, g), "graph_launch")

    def graph_destroy(self, g):
        self.lib.dav1d_hip_graph_destroy(self.h, g)

    def last_kernel_ms(self):
        return float(self.lib.dav1d_hip_last_kernel_ms(self.h))

    def colour(self, lin, matrix=None, enc=None, bpc=None, tone=None):
        """dav1d_hip_colour_create: a handle for DevicePicture.export_rgb_colour from tables of the caller — `lin`: 1 << bpc float32 values (code ->
        linear); `matrix`: None or 9 values, row-major; `enc`: None or COLOUR_ENC_N binary16 bit patterns (uint16, or a float16 array), indexed by the
        binary16 pattern of the clamped linear value.  `tone`: None, or (k, gain) of dav1d_hip_colour_create_toned — three luminance coefficients and
        COLOUR_ENC_N binary16 patterns (uint16 or float16 like enc) indexed by the clamped luminance: the gain that multiplies all three channels
        in front of the matrix.  Copies the tables to the device and waits.  colour_destroy() frees it."""
        lin = np.ascontiguousarray(lin, dtype=np.float32)
        if bpc is None:
            bpc = int(lin.size).bit_length() - 1
        if lin.size != 1 << bpc:
            raise ValueError("lin has 1 << bpc entries")
        d = ColourDesc(bpc=bpc, lin=lin.ctypes.data_as(C.POINTER(C.c_float)), has_matrix=int(matrix is not None))
        if matrix is not None:
            d.m[:] = [float(v) for v in np.asarray(matrix, dtype=np.float32).reshape(9)]
        if enc is not None:
            enc = np.ascontiguousarray(enc)
            enc = np.ascontiguousarray(enc.view(np.uint16) if enc.dtype == np.float16 else enc, dtype=np.uint16)
            if enc.size != COLOUR_ENC_N:
                raise ValueError("enc has COLOUR_ENC_N entries")
            d.enc = enc.ctypes.data_as(C.POINTER(C.c_uint16))
        h = C.c_void_p()
        if tone is None:
            _chk(self.lib.dav1d_hip_colour_create(self.h, C.byref(d), C.byref(h)), "colour_create")
            return h
        t, _keep = _tone_of(tone)
        _chk(self.lib.dav1d_hip_colour_create_toned(self.h, C.byref(d), C.byref(t), C.byref(h)), "colour_create_toned")
        return h

    def colour_for(self, bpc, trc_in, pri_in, trc_out=8, pri_out=1, white_nits=203.0, peak_nits=1000.0, luminance=False):
        """dav1d_hip_colour_tables, then colour(): the handle that takes pictures of AV1's transfer / primaries codes trc_in / pri_in to trc_out /
        pri_out (8: linear light, 1.0 = white_nits).  luminance=True: dav1d_hip_colour_tables_toned — the tone curve as a gain on the pixel's luminance,
        which keeps the hue of saturated highlights, and the HLG OOTF."""
        if luminance:
            lin, m, enc, has_matrix, has_enc, k, gain, has_gain = colour_tables_toned(self.lib, bpc, trc_in, pri_in, trc_out, pri_out, white_nits, peak_nits)
            return self.colour(lin, m if has_matrix else None, enc if has_enc else None, bpc, tone=(k, gain) if has_gain else None)
        lin, m, enc, has_matrix, has_enc = colour_tables(self.lib, bpc, trc_in, pri_in, trc_out, pri_out, white_nits, peak_nits)
        return self.colour(lin, m if has_matrix else None, enc if has_enc else None, bpc)

    def colour_destroy(self, h):
        _chk(self.lib.dav1d_hip_colour_destroy(self.h, h), "colour_destroy")

    def colour_update_tone(self, h, tone):
        """dav1d_hip_colour_update_tone: replaces the tone part of the live handle `h` (one made with tone=) by tone = (k, gain), in stream order
        and without waiting: exports enqueued before use the old part, exports enqueued after the new one.  The arrays may be reused on return."""
        t, _keep = _tone_of(tone)          # (_keep: the array t.gain points into, which may be a copy made here, lives until the call has returned)
        _chk(self.lib.dav1d_hip_colour_update_tone(self.h, h, C.byref(t)), "colour_update_tone")
        del _keep

    def light_stats(self):
        """dav1d_hip_light_stats_create: a zeroed accumulator of per-picture light statistics on this context's device (LightStats)."""
        return LightStats(self)

    def colour_light_table(self, h, bpc):
        """dav1d_hip_colour_light_table: (q, e) of a handle of `bpc` bits — the light table in fixed point of the linear-light exports, q[v] =
        rint(lin[v] 2^(31 - e)) as uint32; HipError where the handle has none (a lin with a negative entry).  Waits."""
        q, e = np.empty(1 << bpc, np.uint32), C.c_int(0)
        _chk(self.lib.dav1d_hip_colour_light_table(self.h, h, q.ctypes.data, C.byref(e)), "colour_light_table")
        return q, e.value

    def export_rgb_scaled_batch(self, surfaces, pics, crops=None, chroma_pos=0, scale=None, bias=None, _filter=None, _reduced=False, _colour=None, _linear=False):
        """dav1d_hip_surface_export_rgb_scaled_batch: item k gets what pics[k].export_rgb_scaled(surfaces[k], crops[k], chroma_pos, scale, bias) writes,
        all items in one launch (two when raster and twin-only pictures are mixed).  Pictures may repeat; `crops` is None (every item whole) or a
        rectangle (x0, y0, w, h) per item.  One format, one sample type and one pixel size (8 bit, or 10 / 12 bit) per batch.  Asynchronous like
        export; a HipError names the item that was refused."""
        n = len(surfaces)
        if len(pics) != n or (crops is not None and len(crops) != n):
            raise ValueError("a batch takes one picture, and one crop if any, per surface")
        dst = (SurfaceDesc * max(n, 1))(*[s.desc for s in surfaces])
        src = (C.POINTER(Picture) * max(n, 1))(*[C.pointer(q.pic) for q in pics])
        rects = None if crops is None else (SurfaceRect * max(n, 1))(*[SurfaceRect(*[int(v) for v in r]) for r in crops])
        p = DevicePicture._rgb_params(chroma_pos, scale, bias)
        bad = C.c_int(-1)
        if _linear:
            rc = self.lib.dav1d_hip_surface_export_rgb_linear_reduced_batch(self.h, n, dst, src, rects, C.byref(p), _colour, int(_filter), C.byref(bad))
            what = "surface_export_rgb_linear_reduced_batch"
        elif _colour is not None:
            rc = self.lib.dav1d_hip_surface_export_rgb_colour_reduced_batch(self.h, n, dst, src, rects, C.byref(p), _colour, int(_filter), C.byref(bad))
            what = "surface_export_rgb_colour_reduced_batch"
        elif _reduced:
            rc = self.lib.dav1d_hip_surface_export_rgb_reduced_batch(self.h, n, dst, src, rects, C.byref(p), int(_filter), C.byref(bad))
            what = "surface_export_rgb_reduced_batch"
        elif _filter is None:
            rc, what = self.lib.dav1d_hip_surface_export_rgb_scaled_batch(self.h, n, dst, src, rects, C.byref(p), C.byref(bad)), "surface_export_rgb_scaled_batch"
        else:
            rc = self.lib.dav1d_hip_surface_export_rgb_resized_batch(self.h, n, dst, src, rects, C.byref(p), int(_filter), C.byref(bad))
            what = "surface_export_rgb_resized_batch"
        _chk(rc, what + (" (item %d)" % bad.value if bad.value >= 0 else ""))

    def export_rgb_resized_batch(self, surfaces, pics, crops=None, chroma_pos=0, scale=None, bias=None, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_resized_batch: export_rgb_scaled_batch whose item k gets what pics[k].export_rgb_resized(surfaces[k], crops[k],
        chroma_pos, scale, bias, filter=filter) writes — a surface may be larger than its crop on either axis, and the items of a batch may mix axes
        that go up, down and nowhere."""
        self.export_rgb_scaled_batch(surfaces, pics, crops, chroma_pos, scale, bias, _filter=filter)

    def export_rgb_reduced_batch(self, surfaces, pics, crops=None, chroma_pos=0, scale=None, bias=None, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_reduced_batch: export_rgb_resized_batch whose item k gets what pics[k].export_rgb_reduced(surfaces[k], crops[k],
        chroma_pos, scale, bias, filter=filter) writes — items over 8:1 (up to 256:1), under it and going up mix freely."""
        self.export_rgb_scaled_batch(surfaces, pics, crops, chroma_pos, scale, bias, _filter=filter, _reduced=True)

    def export_rgb_colour_reduced_batch(self, surfaces, pics, colour, crops=None, chroma_pos=0, scale=None, bias=None, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_colour_reduced_batch: export_rgb_reduced_batch whose item k gets what
        pics[k].export_rgb_colour_reduced(surfaces[k], colour, crops[k], chroma_pos, scale, bias, filter=filter) writes.  One handle serves all items:
        float surfaces only, and every picture has the handle's bit depth."""
        if colour is None:
            raise ValueError("export_rgb_colour_reduced_batch needs a colour handle")
        self.export_rgb_scaled_batch(surfaces, pics, crops, chroma_pos, scale, bias, _filter=filter, _colour=colour)

    def export_rgb_linear_reduced_batch(self, surfaces, pics, colour, crops=None, chroma_pos=0, scale=None, bias=None, filter=RESIZE_BILINEAR):
        """dav1d_hip_surface_export_rgb_linear_reduced_batch: item k gets what pics[k].export_rgb_linear_reduced(surfaces[k], colour, crops[k],
        chroma_pos, scale, bias, filter=filter) writes — scaling in linear light, many items per launch.  One handle serves all items."""
        if colour is None:
            raise ValueError("export_rgb_linear_reduced_batch needs a colour handle")
        self.export_rgb_scaled_batch(surfaces, pics, crops, chroma_pos, scale, bias, _filter=filter, _colour=colour, _linear=True)

    # ---- batched entry points (host task arrays, device arenas)
    def itx_add_batch(self, dst, tasks, coef):
        t = np.ascontiguousarray(tasks, dtype=ITX_TASK)
        _chk(self.lib.dav1d_hip_itx_add_batch(self.h, C.byref(dst.pic), t.ctypes.data, len(t), coef.ptr), "itx_add_batch")

    def mc_batch(self, dst, refs, tasks, prep=None):
        t = np.ascontiguousarray(tasks, dtype=MC_TASK)
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        _chk(self.lib.dav1d_hip_mc_batch(self.h, C.byref(dst.pic), arr, len(refs), t.ctypes.data, len(t),
                                         prep.ptr if prep else None), "mc_batch")

    def comp_batch(self, dst, tasks, prep, mask=None):
        t = np.ascontiguousarray(tasks, dtype=COMP_TASK)
        _chk(self.lib.dav1d_hip_comp_batch(self.h, C.byref(dst.pic), t.ctypes.data, len(t), prep.ptr,
                                           mask.ptr if mask else None), "comp_batch")

    def warp_batch(self, dst, refs, tasks, prep=None):
        t = np.ascontiguousarray(tasks, dtype=WARP_TASK)
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        _chk(self.lib.dav1d_hip_warp_batch(self.h, C.byref(dst.pic), arr, len(refs), t.ctypes.data, len(t),
                                           prep.ptr if prep else None), "warp_batch")

    def mc_scaled_batch(self, dst, refs, tasks, prep=None):
        t = np.ascontiguousarray(tasks, dtype=MC_SCALED_TASK)
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        _chk(self.lib.dav1d_hip_mc_scaled_batch(self.h, C.byref(dst.pic), arr, len(refs), t.ctypes.data, len(t),
                                                prep.ptr if prep else None), "mc_scaled_batch")

    def resize(self, dst, src, plane, dst_w, y0, h, src_w, dx, mx0):
        _chk(self.lib.dav1d_hip_resize(self.h, C.byref(dst.pic), C.byref(src.pic), plane, dst_w, y0, h, src_w, dx, mx0), "resize")

    def emu_edge(self, bpc, bw, bh, iw, ih, x, y, dst, dst_stride, ref, ref_stride):
        """dst / ref: DeviceBuffer (or raw device address); strides in bytes."""
        d = dst.ptr if hasattr(dst, "ptr") else dst
        r = ref.ptr if hasattr(ref, "ptr") else ref
        _chk(self.lib.dav1d_hip_emu_edge(self.h, bpc, bw, bh, iw, ih, x, y, d, dst_stride, r, ref_stride), "emu_edge")

    def cdef_batch(self, dst, src, tasks, damping, dirvar=None):
        t = np.ascontiguousarray(tasks, dtype=CDEF_TASK)
        _chk(self.lib.dav1d_hip_cdef_batch(self.h, C.byref(dst.pic), C.byref(src.pic), t.ctypes.data, len(t), damping,
                                           dirvar.ptr if dirvar else None), "cdef_batch")

    def lf_batch(self, dst, tasks, lvl, b4_stride, lut_e, lut_i):
        t = np.ascontiguousarray(tasks, dtype=LF_TASK)
        e = np.ascontiguousarray(lut_e, dtype=np.uint8)
        i = np.ascontiguousarray(lut_i, dtype=np.uint8)
        assert len(e) == 64 and len(i) == 64
        _chk(self.lib.dav1d_hip_lf_batch(self.h, C.byref(dst.pic), t.ctypes.data, len(t), lvl.ptr, b4_stride,
                                         e.ctypes.data, i.ctypes.data), "lf_batch")

    def ipred_batch(self, dst, tasks, pal_idx=None):
        t = np.ascontiguousarray(tasks, dtype=IPRED_TASK)
        _chk(self.lib.dav1d_hip_ipred_batch(self.h, C.byref(dst.pic), t.ctypes.data, len(t),
                                            pal_idx.ptr if pal_idx else None), "ipred_batch")

    def lr_batch(self, dst, src, lpf, tasks):
        t = np.ascontiguousarray(tasks, dtype=LR_TASK)
        _chk(self.lib.dav1d_hip_lr_batch(self.h, C.byref(dst.pic), C.byref(src.pic), C.byref(lpf.pic), t.ctypes.data, len(t)),
             "lr_batch")

    def fg_apply(self, dst, src, data, is_id=0):
        _chk(self.lib.dav1d_hip_fg_apply(self.h, C.byref(dst.pic), C.byref(src.pic), C.byref(data), is_id), "fg_apply")

    def fg_prepare(self, data, bpc, layout):
        """dav1d_hip_fg_prepare: templates + scaling tables on a side stream; returns the handle for fg_apply_prepared."""
        g = C.c_void_p()
        _chk(self.lib.dav1d_hip_fg_prepare(self.h, C.byref(g), C.addressof(data), bpc, layout), "fg_prepare")
        return g

    def fg_apply_prepared(self, dst, src, g, is_id=0):
        _chk(self.lib.dav1d_hip_fg_apply_prepared(self.h, C.byref(dst.pic), C.byref(src.pic), g, is_id), "fg_apply_prepared")

    def fg_grain_destroy(self, g):
        self.lib.dav1d_hip_fg_grain_destroy(self.h, g)

    def fg_generate_grain(self, data, bpc, layout):
        out = np.zeros((3, 74, 82), np.int16)
        _chk(self.lib.dav1d_hip_fg_generate_grain(self.h, C.byref(data), bpc, layout, out.ctypes.data), "fg_generate_grain")
        return out

    def frame(self, cur, refs):
        return FrameInFlight(self, cur, refs)

    def intra_list(self, batches):
        return _IntraList(self, batches)

    def ipred_list(self, batches):
        return _IpredList(self, batches)

    def intra_flow(self, batches):
        return _IntraFlow(self, batches)

    def intra_sb(self, batches, geometry, sb128=False, col_start_sb=None, row_start_sb=None):
        return _IntraSb(self, batches, geometry, sb128, col_start_sb, row_start_sb)

    # ---- device-resident lists
    def itx_list(self, tasks):
        return _List(self, "itx", tasks, ITX_TASK)

    def mc_list(self, tasks):
        return _List(self, "mc", tasks, MC_TASK)

    def comp_list(self, tasks):
        return _List(self, "comp", tasks, COMP_TASK)

    def recon_list(self, geometry, mc_tasks, comp_tasks, itx_tasks):
        return _ReconList(self, geometry, mc_tasks, comp_tasks, itx_tasks)

    def inter_list(self, mc_tasks, comp_tasks):
        return _InterList(self, mc_tasks, comp_tasks)

    def run_inter_list(self, lst, dst, refs, prep=None, mask=None):
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        p = None if prep is None else (prep.ptr if hasattr(prep, "ptr") else prep)
        m = None if mask is None else (mask.ptr if hasattr(mask, "ptr") else mask)
        _chk(self.lib.dav1d_hip_inter_list_run(self.h, lst.h, C.byref(dst.pic), arr, len(refs), p, m), "inter_list_run")

    def run_itx_list(self, lst, dst, coef):
        _chk(self.lib.dav1d_hip_itx_list_run(self.h, lst.h, C.byref(dst.pic), coef.ptr if hasattr(coef, "ptr") else coef),
             "itx_list_run")

    def run_mc_list(self, lst, dst, refs, prep=None):
        arr = (Picture * len(refs))(*[r.pic for r in refs])
        p = None if prep is None else (prep.ptr if hasattr(prep, "ptr") else prep)
        _chk(self.lib.dav1d_hip_mc_list_run(self.h, lst.h, C.byref(dst.pic), arr, len(refs), p), "mc_list_run")

    def run_comp_list(self, lst, dst, prep, mask=None):
        p = prep.ptr if hasattr(prep, "ptr") else prep
        m = None if mask is None else (mask.ptr if hasattr(mask, "ptr") else mask)
        _chk(self.lib.dav1d_hip_comp_list_run(self.h, lst.h, C.byref(dst.pic), p, m), "comp_list_run")


class _IpredList:
    """dav1d_hip_ipred_list_*: the intra batches of a wavefront, device resident."""

    def __init__(self, ctx, batches):
        self.ctx = ctx
        self.n_batches = len(batches)
        sizes = (C.c_size_t * max(len(batches), 1))(*[len(b) for b in batches])
        allt = np.ascontiguousarray(np.concatenate(batches) if len(batches) else np.zeros(0, IPRED_TASK), dtype=IPRED_TASK)
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_ipred_list_create(ctx.h, C.byref(self.h), allt.ctypes.data, sizes, len(batches)), "ipred_list_create")

    def run_batch(self, k, dst, aux=None):
        _chk(self.ctx.lib.dav1d_hip_ipred_list_run_batch(self.ctx.h, self.h, k, C.byref(dst.pic), aux.ptr if aux else None), "ipred_list_run_batch")

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_ipred_list_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class _IntraList:
    """dav1d_hip_intra_list_*: predictions + residuals of every wavefront step (small blocks paired in one wave)."""

    def __init__(self, ctx, batches):
        """batches: [(ipred tasks, itx tasks)] per wavefront step."""
        self.ctx = ctx
        self.n_batches = len(batches)
        ps = (C.c_size_t * max(len(batches), 1))(*[len(b[0]) for b in batches])
        ts = (C.c_size_t * max(len(batches), 1))(*[len(b[1]) for b in batches])
        allp = np.ascontiguousarray(np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, IPRED_TASK), dtype=IPRED_TASK)
        allt = np.ascontiguousarray(np.concatenate([b[1] for b in batches]) if batches else np.zeros(0, ITX_TASK), dtype=ITX_TASK)
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_intra_list_create(ctx.h, C.byref(self.h), allp.ctypes.data, ps, allt.ctypes.data, ts, len(batches)),
             "intra_list_create")

    def run_batch(self, k, dst, coef, aux=None):
        _chk(self.ctx.lib.dav1d_hip_intra_list_run_batch(self.ctx.h, self.h, k, C.byref(dst.pic), coef.ptr if hasattr(coef, "ptr") else coef,
                                                         aux.ptr if aux else None), "intra_list_run_batch")

    def run_all(self, dst, coef, aux=None):
        _chk(self.ctx.lib.dav1d_hip_intra_list_run_all(self.ctx.h, self.h, C.byref(dst.pic), coef.ptr if hasattr(coef, "ptr") else coef,
                                                       aux.ptr if aux else None), "intra_list_run_all")

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_intra_list_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class _IntraFlow:
    """dav1d_hip_intra_flow_*: the whole wavefront as one launch."""

    def __init__(self, ctx, batches):
        self.ctx = ctx
        ps = (C.c_size_t * max(len(batches), 1))(*[len(b[0]) for b in batches])
        ts = (C.c_size_t * max(len(batches), 1))(*[len(b[1]) for b in batches])
        allp = np.ascontiguousarray(np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, IPRED_TASK), dtype=IPRED_TASK)
        allt = np.ascontiguousarray(np.concatenate([b[1] for b in batches]) if batches else np.zeros(0, ITX_TASK), dtype=ITX_TASK)
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_intra_flow_create(ctx.h, C.byref(self.h), allp.ctypes.data, ps, allt.ctypes.data, ts, len(batches)),
             "intra_flow_create")
        self.n_units = int(ctx.lib.dav1d_hip_intra_flow_units(self.h))

    def run(self, dst, coef, aux=None):
        _chk(self.ctx.lib.dav1d_hip_intra_flow_run(self.ctx.h, self.h, C.byref(dst.pic), coef.ptr if hasattr(coef, "ptr") else coef,
                                                   aux.ptr if aux else None), "intra_flow_run")

    def status(self):
        out = (C.c_uint32 * 3)()
        _chk(self.ctx.lib.dav1d_hip_intra_flow_status(self.ctx.h, self.h, out), "intra_flow_status")
        return tuple(int(v) for v in out)

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_intra_flow_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class _IntraSb:
    """dav1d_hip_intra_sb_*: the wavefront superblock by superblock (a workgroup per superblock, a launch per level).
    col_start_sb / row_start_sb: the tile starts in superblocks, last entry = the end (None: one tile)."""

    def __init__(self, ctx, batches, geometry, sb128=False, col_start_sb=None, row_start_sb=None):
        self.ctx = ctx
        ps = (C.c_size_t * max(len(batches), 1))(*[len(b[0]) for b in batches])
        ts = (C.c_size_t * max(len(batches), 1))(*[len(b[1]) for b in batches])
        allp = np.ascontiguousarray(np.concatenate([b[0] for b in batches]) if batches else np.zeros(0, IPRED_TASK), dtype=IPRED_TASK)
        allt = np.ascontiguousarray(np.concatenate([b[1] for b in batches]) if batches else np.zeros(0, ITX_TASK), dtype=ITX_TASK)
        sb = 128 if sb128 else 64
        w, h = int(geometry.pic.p[0].w), int(geometry.pic.p[0].h)
        cols = list(col_start_sb) if col_start_sb is not None else [0, (w + sb - 1) // sb]
        rows = list(row_start_sb) if row_start_sb is not None else [0, (h + sb - 1) // sb]
        ca = (C.c_uint16 * len(cols))(*cols)
        ra = (C.c_uint16 * len(rows))(*rows)
        self.h = C.c_void_p()
        _chk(ctx.lib.dav1d_hip_intra_sb_create(ctx.h, C.byref(self.h), allp.ctypes.data, ps, allt.ctypes.data, ts, len(batches),
                                               C.byref(geometry.pic), int(bool(sb128)), len(cols) - 1, ca, len(rows) - 1, ra),
             "intra_sb_create")
        self.n_levels = int(ctx.lib.dav1d_hip_intra_sb_levels(self.h))
        self.n_superblocks = int(ctx.lib.dav1d_hip_intra_sb_superblocks(self.h))

    def run(self, dst, coef, aux=None):
        _chk(self.ctx.lib.dav1d_hip_intra_sb_run(self.ctx.h, self.h, C.byref(dst.pic), coef.ptr if hasattr(coef, "ptr") else coef,
                                                 aux.ptr if aux else None), "intra_sb_run")

    def status(self):
        """dav1d_hip_intra_sb_status: waits for the run; raises when superblocks of the one-launch form were left unreconstructed"""
        n = C.c_uint32()
        _chk(self.ctx.lib.dav1d_hip_intra_sb_status(self.ctx.h, self.h, C.byref(n)), "intra_sb_status (%d superblocks gave up)" % n.value)

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_intra_sb_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()


class HostPictureBuf:
    """dav1d_hip_host_picture_*: pinned host planes + the device picture of the same geometry (the buffers behind a
    Dav1dPicAllocator, reference include/dav1d/picture.h)."""

    def __init__(self, ctx, w, h, layout, bpc):
        self.ctx = ctx
        self.hp = HostPicture()
        _chk(ctx.lib.dav1d_hip_host_picture_alloc(ctx.h, C.byref(self.hp), w, h, layout, bpc), "host_picture_alloc")
        self.w, self.h, self.layout, self.bpc = w, h, layout, bpc

    @property
    def dev(self):
        return self.hp.dev

    def fetch(self, src=None, row0=0, row1=1 << 30):
        _chk(self.ctx.lib.dav1d_hip_host_picture_fetch(self.ctx.h, C.byref(self.hp), C.byref(src) if src is not None else None, row0, row1),
             "host_picture_fetch")

    def wait(self):
        _chk(self.ctx.lib.dav1d_hip_host_picture_wait(self.ctx.h), "host_picture_wait")

    def plane(self, pl):
        """numpy view of host plane pl (visible w x h)."""
        p = self.hp.dev.p[pl]
        dt = np.uint16 if self.bpc > 8 else np.uint8
        stride = self.hp.stride[1 if pl else 0]
        buf = (C.c_uint8 * (stride * p.h)).from_address(self.hp.data[pl])
        return np.frombuffer(buf, dtype=dt).reshape(p.h, stride // dt().itemsize)[:, :p.w]

    def release(self):
        if self.hp.alloc:
            _chk(self.ctx.lib.dav1d_hip_host_picture_release(self.ctx.h, C.byref(self.hp)), "host_picture_release")


class FrameInFlight:
    """dav1d_hip_frame_*: one frame in flight (driver-level boundary)."""

    def __init__(self, ctx, cur, refs):
        self.ctx = ctx
        self.cur = cur
        self.h = C.c_void_p()
        arr = (Picture * max(len(refs), 1))(*[r.pic for r in refs])
        _chk(ctx.lib.dav1d_hip_frame_begin(ctx.h, C.byref(self.h), C.byref(cur.pic), arr, len(refs)), "frame_begin")

    def _cur_written(self, filtered):
        # the frame wrote cur's raster planes: its tiled twin is valid only if the frame itself retiled it (option ref_twin = 2)
        same = filtered is not None and filtered.p[0].data == self.cur.pic.p[0].data
        self.cur.pic.twin_ok = filtered.twin_ok if same else 0

    def submit_tile_sbrow(self, mc, comp, itx):
        m = np.ascontiguousarray(mc, dtype=MC_TASK)
        c = np.ascontiguousarray(comp, dtype=COMP_TASK)
        t = np.ascontiguousarray(itx, dtype=ITX_TASK)
        _chk(self.ctx.lib.dav1d_hip_frame_submit_tile_sbrow(self.h, m.ctypes.data, len(m), c.ctypes.data, len(c), t.ctypes.data, len(t)),
             "frame_submit_tile_sbrow")

    def submit_intra_step(self, step, ipred, itx, aux=None):
        a = np.ascontiguousarray(ipred, dtype=IPRED_TASK)
        t = np.ascontiguousarray(itx, dtype=ITX_TASK)
        _chk(self.ctx.lib.dav1d_hip_frame_submit_intra_step(self.h, step, a.ctypes.data, len(a), t.ctypes.data, len(t),
                                                            aux.ptr if aux is not None else None), "frame_submit_intra_step")

    def submit_filter_sbrow(self, lf, cdef, lr):
        a = np.ascontiguousarray(lf, dtype=LF_TASK)
        b = np.ascontiguousarray(cdef, dtype=CDEF_TASK)
        c = np.ascontiguousarray(lr, dtype=LR_TASK)
        _chk(self.ctx.lib.dav1d_hip_frame_submit_filter_sbrow(self.h, a.ctypes.data, len(a), b.ctypes.data, len(b), c.ctypes.data, len(c)),
             "frame_submit_filter_sbrow")

    def set_filters(self, lvl, b4_stride, lut_e, lut_i, cdef_damping, grain=None, is_id=0):
        e = np.ascontiguousarray(lut_e, dtype=np.uint8)
        i = np.ascontiguousarray(lut_i, dtype=np.uint8)
        _chk(self.ctx.lib.dav1d_hip_frame_set_filters(self.h, lvl.ptr, b4_stride, e.ctypes.data, i.ctypes.data, cdef_damping,
                                                      C.addressof(grain) if grain is not None else None, is_id), "frame_set_filters")

    def end(self, coef, prep, mask=None, grain_out=None):
        """Returns the Picture descriptor of the filtered (post CDEF / restoration) picture."""
        filtered = Picture()
        _chk(self.ctx.lib.dav1d_hip_frame_end(self.h, coef.ptr if coef is not None else None, prep.ptr if prep is not None else None,
                                              mask.ptr if mask is not None else None, C.byref(filtered),
                                              C.byref(grain_out.pic) if grain_out is not None else None), "frame_end")
        self._cur_written(filtered)
        return filtered

    def end_async(self, coef, prep, mask=None, grain_out=None, done=None):
        """dav1d_hip_frame_end_async: returns at once; done(rc) is called on the library's thread when the frame is final."""
        cb_t = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p)
        self._cb = cb_t((lambda cookie, rc, pic: done(rc)) if done else (lambda cookie, rc, pic: None))
        _chk(self.ctx.lib.dav1d_hip_frame_end_async(self.h, coef.ptr if coef is not None else None, prep.ptr if prep is not None else None,
                                                    mask.ptr if mask is not None else None,
                                                    C.byref(grain_out.pic) if grain_out is not None else None, self._cb, None), "frame_end_async")

    def progress(self):
        return int(self.ctx.lib.dav1d_hip_frame_progress(self.h))

    def set_progress_callback(self, fn):
        """dav1d_hip_frame_set_progress_callback: fn(rows, picture) on the thread that ends the frame, every time more rows of the
        filtered picture are final (a Picture descriptor valid during the call)."""
        cb_t = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(Picture))
        self._pcb = cb_t(lambda cookie, rows, pic: fn(rows, pic.contents)) if fn else C.cast(None, cb_t)
        _chk(self.ctx.lib.dav1d_hip_frame_set_progress_callback(self.h, self._pcb, None), "frame_set_progress_callback")

    def wait(self):
        filtered = Picture()
        _chk(self.ctx.lib.dav1d_hip_frame_wait(self.h, C.byref(filtered)), "frame_wait")
        self._cur_written(filtered)
        return filtered

    def post_bands(self):
        """Bands the post filters of the last end() were pipelined over (0: stage by stage)."""
        return int(self.ctx.lib.dav1d_hip_frame_post_bands(self.h))

    def destroy(self):
        if self.h:
            self.ctx.lib.dav1d_hip_frame_destroy(self.h)
            self.h = C.c_void_p()
