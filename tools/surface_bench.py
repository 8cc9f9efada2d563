#!/usr/bin/env python3
"""Device time of dav1d_hip_surface_export on 8K 4:2:0 10-bit pictures that live in their tiled twin, against the existing kernel that
does the nearest job, dav1d_hip_picture_untile (twin in, raster planes out), timed by the same loop in the same run on the same pictures.

    python tools/surface_bench.py [--short] [--grain | --scaled | --rgb | --rgb-scaled | --batch | --colour | --reduced | --colour-reduced | --linear-reduced | --toned | --stats] [--pairs 4] [--calls 200] [--repeats 3]

N source pictures and N surfaces in rotation (a picture plus its surface is about 200 MB: four pairs do not fit the 256 MiB Infinity
Cache), 20 warm-up calls, then `calls` timed calls per variant between two HIP events on the context's stream, the variants alternated,
everything repeated `repeats` times to show the spread.  Bytes per call come from the shapes (bytes read + bytes written).  The host
fetch (dav1d_hip_host_picture_fetch + _wait) is printed for orientation only: it crosses PCIe and is no peer of a device-to-device pass.
--grain: the export with film grain fused in (dav1d_hip_surface_export_grain: planar native, P010, RGB native; from twin-only and from raster
sources; luma + both chroma planes, overlap on) against the sequence it replaces, timed the same way in the same run: dav1d_hip_fg_apply_prepared
into a pre-allocated picture, then dav1d_hip_surface_export from that, on sources with valid raster planes (its best case: no un-tile).
--scaled: dav1d_hip_surface_export_scaled at 2:1 (8K to 4K) and 4:1 (8K to 1080p) as planar native, P010 and RGB planar native, against the
yardstick a user pays today before any scaler of their own runs: dav1d_hip_surface_export of the same picture at full size in the same format,
timed the same way in the same run.
--rgb: dav1d_hip_surface_export_rgb (sited chroma, packed RGB / RGBA, binary16) against dav1d_hip_surface_export to RGB planes of the same sample
type in the same run (binary16: the float32 export); where a variant writes more bytes than its yardstick (RGBA: 4/3 of the writes) the
yardstick's times are scaled by the bytes moved.
--rgb-scaled: dav1d_hip_surface_export_rgb_scaled at 2:1, 4:1 and as a 224 x 224 centre crop at 8:1, each as packed RGBA float16 normalised at
chroma_pos 1 and as planar float16 at chroma_pos 0, against the route a user pays today, timed the same way in the same run on the same pictures:
dav1d_hip_surface_export_scaled to planar native into a pre-allocated picture of the output size, then dav1d_hip_surface_export_rgb from it.
--batch: dav1d_hip_surface_export_rgb_scaled_batch against the N single dav1d_hip_surface_export_rgb_scaled calls it replaces, issued back to back with
one pair of events around the N calls, in the same run on the same pictures and destinations; both sides call the library with argument arrays made
once.  (a) N = 8 and N = 32 distinct pictures, the 1792 x 1792 centre crop to 224 x 224; (b) N = 32 crops of ONE picture, tiled over the frame, to 224 x 224;
(c) N = 8 pictures at 4:1; (d) one 4:1 item and 31 of the 224 x 224 items.  (a) to (c) as packed RGBA float16 normalised at chroma_pos 1 and as planar
float16 at chroma_pos 0.  The 32 pictures share one host image (their device memory is their own): the time does not depend on the pixels.
--colour: dav1d_hip_surface_export_rgb_colour with the tables of PQ / BT.2020 -> sRGB / BT.709 (dav1d_hip_colour_tables, 203 / 1000 nits) — (a) lin only,
planar float16; (b) lin + matrix, planar float16; (c) lin + matrix + enc, packed RGBA float16 normalised, chroma_pos 1 — each against
dav1d_hip_surface_export_rgb to the same format and sample with the same parameters, in the same run on the same pictures: the new call moves the
yardstick's bytes and adds three to six table reads a pixel.  --cells 1,2,4: (a) and (c) again with the context option colour_cells set (the cells a wave takes).
--reduced: dav1d_hip_surface_export_rgb_reduced, the whole 8K picture to 224 x 224 RGB planar float16 at chroma_pos 1 (34:1 and 19:1), from twin-only
and from raster sources, against the chain a user can run without it: dav1d_hip_surface_export_scaled at 8:1 to planar native into a pre-allocated
picture, then dav1d_hip_surface_export_rgb_resized from that to 224 x 224.  The variants alternate within a round, at least ten rounds; per variant the
device time between two events around the timed calls, the host clock around issuing them and the final sync, and dav1d_hip_last_kernel_ms of the
last call.  Then dav1d_hip_surface_export_rgb_reduced_batch: 64 crops of 7168 x 4032 of the pictures in rotation to (64, 3, 224, 224).
--colour-reduced: dav1d_hip_surface_export_rgb_colour_reduced with the tables of PQ / BT.2020 -> sRGB / BT.709 from twin-only sources, by the method of
--reduced (variants alternated within a round, at least ten rounds).  1. the whole 8K picture to 224 x 224 planar float16 at chroma_pos 1 against
dav1d_hip_surface_export_rgb_reduced to the same format; 2. dav1d_hip_surface_export_rgb_colour_reduced_batch, 64 crops of 7168 x 4032 to
(64, 3, 224, 224), against dav1d_hip_surface_export_rgb_reduced_batch; 3. 8K to 3840 x 2160 RGBA float16 against the only other route to those bytes,
dav1d_hip_surface_export_scaled into a pre-allocated picture + dav1d_hip_surface_export_rgb_colour from it, with dav1d_hip_surface_export_rgb_scaled
(no colour stage) next to it for what the trip of Q through memory costs.
--linear-reduced: dav1d_hip_surface_export_rgb_linear_reduced (scaling in linear light) with the same tables, by the same method.  1. the whole 8K picture
to 224 x 224 planar float16 against dav1d_hip_surface_export_rgb_colour of the whole picture with a lin-only handle into a planar float16 surface (the
first half of the only other route to the same pixels); 2. its batch, 64 crops of 7168 x 4032 to (64, 3, 224, 224), against the same 64 items as single
calls; without a bar, both next to dav1d_hip_surface_export_rgb_colour_reduced and its batch, and 8K to 3840 x 2160 RGBA float16.
--toned: the tone part of a handle (dav1d_hip_colour_create_toned), by the same method: dav1d_hip_surface_export_rgb_colour at full size,
dav1d_hip_surface_export_rgb_colour_reduced and dav1d_hip_surface_export_rgb_linear_reduced 8K to 224 x 224 and the linear batch of 64, each with the un-toned
handle of dav1d_hip_colour_tables and with the toned one of dav1d_hip_colour_tables_toned, alternated; the ratio toned / un-toned per call, without a bar.
--stats: dav1d_hip_picture_light_stats of the whole picture on uniform noise, a flat picture and a smooth gradient with a letterbox, against
dav1d_hip_surface_export_rgb_colour at full size with a lin-only handle into planar float16 in the same run; then the host time of dav1d_hip_colour_update_tone.
Needs the GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dav1d_amd import api  # noqa: E402

SPEC_TBS, COPY_TBS = 8.0, 6.3         # HBM3E peak (spec) and the copy ceiling measured on the MI355X


class Events:
    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def start(self):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0

    def stop_ms(self):
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value


def grain_data():
    """luma + both chroma planes, overlap on; fixed so that runs compare"""
    from dav1d_amd._lib import FilmGrainData
    d = FilmGrainData()
    d.seed = 1234
    d.num_y_points = 2
    d.y_points[0][0], d.y_points[0][1], d.y_points[1][0], d.y_points[1][1] = 0, 40, 255, 120
    for pl in range(2):
        d.num_uv_points[pl] = 2
        d.uv_points[pl][0][0], d.uv_points[pl][0][1], d.uv_points[pl][1][0], d.uv_points[pl][1][1] = 0, 30, 255, 90
        d.uv_mult[pl], d.uv_luma_mult[pl], d.uv_offset[pl] = 64, 32, 0
        for i in range(25):
            d.ar_coeffs_uv[pl][i] = (i % 5) - 2
    for i in range(24):
        d.ar_coeffs_y[i] = (i % 7) - 3
    d.scaling_shift, d.ar_coeff_lag, d.ar_coeff_shift, d.grain_scale_shift = 9, 3, 7, 0
    d.overlap_flag, d.clip_to_restricted_range = 1, 1
    return d


def grain_runs(a, ctx, ev, pics, variants, src_bytes):
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    handle = ctx.fg_prepare(grain_data(), bpc, layout)
    tmps = [ctx.picture(w, h, layout, bpc) for _ in range(a.pairs)]
    ctx.sync()
    runs, all_surfs = [], []
    for name, fmt, sample, out_bytes in variants:
        surfs = [ctx.surface(w, h, layout, bpc, fmt, sample) for _ in range(a.pairs)]
        all_surfs += surfs

        def two_calls(k, surfs=surfs):
            p, t = pics[k % a.pairs], tmps[k % a.pairs]
            p.pic.twin_ok = 1                  # raster planes and twin agree: nothing to un-tile
            ctx.fg_apply_prepared(t, p, handle)
            t.export(surfs[k % a.pairs])

        def fused(k, surfs=surfs, state=api.TWIN_ONLY):
            p = pics[k % a.pairs]
            p.pic.twin_ok = state
            p.export(surfs[k % a.pairs], grain=handle)
        # the two calls read the source (and the luma again under the chroma), write the picture, read it, write the surface
        runs.append(("fg_apply_prepared + export: " + name, 3 * src_bytes + 2 * w * h + out_bytes, two_calls, None))
        yard = runs[-1][0]
        luma_again = 0 if fmt == api.SURFACE_RGB_PLANAR else 2 * w * ((h + 1) // 2)      # the one extra read: the luma rows under the chroma rows
        runs.append(("fused, twin-only source: " + name, src_bytes + luma_again + out_bytes, fused, yard))
        runs.append(("fused, raster source: " + name, src_bytes + luma_again + out_bytes, lambda k, f=fused: f(k, state=0), yard))
    print("# surface_bench --grain on %s: %dx%d 4:2:0 %d-bit, %d picture / surface pairs in rotation, 20 warm-up + %d timed calls per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, a.pairs, a.calls, a.repeats))
    print("# bytes per call = bytes read + bytes written, from the shapes (templates, tables and offsets not counted)")
    results = {r[0]: [] for r in runs}
    for rep in range(a.repeats):
        for name, nbytes, call, _ in runs:
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            print("repeat %d  %-62s %8.4f ms/call  %7.1f MB/call  %7.0f GB/s" % (rep, name, ms, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (min / median / max ms per call over the repeats)")
    for name, nbytes, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-62s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(results[name]), sorted(results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-62s median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms: %s"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met"))
    ctx.fg_grain_destroy(handle)
    for s in all_surfs:
        s.free()
    for p in tmps + pics:
        p.free()
    ctx.close()


def scaled_runs(a, ctx, ev, pics, variants, src_bytes):
    """2:1 and 4:1 of every format against the plain export of the same picture at full size in the same format (the yardstick)"""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    runs, all_surfs = [], []
    for name, fmt, sample, out_bytes in variants:
        full = [ctx.surface(w, h, layout, bpc, fmt, sample) for _ in range(a.pairs)]
        all_surfs += full

        def plain(k, surfs=full):
            pics[k % a.pairs].export(surfs[k % a.pairs])
        runs.append(("export, full size: " + name, src_bytes + out_bytes, plain, None))
        yard = runs[-1][0]
        for ratio in (2, 4):
            small = [ctx.surface(w // ratio, h // ratio, layout, bpc, fmt, sample) for _ in range(a.pairs)]
            all_surfs += small

            def scaled(k, surfs=small):
                pics[k % a.pairs].export_scaled(surfs[k % a.pairs])
            runs.append(("scaled %d:1 (%dx%d): %s" % (ratio, w // ratio, h // ratio, name), src_bytes + out_bytes // (ratio * ratio), scaled, yard))
    print("# surface_bench --scaled on %s: %dx%d 4:2:0 %d-bit twin-only sources, %d picture / surface pairs in rotation, 20 warm-up + %d timed calls per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, a.pairs, a.calls, a.repeats))
    print("# bytes per call = bytes read + bytes written, from the shapes")
    results = {r[0]: [] for r in runs}
    for rep in range(a.repeats):
        for name, nbytes, call, _ in runs:
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            print("repeat %d  %-62s %8.4f ms/call  %7.1f MB/call  %7.0f GB/s" % (rep, name, ms, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (min / median / max ms per call over the repeats)")
    for name, nbytes, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-62s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(results[name]), sorted(results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-62s median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms: %s"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met"))
    for s in all_surfs:
        s.free()
    for p in pics:
        p.free()
    ctx.close()


def rgb_runs(a, ctx, ev, pics, src_bytes):
    """the RGB export's variants against the plain export to RGB planes of the same sample type (binary16: of float32)"""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    R, K3, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGB_PACKED, api.SURFACE_RGBA_PACKED
    N, F32, F16 = api.SAMPLE_NATIVE, api.SAMPLE_F32, api.SAMPLE_F16
    runs, all_surfs = [], []

    def add(name, fmt, sample, es, pos, yard, plain=False):
        n = 4 if fmt == K4 else 3
        surfs = [ctx.surface(w, h, layout, bpc, fmt, sample) for _ in range(a.pairs)]
        all_surfs.extend(surfs)
        if plain:
            def call(k):
                pics[k % a.pairs].export(surfs[k % a.pairs])
        else:
            def call(k):
                pics[k % a.pairs].export_rgb(surfs[k % a.pairs], pos)
        runs.append((name, src_bytes + n * es * w * h, call, yard))
        return name
    y_n = add("export: RGB planar native (yardstick)", R, N, 2, 0, None, plain=True)
    add("export_rgb: planar native, chroma_pos 0", R, N, 2, 0, y_n)
    add("export_rgb: planar native, chroma_pos 1", R, N, 2, 1, y_n)
    add("export_rgb: planar native, chroma_pos 2", R, N, 2, 2, y_n)
    add("export_rgb: packed RGB native, chroma_pos 1", K3, N, 2, 1, y_n)
    add("export_rgb: packed RGBA native, chroma_pos 1", K4, N, 2, 1, y_n)
    y_f = add("export: RGB planar float32 (yardstick)", R, F32, 4, 0, None, plain=True)
    add("export_rgb: planar float32, chroma_pos 1", R, F32, 4, 1, y_f)
    add("export_rgb: planar float16, chroma_pos 1", R, F16, 2, 1, y_f)
    add("export_rgb: packed RGB float16, chroma_pos 1", K3, F16, 2, 1, y_f)
    add("export_rgb: packed RGBA float16, chroma_pos 1", K4, F16, 2, 1, y_f)
    print("# surface_bench --rgb on %s: %dx%d 4:2:0 %d-bit twin-only sources, %d picture / surface pairs in rotation, 20 warm-up + %d timed calls per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, a.pairs, a.calls, a.repeats))
    print("# bytes per call = bytes read + bytes written, from the shapes")
    results = {r[0]: [] for r in runs}
    nbytes_of = {r[0]: r[1] for r in runs}
    for rep in range(a.repeats):
        for name, nbytes, call, _ in runs:
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            print("repeat %d  %-62s %8.4f ms/call  %7.1f MB/call  %7.0f GB/s" % (rep, name, ms, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (min / median / max ms per call over the repeats)")
    for name, nbytes, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-62s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    for name, nbytes, _, yard in runs:
        if yard is None:
            continue
        f = max(1.0, nbytes / nbytes_of[yard])          # more bytes than the yardstick moves: its time scaled by the bytes; fewer: its time as it is
        v, u = sorted(results[name]), sorted(results[yard])
        ok = v[len(v) // 2] <= f * (u[len(u) // 2] + (u[-1] - u[0]))
        print("condition %-62s median %.4f ms <= %.3f x (yardstick median %.4f ms + its spread %.4f ms): %s"
              % (name, v[len(v) // 2], f, u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met"))
    for s in all_surfs:
        s.free()
    for p in pics:
        p.free()
    ctx.close()


def rgb_scaled_runs(a, ctx, ev, pics, src_bytes):
    """the one call against export_scaled into a picture-shaped buffer + export_rgb from it, per ratio and output variant"""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    mx = (1 << bpc) - 1
    scale, bias = [1.0 / (mx * s) for s in (0.229, 0.224, 0.225)], [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    side = min(w, h, 8 * 224)
    geoms = [("2:1", None, (w // 2, h // 2)), ("4:1", None, (w // 4, h // 4)),
             ("%d:1 centre crop" % (side // 224), (((w - side) // 2) & ~1, ((h - side) // 2) & ~1, side, side), (224, 224))]
    outs = [("packed RGBA float16 normalised, chroma_pos 1", api.SURFACE_RGBA_PACKED, 4, 1, scale, bias),
            ("planar float16, chroma_pos 0", api.SURFACE_RGB_PLANAR, 3, 0, None, None)]
    runs, frees = [], []
    for gname, crop, (dw, dh) in geoms:
        cw, ch = (dw + 1) // 2, (dh + 1) // 2
        sw, sh = (crop[2], crop[3]) if crop else (w, h)
        read = 2 * (sw * sh + 2 * ((sw + 1) // 2) * ((sh + 1) // 2))
        mid = 2 * (dw * dh + 2 * cw * ch)
        tmps = [ctx.picture(dw, dh, layout, bpc) for _ in range(a.pairs)]
        views = [api.Surface.wrap(ctx, [t.pic.p[pl].data for pl in range(3)], [t.pic.p[pl].stride for pl in range(3)], dw, dh, layout, bpc,
                                  api.SURFACE_PLANAR, api.SAMPLE_NATIVE) for t in tmps]
        frees += tmps
        for oname, fmt, n, pos, sc, bi in outs:
            surfs = [ctx.surface(dw, dh, layout, bpc, fmt, api.SAMPLE_F16) for _ in range(a.pairs)]
            frees += surfs
            out_bytes = n * 2 * dw * dh

            def two_calls(k, surfs=surfs, tmps=tmps, views=views, crop=crop, pos=pos, sc=sc, bi=bi):
                pics[k % a.pairs].export_scaled(views[k % a.pairs], crop)
                tmps[k % a.pairs].export_rgb(surfs[k % a.pairs], pos, sc, bi)

            def fused(k, surfs=surfs, crop=crop, pos=pos, sc=sc, bi=bi):
                pics[k % a.pairs].export_rgb_scaled(surfs[k % a.pairs], crop, pos, sc, bi)
            yard = "export_scaled + export_rgb %s (%dx%d): %s" % (gname, dw, dh, oname)
            runs.append((yard, read + 2 * mid + out_bytes, two_calls, None))
            runs.append(("export_rgb_scaled %s (%dx%d): %s" % (gname, dw, dh, oname), read + out_bytes, fused, yard))
    print("# surface_bench --rgb-scaled on %s: %dx%d 4:2:0 %d-bit twin-only sources, %d picture / surface pairs in rotation, 20 warm-up + %d timed calls per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, a.pairs, a.calls, a.repeats))
    print("# bytes per call = bytes read + bytes written, from the shapes (the yardstick writes and reads the scaled planes once more)")
    results = {r[0]: [] for r in runs}
    for rep in range(a.repeats):
        for name, nbytes, call, _ in runs:
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            print("repeat %d  %-96s %8.4f ms/call  %7.1f MB/call  %7.0f GB/s" % (rep, name, ms, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (min / median / max ms per call over the repeats)")
    for name, nbytes, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-96s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(results[name]), sorted(results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-96s median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms: %s"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met"))
    for s in frees:
        s.free()
    for p in pics:
        p.free()
    ctx.close()


def reduced_runs(a, ctx, ev, pics, src_bytes):
    """the one call against export_scaled 8:1 into a picture + export_rgb_resized from it; then a batch of 64"""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    dw = dh = 224
    mw, mh = w // 8, h // 8
    rounds, calls = max(a.repeats, 10), min(a.calls, 40)
    tmps = [ctx.picture(mw, mh, layout, bpc) for _ in range(a.pairs)]
    views = [api.Surface.wrap(ctx, [t.pic.p[pl].data for pl in range(3)], [t.pic.p[pl].stride for pl in range(3)], mw, mh, layout, bpc,
                              api.SURFACE_PLANAR, api.SAMPLE_NATIVE) for t in tmps]
    surfs = [ctx.surface(dw, dh, layout, bpc, api.SURFACE_RGB_PLANAR, api.SAMPLE_F16) for _ in range(a.pairs)]
    out_bytes, mid = 3 * 2 * dw * dh, 2 * (mw * mh + 2 * ((mw + 1) // 2) * ((mh + 1) // 2))
    q_bytes = 2 * (dw * dh + 2 * (dw // 2) * (dh // 2))

    def chain(k, state):
        p = pics[k % a.pairs]
        p.pic.twin_ok = state
        p.export_scaled(views[k % a.pairs], None)
        tmps[k % a.pairs].export_rgb_resized(surfs[k % a.pairs], None, 1)

    def reduced(k, state):
        p = pics[k % a.pairs]
        p.pic.twin_ok = state
        p.export_rgb_reduced(surfs[k % a.pairs], None, 1)
    runs = []
    for sname, state in (("twin-only", api.TWIN_ONLY), ("raster", 0)):
        yard = "export_scaled 8:1 + export_rgb_resized to 224x224, %s source" % sname
        runs.append((yard, src_bytes + 2 * mid + out_bytes, lambda k, state=state: chain(k, state), None))
        runs.append(("export_rgb_reduced to 224x224, %s source" % sname, src_bytes + 2 * q_bytes + out_bytes, lambda k, state=state: reduced(k, state), yard))
    n = 64
    bsurfs = [ctx.surface(dw, dh, layout, bpc, api.SURFACE_RGB_PLANAR, api.SAMPLE_F16) for _ in range(n)]
    cw_, ch_ = min(w, 7168) & ~1, min(h, 4032) & ~1
    crops = [(((w - cw_) * (k % 8) // 7) & ~1, ((h - ch_) * (k // 8) // 7) & ~1, cw_, ch_) for k in range(n)]
    bytes_batch = n * (2 * (cw_ * ch_ + 2 * (cw_ // 2) * (ch_ // 2)) + 2 * q_bytes + out_bytes)
    for sname, state in (("twin-only", api.TWIN_ONLY), ("raster", 0)):
        def batch(k, state=state):
            for p in pics[:a.pairs]:
                p.pic.twin_ok = state
            ctx.export_rgb_reduced_batch(bsurfs, [pics[(k + i) % a.pairs] for i in range(n)], crops, 1)
        runs.append(("export_rgb_reduced_batch, 64 crops of %dx%d to (64, 3, 224, 224), %s sources" % (cw_, ch_, sname), bytes_batch, batch, None))
    print("# surface_bench --reduced on %s: %dx%d 4:2:0 %d-bit sources, %d pictures / surfaces in rotation, 3 warm-up + %d timed calls per variant and round (batch: 4), %d rounds, "
          "the variants alternated within a round" % (socket.gethostname(), w, h, bpc, a.pairs, calls, rounds))
    print("# bytes per call = bytes read + bytes written, from the shapes (the chain writes and reads the 8:1 planes, the new call Q); device ms between two events around the "
          "timed calls; host ms: the clock around issuing them and the sync; last ms: dav1d_hip_last_kernel_ms of the last call")
    results = {r[0]: [] for r in runs}
    for rnd in range(rounds):
        for name, nbytes, call, _ in runs:
            nc = 4 if "batch" in name else calls
            for k in range(3):
                call(k)
            ctx.sync()
            t0 = time.perf_counter()
            ev.start()
            for k in range(nc):
                call(k)
            ms = ev.stop_ms() / nc
            host = (time.perf_counter() - t0) * 1e3 / nc
            last = ctx.last_kernel_ms()
            results[name].append((ms, host, last))
            print("round %2d  %-96s device %8.4f ms/call  host %8.4f  last %8.4f  %7.1f MB/call  %7.0f GB/s  %5.1f %% of copy ceiling"
                  % (rnd, name, ms, host, last, nbytes / 1e6, nbytes / ms / 1e6, nbytes / ms / 1e6 / (COPY_TBS * 10)))
    print("# summary (median [min .. max] over the rounds)")
    for name, nbytes, _, _ in runs:
        cols = [sorted(v[i] for v in results[name]) for i in range(3)]
        med = [c[len(c) // 2] for c in cols]
        print("summary   %-96s device %8.4f [%8.4f .. %8.4f]  host %8.4f [%8.4f .. %8.4f]  last %8.4f [%8.4f .. %8.4f] ms   median %7.0f GB/s, %5.1f %% of the %.1f TB/s copy ceiling"
              % (name, med[0], cols[0][0], cols[0][-1], med[1], cols[1][0], cols[1][-1], med[2], cols[2][0], cols[2][-1], nbytes / med[0] / 1e6,
                 nbytes / med[0] / 1e6 / (COPY_TBS * 10), COPY_TBS))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        for i, clock in ((0, "device"), (1, "host")):
            v, u = sorted(x[i] for x in results[name]), sorted(x[i] for x in results[yard])
            ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
            print("condition %-64s %-6s median %.4f ms <= chain median %.4f ms + its spread %.4f ms: %s"
                  % (name, clock, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met"))
    for s in tmps + surfs + bsurfs + pics:
        s.free()
    ctx.close()


def colour_runs(a, ctx, ev, pics, src_bytes):
    """the colour-managed export against export_rgb to the same format and sample"""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    mx = (1 << bpc) - 1
    scale, bias = [1.0 / s for s in (0.229, 0.224, 0.225)], [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    yscale = [v / mx for v in scale]          # the yardstick's samples are v / max
    lin, m, enc, has_matrix, has_enc = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
    assert has_matrix and has_enc
    handles = {"lin": ctx.colour(lin, bpc=bpc), "lin + matrix": ctx.colour(lin, m, bpc=bpc), "lin + matrix + enc": ctx.colour(lin, m, enc, bpc=bpc)}
    P, K4 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGBA_PACKED
    planar = [ctx.surface(w, h, layout, bpc, P, api.SAMPLE_F16, matrix=9) for _ in range(a.pairs)]
    packed = [ctx.surface(w, h, layout, bpc, K4, api.SAMPLE_F16, matrix=9) for _ in range(a.pairs)]
    runs = []

    def add(name, surfs, n, pos, sc, bi, handle, yard, cells=0, ysc=None):
        if handle is None:
            def call(k):
                pics[k % a.pairs].export_rgb(surfs[k % a.pairs], pos, ysc, bi)
        else:
            def call(k):
                pics[k % a.pairs].export_rgb_colour(surfs[k % a.pairs], handle, pos, sc, bi)
        runs.append((name, src_bytes + n * 2 * w * h, call, yard, cells))
        return name
    y_p = add("export_rgb: planar float16, chroma_pos 1 (yardstick)", planar, 3, 1, None, None, None, None)
    add("(a) export_rgb_colour lin: planar float16, chroma_pos 1", planar, 3, 1, None, None, handles["lin"], y_p)
    add("(b) export_rgb_colour lin + matrix: planar float16, chroma_pos 1", planar, 3, 1, None, None, handles["lin + matrix"], y_p)
    y_k = add("export_rgb: packed RGBA float16 normalised, chroma_pos 1 (yardstick)", packed, 4, 1, None, bias, None, None, ysc=yscale)
    add("(c) export_rgb_colour lin + matrix + enc: packed RGBA float16 normalised, chroma_pos 1", packed, 4, 1, scale, bias, handles["lin + matrix + enc"], y_k)
    for cells in a.cells:
        add("(a) with colour_cells %d" % cells, planar, 3, 1, None, None, handles["lin"], y_p, cells)
        add("(c) with colour_cells %d" % cells, packed, 4, 1, scale, bias, handles["lin + matrix + enc"], y_k, cells)
    print("# surface_bench --colour on %s: %dx%d 4:2:0 %d-bit twin-only sources, %d picture / surface pairs in rotation, 20 warm-up + %d timed calls per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, a.pairs, a.calls, a.repeats))
    print("# tables: PQ / BT.2020 -> sRGB / BT.709, white 203 nits, peak 1000 nits; bytes per call = bytes read + bytes written, from the shapes (tables not counted)")
    results = {r[0]: [] for r in runs}
    for rep in range(a.repeats):
        for name, nbytes, call, _, cells in runs:
            ctx.set_option("colour_cells", cells)
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            print("repeat %d  %-90s %8.4f ms/call  %7.1f MB/call  %7.0f GB/s" % (rep, name, ms, nbytes / 1e6, nbytes / ms / 1e6))
    ctx.set_option("colour_cells", 0)
    print("# summary (min / median / max ms per call over the repeats)")
    for name, nbytes, _, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-90s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    for name, _, _, yard, _ in runs:
        if yard is None:
            continue
        v, u = sorted(results[name]), sorted(results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-90s median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms (min %.4f - max %.4f): %s (ratio %.3f)"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], u[0], u[-1], "met" if ok else "NOT met", v[len(v) // 2] / u[len(u) // 2]))
    ctx.sync()
    for hd in handles.values():
        ctx.colour_destroy(hd)
    for s in planar + packed:
        s.free()
    for p in pics:
        p.free()
    ctx.close()


def batch_runs(a, ctx, ev, pics):
    """one batch call against the N single calls it replaces, per variant and output"""
    from dav1d_amd._lib import Picture, RgbParams, Surface as SurfaceDesc
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    lib = ctx.lib
    mx = (1 << bpc) - 1
    scale, bias = [1.0 / (mx * s) for s in (0.229, 0.224, 0.225)], [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
    side = min(w, h, 8 * 224)
    centre = (((w - side) // 2) & ~1, ((h - side) // 2) & ~1, side, side)
    nx = 8
    ny = 32 // nx
    tiles = [(((w // nx) & ~1) * (k % nx), ((h // ny) & ~1) * (k // nx), (w // nx) & ~1, (h // ny) & ~1) for k in range(32)]
    whole, quarter, thumb = (0, 0, w, h), (w // 4, h // 4), (224, 224)
    n_pics = len(pics)
    variants = [("(a) %d pictures, centre crop to 224x224" % n, [(pics[k % n_pics], centre, thumb) for k in range(n)]) for n in (8, 32)]
    variants.append(("(b) 32 crops of one picture to 224x224", [(pics[0], tiles[k], thumb) for k in range(32)]))
    variants.append(("(c) 8 pictures at 4:1 (%dx%d)" % quarter, [(pics[k % n_pics], whole, quarter) for k in range(8)]))
    mixed = ("(d) one 4:1 item and 31 of 224x224", [(pics[0], whole, quarter)] + [(pics[k % n_pics], centre, thumb) for k in range(1, 32)])
    outs = [("packed RGBA float16 normalised, chroma_pos 1", api.SURFACE_RGBA_PACKED, 4, 1, scale, bias),
            ("planar float16, chroma_pos 0", api.SURFACE_RGB_PLANAR, 3, 0, None, None)]
    runs, frees = [], []
    for vname, items in variants + [mixed]:
        for oname, fmt, nch, pos, sc, bi in outs[:1] if items is mixed[1] else outs:
            n = len(items)
            sizes = [nch * 2 * dw * dh for _, _, (dw, dh) in items]
            buf = ctx.buffer(sum(sizes))
            frees.append(buf)
            dst, at = (SurfaceDesc * n)(), 0
            for k, (_, _, (dw, dh)) in enumerate(items):          # item k behind item k - 1 in one buffer: (N, h, w, 4) or (N, 3, h, w) where the sizes agree
                planes = [buf.ptr + at] if fmt == api.SURFACE_RGBA_PACKED else [buf.ptr + at + c * 2 * dw * dh for c in range(3)]
                dst[k] = api.Surface.wrap(ctx, planes, [nch * 2 * dw] if fmt == api.SURFACE_RGBA_PACKED else [2 * dw] * 3, dw, dh, layout, bpc, fmt, api.SAMPLE_F16).desc
                at += sizes[k]
            src = (C.POINTER(Picture) * n)(*[C.pointer(p.pic) for p, _, _ in items])
            rects = (api.SurfaceRect * n)(*[api.SurfaceRect(*crop) for _, crop, _ in items])
            params = api.DevicePicture._rgb_params(pos, sc, bi)
            single_args = [(ctx.h, C.byref(dst[k]), src[k], C.byref(rects[k]), C.byref(params), 0, dst[k].h) for k in range(n)]

            def singles(_, args=single_args, f=lib.dav1d_hip_surface_export_rgb_scaled):
                for t in args:
                    assert f(*t) == 0

            def batch(_, n=n, dst=dst, src=src, rects=rects, params=params, f=lib.dav1d_hip_surface_export_rgb_scaled_batch):
                assert f(ctx.h, n, dst, src, rects, C.byref(params), None) == 0
            read = sum(2 * (cr[2] * cr[3] + 2 * ((cr[2] + 1) // 2) * ((cr[3] + 1) // 2)) for _, cr, _ in items)
            yard = "%d single calls %s: %s" % (n, vname, oname)
            runs.append((yard, read + sum(sizes), singles, None))
            runs.append(("one batch call %s: %s" % (vname, oname), read + sum(sizes), batch, yard))
    print("# surface_bench --batch on %s: %dx%d 4:2:0 %d-bit twin-only sources, %d pictures, 20 warm-up + %d timed repetitions per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, n_pics, a.calls, a.repeats))
    print("# a repetition is ONE batch call or the N single calls it replaces, between one pair of events; bytes = bytes read + bytes written, from the shapes")
    results = {r[0]: [] for r in runs}
    for rep in range(a.repeats):
        for name, nbytes, call, _ in runs:
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            print("repeat %d  %-110s %8.4f ms/batch  %7.1f MB  %7.0f GB/s" % (rep, name, ms, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (min / median / max ms per batch over the repeats)")
    for name, nbytes, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-110s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(results[name]), sorted(results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-110s median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms: %s (x %.2f)"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met", u[len(u) // 2] / v[len(v) // 2]))
    for s in frees:
        s.free()
    for p in pics:
        p.free()
    ctx.close()


def colour_reduced_runs(a, ctx, ev, pics, src_bytes):
    """dav1d_hip_surface_export_rgb_colour_reduced and its batch against export_rgb_reduced (no colour stage) to the same format, and at 2:1 against the
    only other route to those bytes: export_scaled into a picture + export_rgb_colour from it"""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    dw = dh = 224
    hw, hh = w // 2, h // 2
    rounds, calls = 1 if a.short else max(a.repeats, 10), min(a.calls, 40)
    lin, m, enc, has_matrix, has_enc = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
    assert has_matrix and has_enc
    colour = ctx.colour(lin, m, enc, bpc=bpc)
    P, K4, F16 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGBA_PACKED, api.SAMPLE_F16
    surfs = [ctx.surface(dw, dh, layout, bpc, P, F16, matrix=9) for _ in range(a.pairs)]
    out_bytes, q_bytes = 3 * 2 * dw * dh, 2 * (dw * dh + 2 * (dw // 2) * (dh // 2))
    for p in pics:
        p.pic.twin_ok = api.TWIN_ONLY
    runs = []
    yard = "export_rgb_reduced to 224x224 planar float16 (yardstick)"
    runs.append((yard, src_bytes + 2 * q_bytes + out_bytes, lambda k: pics[k % a.pairs].export_rgb_reduced(surfs[k % a.pairs], None, 1), None))
    runs.append(("1. export_rgb_colour_reduced to 224x224 planar float16", src_bytes + 2 * q_bytes + out_bytes,
                 lambda k: pics[k % a.pairs].export_rgb_colour_reduced(surfs[k % a.pairs], colour, None, 1), yard))
    n = 64
    bsurfs = [ctx.surface(dw, dh, layout, bpc, P, F16, matrix=9) for _ in range(n)]
    cw_, ch_ = min(w, 7168) & ~1, min(h, 4032) & ~1
    crops = [(((w - cw_) * (k % 8) // 7) & ~1, ((h - ch_) * (k // 8) // 7) & ~1, cw_, ch_) for k in range(n)]
    bytes_batch = n * (2 * (cw_ * ch_ + 2 * (cw_ // 2) * (ch_ // 2)) + 2 * q_bytes + out_bytes)
    yard = "export_rgb_reduced_batch, 64 crops of %dx%d to (64, 3, 224, 224) (yardstick)" % (cw_, ch_)
    runs.append((yard, bytes_batch, lambda k: ctx.export_rgb_reduced_batch(bsurfs, [pics[(k + i) % a.pairs] for i in range(n)], crops, 1), None))
    runs.append(("2. export_rgb_colour_reduced_batch, 64 crops of %dx%d to (64, 3, 224, 224)" % (cw_, ch_), bytes_batch,
                 lambda k: ctx.export_rgb_colour_reduced_batch(bsurfs, [pics[(k + i) % a.pairs] for i in range(n)], colour, crops, 1), yard))
    tmps = [ctx.picture(hw, hh, layout, bpc) for _ in range(a.pairs)]
    views = [api.Surface.wrap(ctx, [t.pic.p[pl].data for pl in range(3)], [t.pic.p[pl].stride for pl in range(3)], hw, hh, layout, bpc,
                              api.SURFACE_PLANAR, api.SAMPLE_NATIVE) for t in tmps]
    halves = [ctx.surface(hw, hh, layout, bpc, K4, F16, matrix=9) for _ in range(a.pairs)]
    mid, out4 = 2 * (hw * hh + 2 * ((hw + 1) // 2) * ((hh + 1) // 2)), 4 * 2 * hw * hh

    def chain(k):
        pics[k % a.pairs].export_scaled(views[k % a.pairs], None)
        tmps[k % a.pairs].export_rgb_colour(halves[k % a.pairs], colour, 1)
    yard = "export_scaled 2:1 + export_rgb_colour to %dx%d RGBA float16 (yardstick)" % (hw, hh)
    runs.append((yard, src_bytes + 2 * mid + out4, chain, None))
    runs.append(("3. export_rgb_colour_reduced to %dx%d RGBA float16" % (hw, hh), src_bytes + 2 * mid + out4,
                 lambda k: pics[k % a.pairs].export_rgb_colour_reduced(halves[k % a.pairs], colour, None, 1), yard))
    runs.append(("   export_rgb_scaled to %dx%d RGBA float16 (no colour stage, no bar: Q never reaches memory)" % (hw, hh), src_bytes + out4,
                 lambda k: pics[k % a.pairs].export_rgb_scaled(halves[k % a.pairs], None, 1), None))
    print("# surface_bench --colour-reduced on %s: %dx%d 4:2:0 %d-bit twin-only sources, PQ / BT.2020 to sRGB / BT.709 (lin + matrix + enc), %d pictures / surfaces in rotation, "
          "3 warm-up + %d timed calls per variant and round (batch: 4), %d rounds, the variants alternated within a round" % (socket.gethostname(), w, h, bpc, a.pairs, calls, rounds))
    print("# bytes per call = bytes read + bytes written, from the shapes (Q and the chain's planes written and read once); device ms between two events around the timed calls; "
          "host ms: the clock around issuing them and the sync; last ms: dav1d_hip_last_kernel_ms of the last call")
    results = {r[0]: [] for r in runs}
    for rnd in range(rounds):
        for name, nbytes, call, _ in runs:
            nc = 4 if "batch" in name else calls
            for k in range(3):
                call(k)
            ctx.sync()
            t0 = time.perf_counter()
            ev.start()
            for k in range(nc):
                call(k)
            ms = ev.stop_ms() / nc
            host = (time.perf_counter() - t0) * 1e3 / nc
            last = ctx.last_kernel_ms()
            results[name].append((ms, host, last))
            print("round %2d  %-100s device %8.4f ms/call  host %8.4f  last %8.4f  %7.1f MB/call  %7.0f GB/s" % (rnd, name, ms, host, last, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (median [min .. max] over the rounds)")
    for name, nbytes, _, _ in runs:
        cols = [sorted(v[i] for v in results[name]) for i in range(3)]
        med = [c[len(c) // 2] for c in cols]
        print("summary   %-100s device %8.4f [%8.4f .. %8.4f]  host %8.4f [%8.4f .. %8.4f]  last %8.4f [%8.4f .. %8.4f] ms   median %7.0f GB/s"
              % (name, med[0], cols[0][0], cols[0][-1], med[1], cols[1][0], cols[1][-1], med[2], cols[2][0], cols[2][-1], nbytes / med[0] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(x[0] for x in results[name]), sorted(x[0] for x in results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-84s device median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms: %s (x %.2f)"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met", u[len(u) // 2] / v[len(v) // 2]))
    ctx.sync()
    ctx.colour_destroy(colour)
    for s in tmps + surfs + bsurfs + halves + pics:
        s.free()
    ctx.close()


def linear_reduced_runs(a, ctx, ev, pics, src_bytes):
    """dav1d_hip_surface_export_rgb_linear_reduced and its batch.  1.: against the first half of the only other route to the same
    pixels, dav1d_hip_surface_export_rgb_colour of the whole picture with a lin-only handle into a planar float16 surface (the caller's area mean, matrix
    and re-encode are not counted).  2.: the batch of 64 against the same 64 items as single calls of the new entry point.  Without a bar: both next to
    export_rgb_colour_reduced and its batch, which scale code values, and the whole picture at 2:1 to RGBA float16."""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    dw = dh = 224
    hw, hh = w // 2, h // 2
    rounds, calls = 1 if a.short else max(a.repeats, 10), min(a.calls, 40)
    lin, m, enc, has_matrix, has_enc = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
    assert has_matrix and has_enc
    colour, lin_only = ctx.colour(lin, m, enc, bpc=bpc), ctx.colour(lin, bpc=bpc)
    P, K4, F16 = api.SURFACE_RGB_PLANAR, api.SURFACE_RGBA_PACKED, api.SAMPLE_F16
    surfs = [ctx.surface(dw, dh, layout, bpc, P, F16, matrix=9) for _ in range(a.pairs)]
    fulls = [ctx.surface(w, h, layout, bpc, P, F16, matrix=9) for _ in range(a.pairs)]
    halves = [ctx.surface(hw, hh, layout, bpc, K4, F16, matrix=9) for _ in range(a.pairs)]
    out_bytes, q_bytes = 3 * 2 * dw * dh, 2 * (dw * dh + 2 * (dw // 2) * (dh // 2))
    for p in pics:
        p.pic.twin_ok = api.TWIN_ONLY
    runs = []
    yard = "export_rgb_colour, lin only, to %dx%d planar float16 (yardstick)" % (w, h)
    runs.append((yard, src_bytes + 3 * 2 * w * h, lambda k: pics[k % a.pairs].export_rgb_colour(fulls[k % a.pairs], lin_only, 1), None))
    runs.append(("1. export_rgb_linear_reduced to 224x224 planar float16", src_bytes + out_bytes,
                 lambda k: pics[k % a.pairs].export_rgb_linear_reduced(surfs[k % a.pairs], colour, None, 1), yard))
    runs.append(("   export_rgb_colour_reduced to 224x224 planar float16 (code values, no bar)", src_bytes + 2 * q_bytes + out_bytes,
                 lambda k: pics[k % a.pairs].export_rgb_colour_reduced(surfs[k % a.pairs], colour, None, 1), None))
    n = 64
    bsurfs = [ctx.surface(dw, dh, layout, bpc, P, F16, matrix=9) for _ in range(n)]
    cw_, ch_ = min(w, 7168) & ~1, min(h, 4032) & ~1
    crops = [(((w - cw_) * (k % 8) // 7) & ~1, ((h - ch_) * (k // 8) // 7) & ~1, cw_, ch_) for k in range(n)]
    bytes_batch = n * (2 * (cw_ * ch_ + 2 * (cw_ // 2) * (ch_ // 2)) + out_bytes)

    def singles(k):
        for i in range(n):
            pics[(k + i) % a.pairs].export_rgb_linear_reduced(bsurfs[i], colour, crops[i], 1)
    yard = "64 single calls in place of the batch: export_rgb_linear_reduced, crops of %dx%d to 224x224 (yardstick)" % (cw_, ch_)
    runs.append((yard, bytes_batch, singles, None))
    runs.append(("2. export_rgb_linear_reduced_batch, 64 crops of %dx%d to (64, 3, 224, 224)" % (cw_, ch_), bytes_batch,
                 lambda k: ctx.export_rgb_linear_reduced_batch(bsurfs, [pics[(k + i) % a.pairs] for i in range(n)], colour, crops, 1), yard))
    runs.append(("   export_rgb_colour_reduced_batch, the same 64 items (code values, no bar)", bytes_batch + n * 2 * q_bytes,
                 lambda k: ctx.export_rgb_colour_reduced_batch(bsurfs, [pics[(k + i) % a.pairs] for i in range(n)], colour, crops, 1), None))
    runs.append(("3. export_rgb_linear_reduced to %dx%d RGBA float16 (no bar)" % (hw, hh), src_bytes + 4 * 2 * hw * hh,
                 lambda k: pics[k % a.pairs].export_rgb_linear_reduced(halves[k % a.pairs], colour, None, 1), None))
    print("# surface_bench --linear-reduced on %s: %dx%d 4:2:0 %d-bit twin-only sources, PQ / BT.2020 to sRGB / BT.709 (lin + matrix + enc), %d pictures / surfaces in rotation, "
          "3 warm-up + %d timed calls per variant and round (batch and its 64 single calls: 4), %d rounds, the variants alternated within a round"
          % (socket.gethostname(), w, h, bpc, a.pairs, calls, rounds))
    print("# bytes per call = bytes read + bytes written, from the shapes; device ms between two events around the timed calls; host ms: the clock around issuing them and "
          "the sync; last ms: dav1d_hip_last_kernel_ms of the last call")
    results = {r[0]: [] for r in runs}
    for rnd in range(rounds):
        for name, nbytes, call, _ in runs:
            nc = 4 if "batch" in name else calls
            for k in range(3):
                call(k)
            ctx.sync()
            t0 = time.perf_counter()
            ev.start()
            for k in range(nc):
                call(k)
            ms = ev.stop_ms() / nc
            host = (time.perf_counter() - t0) * 1e3 / nc
            last = ctx.last_kernel_ms()
            results[name].append((ms, host, last))
            print("round %2d  %-100s device %8.4f ms/call  host %8.4f  last %8.4f  %7.1f MB/call  %7.0f GB/s" % (rnd, name, ms, host, last, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (median [min .. max] over the rounds)")
    for name, nbytes, _, _ in runs:
        cols = [sorted(v[i] for v in results[name]) for i in range(3)]
        med = [c[len(c) // 2] for c in cols]
        print("summary   %-100s device %8.4f [%8.4f .. %8.4f]  host %8.4f [%8.4f .. %8.4f]  last %8.4f [%8.4f .. %8.4f] ms   median %7.0f GB/s"
              % (name, med[0], cols[0][0], cols[0][-1], med[1], cols[1][0], cols[1][-1], med[2], cols[2][0], cols[2][-1], nbytes / med[0] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(x[0] for x in results[name]), sorted(x[0] for x in results[yard])
        ok = v[len(v) // 2] <= u[len(u) // 2] + (u[-1] - u[0])
        print("condition %-84s device median %.4f ms <= yardstick median %.4f ms + its spread %.4f ms: %s (x %.2f)"
              % (name, v[len(v) // 2], u[len(u) // 2], u[-1] - u[0], "met" if ok else "NOT met", u[len(u) // 2] / v[len(v) // 2]))
    ctx.sync()
    ctx.colour_destroy(colour)
    ctx.colour_destroy(lin_only)
    for s in surfs + fulls + bsurfs + halves + pics:
        s.free()
    ctx.close()


def toned_runs(a, ctx, ev, pics, src_bytes):
    """the tone part of a handle: each of the three single calls and the 64-item linear batch with the un-toned handle of
    dav1d_hip_colour_tables(10, 16, 9, 13, 1, 203, 1000) and with the toned one of dav1d_hip_colour_tables_toned, alternated within a round.  A
    library without dav1d_hip_colour_create_toned (the commit before the tone part) runs the un-toned half alone: the same command there gives the
    yardstick the un-toned calls are held against."""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    dw = dh = 224
    rounds, calls = 1 if a.short else max(a.repeats, 10), min(a.calls, 40)
    lin, m, enc, has_matrix, has_enc = api.colour_tables(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
    assert has_matrix and has_enc
    handles = [("un-toned", ctx.colour(lin, m, enc, bpc=bpc))]
    if hasattr(ctx.lib, "dav1d_hip_colour_create_toned"):
        handles.append(("toned", ctx.colour_for(bpc, 16, 9, 13, 1, 203.0, 1000.0, luminance=True)))
    P, F16 = api.SURFACE_RGB_PLANAR, api.SAMPLE_F16
    fulls = [ctx.surface(w, h, layout, bpc, P, F16, matrix=9) for _ in range(a.pairs)]
    surfs = [ctx.surface(dw, dh, layout, bpc, P, F16, matrix=9) for _ in range(a.pairs)]
    n = 64
    bsurfs = [ctx.surface(dw, dh, layout, bpc, P, F16, matrix=9) for _ in range(n)]
    cw_, ch_ = min(w, 7168) & ~1, min(h, 4032) & ~1
    crops = [(((w - cw_) * (k % 8) // 7) & ~1, ((h - ch_) * (k // 8) // 7) & ~1, cw_, ch_) for k in range(n)]
    out_bytes, q_bytes = 3 * 2 * dw * dh, 2 * (dw * dh + 2 * (dw // 2) * (dh // 2))
    bytes_batch = n * (2 * (cw_ * ch_ + 2 * (cw_ // 2) * (ch_ // 2)) + out_bytes)
    for p in pics:
        p.pic.twin_ok = api.TWIN_ONLY
    runs = []
    for hname, hd in handles:
        yard = None if hname == "un-toned" else lambda name: name.replace("toned", "un-toned", 1)
        for name, nbytes, call in (
                ("1. export_rgb_colour to %dx%d planar float16, %s" % (w, h, hname), src_bytes + 3 * 2 * w * h,
                 lambda k, hd=hd: pics[k % a.pairs].export_rgb_colour(fulls[k % a.pairs], hd, 1)),
                ("2. export_rgb_colour_reduced to 224x224 planar float16, %s" % hname, src_bytes + 2 * q_bytes + out_bytes,
                 lambda k, hd=hd: pics[k % a.pairs].export_rgb_colour_reduced(surfs[k % a.pairs], hd, None, 1)),
                ("3. export_rgb_linear_reduced to 224x224 planar float16, %s" % hname, src_bytes + out_bytes,
                 lambda k, hd=hd: pics[k % a.pairs].export_rgb_linear_reduced(surfs[k % a.pairs], hd, None, 1)),
                ("4. export_rgb_linear_reduced_batch, 64 crops of %dx%d to (64, 3, 224, 224), %s" % (cw_, ch_, hname), bytes_batch,
                 lambda k, hd=hd: ctx.export_rgb_linear_reduced_batch(bsurfs, [pics[(k + i) % a.pairs] for i in range(n)], hd, crops, 1))):
            runs.append((name, nbytes, call, yard(name) if yard else None))
    runs.sort(key=lambda r: (r[0][:2], r[3] is not None))          # a call with the un-toned handle, then the same call with the toned one
    print("# surface_bench --toned on %s: %dx%d 4:2:0 %d-bit twin-only sources, PQ / BT.2020 to sRGB / BT.709 (lin + matrix + enc; toned: the curve as a gain on the luminance), "
          "chroma_pos 1, %d pictures / surfaces in rotation, 3 warm-up + %d timed calls per variant and round (batch: 4), %d rounds, the variants alternated within a round"
          % (socket.gethostname(), w, h, bpc, a.pairs, calls, rounds))
    print("# bytes per call = bytes read + bytes written, from the shapes (tables not counted); device ms between two events around the timed calls; host ms: the clock around "
          "issuing them and the sync; last ms: dav1d_hip_last_kernel_ms of the last call")
    results = {r[0]: [] for r in runs}
    for rnd in range(rounds):
        for name, nbytes, call, _ in runs:
            nc = 4 if "batch" in name else calls
            for k in range(3):
                call(k)
            ctx.sync()
            t0 = time.perf_counter()
            ev.start()
            for k in range(nc):
                call(k)
            ms = ev.stop_ms() / nc
            host = (time.perf_counter() - t0) * 1e3 / nc
            last = ctx.last_kernel_ms()
            results[name].append((ms, host, last))
            print("round %2d  %-100s device %8.4f ms/call  host %8.4f  last %8.4f  %7.1f MB/call  %7.0f GB/s" % (rnd, name, ms, host, last, nbytes / 1e6, nbytes / ms / 1e6))
    print("# summary (median [min .. max] over the rounds)")
    for name, nbytes, _, _ in runs:
        cols = [sorted(v[i] for v in results[name]) for i in range(3)]
        med = [c[len(c) // 2] for c in cols]
        print("summary   %-100s device %8.4f [%8.4f .. %8.4f]  host %8.4f [%8.4f .. %8.4f]  last %8.4f [%8.4f .. %8.4f] ms   median %7.0f GB/s"
              % (name, med[0], cols[0][0], cols[0][-1], med[1], cols[1][0], cols[1][-1], med[2], cols[2][0], cols[2][-1], nbytes / med[0] / 1e6))
    for name, _, _, yard in runs:
        if yard is None:
            continue
        v, u = sorted(x[0] for x in results[name]), sorted(x[0] for x in results[yard])
        print("ratio     %-100s device median %.4f ms / un-toned median %.4f ms = %.3f (no bar; the un-toned call spreads over %.4f ms)"
              % (name, v[len(v) // 2], u[len(u) // 2], v[len(v) // 2] / u[len(u) // 2], u[-1] - u[0]))
    ctx.sync()
    for _, hd in handles:
        ctx.colour_destroy(hd)
    for s in fulls + surfs + bsurfs + pics:
        s.free()
    ctx.close()


def stats_runs(a, ctx, ev, pics, src_bytes):
    """per-picture light statistics: dav1d_hip_picture_light_stats of the whole picture on three contents — uniform noise, a flat
    picture, a smooth gradient with a letterbox — against dav1d_hip_surface_export_rgb_colour of the noise pictures at full size with a lin-only handle
    into planar float16 (the same samples, the same three lookups a pixel, and a surface written on top), alternated within a round; then the host
    time of dav1d_hip_colour_update_tone with an export right behind it."""
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    rounds, calls = 1 if a.short else max(a.repeats, 10), min(a.calls, 40)
    lin, m, enc, has_matrix, has_enc, K, gain, has_gain = api.colour_tables_toned(ctx.lib, bpc, 16, 9, 13, 1, 203.0, 1000.0)
    plain, toned = ctx.colour(lin, bpc=bpc), ctx.colour(lin, m, enc, bpc=bpc, tone=(K, gain))
    k = (K.astype(np.float64) / 10.0).astype(np.float32)
    contents = {"noise": pics}
    for name in ("flat", "gradient + letterbox"):
        group = []
        for i in range(a.pairs):
            p = ctx.picture(w, h, layout, bpc)
            for pl in range(3):
                shape = p.padded_shape(pl)
                if name == "flat":
                    plane = np.full(shape, (500, 520, 500)[pl] + i, np.uint16)
                else:
                    yy, xx = np.arange(shape[0])[:, None], np.arange(shape[1])[None, :]
                    plane = (64 + (xx * 700 // shape[1] + yy * 100 // shape[0] + i)).astype(np.uint16) if pl == 0 else np.full(shape, 512, np.uint16)
                    bar = shape[0] // 8          # 2.39:1 in 16:9 leaves about an eighth above and below
                    plane[:bar] = plane[shape[0] - bar:] = 64 if pl == 0 else 512
                p.upload(pl, plane)
            p.retile()
            p.pic.twin_ok = api.TWIN_ONLY
            group.append(p)
        contents[name] = group
    ctx.sync()
    fulls = [ctx.surface(w, h, layout, bpc, api.SURFACE_RGB_PLANAR, api.SAMPLE_F16, matrix=9) for _ in range(a.pairs)]
    stats = ctx.light_stats()
    runs = [("0. export_rgb_colour to %dx%d planar float16, lin only, noise (yardstick)" % (w, h), src_bytes + 3 * 2 * w * h,
             lambda i: pics[i % a.pairs].export_rgb_colour(fulls[i % a.pairs], plain, 1))]
    for name, group in contents.items():
        runs.append(("1. picture_light_stats, %s" % name, src_bytes, lambda i, group=group: stats.add(group[i % a.pairs], plain, k, matrix=9, chroma_pos=1)))
    print("# surface_bench --stats on %s: %dx%d 4:2:0 %d-bit twin-only sources, PQ lin, chroma_pos 1, %d pictures in rotation, 3 warm-up + %d timed calls per variant and round, "
          "%d rounds, the variants alternated within a round" % (socket.gethostname(), w, h, bpc, a.pairs, calls, rounds))
    print("# bytes per call = bytes read + bytes written, from the shapes (tables not counted); device ms between two events around the timed calls; host ms: the clock around "
          "issuing them and the sync; last ms: dav1d_hip_last_kernel_ms of the last call")
    results = {r[0]: [] for r in runs}
    for rnd in range(rounds):
        for name, nbytes, call in runs:
            for i in range(3):
                call(i)
            ctx.sync()
            stats.reset()
            t0 = time.perf_counter()
            ev.start()
            for i in range(calls):
                call(i)
            ms = ev.stop_ms() / calls
            host = (time.perf_counter() - t0) * 1e3 / calls
            last = ctx.last_kernel_ms()
            results[name].append((ms, host, last))
            print("round %2d  %-90s device %8.4f ms/call  host %8.4f  last %8.4f  %7.1f MB/call  %7.0f GB/s" % (rnd, name, ms, host, last, nbytes / 1e6, nbytes / ms / 1e6))
            if name.startswith("1."):
                d = stats.read()
                assert d["n"] == calls * w * h and int(d["hist"].sum()) == d["n"], "every pixel of every call was counted"
    print("# summary (median [min .. max] over the rounds)")
    med = {}
    for name, nbytes, _ in runs:
        cols = [sorted(v[i] for v in results[name]) for i in range(3)]
        m3 = [c[len(c) // 2] for c in cols]
        med[name] = (m3[0], cols[0][-1] - cols[0][0])
        print("summary   %-90s device %8.4f [%8.4f .. %8.4f]  host %8.4f [%8.4f .. %8.4f]  last %8.4f [%8.4f .. %8.4f] ms   median %7.0f GB/s"
              % (name, m3[0], cols[0][0], cols[0][-1], m3[1], cols[1][0], cols[1][-1], m3[2], cols[2][0], cols[2][-1], nbytes / m3[0] / 1e6))
    names = [r[0] for r in runs]
    print("ratio     stats on noise / yardstick = %.3f (should not exceed 1; the yardstick spreads over %.4f ms)" % (med[names[1]][0] / med[names[0]][0], med[names[0]][1]))
    print("ratio     stats flat / noise = %.3f; gradient + letterbox / noise = %.3f (the contention handling)" % (med[names[2]][0] / med[names[1]][0], med[names[3]][0] / med[names[1]][0]))
    # dav1d_hip_colour_update_tone: the host time of the call, an export right behind each
    n = 40
    for i in range(4):
        ctx.colour_update_tone(toned, (K, gain))
        pics[i % a.pairs].export_rgb_colour(fulls[i % a.pairs], toned, 1)
    ctx.sync()
    host_us = []
    ev.start()
    for i in range(n):
        t0 = time.perf_counter()
        ctx.colour_update_tone(toned, (K, gain))
        host_us.append((time.perf_counter() - t0) * 1e6)
        pics[i % a.pairs].export_rgb_colour(fulls[i % a.pairs], toned, 1)
    ms = ev.stop_ms() / n
    host_us.sort()
    print("update    colour_update_tone + export_rgb_colour (toned, planar float16): host time of the update through Python median %.1f us [%.1f .. %.1f]; device %.4f ms per pair "
          "(the export alone is line 1 of --toned)" % (host_us[n // 2], host_us[0], host_us[-1], ms))
    stats.free()
    ctx.colour_destroy(plain)
    ctx.colour_destroy(toned)
    for group in contents.values():
        for p in group:
            p.free()
    for s_ in fulls:
        s_.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short", action="store_true", help="40 calls, one repeat (for a kernel trace)")
    ap.add_argument("--grain", action="store_true", help="the fused grain + export variants against fg_apply_prepared + export")
    ap.add_argument("--scaled", action="store_true", help="dav1d_hip_surface_export_scaled at 2:1 and 4:1 against the plain export at full size")
    ap.add_argument("--rgb", action="store_true", help="dav1d_hip_surface_export_rgb (sited chroma, packed, float16) against the plain export to RGB planes")
    ap.add_argument("--rgb-scaled", action="store_true", help="dav1d_hip_surface_export_rgb_scaled against export_scaled into a picture + export_rgb from it")
    ap.add_argument("--batch", action="store_true", help="dav1d_hip_surface_export_rgb_scaled_batch against the N single calls it replaces")
    ap.add_argument("--colour", action="store_true", help="dav1d_hip_surface_export_rgb_colour (PQ / BT.2020 -> sRGB / BT.709) against export_rgb to the same format")
    ap.add_argument("--reduced", action="store_true", help="dav1d_hip_surface_export_rgb_reduced to 224 x 224 against export_scaled 8:1 + export_rgb_resized; a batch of 64")
    ap.add_argument("--colour-reduced", action="store_true", help="dav1d_hip_surface_export_rgb_colour_reduced and its batch against export_rgb_reduced; at 2:1 against export_scaled + export_rgb_colour")
    ap.add_argument("--linear-reduced", action="store_true", help="dav1d_hip_surface_export_rgb_linear_reduced against a full-size export_rgb_colour; its batch against 64 single calls")
    ap.add_argument("--toned", action="store_true", help="the three colour-managed single calls and the linear batch of 64 with an un-toned and a toned handle, alternated")
    ap.add_argument("--stats", action="store_true", help="dav1d_hip_picture_light_stats on noise, a flat picture and a gradient with a letterbox against a full-size export_rgb_colour; update_tone's host time")
    ap.add_argument("--cells", type=lambda v: [int(x) for x in v.split(",") if x], default=[], help="--colour: variants (a) and (c) again with these values of the option colour_cells")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    a = ap.parse_args()
    if a.short:
        a.calls, a.repeats = 40, 1
    w, h, bpc, layout = a.width, a.height, 10, api.LAYOUT_I420
    cw, ch = (w + 1) // 2, (h + 1) // 2
    ctx = api.Context(0)
    ev = Events(ctx.lib.dav1d_hip_stream(ctx.h))
    rng = np.random.default_rng(1)
    pics, shared = [], {}
    for _ in range(32 if a.batch else a.pairs):
        p = ctx.picture(w, h, layout, bpc)
        for pl in range(3):
            shape = p.padded_shape(pl)
            if not a.batch or pl not in shared:
                shared[pl] = rng.integers(0, 1 << bpc, size=shape, dtype=np.uint16)
            p.upload(pl, shared[pl])
        p.retile()
        p.pic.twin_ok = api.TWIN_ONLY
        pics.append(p)
    ctx.sync()
    src_bytes = 2 * (w * h + 2 * cw * ch)
    P, S, R = api.SURFACE_PLANAR, api.SURFACE_SEMIPLANAR, api.SURFACE_RGB_PLANAR
    variants = [("planar native", P, api.SAMPLE_NATIVE, src_bytes), ("P010 (semi-planar MSB16)", S, api.SAMPLE_MSB16, src_bytes),
                ("RGB planar native BT.709 limited", R, api.SAMPLE_NATIVE, 3 * 2 * w * h), ("RGB planar float32 BT.709 limited", R, api.SAMPLE_F32, 3 * 4 * w * h)]
    if a.short:
        variants = variants[:3]
    if a.grain:
        return grain_runs(a, ctx, ev, pics, variants[:3], src_bytes)
    if a.scaled:
        return scaled_runs(a, ctx, ev, pics, variants[:3], src_bytes)
    if a.rgb:
        return rgb_runs(a, ctx, ev, pics, src_bytes)
    if a.rgb_scaled:
        return rgb_scaled_runs(a, ctx, ev, pics, src_bytes)
    if a.batch:
        return batch_runs(a, ctx, ev, pics)
    if a.colour:
        return colour_runs(a, ctx, ev, pics, src_bytes)
    if a.reduced:
        return reduced_runs(a, ctx, ev, pics, src_bytes)
    if a.colour_reduced:
        return colour_reduced_runs(a, ctx, ev, pics, src_bytes)
    if a.linear_reduced:
        return linear_reduced_runs(a, ctx, ev, pics, src_bytes)
    if a.toned:
        return toned_runs(a, ctx, ev, pics, src_bytes)
    if a.stats:
        return stats_runs(a, ctx, ev, pics, src_bytes)
    runs = []
    for name, fmt, sample, out_bytes in variants:
        surfs = [ctx.surface(w, h, layout, bpc, fmt, sample) for _ in range(a.pairs)]

        def export(k, surfs=surfs):
            p = pics[k % a.pairs]
            p.pic.twin_ok = api.TWIN_ONLY      # (the yardstick's untile leaves 1: the twin is still the picture, and it is what gets read)
            p.export(surfs[k % a.pairs])
        runs.append((name, src_bytes + out_bytes, surfs, export))

    def untile(k):
        p = pics[k % a.pairs]
        p.pic.twin_ok = api.TWIN_ONLY          # (untile leaves 1; the twin is still the picture)
        p.untile()
    # untile writes whole padded rows of the allocation: count what it moves
    up = pics[0]
    untile_bytes = 2 * sum(up.pic.p[pl].stride * (((up.pic.p[pl].h + 7) // 8) * 8) for pl in range(3))
    runs.insert(0, ("dav1d_hip_picture_untile (yardstick)", untile_bytes, None, untile))

    print("# surface_bench on %s: %dx%d 4:2:0 %d-bit, %d picture / surface pairs in rotation, 20 warm-up + %d timed calls per variant, %d repeats"
          % (socket.gethostname(), w, h, bpc, a.pairs, a.calls, a.repeats))
    print("# bytes per call = bytes read + bytes written, from the shapes; share of %.1f TB/s (spec) and of the %.1f TB/s copy ceiling" % (SPEC_TBS, COPY_TBS))
    results = {name: [] for name, _, _, _ in runs}
    for rep in range(a.repeats):
        for name, nbytes, _, call in runs:
            for k in range(20):
                call(k)
            ctx.sync()
            ev.start()
            for k in range(a.calls):
                call(k)
            ms = ev.stop_ms() / a.calls
            results[name].append(ms)
            gbs = nbytes / ms / 1e6
            print("repeat %d  %-40s %8.4f ms/call  %7.1f MB/call  %7.0f GB/s  %5.1f %% of spec  %5.1f %% of copy ceiling"
                  % (rep, name, ms, nbytes / 1e6, gbs, gbs / (SPEC_TBS * 10), gbs / (COPY_TBS * 10)))
    print("# summary (min / median / max ms per call over the repeats)")
    for name, nbytes, _, _ in runs:
        v = sorted(results[name])
        print("summary   %-40s %8.4f / %8.4f / %8.4f ms   median %7.0f GB/s" % (name, v[0], v[len(v) // 2], v[-1], nbytes / v[len(v) // 2] / 1e6))
    u = sorted(results[runs[0][0]])
    spread = u[-1] - u[0]
    for name in (runs[1][0], runs[2][0]):
        v = sorted(results[name])
        print("condition %-40s median %.4f ms <= untile median %.4f ms + its spread %.4f ms: %s"
              % (name, v[len(v) // 2], u[len(u) // 2], spread, "met" if v[len(v) // 2] <= u[len(u) // 2] + spread else "NOT met"))
    # orientation only: the way out that exists without this call (host fetch: crosses PCIe, not a fair peer)
    hp = api.HostPictureBuf(ctx, w, h, layout, bpc)
    n = 3 if a.short else 10
    for k in range(2):
        hp.fetch(pics[k % a.pairs].pic)
        hp.wait()
    t0 = time.perf_counter()
    for k in range(n):
        hp.fetch(pics[k % a.pairs].pic)
        hp.wait()
    ms = (time.perf_counter() - t0) * 1e3 / n
    print("orientation only, NOT a peer (device to host over PCIe): dav1d_hip_host_picture_fetch + _wait  %8.3f ms/picture (host clock, %d calls)" % (ms, n))
    hp.release()
    for _, _, surfs, _ in runs:
        for s in surfs or []:
            s.free()
    for p in pics:
        p.free()
    ctx.close()


if __name__ == "__main__":
    main()
