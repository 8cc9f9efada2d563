#!/usr/bin/env python3
"""Headline benchmark: reconstructed Mpixels/s of the itx+mc reconstruction path at
8K 4:2:0 10-bit on N MI355X GPUs (BASELINE.json metric), one process per GPU.

A "step" = one pass of the hot path over one synthetic 8K inter frame whose task lists
(tests/synth_frames.py, SURVEY.md §8d config C2's itx+mc subset) are already resident in HBM:
    mc put/prep (all blocks, 3 planes) -> compound avg (25 % of blocks) -> itxfm_add (all blocks).
Every step consumes its own pristine copy of the coefficient arena (the kernels zero the
slabs they consume, as the reference does) and rotates over 4 output pictures, so no step
runs on cached or already-zeroed data.  N > 1: frame-parallel replicas, one frame stream
per GPU, no data-path collective ("weak" scaling).

A plain run sets up, warms up, times the steps, writes the last step's pictures when
--dump-outputs DIR is given, and prints ONE JSON line (rank 0) with the throughput and
ms_per_step.  --full adds everything else the benchmark measures or checks: the parity gate
against the oracle, the roofline of the dominant kernel (measured live with HIP events on the
launch stream), the CPU baseline (the oracle replayed on the host cores for a bounded number
of frames), the other layouts, precisions, sizes and legs, and with N > 1 the C3 / C4 legs.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
# the CPU peers this file times (cpu_baseline, reference_pass2, the peer of the dav1d_task_loop legs) are the reference built the way dav1d
# ships (oracle/_ref_release, oracle/_ref_hooked_release: -O3 -DNDEBUG -fomit-frame-pointer -ffast-math), when those builds travelled with
# the repo; the asserts-on build stays the parity checker of tests/ (tests/util.py REF_SO), and tests/test_oracle.py holds the two equal
if all(os.path.exists(os.path.join(ROOT, "oracle", d_, f_)) for d_, f_ in (("_ref_release", "libdav1d_ref.so"), ("_ref_hooked_release", "libdav1d_hooked.so"))):
    os.environ.setdefault("DAV1D_REF_BUILD", "release")

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60, help="timed steps (default 60: 15 ms of device time at 8K; with two frames in flight the first and the last step run alone, and a run of 20 shows it — same box 0.246 - 0.254 ms per step at 20, 0.234 at 60, profiles/r06/streams.txt)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bpc", type=int, default=10)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget of the cpu_baseline leg")
    ap.add_argument("--mv-range", type=int, default=64, help="synthetic MV range in pixels (experiments)")
    ap.add_argument("--edge-frac", type=float, default=0.05, help="fraction of blocks pointing outside the picture")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--layout", choices=["tiled", "raster"], default="tiled",
                    help="where the step's pictures live: tiled = references read through their tiled twins and the reconstructed picture written as 8x8 "
                         "tiles ONLY (dav1d_hip_recon_list_run_tiled; raster rows exist at the output only, made by the un-tiling download), "
                         "raster = the reference's plane layout throughout (rounds 1-4)")
    ap.add_argument("--no-pmc", action="store_true", help="do not count roofline.traffic with rocprofv3 children (the committed profile's figure is reported instead)")
    ap.add_argument("--frame-contexts", type=int, default=2,
                    help="frame contexts of the headline step (dav1d's n_fc): the steps — one independent frame each — are dealt over that many library "
                         "contexts with streams of their own, so that a frame's launches run under the tail of the frame before; 1 = one frame at a time")
    ap.add_argument("--no-inflight", action="store_true", help="skip the frames-in-flight leg of the full table")
    ap.add_argument("--packed", action="store_true", help="feed the residuals in the sparse wire format (DAV1D_HIP_ITX_PACKED)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end leg (hand-off arrays -> lister -> device)")
    ap.add_argument("--e2e-tile-cols", type=int, default=16, help="tile columns of the end-to-end leg (one listing thread per tile)")
    ap.add_argument("--e2e-tile-rows", type=int, default=8, help="tile rows of the end-to-end leg")
    ap.add_argument("--e2e-threads", type=int, default=64, help="listing threads (of the library, dav1d_hip_lister_run) of the one-frame-at-a-time end-to-end legs (0: one per tile).  The MI355X boxes of this pool give the container 16 cores' worth of CPU time per 100 ms (cgroup cpu.max): a burst on 64 threads runs at full speed until that is spent, then every thread stops for the rest of the period — the frames-in-flight legs report both ways")
    ap.add_argument("--stream-frames", type=int, default=25, help="frames of the AV1 stream of the dav1d_task_loop_real_pass1 leg (every one compared with dav1d's)")
    ap.add_argument("--no-c1", action="store_true", help="skip the 4K 8-bit (BASELINE configs[1]) line that the default run appends")
    ap.add_argument("--no-full", action="store_true", help="with --full: skip the full-DSP-table leg (deblock, CDEF, restoration, film grain)")
    ap.add_argument("--two-phase", action="store_true",
                    help="run the step as dav1d_hip_inter_list_run + dav1d_hip_itx_list_run (every residual after every prediction) "
                         "instead of the pipelined dav1d_hip_recon_list_run")
    ap.add_argument("--step-only", action="store_true",
                    help="run the warm-up and the timed steps and nothing else (no per-kernel timing, parity, CPU or full-table legs): "
                         "what tools/pmc_profile.sh counts the step's HBM traffic on")
    ap.add_argument("--shard", choices=["frames", "tile-cols"], default="frames",
                    help="N > 1: frames = one independent frame stream per GPU (weak scaling, no data-path collective); "
                         "tile-cols = GPU g reconstructs tile column g of the SAME frame and one all-gather per frame rebuilds "
                         "the picture everywhere (SURVEY 8e config C3, strong scaling)")
    ap.add_argument("--config", choices=["c2", "c4"], default="c2",
                    help="c2 (default): the itx+mc recon step of the headline; c4 (BASELINE configs[4]): every rank takes a frame of its own through the "
                         "FULL table (recon, deblock, CDEF, restoration) and film grain per step (dav1d_amd.dist.C4Workload)")
    ap.add_argument("--dependent", action="store_true",
                    help="with --config c4: reference 0 of a rank's frame is the picture rank - 1 produced one step earlier; every owner broadcasts "
                         "its finished picture to all ranks after its step (RCCL broadcast, the publication rule of src/thread_task.c:416-433)")
    ap.add_argument("--mix", choices=["c2", "c1"], default="c2",
                    help="block mix of the synthetic frame: c2 = SURVEY 8d's C2 mix (64/32/16/8/4 = 20/30/30/15/5 %% by area, 25 %% compound); "
                         "c1 = SURVEY 8d's C1 spec (every block 16x16: TX_16X16 luma / TX_8X8 chroma, single reference)")
    ap.add_argument("--emu", action="store_true",
                    help="CPU run on the SIMT-emulated build of the same kernel sources (tests/emu), torch.distributed over gloo: what "
                         "tests/test_dist.py uses to run `bench.py --gpus 2` without a GPU (tiny sizes; no timing means anything)")
    ap.add_argument("--one-leg", action="store_true",
                    help="N > 1 with --full: only the leg the other flags select (default there: three legs in one line — frame-parallel replicas, "
                         "tile columns with in-loop filters (C3), dependent frames with film grain (C4)); without --full only that leg runs anyway")
    ap.add_argument("--tc-filters", action="store_true",
                    help="tile-cols only: the step also runs deblocking, CDEF and loop restoration of the rank's column after a halo "
                         "exchange of 16 luma columns with its neighbours (dav1d_amd/dist.py), and gathers the FILTERED columns")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, everything else: parity against the oracle, per-kernel roofline and counted traffic, CPU "
                         "baselines, the other layouts, the packed format, the full-table, end-to-end and task-loop legs, the 4K 8-bit lines, "
                         "and with N > 1 the C3 / C4 legs (the --no-* flags above trim this).  Off: the headline step alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the pictures the last timed step produced (rank 0) as DIR/<name>.npy, float32, visible area only; %d samples "
                         "at most in all: a plane above its share is cut to a fixed, seeded sample of whole rows (sorted)" % DUMP_SAMPLES)
    return ap.parse_args()


DUMP_SAMPLES = 15 << 20         # float32: 60 MiB in all, under 64 MB


def dump_outputs(out_dir, planes):
    """planes: [(name, 2-D array of pixel values)] -> out_dir/<name>.npy as float32 (pixels of up to 16 bits are exact).  A plane
    above its share of DUMP_SAMPLES keeps a seeded choice of whole rows, the same rows for the same plane shape in every run."""
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_SAMPLES // len(planes)
    for name, p in planes:
        p = np.asarray(p)
        if p.size > share:
            n_rows = max(1, share // p.shape[1])
            rows = np.sort(np.random.default_rng(0xD0C5 + p.shape[0] * 65536 + p.shape[1]).choice(p.shape[0], n_rows, replace=False))
            p = p[rows]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(p, dtype=np.float32))


def visible(planes, w, h):
    """the picture area of the three (padded) planes of a 4:2:0 picture"""
    return [pl[:h, :w] if k == 0 else pl[:(h + 1) >> 1, :(w + 1) >> 1] for k, pl in enumerate(planes)]


def algorithmic_bytes(frame):
    """per reconstructed coded single-ref inter sample
    P (ref read) + C (coef read) + C (coef zero-write) + P (dst write); compound adds one P."""
    P = 1 if frame.bpc == 8 else 2
    Cb = 2 if frame.bpc == 8 else 4
    comp_samples = int((frame.comp["w"].astype(np.int64) * frame.comp["h"]).sum())
    return frame.n_samples * (2 * P + 2 * Cb) + comp_samples * P


def pmc_traffic(kernel, w, h, bpc):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes of this very workload
    (tools/pmc_profile.sh -> profiles/*/traffic.json: FETCH_SIZE x 2 (gfx950 correction for wide
    reads, validated on the 179.5 MB arena copy in the same profile) + WRITE_SIZE); None when no
    profile of the default workload is available or the workload differs."""
    if (w, h, bpc) != (7680, 4320, 10):
        return None
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "traffic.json")))
    if not files:
        return None
    m = re.match(r"(mc|itx|recon)_(\d+)x(\d+)", kernel)
    if not m:
        return None
    d = json.load(open(files[-1]))
    if m.group(1) == "recon":
        key = "recon_fused_kernel<%d,u16,int>" % (int(m.group(2)).bit_length() - 3)
    elif m.group(1) == "mc":
        key = "mc_kernel<%s,%s,u16>" % (m.group(2), m.group(3))
    else:
        import synth_frames as synth
        tx = [i for i in range(19) if synth.TX_W[i] == int(m.group(2)) and synth.TX_H[i] == int(m.group(3))][0]
        key = "itx_add_kernel<%d,u16,int>" % tx
    if key not in d:        # the kernels carry their variants in the name (cooperative / tiled references / wide stores): the plain one has them all off
        cand = [k for k in d if k.startswith(key[:-1] + ",") and set(k[len(key):-1].split(",")) <= {"false"}]
        if not cand:
            return None
        key = cand[0]
    return int(d[key]["fetch_bytes_x2"] + d[key]["write_bytes"])


def step_traffic(w, h, bpc, a):
    """HBM bytes one step of the default workload moves: (FETCH_SIZE x 2 + WRITE_SIZE) summed over every kernel of
    `bench.py --step-only` under rocprofv3, divided by the steps it ran (tools/pmc_profile.sh -> profiles/*/step_traffic.json)."""
    if (w, h, bpc) != (7680, 4320, 10) or a.packed or a.two_phase or a.shard != "frames":
        return None
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "step_traffic.json")))
    if not files:
        return None
    return json.load(open(files[-1])).get("bytes_per_step")

def _kernel_pattern(name):
    """bench's kernel label -> regular expression on the HIP kernel's demangled name"""
    import re
    m = re.match(r"(mc|itx|recon)_(\d+)x(\d+)", name)
    if not m:
        return None
    if m.group(1) == "recon":
        return r"recon_fused_kernel<%d," % (int(m.group(2)).bit_length() - 3)
    if m.group(1) == "mc":
        return r"mc_(?:twin_)?kernel<%s, %s," % (m.group(2), m.group(3))
    import synth_frames as synth
    tx = [i for i in range(19) if synth.TX_W[i] == int(m.group(2)) and synth.TX_H[i] == int(m.group(3))][0]
    return r"itx_add(?:_wide)?_kernel<%d," % tx


def counted_traffic(a, timeout=240):
    """HBM bytes of the step's kernels counted in THIS run on THIS box: two rocprofv3 children (FETCH_SIZE and WRITE_SIZE take a pass
    each, MI355X_MICROARCH.md "rocprofv3 PMC slots"; kernel trace only, no other trace domain) over `bench.py --step-only` with the
    same workload arguments.  Returns {"per_kernel": {demangled name: bytes per launch}, "per_step": bytes, "launches": n} or
    {"error": ...}.  HBM bytes = FETCH_SIZE x 2 (gfx950: 128-byte requests are tallied as 64, calibrated in
    profiles/r02_calib_fetch_size.txt) + WRITE_SIZE, both reported in KiB."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return {"error": "no rocprofv3 on this host"}
    steps, warm = 2, 1
    args = [sys.executable, os.path.abspath(__file__), "--step-only", "--steps", str(steps), "--warmup", str(warm), "--width", str(a.width),
            "--height", str(a.height), "--bpc", str(a.bpc), "--mix", a.mix, "--mv-range", str(a.mv_range), "--edge-frac", str(a.edge_frac),
            "--layout", a.layout]
    if a.packed:
        args.append("--packed")
    if a.two_phase:
        args.append("--two-phase")
    env = dict(os.environ, DAV1D_BENCH_CHILD="1", TMPDIR="/tmp")
    tot = {}
    tmp = tempfile.mkdtemp(prefix="bench_pmc_", dir="/tmp")
    try:
        for cname in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, cname)
            try:
                r = subprocess.run([exe, "--kernel-trace", "--pmc", cname, "--output-format", "csv", "-d", out, "--"] + args, cwd="/tmp", env=env,
                                   capture_output=True, text=True, timeout=timeout)
            except subprocess.TimeoutExpired:
                return {"error": "rocprofv3 --pmc %s timed out after %d s" % (cname, timeout)}
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode or not files:
                return {"error": "rocprofv3 --pmc %s: rc %d, %d counter files: %s" % (cname, r.returncode, len(files), (r.stderr or r.stdout)[-200:])}
            for f in files:
                for row in csv.DictReader(open(f)):
                    if row["Counter_Name"] != cname:
                        continue
                    e = tot.setdefault(row["Kernel_Name"], {"FETCH_SIZE": 0.0, "WRITE_SIZE": 0.0, "n": 0})
                    e[cname] += float(row["Counter_Value"]) * 1024
                    if cname == "FETCH_SIZE":
                        e["n"] += 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    import re
    step_re = re.compile(r"(mc_kernel|mc_twin_kernel|itx_add_kernel|itx_add_wide_kernel|recon_fused_kernel|comp_kernel|mc_all_kernel|itx_multi_kernel)<")
    per_kernel, per_step = {}, 0.0
    for k, e in tot.items():
        if not e["n"] or not step_re.search(k):        # fills / copies of the harness are not the step
            continue
        b = 2 * e["FETCH_SIZE"] + e["WRITE_SIZE"]
        per_kernel[k] = b / e["n"]
        per_step += b / (steps + warm)
    if not per_kernel:
        return {"error": "no kernel of the step in the counter files"}
    return {"per_kernel": per_kernel, "per_step": per_step, "launches": steps + warm}


def device_probe(torch):
    """What this particular box is: boxes of one pool have measured 10-15 % apart on every kernel of the step (and 2.7x on the
    64x64 transform launch) with the same build; the compute units the runtime reports and a plain 1 GiB
    device-to-device copy timed here let a reader tell a slow box from a slow kernel."""
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        n = 1 << 28
        a = torch.empty(n, dtype=torch.int32, device="cuda")
        b = torch.empty(n, dtype=torch.int32, device="cuda")
        a.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(4):
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        del a, b
        return {"name": pr.name, "compute_units": int(pr.multi_processor_count),
                "copy_1gib_gbs": round(2 * 4 * n / (best * 1e-3) / 1e9, 1)}       # read + write
    except Exception as e:       # noqa: BLE001
        return {"error": str(e)[:120]}


def frames_in_flight(api, device, frame, itx_tasks, coef_host, intra, post, ref_host, dst_host, w, h, bpc, want_res, n_ctx_list=(1, 2, 4, 8), n_frames=4):
    """The full DSP table as dav1d's frame threading would drive it: n contexts (one per frame in flight, own streams), each
    running whole frames — recon list, intra waves, deblock, CDEF, restoration, film grain — from device-resident lists, one host
    thread per context.  Wall clock over n_frames frames per context, everything included (task-list uploads of the in-loop
    filters, stream synchronisation between stages).  One frame in flight leaves the GPU to the ~50 dependent launches of the
    intra waves for a third of the time; a second frame fills it.  The frames do not reference each other (in a stream, frames
    in flight reference pictures that are already final, src/thread_task.c:416-433).  Every context's last picture is compared
    with the stage-by-stage result that was checked against the oracle."""
    import threading
    out = {}
    states = []

    def make(k):
        ctx = api.Context(device)
        st = {"ctx": ctx}
        st["refs"] = []
        for rp in ref_host:
            r = ctx.picture(w, h, api.LAYOUT_I420, bpc)
            for pl in range(3):
                r.upload(pl, rp[pl])
            st["refs"].append(r)
        st["pics"] = [ctx.picture(w, h, api.LAYOUT_I420, bpc) for _ in range(4)]         # reconstructed / deblocked, CDEF, restored, grain
        st["recon"] = ctx.recon_list(st["pics"][0], frame.mc, frame.comp, itx_tasks)
        st["intra"] = ctx.intra_list(intra.batches)
        st["prep"] = ctx.buffer(frame.prep_elems * 2)
        st["prep"].zero()
        st["coef"] = [ctx.buffer_from(coef_host) for _ in range(n_frames + 1)]            # the residual launches zero what they read
        st["icoef"] = [ctx.buffer_from(intra.coef) for _ in range(n_frames + 1)]          # (the last one is the warm-up frame's)
        st["lvl"] = ctx.buffer_from(post.lvl)
        st["grain"] = ctx.fg_prepare(post.fg, bpc, api.LAYOUT_I420) if post.fg is not None else None
        ctx.sync()
        return st

    def one_frame(st, i):
        ctx = st["ctx"]
        rec, cdf, res, grn = st["pics"]
        st["recon"].run(rec, st["refs"], st["prep"], st["coef"][i])
        st["intra"].run_all(rec, st["icoef"][i])
        ctx.lf_batch(rec, post.lf, st["lvl"], post.b4_stride, post.lut_e, post.lut_i)
        ctx.cdef_batch(cdf, rec, post.cdef, post.cdef_damping)
        ctx.lr_batch(res, cdf, rec, post.lr)
        if st["grain"] is not None:
            ctx.fg_apply_prepared(grn, res, st["grain"])
        ctx.sync()

    def reset(st):
        for pl in range(3):
            st["pics"][0].upload(pl, dst_host[pl])
        for b in st["coef"]:
            b.upload(coef_host)
        for b in st["icoef"]:
            b.upload(intra.coef)
        st["ctx"].sync()

    try:
        for n in n_ctx_list:
            while len(states) < n:
                states.append(make(len(states)))
            for st in states[:n]:
                reset(st)
                one_frame(st, n_frames)             # warm-up: first-use allocations of the context's pools, code objects
            errs = []

            def work(st):
                try:
                    for i in range(n_frames):       # the blocks cover the picture: every frame rewrites all of it
                        one_frame(st, i)
                except Exception as e:      # noqa: BLE001
                    errs.append(e)
            th = [threading.Thread(target=work, args=(st,)) for st in states[:n]]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            dt = time.perf_counter() - t0
            if errs:
                raise errs[0]
            for st in states[:n]:
                for pl in range(3):
                    vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
                    if not np.array_equal(st["pics"][2].download(pl)[:vh, :vw], want_res[pl][:vh, :vw]):
                        raise SystemExit("bench: %d frames in flight: restored picture differs from the checked stage-by-stage result" % n)
            out[str(n)] = round(dt / (n * n_frames) * 1e3, 4)
    finally:
        for st in states:
            ctx = st["ctx"]
            if st.get("grain") is not None:
                ctx.fg_grain_destroy(st["grain"])
            st["recon"].destroy()
            st["intra"].destroy()
            for o in st["refs"] + st["pics"] + st["coef"] + st["icoef"] + [st["prep"], st["lvl"]]:
                o.free()
            ctx.close()
    return out


class _NoEvent:
    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        pass

    def elapsed_time(self, other):
        return 1e-3


def _emu_torch(torch):
    """--emu: the torch.cuda calls of this file become no-ops (the kernels run on the CPU inside the emulated library)"""
    torch.cuda.synchronize = lambda *a, **k: None
    torch.cuda.set_device = lambda *a, **k: None
    torch.cuda.is_available = lambda: True
    torch.cuda.Event = _NoEvent


def respawn_under_launcher(a):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: the same command line once per GPU under torch.distributed.run
    (one process per GPU, RCCL rendezvous on 127.0.0.1)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.execv(sys.executable, cmd)

# ---- the line the driver parses.  Everything a run measures goes to bench_legs.json (next to this file, and to gpurun_out/ when that
# exists) and to stderr; stdout carries ONE line of well under 8 KB (round 4's line had grown to 23 KB and the driver's record of it
# came back unparsed): the contract fields, flat roofline / cpu_baseline scalars and one number + parity per leg.
LINE_LIMIT = 8000


def _short(v, n=160):
    return v if not isinstance(v, str) or len(v) <= n else v[:n - 3] + "..."


def _leg_digest(name, leg):
    """one number + parity per leg"""
    if not isinstance(leg, dict):
        return None
    if "error" in leg:
        return {"error": _short(leg["error"], 80)}
    if "status" in leg:
        return {"status": _short(leg["status"], 80)}
    d = {}
    ss = leg.get("steady_state")
    if isinstance(ss, dict):
        d["fps"] = ss.get("fps")
        ps = leg.get("peer_steady_state")
        if isinstance(ps, dict):
            d["peer_fps"] = ps.get("fps")
        if "frame_end_ms" in ss:
            d["frame_end_ms"] = ss.get("frame_end_ms")
    for k in ("ms_per_frame", "ms_per_step", "total_ms", "frame_end_ms", "list_ms", "cost_pct", "host_cpu_ms_per_frame", "value", "frac", "save_tmvs_ms"):
        if k in leg and not isinstance(leg[k], (dict, list)) and k not in d:
            d[k] = leg[k]
        if len(d) >= 4:
            break
    par = leg.get("parity")
    if isinstance(par, str):
        d["parity"] = "bit-exact" if par.startswith(("bit-exact", "every stage bit-exact")) else _short(par, 40)
    return d or None


def compact_line(full, legs=None):
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    line = {k: full.get(k) for k in keep}
    cfg = full.get("config") or {}
    line["config"] = {k: _short(cfg.get(k), 330) for k in ("workload", "parallelism", "parity", "frames_per_step", "frame_contexts", "coef_format", "step", "picture_layout", "ms_per_step_by_layout") if k in cfg}
    roof = full.get("roofline")
    if isinstance(roof, dict):
        r = {k: roof.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "algorithmic_bytes_per_launch",
                                       "frac_measured_traffic", "traffic_over_algorithmic", "path_frac", "path_achieved", "path_ms", "path_traffic",
                                       "path_traffic_over_algorithmic", "class_4x4_frac", "class_4x4_ms", "full_table_frac",
                                       "full_table_ms_per_frame", "full_table_achieved", "kernels_ms", "kernels_frac", "kernels_traffic", "what") if k in roof}
        r["traffic_source"] = _short(roof.get("traffic_source"), 200)
        line["roofline"] = r
    else:
        line["roofline"] = roof
    cpu = full.get("cpu_baseline")
    if isinstance(cpu, dict):
        line["cpu_baseline"] = {k: _short(cpu.get(k), 200) for k in ("value", "unit", "cores", "kind", "flags", "sample", "host_cores_available", "all_cores_value",
                                                                       "all_cores_cores", "reference_pass2_value", "reference_pass2_cores", "avx2") if k in cpu}
    else:
        line["cpu_baseline"] = cpu
    line["n_ranks_seen"] = full.get("n_ranks_seen")
    dg = dict(legs or {})
    for k, v in full.items():
        if k in keep or k in ("config", "roofline", "cpu_baseline", "n_ranks_seen", "legs", "device", "streams"):
            continue
        if k == "end_to_end_frames_in_flight" and isinstance(v, dict):
            for kk, vv in v.items():
                e = _leg_digest(kk, vv) if isinstance(vv, dict) else None
                if e:
                    dg["in_flight_" + kk] = e
            continue
        e = _leg_digest(k, v)
        if e:
            dg[k] = e
    if isinstance(full.get("full_table"), dict) and isinstance(full["full_table"].get("stages_ms"), dict):
        dg.setdefault("full_table", {})["stages_ms"] = full["full_table"]["stages_ms"]
    line["legs"] = dg
    if isinstance(full.get("device"), dict):
        line["device"] = full["device"]
    line["legs_file"] = "bench_legs.json (every leg in full; also on stderr)"
    txt = json.dumps(line)
    if len(txt) >= LINE_LIMIT:          # never lose the headline to an oversized digest
        line["legs"] = {k: {kk: vv for kk, vv in v.items() if kk in ("fps", "ms_per_frame", "ms_per_step", "value", "parity", "error")} for k, v in dg.items()}
        txt = json.dumps(line)
    if len(txt) >= LINE_LIMIT:
        line["legs"] = "see legs_file"
        txt = json.dumps(line)
    return txt


def emit(full, legs=None):
    if legs:
        full["legs"] = legs
    blob = json.dumps(full)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_legs.json"), "w") as f:
                    f.write(blob + "\n")
            except OSError:
                pass
    print(blob, file=sys.stderr)
    sys.stderr.flush()
    if full.get("step_only"):
        print(blob)
    else:
        print(compact_line(full, legs))
    sys.stdout.flush()


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_launcher(a)
    import torch
    import torch.distributed as dist
    from dav1d_amd import dist as dd
    rank, local, world = dd.env()
    assert world == a.gpus, "launch with torch.distributed.run --nproc-per-node %d (or without a launcher: bench.py starts one)" % a.gpus
    if a.emu:
        _emu_torch(torch)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    torch.cuda.set_device(local)
    if world > 1:
        if a.emu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    ranks_seen = 1
    if world > 1:
        t = torch.ones(1, dtype=torch.int32, device=DEV(a))
        dist.all_reduce(t)                       # RCCL (gloo with --emu): how many ranks really take part
        ranks_seen = int(t.item())
    if world > 1 and a.full and not a.one_leg and a.shard == "frames" and a.config == "c2" and not a.step_only:
        # ---- three legs in one line: replicas (the headline step on every GPU), C3, C4
        import copy
        primary = run_job(a, rank, local, world)
        a3 = copy.copy(a)
        a3.shard, a3.tc_filters, a3.no_cpu = "tile-cols", True, True
        c3 = run_job(a3, rank, local, world)
        a4 = copy.copy(a)
        a4.config, a4.dependent, a4.no_cpu = "c4", True, True
        c4 = run_job(a4, rank, local, world)
        # dav1d's own loop over the N devices, ONE process: rank 0 runs it in a child while the other ranks wait on the CPU (a gloo barrier:
        # an RCCL one would keep a spinning kernel on the GPUs the child is about to use)
        n_leg = None
        if (a.emu and os.environ.get("DAV1D_BENCH_N_DEVICES_LEG")) or (not a.emu and not a.no_e2e and not a.no_check):
            import datetime
            try:
                cpu_group = dist.new_group(backend="gloo", timeout=datetime.timedelta(seconds=1500))
            except Exception as e:       # noqa: BLE001  (the leg is an extra: without a CPU-side group it is left out, on every rank alike)
                cpu_group = None
                n_leg = {"status": "skipped: no gloo group next to the RCCL one (%s)" % str(e)[:80]}
            if cpu_group is not None:
                if rank == 0:
                    n_leg = task_loop_n_gpus_leg(a, world)
                try:
                    dist.barrier(group=cpu_group)
                except Exception:        # noqa: BLE001
                    pass
        if rank == 0:
            primary["dav1d_task_loop_n_gpus"] = n_leg
            def digest(line):
                return {"metric": line["metric"], "value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"], "scaling": line["scaling"],
                        "parallelism": line["config"].get("parallelism"), "parity": line["config"].get("parity"),
                        "roofline_frac": (line.get("roofline") or {}).get("frac"), "n_ranks_seen": ranks_seen}
            primary["n_ranks_seen"] = ranks_seen
            emit(primary, {"replicas": digest(primary), "c3_tile_columns_with_in_loop_filters": digest(c3), "c4_dependent_frames_full_table_film_grain": digest(c4)})
    else:
        line = run_job(a, rank, local, world)
        if rank == 0 and line is not None:
            line["n_ranks_seen"] = ranks_seen
            if a.full or a.step_only:
                emit(line)
            else:               # a plain run: the headline line alone
                print(json.dumps(line))
                sys.stdout.flush()
    if world > 1:
        dist.barrier()
        dd.close_peers()
        dist.destroy_process_group()


def task_loop_n_gpus_leg(a, world):
    """--gpus N: dav1d is ONE process — the chain of the dav1d_task_loop leg with the binding's frames ending on N devices of one process in
    turn (Dav1dHipGlueOptions.n_devices; a reference of another device is copied over first), next to one device, in a child process
    (tools/task_loop_n_devices.py) so that whatever happens in there stays out of this line."""
    import subprocess
    try:
        cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "task_loop_n_devices.py"), str(world),
               "--width", str(a.width), "--height", str(a.height), "--bpc", str(a.bpc), "--frames", "16"]
        if a.emu:                # ($DAV1D_BENCH_N_DEVICES_LEG: the flow of this leg on emulated devices, tests/test_dist.py)
            cmd += ["--emu", "--frames", "6", "--threads", "4"]
        child = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        last = child.stdout.strip().splitlines()[-1] if child.stdout.strip() else ""
        return json.loads(last) if child.returncode == 0 and last.startswith("{") else {"error": "rc %d: %s" % (child.returncode, child.stderr[-160:])}
    except Exception as e:       # noqa: BLE001  (a reported extra)
        return {"error": str(e)[:200]}



def DEV(a):
    return "cpu" if a.emu else "cuda"


def run_job(a, rank, local, world):
    """One measurement (the mode `a` selects) on the process group main() set up; returns the JSON line on rank 0, None elsewhere."""
    import torch
    from dav1d_amd import dist as dd
    from dav1d_amd import api
    import synth_frames as synth
    dev = DEV(a)

    if a.emu:
        a.no_full = a.no_e2e = a.no_c1 = a.no_inflight = True         # (legs that time GPU streams)
        import util
        ctx = util.make_context("emu")
        stream = None
    else:
        stream = torch.cuda.current_stream()
        ctx = api.Context(local, stream=stream.cuda_stream)
    w, h, bpc = a.width, a.height, a.bpc
    t_gen = time.time()
    tile_cols = a.shard == "tile-cols"
    # tile-column mode: every rank holds the same frame; dependent C4 frames likewise (rank 0 replays the whole chain on the oracle, and
    # the chain still tells a stale broadcast from a fresh one: every step's picture differs from the one before)
    srank = 0 if tile_cols or (a.config == "c4" and a.dependent) else rank
    mix_kw = dict(mix=(0.0, 0.0, 1.0, 0.0, 0.0), compound_frac=0.0) if a.mix == "c1" else {}
    frame = synth.make_frame(w, h, bpc, seed=0xDA71D002 + srank, mv_range_px=a.mv_range, edge_frac=a.edge_frac, **mix_kw,
                             n_refs=int(os.environ.get("BENCH_N_REFS", "3")))
    rng = np.random.default_rng(1234 + srank)
    ref_host = [synth.make_planes(rng, w, h, bpc) for _ in range(frame.n_refs)]
    dst_host = synth.make_planes(rng, w, h, bpc, smooth=False)
    t_gen = time.time() - t_gen

    if a.config == "c4":
        # BASELINE configs[4]: frames in flight one per GPU, full table + film grain (+ dependent frames): its own short path
        post = synth.make_post_filters(frame, seed=0xF11 + srank)
        wl = dd.C4Workload(ctx, frame, post, ref_host, dst_host, rank, world, dev, a.dependent)
        tdt = torch.int16 if bpc == 8 else torch.int32
        pristine = torch.from_numpy(frame.coef).to(dev)
        n_arena = a.steps + a.warmup + 1
        arenas = torch.empty((n_arena, pristine.numel()), dtype=tdt, device=dev)
        for i in range(n_arena):
            arenas[i].copy_(pristine)
        torch.cuda.synchronize()
        for i in range(a.warmup):
            wl.step(arenas[i].data_ptr())
        torch.cuda.synchronize()
        parity = "skipped"
        if rank == 0 and a.full and not a.no_check and a.dependent and a.warmup:
            # the chain so far (every rank runs the same frame, reference 0 = what rank - 1 restored one step earlier) against the
            # oracle's replay of the same number of steps
            import util
            import test_frame
            import test_postchain
            oracle = util.default_oracle()
            prev = None
            for sidx in range(a.warmup):
                rl = list(ref_host)
                if sidx:
                    rl[0] = prev
                rec, _, _ = test_frame.oracle_frame(oracle, frame, dst_host, rl, threads=min(64, os.cpu_count() or 1))
                _, _, want_res, want_grn = test_postchain.oracle_post(oracle, post, rec, w, h, bpc)
                prev = want_res
            got_res, got_grn = wl.outputs()
            for pl in range(3):
                vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
                if not np.array_equal(got_res[pl][:vh, :vw], want_res[pl][:vh, :vw]) or not np.array_equal(got_grn[pl][:vh, :vw], want_grn[pl][:vh, :vw]):
                    raise SystemExit("bench --config c4 --dependent: plane %d differs from the oracle's chain after %d steps" % (pl, a.warmup))
            parity = ("bit-exact vs %s oracle: restoration and film grain output of rank 0 after a chain of %d dependent steps (reference 0 of every step = "
                      "the picture rank - 1 broadcast one step earlier)" % (oracle.which, a.warmup))
        dd.barrier(world)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.warmup, a.warmup + a.steps):
            wl.step(arenas[i].data_ptr())
        torch.cuda.synchronize()
        dd.barrier(world)
        dt = dd.max_over_ranks(time.perf_counter() - t0, world, device=dev)
        if rank == 0 and a.dump_outputs:
            got_res, got_grn = wl.outputs()
            dump_outputs(a.dump_outputs, [("restored_" + c, p) for c, p in zip("yuv", visible(got_res, w, h))] +
                         [("grain_" + c, p) for c, p in zip("yuv", visible(got_grn, w, h))])
        if rank == 0 and a.full and not a.no_check and not a.dependent:
            # this rank's last frame against the oracle's replay of the same lists (independent frames: every step gives the same picture)
            import util
            import test_frame
            import test_postchain
            oracle = util.default_oracle()
            rec, _, _ = test_frame.oracle_frame(oracle, frame, dst_host, ref_host, threads=min(64, os.cpu_count() or 1))
            _, _, want_res, want_grn = test_postchain.oracle_post(oracle, post, rec, w, h, bpc)
            got_res, got_grn = wl.outputs()
            for pl in range(3):
                vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
                if not np.array_equal(got_res[pl][:vh, :vw], want_res[pl][:vh, :vw]) or not np.array_equal(got_grn[pl][:vh, :vw], want_grn[pl][:vh, :vw]):
                    raise SystemExit("bench --config c4: plane %d differs from the oracle" % pl)
            parity = "bit-exact vs %s oracle (restoration output and film grain output of rank 0's last frame)" % oracle.which
        line = None
        if rank == 0:
            P, Cb = (1, 2) if bpc == 8 else (2, 4)
            full_bytes = algorithmic_bytes(frame) + 8 * P * frame.n_samples        # + deblock, CDEF, restoration, grain: 2 P each
            ms = dt / a.steps * 1e3
            line = ({
                "metric": "reconstructed luma Mpixels/s (%dx%d 4:2:0 %d-bit), full DSP table + film grain, one frame per GPU per step" % (w, h, bpc),
                "value": round(dd.job_throughput(frame.luma_pixels, a.steps, dt, world) / 1e6, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": a.steps,
                "warmup": a.warmup, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "int32" if bpc > 8 else "int16", "data": "synthetic",
                "config": {"workload": "BASELINE configs[4]: %dx%d 4:2:0 %d-bit, recon list + deblock + CDEF + restoration + film grain on every rank's own frame; %s"
                                       % (w, h, bpc, "reference 0 = the picture of rank - 1 from the step before: every owner broadcasts its restored picture to all "
                                          "ranks after its step (one RCCL broadcast per owner)" if a.dependent else "independent frames (closed GOPs): no data-path collective"),
                           "parallelism": "frame-parallel x%d%s" % (world, ", dependent" if a.dependent else ""), "parity": parity},
                "roofline": {"bound": "hbm", "achieved": round(full_bytes / (ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(full_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                             "what": "whole step on algorithmic bytes (28 B per coded inter sample at 10 bits), wall clock incl. the host side of the batch calls"},
                "cpu_baseline": None})
        dd.barrier(world)
        return line

    # ---- device-resident state
    refs = []
    for rp in ref_host:
        r = ctx.picture(w, h, api.LAYOUT_I420, bpc)
        for pl in range(3):
            r.upload(pl, rp[pl])
        refs.append(r)
    tiled = a.layout == "tiled" and not tile_cols and not a.two_phase
    if tiled:
        for r in refs:
            r.retile()          # (a reference of a running chain was left in its twin by the frame that made it)
    NDST = 4
    dsts = []
    cols = dd.tile_columns(w, world) if tile_cols else None
    for _ in range(NDST):
        # tile-column mode: torch owns the picture memory so that RCCL can move the column strips
        d = dd.SharedPicture(ctx, w, h, api.LAYOUT_I420, bpc, dev) if tile_cols else ctx.picture(w, h, api.LAYOUT_I420, bpc)
        for pl in range(3):
            d.upload(pl, dst_host[pl])
        dsts.append(d)
    whole = frame
    if tile_cols:
        import copy
        mine = dd.tasks_by_column(frame.mc, frame.comp, frame.itx, [dsts[0].view.stride_px(pl) for pl in range(3)], cols)[rank]
        frame = copy.copy(whole)               # this rank's share of the lists; arenas and offsets stay the frame's
        frame.mc, frame.comp, frame.itx = whole.mc[mine[0]], whole.comp[mine[1]], whole.itx[mine[2]]
        frame.n_samples = int((np.asarray(synth.TX_W, np.int64)[frame.itx["tx"]] * np.asarray(synth.TX_H, np.int64)[frame.itx["tx"]]).sum())
    itx_tasks, coef_host = synth.pack_frame_coefs(frame) if a.packed else (frame.itx, frame.coef)
    inter_list, itx_list = ctx.inter_list(frame.mc, frame.comp), ctx.itx_list(itx_tasks)      # also used by the per-kernel timing below
    recon_list = None if a.two_phase else ctx.recon_list(dsts[0], frame.mc, frame.comp, itx_tasks)
    prep = torch.zeros(frame.prep_elems, dtype=torch.int16, device=dev)
    # frame contexts (dav1d's n_fc, src/lib.c:177-195: the frames a decoder has in flight): context k takes steps k, k + n_fc, ...; each has its
    # streams, its list and its compound scratch; the pictures and the references are the same memory for all of them
    n_fc = 1 if (a.emu or a.two_phase or tile_cols or recon_list is None) else max(1, a.frame_contexts)
    lanes = [(ctx, recon_list, prep, None)]
    for _ in range(n_fc - 1):
        st_k = torch.cuda.Stream(device=dev)
        ctx_k = api.Context(local, stream=st_k.cuda_stream)
        lanes.append((ctx_k, ctx_k.recon_list(dsts[0], frame.mc, frame.comp, itx_tasks), torch.zeros(frame.prep_elems, dtype=torch.int16, device=dev), st_k))
    tdt = torch.int16 if bpc == 8 else torch.int32
    pristine = torch.from_numpy(coef_host).to(dev)
    n_arena = a.steps + a.warmup + 8
    if not a.packed and not a.emu:
        # at most half the free device memory for the arenas: a smaller pool is refilled (untimed) whenever its arenas are all consumed,
        # and the timed steps run in chunks of what is left fresh (one chunk whenever the whole run fits, as the default does)
        fit = int(torch.cuda.mem_get_info()[0] * 0.5) // (pristine.numel() * pristine.element_size())
        n_arena = min(n_arena, max(a.warmup + 16, fit))
    if a.packed:        # a packed arena is read-only: every step reads the same one
        arenas = [pristine] * n_arena
    else:
        arenas = torch.empty((n_arena, pristine.numel()), dtype=tdt, device=dev)
        for i in range(n_arena):
            arenas[i].copy_(pristine)
    torch.cuda.synchronize()
    # what the boundary costs when the residuals arrive from the host every frame (reported next to `value`, never in it)
    h2d_ms = None
    if rank == 0 and a.full and not a.emu:
        pinned = torch.from_numpy(coef_host).pin_memory()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(3):
            e0.record()
            pristine.copy_(pinned, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        h2d_ms = round(best, 3)
        del pinned

    tc_post = None
    if tile_cols and a.tc_filters:
        # this rank's share of the frame's in-loop filter tasks (margins included) and the two extra pictures of the chain
        post_all = synth.make_post_filters(whole, seed=0xF11)
        lf_c, cdef_c, lr_c = dd.post_tasks_of_column(post_all.lf, post_all.cdef, post_all.lr,
                                                     [dsts[0].view.stride_px(pl) for pl in range(3)], cols[rank])
        tc_post = {"all": post_all, "lf": lf_c, "cdef": cdef_c, "lr": lr_c, "lvl": ctx.buffer_from(post_all.lvl),
                   "cdf": dd.SharedPicture(ctx, w, h, api.LAYOUT_I420, bpc, dev), "res": dd.SharedPicture(ctx, w, h, api.LAYOUT_I420, bpc, dev)}
    final_pic = {}

    def step(i):
        d = dsts[i % NDST]
        if recon_list is not None and tiled:
            _, rl_k, prep_k, _ = lanes[i % n_fc]
            rl_k.run_tiled(d, refs, prep_k.data_ptr(), arenas[i % n_arena].data_ptr())
        elif recon_list is not None:
            _, rl_k, prep_k, _ = lanes[i % n_fc]
            rl_k.run(d, refs, prep_k.data_ptr(), arenas[i % n_arena].data_ptr())
        else:
            ctx.run_inter_list(inter_list, d, refs, prep.data_ptr())
            ctx.run_itx_list(itx_list, d, arenas[i % n_arena].data_ptr())
        if tile_cols and tc_post is not None:
            dd.exchange_halo(d, cols, rank, world)       # enqueued on the context's stream behind the reconstruction (dav1d_hip_peer_exchange_halo)
            pa, cdf, res = tc_post["all"], tc_post["cdf"], tc_post["res"]
            ctx.lf_batch(d.view, tc_post["lf"], tc_post["lvl"], pa.b4_stride, pa.lut_e, pa.lut_i)
            # no picture copies under CDEF and restoration (round 4's frame path dropped them; this leg still made them with torch): the
            # column's own units and stripes are all listed — the strip kernel writes every listed unit, restoration every listed stripe —
            # and what lies outside the column is overwritten by the other ranks' strips when the gather lands
            ctx.cdef_batch(cdf.view, d.view, tc_post["cdef"], pa.cdef_damping)
            dd.wait_gathers(res, rank, world)                 # (one restoration picture: the gather of the frame before has to be through;
                                                              #  it ran next to this frame's reconstruction, deblocking and CDEF)
            ctx.lr_batch(res.view, cdf.view, d.view, tc_post["lr"])
            dd.allgather_tile_columns(res, cols, rank, world, overlap=True)
            final_pic[0] = res
        elif tile_cols:
            # on the peer's side stream: the next frame's reconstruction (other pictures) is enqueued before this gather completes; the
            # context's stream only waits for the gather of the picture it is about to overwrite (NDST frames back)
            dd.wait_gathers(d, rank, world, lag=NDST - 2)
            dd.allgather_tile_columns(d, cols, rank, world, overlap=True)

    # ---- parity gate on this very workload: frame `warmup-0` output vs the oracle replay (bounded: luma rows)
    check = "skipped"
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()

    def barrier():
        dd.barrier(world)

    barrier()
    torch.cuda.synchronize()
    dt, i, fresh = 0.0, a.warmup, n_arena - a.warmup
    while i < a.warmup + a.steps:
        if not fresh:
            for k in range(n_arena):
                arenas[k].copy_(pristine)
            torch.cuda.synchronize()
            barrier()
            fresh = n_arena
        j = min(a.warmup + a.steps, i + fresh)
        t0 = time.perf_counter()
        for k in range(i, j):
            step(k)
        torch.cuda.synchronize()
        barrier()
        dt += time.perf_counter() - t0
        fresh -= j - i
        i = j
    dt = dd.max_over_ranks(dt, world, device=dev)

    ms_per_step = dt / a.steps * 1e3
    # whole-job luma Mpixels/s: N frames per step (one per GPU) when sharded by frame, ONE frame per step over tile columns
    value = (whole.luma_pixels * a.steps / dt if tile_cols else dd.job_throughput(frame.luma_pixels, a.steps, dt, world)) / 1e6
    if rank == 0 and a.dump_outputs:
        last = final_pic[0] if tc_post is not None else dsts[(a.warmup + a.steps - 1) % NDST]
        dump_outputs(a.dump_outputs, [("picture_" + c, p) for c, p in zip("yuv", visible([last.download(pl) for pl in range(3)], w, h))])
    label = "8K" if (w, h) == (7680, 4320) else "4K" if (w, h) == (3840, 2160) else "%dx%d" % (w, h)
    metric = "reconstructed luma Mpixels/s (%s 4:2:0 %d-bit) on the itx+mc recon path; bit-exact vs C" % (label, bpc)
    scaling = "strong" if tile_cols else "weak"

    # ---- the same step fed with the sparse coefficient format (DAV1D_HIP_ITX_PACKED): reported next to `value`, which keeps
    # the dense reference layout SURVEY 8d prices; rank 0 of a one-GPU run only, and checked against the same oracle pictures
    if a.step_only:
        barrier()
        return {"step_only": True, "ms_per_step": round(ms_per_step, 4), "value": round(value, 1), "steps": a.steps, "warmup": a.warmup} if rank == 0 else None
    if not a.full:
        barrier()
        return {"metric": metric, "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
                "dtype": "int32" if bpc > 8 else "int16", "data": "synthetic",
                "config": {"frame_contexts": n_fc, "picture_layout": "tiled" if tiled else "raster", "parity": "not checked in this run (bench.py --full checks it)"},
                "roofline": None, "cpu_baseline": None} if rank == 0 else None
    if n_arena < a.warmup + a.steps + 8 and not a.packed:       # the legs below take arenas from the start of the pool again
        for k in range(n_arena):
            arenas[k].copy_(pristine)
        torch.cuda.synchronize()
    packed_leg = None
    if rank == 0 and world == 1 and not a.packed and not a.two_phase:
        p_tasks, p_coef = synth.pack_frame_coefs(frame)
        p_list = ctx.recon_list(dsts[0], frame.mc, frame.comp, p_tasks)
        p_arena = torch.from_numpy(p_coef).to(dev)
        p_run = p_list.run_tiled if tiled else p_list.run
        for i in range(a.warmup):
            p_run(dsts[i % NDST], refs, prep.data_ptr(), p_arena.data_ptr())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            p_run(dsts[i % NDST], refs, prep.data_ptr(), p_arena.data_ptr())
        torch.cuda.synchronize()
        dt_p = time.perf_counter() - t0
        p_out = [dsts[(a.steps - 1) % NDST].download(pl) for pl in range(3)]
        packed_leg = {"ms_per_step": round(dt_p / a.steps * 1e3, 4), "value": round(frame.luma_pixels * a.steps / dt_p / 1e6, 1),
                      "unit": "Mpixels/s", "coef_bytes_per_frame": int(p_coef.nbytes), "_pictures": p_out}
        p_list.destroy()
        del p_arena

    # ---- the same step with the pictures laid out the other ways, same box, same run (reported, never `value`): raster planes throughout
    # (the reference's layout, rounds 1-4) and raster destination + tiled references
    by_layout = None
    if rank == 0 and world == 1 and tiled and recon_list is not None and not a.packed and not a.emu and not os.environ.get("DAV1D_BENCH_CHILD") \
            and n_arena >= a.warmup + a.steps:
        by_layout = {"tiled": round(ms_per_step, 4)}
        alt = [ctx.picture(w, h, api.LAYOUT_I420, bpc) for _ in range(2)]
        for d in alt:
            for pl in range(3):
                d.upload(pl, dst_host[pl])
        for name, ref_twin in (("raster", 0), ("raster_destination_tiled_references", 1)):
            ctx.set_option("ref_twin", ref_twin)
            for k in range(a.warmup + a.steps):
                arenas[k].copy_(pristine)
            torch.cuda.synchronize()
            for k in range(a.warmup):
                recon_list.run(alt[k % 2], refs, prep.data_ptr(), arenas[k].data_ptr())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.warmup, a.warmup + a.steps):
                recon_list.run(alt[k % 2], refs, prep.data_ptr(), arenas[k].data_ptr())
            torch.cuda.synchronize()
            by_layout[name] = round((time.perf_counter() - t0) / a.steps * 1e3, 4)
        ctx.set_option("ref_twin", 1)
        for d in alt:
            d.free()

    out = None
    if rank == 0:
        # ---- per-kernel durations (HIP events on the launch stream), one instrumented step
        i = a.warmup + a.steps
        ms_mc = (C.c_float * 16)()
        cnt_mc = (C.c_size_t * 16)()
        ms_itx = (C.c_float * 19)()
        cnt_itx = (C.c_size_t * 19)()
        rarr = (api.Picture * len(refs))(*[r.pic for r in refs])
        d = dsts[i % NDST]
        # three instrumented passes (each on its own pristine arena), keep the per-kernel minimum:
        # the serial, event-bracketed launches are sensitive to clock ramps after an idle gap
        best_mc, best_itx = [1e9] * 16, [1e9] * 19
        for rep in range(3):
            rc = ctx.lib.dav1d_hip_inter_list_run_timed(ctx.h, inter_list.h, C.byref(d.pic), rarr, len(refs), prep.data_ptr(), None,
                                                        ms_mc, cnt_mc)
            assert rc == 0
            rc = ctx.lib.dav1d_hip_itx_list_run_timed(ctx.h, itx_list.h, C.byref(d.pic), arenas[(i + rep) % n_arena].data_ptr(), ms_itx, cnt_itx)
            assert rc == 0
            torch.cuda.synchronize()
            best_mc = [min(x, y) for x, y in zip(best_mc, ms_mc)]
            best_itx = [min(x, y) for x, y in zip(best_itx, ms_itx)]
        ms_mc, ms_itx = best_mc, best_itx
        i = i + 2
        P = 1 if bpc == 8 else 2
        Cb = 2 if bpc == 8 else 4
        kernels = []
        tile_w = [4, 8, 16, 32, 64]
        tile_h = [4, 8, 16]
        def cls_of(wv, hv):
            c = lambda v: np.where(v <= 4, 0, np.where(v <= 8, 1, np.where(v <= 16, 2, np.where(v <= 32, 3, 4))))
            return c(np.minimum(wv, 64)) * 3 + c(np.minimum(hv, 16))
        mc_bytes = np.zeros(15, np.int64)
        mpx = frame.mc["w"].astype(np.int64) * frame.mc["h"]
        np.add.at(mc_bytes, cls_of(frame.mc["w"], frame.mc["h"]), np.where(frame.mc["kind"] == 0, 2 * P, P) * mpx)
        if len(frame.comp):
            cpx = frame.comp["w"].astype(np.int64) * frame.comp["h"]
            np.add.at(mc_bytes, cls_of(frame.comp["w"], frame.comp["h"]), P * cpx)
        for b in range(15):
            if cnt_mc[b]:
                # algorithmic bytes: one P written per output pixel, one P read per predicted pixel
                # (tiles of fused compound blocks read two references: counted via the task lists below)
                kernels.append(("mc_%dx%d" % (tile_w[b // 3], tile_h[b % 3]), ms_mc[b], int(mc_bytes[b])))
        if cnt_mc[15]:
            kernels.append(("comp_unfused", ms_mc[15], 0))
        for b in range(19):
            if cnt_itx[b]:
                px = cnt_itx[b] * synth.TX_W[b] * synth.TX_H[b]
                cf = cnt_itx[b] * min(synth.TX_W[b], 32) * min(synth.TX_H[b], 32)
                kernels.append(("itx_%dx%d" % (synth.TX_W[b], synth.TX_H[b]), ms_itx[b], cf * 2 * Cb + px * 2 * P))
        kernels_two_phase = sorted(kernels, key=lambda k: -k[1])
        if recon_list is not None:
            # the launches the step really makes (paired prediction + residual kernels for some sizes, the rest as prediction
            # and residual launches), each on its own between events; algorithmic bytes: SURVEY 8d per sample
            ms40, cnt40 = (C.c_float * 40)(), (C.c_size_t * 40)()
            best40 = [1e9] * 40
            for rep in range(3):
                rarr = (api.Picture * len(refs))(*[r.pic for r in refs])
                fn = ctx.lib.dav1d_hip_recon_list_run_tiled_timed if tiled else ctx.lib.dav1d_hip_recon_list_run_timed
                rc = fn(ctx.h, recon_list.h, C.byref(d.pic), rarr, len(refs), prep.data_ptr(), None, arenas[(i + 3 + rep) % n_arena].data_ptr(), ms40, cnt40)
                assert rc == 0, rc
                best40 = [min(x, y) for x, y in zip(best40, ms40)]
            step_kernels = []
            for k in range(5):
                if cnt40[k]:
                    W_ = 4 << k
                    px = cnt40[k] * W_ * W_
                    cfs = cnt40[k] * min(W_, 32) ** 2
                    csel = (frame.comp["w"] == W_) & (frame.comp["h"] == W_) if len(frame.comp) else np.zeros(0, bool)
                    step_kernels.append(("recon_%dx%d" % (W_, W_), best40[k], int(px * 2 * P + cfs * 2 * Cb + int(csel.sum()) * W_ * W_ * P)))
            for b in range(15):
                if cnt40[5 + b] and cnt_mc[b]:
                    step_kernels.append(("mc_%dx%d" % (tile_w[b // 3], tile_h[b % 3]), best40[5 + b], int(mc_bytes[b] * cnt40[5 + b] / cnt_mc[b])))
            if cnt40[20]:
                step_kernels.append(("comp_unfused", best40[20], 0))
            for b in range(19):
                if cnt40[21 + b]:
                    px = cnt40[21 + b] * synth.TX_W[b] * synth.TX_H[b]
                    cfs = cnt40[21 + b] * min(synth.TX_W[b], 32) * min(synth.TX_H[b], 32)
                    step_kernels.append(("itx_%dx%d" % (synth.TX_W[b], synth.TX_H[b]), best40[21 + b], cfs * 2 * Cb + px * 2 * P))
            kernels = step_kernels
        kernels.sort(key=lambda k: -k[1])
        dom = kernels[0]
        if a.emu:
            kernels = [(k[0], max(k[1], 1e-6), k[2]) for k in kernels]       # the emulated events measure nothing
            dom = kernels[0]
        ach = dom[2] / (dom[1] * 1e-3) / 1e9
        path_bytes = algorithmic_bytes(frame)
        roof = {"bound": "hbm", "kernel": dom[0], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(dom[0], w, h, bpc),
                "kernel_ms": round(dom[1], 4), "algorithmic_bytes_per_launch": int(dom[2]),
                "path": {"algorithmic_bytes_per_frame": int(path_bytes),
                         "achieved": round(path_bytes / (ms_per_step * 1e-3) / 1e9, 1),
                         "frac": round(path_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                "kernels_ms": {k[0]: round(k[1], 4) for k in kernels},
                # every kernel of the step against the same roofline (algorithmic bytes of its launch / its time / peak): the
                # dominant one above is the longest, not the best or the worst
                "kernels_frac": {k[0]: round(k[2] / (k[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) for k in kernels if k[1] > 0 and k[2] > 0},
                "kernels_two_phase_ms": {k[0]: round(k[1], 4) for k in kernels_two_phase}}
        # measured HBM bytes of the whole step (sum of the committed per-kernel PMC figures) next to the algorithmic ones:
        # what the memory system really moved per frame, and the rate that is at this step time
        step_bytes = step_traffic(w, h, bpc, a)
        if step_bytes:
            roof["path"]["hbm_traffic_bytes_per_frame"] = int(step_bytes)
            roof["path"]["hbm_traffic_achieved"] = round(step_bytes / (ms_per_step * 1e-3) / 1e9, 1)
            roof["path"]["hbm_traffic_frac"] = round(step_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        # the dominant mc kernel's reads including the filter halo ((w + 7) x (h + 7) window per predicted block, which
        # random motion vectors cannot share between blocks): the floor of its fetch traffic on this workload
        if dom[0].startswith("mc_"):
            b = [k[0] for k in kernels].index(dom[0])
            tw_, th_ = (int(v) for v in dom[0][3:].split("x"))
            sel_m = (np.minimum(frame.mc["w"], 64) == tw_) & (np.minimum(frame.mc["h"], 16) == th_)
            n_tiles = int((((frame.mc["w"][sel_m].astype(np.int64) + tw_ - 1) // tw_) * ((frame.mc["h"][sel_m].astype(np.int64) + th_ - 1) // th_)).sum())
            roof["window_bytes_per_launch"] = int(n_tiles * (tw_ + 7) * (th_ + 7) * P + dom[2] // 2)
            roof["frac_incl_halo"] = round(roof["window_bytes_per_launch"] / (dom[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        if roof["traffic"]:
            roof["frac_measured_traffic"] = round(roof["traffic"] / (dom[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        # scalars next to the nested objects (a reader that keeps only flat values still sees the whole path and the 4x4 class)
        roof["path_frac"] = roof["path"]["frac"]
        roof["path_achieved"] = roof["path"]["achieved"]
        roof["path_ms"] = round(ms_per_step, 4)
        k44 = [k for k in kernels if k[0] in ("mc_4x4", "itx_4x4", "recon_4x4")]
        if k44:
            roof["class_4x4_frac"] = round(sum(k[2] for k in k44) / (sum(k[1] for k in k44) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            roof["class_4x4_ms"] = round(sum(k[1] for k in k44), 4)
        # where `traffic` comes from: PMC counters cannot be read from inside a run (rocprofv3 wraps the process), so the figure is the
        # committed pass of tools/pmc_profile.sh over this very command — the profile's own directory says which box and build it saw
        roof["traffic_source"] = "profiles/*/traffic.json (rocprofv3 --pmc FETCH_SIZE WRITE_SIZE over `bench.py --step-only`, FETCH_SIZE x 2 as calibrated in profiles/r02_calib_fetch_size.txt); not counted in this run"
        if world == 1 and not a.emu and not a.no_pmc and not tile_cols and not os.environ.get("DAV1D_BENCH_CHILD"):
            import re
            ct = counted_traffic(a)
            if "error" in ct:
                roof["traffic_source"] += "; counting it here failed: " + ct["error"]
            else:
                pat = _kernel_pattern(dom[0])
                hit = [v for k, v in ct["per_kernel"].items() if pat and re.search(pat, k)]
                roof["traffic"] = int(hit[0]) if hit else None
                roof["path_traffic"] = int(ct["per_step"])
                roof["path_traffic_over_algorithmic"] = round(ct["per_step"] / path_bytes, 3)
                if hit:
                    roof["frac_measured_traffic"] = round(hit[0] / (dom[1] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                    roof["traffic_over_algorithmic"] = round(hit[0] / dom[2], 3)
                roof["path"]["hbm_traffic_bytes_per_frame"] = int(ct["per_step"])
                roof["path"]["hbm_traffic_achieved"] = round(ct["per_step"] / (ms_per_step * 1e-3) / 1e9, 1)
                roof["path"]["hbm_traffic_frac"] = round(ct["per_step"] / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                roof["kernels_traffic"] = {}
                for kn in kernels:
                    kp = _kernel_pattern(kn[0])
                    hv = [v for k, v in ct["per_kernel"].items() if kp and re.search(kp, k)]
                    if hv:
                        roof["kernels_traffic"][kn[0]] = int(hv[0])
                roof["traffic_source"] = ("counted in this run on this box: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (one pass each) over "
                                          "`bench.py --step-only`, %d launches per kernel; HBM bytes = FETCH_SIZE x 2 (gfx950, profiles/r02_calib_fetch_size.txt) + WRITE_SIZE" % ct["launches"])

        # ---- parity gate + CPU baseline: the oracle replays the SAME lists on the host
        cpu = None
        if not a.no_cpu or not a.no_check:
            import util
            import test_frame
            oracle = util.default_oracle()
            reps, t_cpu = 0, 0.0
            want = None
            while True:
                tm = {}
                want = test_frame.oracle_frame(oracle, whole, dst_host, ref_host, timing=tm)
                t_cpu += tm["seconds"]
                reps += 1
                if a.no_cpu or t_cpu >= a.cpu_seconds or reps >= 8:
                    break
            if not a.no_check and tc_post is not None:
                # tile columns with in-loop filters: the gathered picture against the oracle's whole-frame chain
                import test_postchain
                _, _, r_, _ = test_postchain.oracle_post(oracle, tc_post["all"], want[0], w, h, bpc, with_grain=False)
                got = [final_pic[0].download(pl) for pl in range(3)]
                ok = all(np.array_equal(got[pl][:(h >> (pl > 0)), :(w >> (pl > 0))], r_[pl][:(h >> (pl > 0)), :(w >> (pl > 0))]) for pl in range(3))
                check = "bit-exact vs %s oracle after deblock + CDEF + restoration (gathered columns)" % oracle.which if ok else "MISMATCH"
                if not ok:
                    raise SystemExit("bench: the filtered tile columns differ from the oracle's whole-frame chain")
            elif not a.no_check:
                got = [dsts[i % NDST].download(pl) for pl in range(3)]
                ok = all(np.array_equal(got[pl], want[0][pl]) for pl in range(3))
                ok = ok and (a.packed or not bool(arenas[i % n_arena].any().item()))
                check = "bit-exact vs %s oracle (3 planes of the last frame)" % oracle.which if ok else "MISMATCH"
                if not ok:
                    raise SystemExit("bench: GPU output differs from the oracle")
                if packed_leg is not None:
                    if not all(np.array_equal(packed_leg["_pictures"][pl], want[0][pl]) for pl in range(3)):
                        raise SystemExit("bench: the packed-coefficient step differs from the oracle")
                    packed_leg["parity"] = "bit-exact vs %s oracle" % oracle.which
            cpu = {"value": round(frame.luma_pixels * reps / t_cpu / 1e6, 2), "unit": "Mpixels/s", "cores": 1,
                   "kind": "reference" if oracle.which == "ref" else "port",
                   "flags": util.REF_FLAGS if oracle.which == "ref" else "oracle/port: -O2",
                   "sample": "%d full %dx%d frame(s) of the same task lists through the oracle's C DSP entries, "
                             "1 thread, %.1f s" % (reps, w, h, t_cpu),
                   "host_cores_available": os.cpu_count()}
            if not a.no_cpu:
                # the same replay spread over the host's cores: a few thread counts, the best one is reported
                ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
                cands = sorted({c for c in (ncpu // 8, ncpu // 4, ncpu // 2, ncpu) if c > 1})
                tried, best, same = {}, None, True
                for nthr in cands:
                    reps_mt, t_mt = 0, 0.0
                    while t_mt < a.cpu_seconds / 12 and reps_mt < 8:
                        tm = {}
                        w_mt = test_frame.oracle_frame(oracle, whole, dst_host, ref_host, threads=nthr, timing=tm)
                        t_mt += tm["seconds"]
                        reps_mt += 1
                        if reps_mt == 1:
                            same = same and all(np.array_equal(w_mt[0][pl], want[0][pl]) for pl in range(3))
                    rate = frame.luma_pixels * reps_mt / t_mt / 1e6
                    tried[str(tm["threads"])] = round(rate, 1)
                    if best is None or rate > best[0]:
                        best = (rate, tm["threads"], reps_mt, t_mt)
                if best:
                    cpu["all_cores"] = {"value": round(best[0], 2), "unit": "Mpixels/s", "cores": best[1],
                                        "sample": "%d frame(s), %d threads over the task lists (barrier between mc / compound / itx), "
                                                  "%.1f s inside the replay" % (best[2], best[1], best[3]),
                                        "mpixels_per_s_by_threads": tried, "equals_one_thread": bool(same)}
        # ---- the reference itself as the CPU peer: its own pass 2 (dav1d_decode_tile_sbrow, C DSP functions) on the same kind of
        # frame from hand-off arrays, tiles on a pool of workers (oracle/ref_frame.c dav1d_ref_frame_recon_mt); and whether the
        # assembly path could have been built here
        if cpu is not None and not a.no_cpu and rank == 0 and world == 1:
            import shutil
            import lister_util as lu
            try:
                ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
                thr = sorted({t for t in (1, 16, 32, 64, 128) if t <= max(1, ncpu)})
                rates = lu.reference_pass2_rate(ctx, w, h, bpc, 16, 8, threads=thr)
                if rates:
                    bt = max(rates, key=lambda k: rates[k])
                    cpu["reference_pass2"] = {"value": rates[bt], "unit": "Mpixels/s", "cores": int(bt), "kind": "reference",
                                              "sample": "1 frame per thread count, %dx%d %d-bit inter frame in 16 x 8 tiles, the reference's "
                                                        "dav1d_decode_tile_sbrow (pass 2, C DSP) with one worker per tile in flight" % (w, h, bpc),
                                              "mpixels_per_s_by_threads": {str(k): v for k, v in rates.items()}}
            except Exception as e:       # the peer is a reported baseline, never a reason to lose the line
                cpu["reference_pass2"] = {"error": str(e)[:200]}
            cpu["avx2"] = ("unavailable: no nasm on this host (the reference's src/x86/*.asm cannot be assembled; SURVEY 8c)"
                           if shutil.which("nasm") is None else
                           "nasm present but the assembly build is not wired up (oracle/Makefile builds the C path only)")
        # ---- full DSP table on the same frame (BASELINE configs[2]): recon above + deblock + CDEF + restoration + grain,
        # one frame, kernel time per stage from HIP events, every stage checked against the oracle's replay
        full = None
        if not a.no_full and not tile_cols:      # the post filters cross tile edges: their halo exchange is a later row
            import test_postchain
            post = synth.make_post_filters(frame, seed=0xF11 + rank)
            intra = synth.make_intra_pass(frame, seed=0x1A7 + rank)
            want_post, t_post_cpu = [None] * 4, 0.0
            if a.no_check:
                got = [dsts[i % NDST].download(pl) for pl in range(3)]
            # intra pass (1/9 of the regions re-coded as intra, wavefront batches) on the reconstructed picture
            rec = ctx.picture(w, h, api.LAYOUT_I420, bpc)
            rec0 = [np.array(g, copy=True) for g in got]
            for pl in range(3):
                rec.upload(pl, got[pl])
            rec2 = ctx.picture(w, h, api.LAYOUT_I420, bpc)
            for pl in range(3):
                rec2.upload(pl, got[pl])
            # the chain of ~200 small dependent launches twice: enqueued launch by launch, and recorded once + replayed as a
            # HIP graph (dav1d_hip_graph_*); both must give the same picture, the faster one is the stage time
            ms_intra_plain = test_postchain.hip_intra(ctx, intra, rec2, timed=True)
            ms_intra_graph = test_postchain.hip_intra(ctx, intra, rec, timed=True, graph=True)
            got = [rec.download(pl) for pl in range(3)]
            if not all(np.array_equal(got[pl], rec2.download(pl)) for pl in range(3)):
                raise SystemExit("bench: graph replay of the intra pass differs from the enqueued launches")
            # ... and superblock by superblock (dav1d_hip_intra_sb_*: a workgroup per superblock, a launch per level): what a frame of
            # the driver-level API runs by default
            for pl in range(3):
                rec2.upload(pl, rec0[pl])
            test_postchain.hip_intra(ctx, intra, rec2, timed=True, sb=True)       # warm-up (first use of the kernel)
            for pl in range(3):
                rec2.upload(pl, rec0[pl])
            ms_intra_sb = test_postchain.hip_intra(ctx, intra, rec2, timed=True, sb=True)
            if not all(np.array_equal(got[pl], rec2.download(pl)) for pl in range(3)):
                raise SystemExit("bench: the superblock route of the intra pass differs from the launches per step")
            ms_intra = min(ms_intra_plain, ms_intra_graph, ms_intra_sb)
            rec.free()
            rec2.free()
            intra_ok = None
            if not a.no_check:
                t1 = time.perf_counter()
                want_rec = synth.copy_planes(want[0])
                test_postchain.oracle_intra(oracle, intra, want_rec, w, h, bpc)
                intra_ok = all(np.array_equal(got[pl], want_rec[pl]) for pl in range(3))
                if not intra_ok:
                    raise SystemExit("bench: intra pass differs from the oracle")
                want_post = test_postchain.oracle_post(oracle, post, want_rec, w, h, bpc)
                t_post_cpu = time.perf_counter() - t1
            pics = [ctx.picture(w, h, api.LAYOUT_I420, bpc) for _ in range(4)]
            dbl, cdf, res, grn = pics
            for pl in range(3):
                dbl.upload(pl, got[pl])
            lvl = ctx.buffer_from(post.lvl)
            stage_ms = {"intra_waves": ms_intra}
            # the grain templates depend on the frame header only: their generation is enqueued here, on a side stream, the way
            # dav1d_hip_frame_set_filters does it at frame start; the film grain stage below then times the application proper
            grain_handle = ctx.fg_prepare(post.fg, bpc, api.LAYOUT_I420) if post.fg is not None else None
            for rep in range(2):            # second pass = warm clocks; deblocking is in place, so re-seed its input
                for pl in range(3):
                    dbl.upload(pl, got[pl])
                ctx.lf_batch(dbl, post.lf, lvl, post.b4_stride, post.lut_e, post.lut_i)
                stage_ms["deblock"] = ctx.last_kernel_ms()
                ctx.cdef_batch(cdf, dbl, post.cdef, post.cdef_damping)
                stage_ms["cdef"] = ctx.last_kernel_ms()
                ctx.lr_batch(res, cdf, dbl, post.lr)
                stage_ms["restoration"] = ctx.last_kernel_ms()
                if rep == 0:
                    ctx.fg_apply(grn, res, post.fg)                                   # templates + application back to back
                    fg_one_call_ms = ctx.last_kernel_ms()
                else:
                    ctx.fg_apply_prepared(grn, res, grain_handle)
                    stage_ms["film_grain"] = ctx.last_kernel_ms()
            names = ["deblock", "cdef", "restoration", "film_grain"]
            okp = True
            for pic, wantp, nm in zip(pics, want_post, names):
                if wantp is None:
                    continue
                for pl in range(3):
                    vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
                    if not np.array_equal(pic.download(pl)[:vh, :vw], wantp[pl][:vh, :vw]):
                        okp = False
                        print("bench: full-table stage %s plane %d differs from the oracle" % (nm, pl), file=sys.stderr)
            if not okp:
                raise SystemExit("bench: full-table GPU output differs from the oracle")
            # deblock -> CDEF -> restoration once more through the driver-level API, which pipelines the three stages over
            # bands of superblock rows on three streams (dav1d_hip_frame_*): device time of that section, same pictures
            post_piped = None
            for pl in range(3):
                dbl.upload(pl, got[pl])
            fr = ctx.frame(dbl, [])
            fr.set_filters(lvl, post.b4_stride, post.lut_e, post.lut_i, post.cdef_damping, None, 0)
            fr.submit_filter_sbrow(post.lf, post.cdef, post.lr)
            ctx.set_option("post_bands", int(os.environ.get("DAV1D_HIP_POST_BANDS", "4")))     # off by default in the library
            filt = fr.end(None, None, None, None)
            ctx.set_option("post_bands", 0)
            if fr.post_bands():
                fo = api.DevicePicture.view(ctx, filt, w, h, api.LAYOUT_I420, bpc)
                for pl in range(3):
                    vh, vw = (h, w) if pl == 0 else (h // 2, w // 2)
                    if not np.array_equal(fo.download(pl)[:vh, :vw], res.download(pl)[:vh, :vw]):
                        raise SystemExit("bench: the band-pipelined post filters differ from the stage-by-stage result (plane %d)" % pl)
                post_piped = {"ms": round(ctx.last_kernel_ms(), 4), "bands": fr.post_bands(),
                              "stage_by_stage_ms": round(stage_ms["deblock"] + stage_ms["cdef"] + stage_ms["restoration"], 4)}
            fr.destroy()
            in_flight = None
            if not a.no_inflight and rank == 0 and world == 1 and not a.packed:
                res_host = [res.download(pl) for pl in range(3)]
                try:
                    in_flight = frames_in_flight(api, local, frame, itx_tasks, coef_host, intra, post, ref_host, dst_host, w, h, bpc, res_host)
                except SystemExit:
                    raise
                except Exception as e:       # noqa: BLE001  (a reported extra, never a reason to lose the line)
                    in_flight = {"error": str(e)[:200]}
                del res_host
            if grain_handle is not None:
                ctx.fg_grain_destroy(grain_handle)
            for o in pics + [lvl]:
                o.free()
            P = 1 if bpc == 8 else 2
            post_ms = sum(stage_ms.values())
            if post_piped and post_piped["ms"] < post_piped["stage_by_stage_ms"]:      # the frame counts the faster of the two
                post_ms -= post_piped["stage_by_stage_ms"] - post_piped["ms"]
            # a frame WITH an intra pass and in-loop filters reconstructs into raster planes (those stages read and write them; only the
            # frame's references are read through their twins): its reconstruction stage is the step timed that way in this run, not the
            # tiled-only headline step
            recon_ms = (by_layout or {}).get("raster_destination_tiled_references") or ms_per_step
            full_ms = recon_ms + post_ms
            Cb = 2 if bpc == 8 else 4
            # each post filter: one read + one write per sample; intra samples: coefficients + prediction write + residual RMW
            full_bytes = path_bytes + frame.n_samples * 2 * P * 4 + intra.n_samples * (2 * Cb + 3 * P)
            full = {"workload": "same frame through the full DSP table: itx+mc recon, intra pass (1/9 of the 64x64 regions re-coded as intra, "
                                "%d wavefront batches of prediction + residual), deblock (levels 16-32, masks from the transform grid), " % len(intra.batches) +
                                "CDEF (y 17 / uv 5, every 8x8), Wiener Y + SGR-mix UV (64-px units), film grain (lag 3, overlap)",
                    "ms_per_frame": round(full_ms, 4), "value": round(frame.luma_pixels / (full_ms * 1e-3) / 1e6, 1), "unit": "Mpixels/s",
                    "stages_ms": dict({"recon_itx_mc": round(recon_ms, 4)}, **{k: round(v, 4) for k, v in stage_ms.items()}),
                    "recon_stage": "raster destination, tiled references (the intra pass and the filters work on raster planes)" if recon_ms != ms_per_step else "the headline step",
                    "film_grain_modes_ms": {"templates_then_apply_in_one_call": round(fg_one_call_ms, 4),
                                            "apply_with_templates_prepared_on_a_side_stream": round(stage_ms["film_grain"], 4)},
                    "post_filters_pipelined": post_piped,
                    # wall clock per frame, everything included, with 1, 2, 4 and 8 frames in flight on this GPU (one context and host
                    # thread per frame, the way dav1d's frame threading would drive the backend); ms_per_frame above is the sum of
                    # the stages' device times of ONE frame
                    "wall_ms_per_frame_by_frames_in_flight": in_flight,
                    "intra_launch_modes_ms": {"enqueued": round(ms_intra_plain, 4), "graph_replay": round(ms_intra_graph, 4),
                                              "graph_nodes": int(test_postchain.hip_intra.last_nodes), "wavefront_steps": len(intra.batches),
                                              "superblocks": round(ms_intra_sb, 4), "superblock_levels": int(test_postchain.hip_intra.sb_levels),
                                              "superblocks_with_intra_units": int(test_postchain.hip_intra.sb_superblocks)},
                    "tasks": {"ipred": intra.n_blocks, "lf": int(len(post.lf)), "cdef": int(len(post.cdef)), "lr": int(len(post.lr))},
                    "algorithmic_bytes_per_frame": int(full_bytes),
                    "achieved": round(full_bytes / (full_ms * 1e-3) / 1e9, 1), "frac": round(full_bytes / (full_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "parity": "skipped" if a.no_check else "every stage bit-exact vs %s oracle" % oracle.which,
                    "cpu_post_filters_s": round(t_post_cpu, 2)}
        # ---- end to end: the same kind of frame from dav1d's pass-1 hand-off arrays (Av1Block / cbi / cf) through the pass-2
        # lister on host threads, the chunk preparation, the coefficient upload and frame_end; checked against the reference's OWN
        # pass 2 (dav1d_decode_tile_sbrow on a real Dav1dFrameContext, oracle/ref_frame.c) when the reference build is there
        e2e_leg = key_leg = full_route = e2e_packed = key_packed = None
        if world == 1 and not a.no_e2e:
            import e2e

            def e2e_check(ho, planes, ref_pics, is_inter=True):
                import lister_util as lu
                try:
                    return lu.check_handoff_against_reference(ho, planes, ref_pics, is_inter)
                except AssertionError as e:
                    raise SystemExit("bench: end-to-end leg differs from the reference's pass 2: %s" % e)
            e2e_leg = e2e.run(ctx, w, h, bpc, frames=6, threads=a.e2e_threads or None, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows,
                              check=None if a.no_check else e2e_check)
            # the key-frame worst case (reference src/recon_tmpl.c:1239-1333, every block through the intra wavefront): same route
            key_leg = e2e.run(ctx, w, h, bpc, frames=4, threads=a.e2e_threads or None, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows, key_frame=True, seed=0xE2F,
                              check=None if a.no_check else (lambda ho, planes, refs: e2e_check(ho, planes, refs, is_inter=False)))
            # the same two legs through the PACKING lister (Dav1dHipFrameDesc.cf: eob + 1 values per block into the frame's own arena; what
            # INTEGRATION.md recommends and the frames-in-flight legs below use): the 200 MB dense upload is gone from the frame's time
            e2e_packed = e2e.run(ctx, w, h, bpc, frames=5, threads=a.e2e_threads or None, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows, packed=True,
                                 check=None if a.no_check else e2e_check)
            key_packed = e2e.run(ctx, w, h, bpc, frames=4, threads=a.e2e_threads or None, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows, key_frame=True,
                                 seed=0xE2F, packed=True, check=None if a.no_check else (lambda ho, planes, refs: e2e_check(ho, planes, refs, is_inter=False)))
            # the whole frame — reconstruction AND in-loop filters — from pass 1's outputs, checked against the reference's own
            # dav1d_decode_tile_sbrow + dav1d_filter_sbrow (needs the reference build oracle/_ref for the filter inputs and the check)
            if not a.no_check:
                import lister_util as lu
                try:
                    full_route = lu.full_route_rate(ctx, w, h, bpc, a.e2e_tile_cols, a.e2e_tile_rows, threads=a.e2e_threads or 64, frames=5)
                except AssertionError as e:
                    raise SystemExit("bench: full end-to-end leg differs from the reference: %s" % e)
                except Exception as e:       # noqa: BLE001  (a reported extra)
                    full_route = {"error": str(e)[:200]}
        # ---- splat_mv / save_tmvs of the frame's blocks on a frame-level refmvs map (csrc/refmvs.hip; bit-exact against the
        # reference's functions in tests/test_refmvs.py).  Timed, not wired into a decode loop: pass 1 needs the rows on the host for its own
        # motion vector prediction, so the device copy would be a second splat, not a saved one.
        refmvs_leg = None
        if world == 1 and not a.no_full and (w, h, bpc) == (7680, 4320, 10):
            try:
                SPLAT = np.dtype([("bx4", "<u2"), ("by4", "<u2"), ("bw4", "u1"), ("bh4", "u1"), ("pad", "u1", 2), ("rmv", "<u4", 3)])
                ystride = ctx.picture(w, h, api.LAYOUT_I420, bpc)
                sp_px = ystride.pic.p[0].stride // 2
                ystride.free()
                blk = [(t["dst_off"], t["w"], t["h"]) for t in (frame.mc[(frame.mc["plane"] == 0) & (frame.mc["kind"] == 0)], frame.comp[frame.comp["plane"] == 0])]
                off = np.concatenate([b[0] for b in blk]).astype(np.int64)
                bw = np.concatenate([b[1] for b in blk]).astype(np.int64)
                bh = np.concatenate([b[2] for b in blk]).astype(np.int64)
                tasks = np.zeros(len(off), SPLAT)
                tasks["bx4"], tasks["by4"] = (off % sp_px) // 4, (off // sp_px) // 4
                tasks["bw4"], tasks["bh4"] = np.minimum(bw // 4, 32), np.minimum(bh // 4, 32)
                rgen = np.random.default_rng(3)
                tasks["rmv"][:, 0] = rgen.integers(0, 1 << 32, len(off), dtype=np.uint64).astype(np.uint32) & 0x03ff03ff
                tasks["rmv"][:, 2] = 1 | (0xff << 8) | (12 << 16)
                stride4, h4 = (w + 127) // 128 * 32, (h + 127) // 128 * 32
                rmap = ctx.buffer(stride4 * h4 * 12)
                rmap.zero()
                rp_stride = ((w + 127) & ~127) >> 3
                rp = ctx.buffer(rp_stride * (h // 8) * 5 + 64)
                sign = np.array([1, 0, 1, 1, 0, 1, 0], np.uint8)
                ms = []
                for _ in range(4):
                    ctx.sync()
                    t0 = time.perf_counter()
                    assert ctx.lib.dav1d_hip_refmvs_splat_batch(ctx.h, rmap.ptr, stride4, tasks.ctypes.data, len(tasks)) == 0
                    ctx.sync()
                    t1 = time.perf_counter()
                    assert ctx.lib.dav1d_hip_refmvs_save_tmvs(ctx.h, rp.ptr, rp_stride, rmap.ptr, stride4, sign.ctypes.data, 0, w // 8, 0, h // 8) == 0
                    ctx.sync()
                    ms.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
                refmvs_leg = {"blocks": int(len(tasks)), "splat_ms_with_task_upload": round(min(m[0] for m in ms), 3), "save_tmvs_ms": round(min(m[1] for m in ms), 3),
                              "map_bytes": int(stride4 * h4 * 12), "parity": "tests/test_refmvs.py (bit-exact vs the reference's splat_mv / save_tmvs)"}
                rmap.free()
                rp.free()
            except Exception as e:       # noqa: BLE001  (a reported extra)
                refmvs_leg = {"error": str(e)[:200]}
        # ---- row-granular progress (reference src/thread_task.c:888-896 publishes per superblock row): what a listener costs
        row_progress = None
        if world == 1 and not a.no_e2e and not a.no_check:
            try:
                import lister_util as lu
                row_progress = lu.row_progress_cost(ctx, w, h, bpc, a.e2e_tile_cols, a.e2e_tile_rows, threads=a.e2e_threads or 64)
            except AssertionError as e:
                raise SystemExit("bench: row progress leg differs from the reference: %s" % e)
            except Exception as e:       # noqa: BLE001
                row_progress = {"error": str(e)[:200]}
        # ---- BASELINE configs[2] says 4 tile columns: the end-to-end legs again with the frame cut that way (a tile's superblock rows are
        # listed top to bottom, so 4 tiles are 4 listing threads), next to the many-tile runs above
        e2e_c2 = full_route_c2 = None
        if world == 1 and not a.no_e2e:
            import e2e
            e2e_c2 = e2e.run(ctx, w, h, bpc, frames=4, threads=4, tile_cols=4, tile_rows=1, check=None if a.no_check else e2e_check)
            if not a.no_check:
                import lister_util as lu
                try:
                    full_route_c2 = lu.full_route_rate(ctx, w, h, bpc, 4, 1, threads=4, frames=4)
                except AssertionError as e:
                    raise SystemExit("bench: full end-to-end leg (4 tile columns) differs from the reference: %s" % e)
                except Exception as e:       # noqa: BLE001
                    full_route_c2 = {"error": str(e)[:200]}
        # ---- frames in flight (round 3): frame n + 1 is listed while frame n runs on the device, the packing lister sends the
        # coefficients that exist instead of the dense arena.  ms_per_frame = sustained over the frames after the warm-up.
        sustained = None
        if world == 1 and not a.no_e2e:
            import e2e
            sustained = {}
            try:
                # paced: as many listing threads as the container's CPU quota sustains (e2e.host_threads), 24 frames; burst: 64 threads over 16
                # frames, which fits the quota's 100 ms period — what a host without the quota would sustain
                sustained["recon"] = e2e.run_sustained(ctx, w, h, bpc, frames=24, threads=None, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows,
                                                       check=None if a.no_check else e2e_check)
                sustained["recon_burst_64_threads"] = e2e.run_sustained(ctx, w, h, bpc, frames=16, threads=64, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows)
                # key frames the same way: the listing of frame n + 1 under the superblock launch of frame n
                sustained["all_intra"] = e2e.run_sustained(ctx, w, h, bpc, frames=8, threads=64, tile_cols=a.e2e_tile_cols, tile_rows=a.e2e_tile_rows, seed=0xE2F,
                                                           key_frame=True, check=None if a.no_check else (lambda ho, planes, refs: e2e_check(ho, planes, refs, is_inter=False)))
                sustained["recon_4_tile_columns"] = e2e.run_sustained(ctx, w, h, bpc, frames=6, threads=4, tile_cols=4, tile_rows=1,
                                                                      check=None if a.no_check else e2e_check)
                if not a.no_check:
                    import lister_util as lu
                    sustained["full_table"] = lu.full_route_sustained(ctx, w, h, bpc, a.e2e_tile_cols, a.e2e_tile_rows, threads=None, frames=24)
                    sustained["full_table_burst_64_threads"] = lu.full_route_sustained(ctx, w, h, bpc, a.e2e_tile_cols, a.e2e_tile_rows, threads=64, frames=16)
                    sustained["full_table_4_tile_columns"] = lu.full_route_sustained(ctx, w, h, bpc, 4, 1, threads=4, frames=6)
            except AssertionError as e:
                raise SystemExit("bench: frames-in-flight leg differs from the reference: %s" % e)
            except Exception as e:       # noqa: BLE001  (a reported extra)
                sustained["error"] = str(e)[:200]
        # ---- BASELINE configs[0]: 1080p 8-bit on ONE host thread (the reference C), and the same reference code with the HIP DSP table
        c0 = None
        if world == 1 and not a.no_cpu and not a.no_check and (w, h, bpc) == (7680, 4320, 10):
            try:
                import lister_util as lu
                c0 = lu.c0_line(ctx, strict=False)        # a bring-up path, reported: the line says so if the pictures ever differ
            except AssertionError as e:
                raise SystemExit("bench: %s" % e)
            except Exception as e:       # noqa: BLE001
                c0 = {"error": str(e)[:200]}
        # ---- the backend inside dav1d's OWN task loop (oracle/_ref_hooked: the reference with src/thread_task.c patched at the hook
        # points of INTEGRATION.md 2; dav1d_open, dav1d_submit_frame, the worker threads, check_tile, dav1d_get_picture are dav1d's):
        # a chain of dependent 8K frames at BASELINE configs[2]'s 4 tile columns, every picture checked against dav1d's own pass 2 +
        # filters under the same loop
        task_loop = None
        if world == 1 and not a.no_e2e and not a.no_check:
            try:
                import hooked_util as hk
                from dav1d_amd import _lib as _l
                if hk.lib() is None:
                    task_loop = {"status": "skipped: oracle/_ref_hooked is not built (needs /root/reference at build time)"}
                else:
                    ctx.sync()
                    task_loop = hk.task_loop_rate(_l.DEFAULT_PATH, w, h, bpc, tiles=(4, 1), threads=min(64, os.cpu_count() or 8), frame_delay=8, frames=24)
            except AssertionError as e:
                raise SystemExit("bench: the dav1d task loop leg differs from dav1d's own pass 2 + filters: %s" % e)
            except Exception as e:       # noqa: BLE001  (a reported extra)
                task_loop = {"error": str(e)[:200]}
        # ---- ... and behind dav1d's REAL pass 1: an AV1 stream (tests/av1_obu.py: real headers, every tool, random tile payloads) through
        # dav1d_send_data / dav1d_parse_obus / msac / decode_b unmodified; EVERY picture of the chain compared with dav1d's own
        task_loop_stream = None
        if world == 1 and not a.no_e2e and not a.no_check:
            try:
                import stream_util as sut
                from dav1d_amd import _lib as _l
                if sut.lib() is None:
                    task_loop_stream = {"status": "skipped: oracle/_ref_hooked is not built (needs /root/reference at build time)"}
                else:
                    ctx.sync()
                    task_loop_stream = sut.task_loop_rate(_l.DEFAULT_PATH, w, h, bpc, tiles_log2=(2, 0), threads=min(64, os.cpu_count() or 8), frame_delay=8,
                                                          frames=a.stream_frames)
                    # the same with every segment pinned to a reference frame (random payloads otherwise make three quarters of the blocks
                    # intra, and the frame waits for the intra wavefront): more of the stream is motion compensation
                    try:
                        pinned = sut.task_loop_rate(_l.DEFAULT_PATH, w, h, bpc, tiles_log2=(2, 0), threads=min(64, os.cpu_count() or 8), frame_delay=8,
                                                    frames=a.stream_frames, seg_pin=1)
                        task_loop_stream["segments_pinned"] = {k: pinned.get(k) for k in ("steady_state", "peer_steady_state", "fps", "peer_fps", "parity")}
                        t = pinned.get("tools_in_the_stream") or {}
                        task_loop_stream["segments_pinned"]["blocks_intra_inter"] = [t.get("b_intra"), t.get("b_inter")]
                    except AssertionError:
                        raise
                    except Exception as e:       # noqa: BLE001
                        task_loop_stream["segments_pinned"] = {"error": str(e)[:200]}
            except AssertionError as e:
                raise SystemExit("bench: the dav1d task loop leg behind dav1d's real pass 1 differs from dav1d: %s" % e)
            except Exception as e:       # noqa: BLE001  (a reported extra)
                task_loop_stream = {"error": str(e)[:200]}
        if full is not None and isinstance(full, dict):
            for kk in ("ms_per_frame", "frac", "achieved"):
                if kk in full:
                    roof["full_table_" + kk] = full[kk]
        if cpu is not None:
            if isinstance(cpu.get("all_cores"), dict):
                cpu["all_cores_value"], cpu["all_cores_cores"] = cpu["all_cores"].get("value"), cpu["all_cores"].get("cores")
            if isinstance(cpu.get("reference_pass2"), dict) and "value" in cpu["reference_pass2"]:
                cpu["reference_pass2_value"], cpu["reference_pass2_cores"] = cpu["reference_pass2"]["value"], cpu["reference_pass2"]["cores"]
        out = {"metric": metric,
               "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
               "dtype": "int32" if bpc > 8 else "int16", "data": "synthetic",
               "config": {"workload": ("%dx%d 4:2:0 %d-bit inter frame, itx+mc recon (SURVEY §8d C1 spec: every block 16x16, TX_16X16 luma / TX_8X8 "
                                       "chroma, single reference, all blocks coded, 3 refs); lists resident in HBM" if a.mix == "c1" else
                                       "%dx%d 4:2:0 %d-bit inter frame, itx+mc recon (SURVEY §8d C2 mix 64/32/16/8/4 = "
                                       "20/30/30/15/5 %% by area, 25 %% compound avg, all blocks coded, 3 refs); "
                                       "lists resident in HBM") % (w, h, bpc),
                          "step": ("inter list, then itx list" if a.two_phase else
                                   "recon list: residual launches wait only for the prediction launches under their blocks (2 streams)"),
                          "picture_layout": ("tiled: references read through 8x8-tiled twins, the reconstructed picture written as tiles only (one 128-byte line per 8x8 "
                                             "block at 10 bits); raster rows are made by the un-tiling download the parity check reads" if tiled else "raster planes (src/picture.c:46-63)"),
                          "ms_per_step_by_layout": by_layout,
                          "frames_per_step": 1, "frame_contexts": n_fc, "parallelism": (("tile-columns x%d, in-loop filters per column after a 16-column halo exchange, one all-gather of the filtered columns per frame"
                                                            if a.tc_filters else "tile-columns x%d + one all-gather per frame") if tile_cols else "frame-parallel x%d" + (", %d frame contexts per GPU (independent frames in flight, like dav1d's n_fc)" % n_fc if n_fc > 1 else "")) % world,
                          "tasks": {"mc": int(len(frame.mc)), "comp": int(len(frame.comp)), "itx": int(len(frame.itx))},
                          "coef_format": "packed: eob + 1 scan-order values per block" if a.packed else "dense cf arena (reference layout)",
                          "coef_bytes_per_frame": int(coef_host.nbytes), "coef_h2d_ms_per_frame": h2d_ms,
                          "samples_per_frame": frame.n_samples, "parity": check, "gen_seconds": round(t_gen, 1)},
               "roofline": roof, "cpu_baseline": cpu, "full_table": full, "end_to_end": e2e_leg, "all_intra": key_leg, "end_to_end_packing_lister": e2e_packed, "all_intra_packing_lister": key_packed, "end_to_end_full_table": full_route, "end_to_end_4_tile_columns": e2e_c2, "end_to_end_full_table_4_tile_columns": full_route_c2,
               "end_to_end_frames_in_flight": sustained, "row_progress": row_progress, "refmvs": refmvs_leg, "dav1d_task_loop": task_loop, "dav1d_task_loop_real_pass1": task_loop_stream, "config_c0_1080p_8bit": c0,
               "device": None if a.no_check else device_probe(torch)}       # (not under the profiler: its copies would sit in the kernel statistics)
        # BASELINE configs[1] (4K 8-bit, the reference's CPU-runnable size) next to the headline: the same bench in a child process,
        # its digest under "config_c1_4k_8bit"
        if world == 1 and not a.no_c1 and not a.step_only and (w, h, bpc) == (7680, 4320, 10):
            import subprocess
            for key, mix in (("config_c1_4k_8bit", "c1"), ("config_c1_4k_8bit_c2_mix", "c2")):
                try:
                    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--full", "--width", "3840", "--height", "2160", "--bpc", "8", "--no-c1", "--mix", mix,
                                            "--no-full", "--no-e2e", "--no-cpu", "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                           capture_output=True, text=True, timeout=600)
                    cj = json.loads(child.stdout.strip().splitlines()[-1])
                    out[key] = {"metric": cj["metric"], "value": cj["value"], "unit": cj["unit"], "ms_per_step": cj["ms_per_step"],
                                "dtype": cj["dtype"], "roofline": {k: cj["roofline"].get(k) for k in ("kernel", "frac", "path_frac", "path_achieved")},
                                "parity": cj["config"]["parity"], "workload": cj["config"]["workload"]}
                except Exception as e:
                    out[key] = {"error": str(e)[:200]}
        # $DAV1D_STREAMS: real AV1 streams on the GPU box.  Decoding one needs dav1d's pass 1 (OBU parsing + entropy
        # decoding), which stays in dav1d by design and is not built here; the hook reports what it found
        sdir = os.environ.get("DAV1D_STREAMS")
        if sdir:
            import glob
            import shutil
            files = sorted(glob.glob(os.path.join(sdir, "**", "*.ivf"), recursive=True) + glob.glob(os.path.join(sdir, "**", "*.obu"), recursive=True))
            out["streams"] = {"dir": sdir, "files": len(files), "dav1d_cli": shutil.which("dav1d"),
                              "status": "not run: stream-level md5 / fps / argon need a dav1d build bound to libdav1d_hip (INTEGRATION.md); "
                                        "this repository holds the pass-2 backend and its hand-off, not pass 1"}
        else:
            out["streams"] = {"status": "no $DAV1D_STREAMS supplied"}
        if packed_leg is not None:
            packed_leg.pop("_pictures", None)
            packed_leg.setdefault("parity", "skipped")
            out["packed_coefficients"] = packed_leg
    barrier()
    return out


if __name__ == "__main__":
    main()
