#!/usr/bin/env python3
"""Register / LDS / scratch budget and occupancy of every kernel of one HIP source, as the compiler reports it
(-Rpass-analysis=kernel-resource-usage).  usage: tools/kernel_resources.py [-DNAME[=VALUE] ...] recon.hip [mc.hip ...]
(-DDV_LEAN: only what the 10-bit tiled step launches, a tenth of the compile time; tests/test_kernel_resources.py reads report())"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return out[:len(names)] if len(out) >= len(names) else names
    except OSError:
        return names


def report(src, flags=()):
    """One dict per kernel of dav1d_amd/csrc/<src>: name (demangled, without arguments), vgpr, agpr, sgpr, scratch (bytes per lane), lds, occ."""
    path = os.path.join(ROOT, "dav1d_amd", "csrc", src)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), *flags,
                        "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", "/dev/null"], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stderr[-4000:]))
    out, cur = [], {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function )?Name: (\S+)", line) or re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            continue
        for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
        if "lds" in cur and "name" in cur:
            out.append(cur)
            cur = {}
    for k, n in zip(out, demangle([k["name"] for k in out])):
        k["name"] = re.sub(r"\(anonymous namespace\)::", "", n).split("(")[0]
    return out


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("-")]
    for src in (a for a in sys.argv[1:] if not a.startswith("-")):
        for k in report(src, flags):
            print("%-12s vgpr %3d agpr %3d sgpr %3d scratch %4d lds %6d occ %2d  %s" % (src, k.get("vgpr", -1), k.get("agpr", -1), k.get("sgpr", -1),
                                                                                        k.get("scratch", -1), k["lds"], k.get("occ", -1), k["name"][:100]))
