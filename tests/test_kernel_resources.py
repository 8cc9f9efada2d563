"""What the compiler made of the paired reconstruction kernels and the wide residual kernels, read from its own resource remarks
(-Rpass-analysis=kernel-resource-usage, the compile of tools/kernel_resources.py): no private (scratch) memory in any instantiation —
neither a spilled register nor a copy of a kernel argument made to be indexed (a per-lane choice among the members of `dst`
once cost every 16x16 / 32x32 wave 4 KB of stores before its first load) — and the register budgets the occupancy of the step's
kernels rests on.  No GPU: hipcc cross-compiles.  Only the remarks are read, never the assembly."""
import importlib.util
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

# the four paired kernels the 10-bit tiled step launches: recon_fused_kernel<CLS, unsigned short, int, false, true, true>.
# VGPRs no higher / waves per SIMD no lower than before the argument copy was removed (72 / 72 / 72 / 88, 7 / 7 / 7 / 5)
STEP_VGPR = {0: 72, 1: 72, 2: 72, 3: 88}
STEP_OCC = {0: 7, 1: 7, 2: 7, 3: 5}


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def reports():
    """recon.hip lean (what the step launches) and in full, itx.hip in full: three compiles side by side, each made once"""
    kr = _tool()
    jobs = {"recon-lean": ("recon.hip", ["-DDV_LEAN"]), "recon": ("recon.hip", []), "itx": ("itx.hip", [])}
    with ThreadPoolExecutor(len(jobs)) as ex:
        futs = {k: ex.submit(kr.report, src, flags) for k, (src, flags) in jobs.items()}
        return {k: f.result() for k, f in futs.items()}


def _of(kernels, prefix):
    return [k for k in kernels if re.match(r"(void )?" + prefix + "<", k["name"])]


@pytest.mark.parametrize("build, n_min", [("recon-lean", 5), ("recon", 80)])
def test_paired_kernels_use_no_scratch_memory(reports, build, n_min):
    ks = _of(reports[build], "recon_fused_kernel")
    assert len(ks) >= n_min, [k["name"] for k in ks]
    bad = ["%s: %d bytes per lane" % (k["name"], k["scratch"]) for k in ks if k["scratch"] != 0]
    assert not bad, "\n".join(bad)


def test_wide_residual_kernels_use_no_scratch_memory(reports):
    ks = _of(reports["itx"], "itx_add_wide_kernel")
    assert len(ks) == 38, [k["name"] for k in ks]          # 19 transform sizes, two pixel types
    bad = ["%s: %d bytes per lane" % (k["name"], k["scratch"]) for k in ks if k["scratch"] != 0]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("build", ["recon-lean", "recon"])
def test_register_budget_of_the_step_kernels(reports, build):
    seen = set()
    for k in _of(reports[build], "recon_fused_kernel"):
        m = re.search(r"recon_fused_kernel<(\d), unsigned short, int, false, true, true>", k["name"])
        if not m or int(m.group(1)) not in STEP_VGPR:
            continue
        cls = int(m.group(1))
        seen.add(cls)
        print("%s: vgpr %d occupancy %d" % (k["name"], k["vgpr"], k["occ"]))
        assert k["vgpr"] <= STEP_VGPR[cls], (k["name"], k["vgpr"])
        assert k["occ"] >= STEP_OCC[cls], (k["name"], k["occ"])
    assert seen == set(STEP_VGPR), seen
