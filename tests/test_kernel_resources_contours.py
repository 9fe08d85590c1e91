"""Register audit of the label-contour translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel in it -- its own four and the rocprim compaction kernels it instantiates -- may
use scratch memory, and the trace kernel's LDS is the 4 KB bit mask plus the 512 B candidate queue, so that LDS never
limits the single-wave workgroups per CU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("ct_scan_kernel", "ct_trace_kernel", "ct_offsets_kernel", "ct_emit_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/contours.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "contours.s"]


def test_contour_kernels_use_no_scratch_and_little_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1]
    own = [short(r) for r in rows if short(r).startswith("ct_")]
    assert sorted(own) == sorted(KERNELS), sorted(own)
    assert len(rows) > len(own)                                      # the library kernels of the compaction are in the table too
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {short(r): r["lds"] for r in rows if short(r) in KERNELS}
    assert lds["ct_trace_kernel"] == 32768 // 8 + 2 * 64 * 4
    assert lds["ct_scan_kernel"] == 0 and lds["ct_emit_kernel"] == 0 and lds["ct_offsets_kernel"] <= 1024
