"""not-gpu: the register budget of the single-level task-QP kernel in the BUILT library, read from the metadata notes of its gfx950 code
objects by tools/kernel_resources.py.  The kernel holds no scratch only because the contact stage's mask and the pointer its unused stores
go through are kernel arguments (TqIO::cs_mask, TqIO::cs_out; libdwbc_amd/csrc/dwbc_task_qp.h): with either folded to a constant it spills
954 VGPRs, 3.4 KB of scratch per lane.  A compiler that folds them again shows here, not in a rate."""
import os
import re
import subprocess
import sys

from tests import cases

KERNELS = ("dwbc::dwbc_task_qp_kernel<39, 34, dwbc::TopoTocabi>", "dwbc::dwbc_task_qp_kernel<39, 34, dwbc::TopoGeneric>")


def test_no_scratch_and_no_spilled_vgpr_under_the_register_cap():
    from libdwbc_amd import _lib

    out = subprocess.check_output([sys.executable, os.path.join(cases.ROOT, "tools", "kernel_resources.py"), _lib.LIB_PATH, "dwbc_task_qp_kernel"], text=True)
    rows = {}
    for line in out.splitlines():
        m = re.match(r"void (\S.*?>)\(.*\bvgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+vspill\s+(\d+)\s+sspill\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    print(out)
    assert sorted(rows) == sorted(KERNELS), rows
    for name, (vgpr, agpr, sgpr, vspill, sspill, scratch) in rows.items():
        assert scratch == 0 and vspill == 0, (name, vspill, scratch)
        assert vgpr + agpr <= 256, (name, vgpr, agpr)  # amdgpu_waves_per_eu(2): two waves per SIMD
