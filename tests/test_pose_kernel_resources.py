"""Register, scratch and LDS budget of the pose refinement's kernel (csrc/lfd_pose.hip: for 4, 8 and 16 slots, 2- and 4-channel warps - six
instantiations, what the launcher can reach), read from the compiler's own report of a gfx950 cross-compile with the library's flags, the way
tests/test_audit_kernel_resources.py reads the audit kernel's.  The kernel is a gather with f64 arithmetic and a reduction behind it: nothing
may go to scratch memory, a workgroup's LDS is at most the staged slots (16 of 80 bytes), the pairs' constants (16 of 256 bytes) and a table
of 16 x 32 accumulators of 8 bytes - 9 472 bytes, within 12 288 - and a wave takes at most 256 vector registers.  The target is 128 (four
waves per SIMD); the figures reached are printed and stand in DESIGN.md 4.28.  No GPU needed; skipped only where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import _build_module, parse_resource_usage

MAX_VGPRS, MAX_SCRATCH, MAX_LDS = 256, 0, 12288


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    obj = str(tmp_path_factory.mktemp("res") / "lfd_pose.o")
    cmd = bld.compile_command("lfd_pose.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return {k: v for k, v in parse_resource_usage(res.stderr).items() if "lfd_pose_" in k}


def test_every_kernel_stays_inside_its_budget(usage):
    assert len([k for k in usage if "lfd_pose_kernel" in k]) == 6, sorted(usage)
    assert len(usage) == 6, sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["VGPRs"] <= MAX_VGPRS, (kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
        assert u["LDS Size [bytes/block]"] <= MAX_LDS, (kernel, u)
