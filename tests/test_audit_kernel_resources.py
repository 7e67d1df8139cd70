"""Register, scratch and LDS budget of the epipolar audit's kernel (csrc/lfd_audit.hip: for 4, 8 and 16 slots, 2- and 4-channel warps, with
the in-wave aggregation and with plain per-lane LDS atomics - twelve instantiations, what the launcher can reach), read from the compiler's
own report of a gfx950 cross-compile with the library's flags, the way tests/test_far_kernel_resources.py reads the far kernel's.  The kernel
is a gather with a reduction behind it: occupancy hides the latency, so nothing may go to scratch memory, a wave must not take more than 128
vector registers (the most that lets four waves share a SIMD's 512), and a workgroup's LDS is at most the staged slots (16 of 80 bytes), the
pairs' matrices (16 of 72 bytes), a table of 16 x 66 counters of at most 8 bytes and a few words: 12 288 bytes or less.  No GPU needed;
skipped only where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import _build_module, parse_resource_usage

MAX_VGPRS, MAX_SCRATCH, MAX_LDS = 128, 0, 12288


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    obj = str(tmp_path_factory.mktemp("res") / "lfd_audit.o")
    cmd = bld.compile_command("lfd_audit.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return {k: v for k, v in parse_resource_usage(res.stderr).items() if "lfd_audit_" in k}


def test_every_kernel_stays_inside_its_budget(usage):
    assert len([k for k in usage if "lfd_audit_kernel" in k]) == 12, sorted(usage)
    assert len(usage) == 12, sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["VGPRs"] <= MAX_VGPRS, (kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
        assert u["LDS Size [bytes/block]"] <= MAX_LDS, (kernel, u)
