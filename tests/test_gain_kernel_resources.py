"""Register and scratch budget of the six instantiations of the gain statistics kernel (csrc/lfd_gain.hip: 4, 8 and 16 slots, 2- and
4-channel warps), read from the compiler's own report of a gfx950 cross-compile with the library's flags, the way
tests/test_colour_kernel_resources.py reads the colour kernel's.  The kernel is the colour kernel's gather with a reduction behind it:
occupancy hides the latency, so nothing may go to scratch memory and a wave must not take more than 128 vector registers, the most that lets
four waves share a SIMD's 512.  No GPU needed; skipped only where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import _build_module, parse_resource_usage

MAX_VGPRS, MAX_SCRATCH = 128, 0


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    obj = str(tmp_path_factory.mktemp("res") / "lfd_gain.o")
    cmd = bld.compile_command("lfd_gain.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return {k: v for k, v in parse_resource_usage(res.stderr).items() if "lfd_gain_kernel" in k}


def test_every_instantiation_stays_inside_its_budget(usage):
    assert len(usage) == 6, sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["VGPRs"] <= MAX_VGPRS, (kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
