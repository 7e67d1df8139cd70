"""Register and scratch budget of the three instantiations of the photo-consistency kernel (csrc/lfd_photo.hip: window radius 1, 2 and 3), read
from the compiler's own report of a gfx950 cross-compile with the library's flags, the way tests/test_colour_kernel_resources.py reads the
colour kernel's.  That file's reasoning applies unchanged: the kernel is a gather, occupancy hides its latency, so the window row's values and
the six sums must stay in registers - no scratch memory - and a wave must not take more than 128 vector registers, the most that lets four
waves share a SIMD's 512.  No GPU needed; skipped only where hipcc is absent."""
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
    obj = str(tmp_path_factory.mktemp("res") / "lfd_photo.o")
    cmd = bld.compile_command("lfd_photo.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return {k: v for k, v in parse_resource_usage(res.stderr).items() if "lfd_photo_count_kernel" in k}


def test_every_instantiation_stays_inside_its_budget(usage):
    assert len(usage) == 3, sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["VGPRs"] <= MAX_VGPRS, (kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
