"""Register and scratch budget of the depth-map renderer's kernels (csrc/lfd_depth.hip: fill, splat, resolve), read from the compiler's own
report of a gfx950 cross-compile with the library's flags, the way tests/test_dense_kernel_resources.py reads the dense kernels'.  The splat is a
stream of projections and atomics and the resolve a stencil over LDS: occupancy hides their latency, so nothing may go to scratch memory and a wave
must not take more than 128 vector registers, the most that lets four waves share a SIMD's 512.  No GPU needed; skipped only where hipcc is
absent."""
import os
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import _build_module, parse_resource_usage

MAX_VGPRS, MAX_SCRATCH = 128, 0
KERNELS = ["lfd_depth_fill_kernel", "lfd_depth_splat_kernel", "lfd_depth_resolve_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    assert "lfd_depth.hip" in bld.SOURCES and "lfd_depth.hpp" in bld.HEADERS
    obj = str(tmp_path_factory.mktemp("res") / "lfd_depth.o")
    cmd = bld.compile_command("lfd_depth.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return {k: v for k, v in parse_resource_usage(res.stderr).items() if k.startswith("lfd_depth_")}


def test_every_kernel_stays_inside_its_budget(usage):
    assert sorted(usage) == sorted(KERNELS), sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["VGPRs"] <= MAX_VGPRS, (kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
