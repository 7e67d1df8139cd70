"""Register and scratch budget of the two kernels of the footprint-adaptive thinning (csrc/lfd_thin.hip: lfd_thin_keys_kernel and
lfd_thin_cells_kernel), read from the compiler's own report of a gfx950 cross-compile with the library's flags, the way
tests/test_colour_kernel_resources.py reads the colour kernel's.  Both stream their input once and are bound by memory: no scratch memory, and few
enough vector registers for eight waves per SIMD (64).  As built: lfd_thin_keys_kernel 30 VGPRs, 68 SGPRs; lfd_thin_cells_kernel 11 VGPRs, 29
SGPRs; 84 bytes of LDS each; no scratch.  No GPU needed; skipped only where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import _build_module, parse_resource_usage

MAX_VGPRS, MAX_SCRATCH = 64, 0
KERNELS = ("lfd_thin_keys_kernel", "lfd_thin_cells_kernel")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    assert "lfd_thin.hip" in bld.SOURCES and "lfd_thin.hpp" in bld.HEADERS
    obj = str(tmp_path_factory.mktemp("res") / "lfd_thin.o")
    cmd = bld.compile_command("lfd_thin.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return parse_resource_usage(res.stderr)


def test_both_kernels_use_no_scratch_and_few_registers(usage):
    assert sorted(usage) == sorted(KERNELS), sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
        assert u["VGPRs"] <= MAX_VGPRS, (kernel, u)
