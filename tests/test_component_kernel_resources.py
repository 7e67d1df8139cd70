"""Register and scratch budget of the kernels of the connected-component filter (csrc/lfd_component.hip), read from the compiler's own report
of a gfx950 cross-compile with the library's flags, the way tests/test_thin_kernel_resources.py reads the thinning's.  No kernel uses scratch
memory; the link kernel - a gather over the sorted cloud with a union-find step per agreeing candidate - stays within the 128 vector registers
the project's other gather kernels hold (four waves per SIMD).  No GPU needed; skipped only where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import _build_module, parse_resource_usage

MAX_LINK_VGPRS, MAX_SCRATCH = 128, 0
KERNELS = ("lfd_component_gather_kernel", "lfd_component_link_kernel", "lfd_component_flatten_kernel", "lfd_component_size_kernel",
           "lfd_component_mark_kernel")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    assert "lfd_component.hip" in bld.SOURCES and "lfd_component.hpp" in bld.HEADERS
    obj = str(tmp_path_factory.mktemp("res") / "lfd_component.o")
    cmd = bld.compile_command("lfd_component.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return parse_resource_usage(res.stderr)


def test_no_kernel_uses_scratch_and_the_link_kernel_keeps_its_register_budget(usage):
    assert sorted(usage) == sorted(KERNELS), sorted(usage)
    for kernel, u in sorted(usage.items()):
        print(kernel, u)
        assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, (kernel, u)
        assert u["VGPRs"] <= MAX_LINK_VGPRS, (kernel, u)
    assert usage["lfd_component_link_kernel"]["VGPRs"] <= MAX_LINK_VGPRS
