"""Register, scratch, LDS and occupancy budget of the eight fused dense kernels (csrc/lfd_kernels.hip), read from the compiler's own
report of a gfx950 cross-compile with the library's flags (csrc/build.py).  Every attempt that left this budget lost 5-17 % of the
kernel's time, and nothing else in the suite would notice: the results stay the same.  No GPU needed; skipped only
where hipcc is absent."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

DENSE_KERNELS = ["lfd_dense_kernel", "lfd_dense_exact_kernel", "lfd_dense_ply_kernel", "lfd_dense_ply_exact_kernel",
                 "lfd_dense_segments_kernel", "lfd_dense_segments_exact_kernel", "lfd_dense_ply_segments_kernel",
                 "lfd_dense_ply_segments_exact_kernel"]
MAX_VGPRS, MAX_SCRATCH, MAX_LDS, MIN_WAVES = 64, 0, 20480, 8


def _build_module():
    spec = importlib.util.spec_from_file_location("_lfd_build_res", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parse_resource_usage(text):
    """{kernel: {field: int}} from -Rpass-analysis=kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z][A-Za-z \[\]/]*?): (\d+)) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1):
            cur = out.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    return out


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    obj = str(tmp_path_factory.mktemp("res") / "lfd_kernels.o")
    cmd = bld.compile_command("lfd_kernels.hip", obj, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return parse_resource_usage(res.stderr)


def test_parser_reads_a_remark_block():
    text = ("k.hip:1:1: remark: Function Name: lfd_dense_kernel [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:1:1: remark:     VGPRs: 63 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:1:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]\n"
            "k.hip:1:1: remark:     LDS Size [bytes/block]: 20424 [-Rpass-analysis=kernel-resource-usage]\n")
    assert parse_resource_usage(text) == {"lfd_dense_kernel": {"VGPRs": 63, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 8,
                                                               "LDS Size [bytes/block]": 20424}}


@pytest.mark.parametrize("kernel", DENSE_KERNELS)
def test_dense_kernel_stays_inside_its_budget(usage, kernel):
    assert kernel in usage, sorted(usage)
    u = usage[kernel]
    print(kernel, u)
    assert u["VGPRs"] <= MAX_VGPRS, u
    assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, u
    assert u["LDS Size [bytes/block]"] <= MAX_LDS, u
    assert u["Occupancy [waves/SIMD]"] >= MIN_WAVES, u
