"""The production-shape instantiation of the ordered dense kernel (lfd_dense_prod_kernel, csrc/lfd_kernels.hip) against the generic one,
from ONE gfx950 cross-compile with the library's flags (csrc/build.py): it stays inside the dense kernels' budget, and it is there to issue
less - fewer SGPR spills (each one is a v_writelane / v_readlane, a vector instruction) and fewer vector instructions than lfd_dense_kernel.
Both counts are read from that compile; no constant is fixed here.  No GPU needed; skipped only where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

from test_dense_kernel_resources import MAX_SCRATCH, MAX_VGPRS, MIN_WAVES, _build_module, parse_resource_usage

GENERIC, PROD = "lfd_dense_kernel", "lfd_dense_prod_kernel"


def function_bodies(asm):
    """{function: [instruction lines]} of an AMDGPU assembly listing: from the function's label to its .Lfunc_end."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_]\w*):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t") and not line.startswith("\t."):
            cur.append(line.split(";")[0].strip())
    return out


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    bld = _build_module()
    asm = str(tmp_path_factory.mktemp("prod") / "lfd_kernels.s")
    cmd = bld.compile_command("lfd_kernels.hip", asm, ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"])
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    with open(asm) as fh:
        return parse_resource_usage(res.stderr), function_bodies(fh.read())


def test_function_bodies_reads_a_listing():
    text = ("\t.globl\tk\nk:                                      ; @k\n; %bb.0:\n\ts_load_dword s0, s[0:1], 0x0\n\tv_add_u32_e32 v0, s0, v0 ; note\n"
            ".LBB0_1:\n\tv_mov_b32_e32 v1, 0\n\ts_endpgm\n\t.section\t.rodata\n.Lfunc_end0:\n\tv_not_counted v0\n")
    assert function_bodies(text) == {"k": ["s_load_dword s0, s[0:1], 0x0", "v_add_u32_e32 v0, s0, v0", "v_mov_b32_e32 v1, 0", "s_endpgm"]}


def test_production_kernel_stays_inside_the_dense_budget(compiled):
    usage, _ = compiled
    assert PROD in usage and GENERIC in usage, sorted(usage)
    u, g = usage[PROD], usage[GENERIC]
    print(PROD, u)
    print(GENERIC, g)
    assert u["VGPRs"] <= MAX_VGPRS, u
    assert u["ScratchSize [bytes/lane]"] <= MAX_SCRATCH, u
    assert u["Occupancy [waves/SIMD]"] >= MIN_WAVES, u
    assert u["LDS Size [bytes/block]"] <= g["LDS Size [bytes/block]"], (u, g)


def test_production_kernel_issues_less_than_the_generic_one(compiled):
    usage, bodies = compiled
    spills = {k: usage[k]["SGPRs Spill"] for k in (PROD, GENERIC)}
    valu = {k: sum(1 for ins in bodies[k] if ins.startswith("v_")) for k in (PROD, GENERIC)}
    print("SGPR spills", spills, "static vector instructions", valu)
    assert valu[GENERIC] > 0 and valu[PROD] > 0, valu                  # (both functions were found in the listing)
    assert spills[PROD] < spills[GENERIC], spills
    assert valu[PROD] < valu[GENERIC], valu
