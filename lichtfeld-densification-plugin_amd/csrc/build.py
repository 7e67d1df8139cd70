"""Build the HIP library in-tree: ``python build.py`` -> ../liblfd_densify.so (gfx950).

hipcc cross-compiles without a GPU.  -ffp-contract=off: every rounding in lfd_geometry.hpp is
explicit (mul+add vs fma) so the host build of the per-cell routine and the device build agree.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "liblfd_densify.so")
SOURCES = ["lfd_api.hip", "lfd_kernels.hip", "lfd_select.hip", "lfd_writer.hip", "lfd_host.hip", "lfd_image.hip", "lfd_voxel.hip", "lfd_corr.hip", "lfd_cycle.hip", "lfd_support.hip", "lfd_refine.hip", "lfd_sigma.hip", "lfd_normals.hip", "lfd_colour.hip", "lfd_gain.hip", "lfd_far.hip", "lfd_audit.hip", "lfd_pose.hip", "lfd_consensus.hip", "lfd_component.hip", "lfd_undistort.hip", "lfd_freespace.hip", "lfd_depth.hip", "lfd_fuse.hip", "lfd_knn.hip", "lfd_block.hip", "lfd_cap.hip", "lfd_head.hip", "lfd_thin.hip", "lfd_photo.hip"]
HEADERS = ["lfd_device.hpp", "lfd_geometry.hpp", "lfd_context.hpp", "lfd_corr.hpp", "lfd_cycle.hpp", "lfd_support.hpp", "lfd_refine.hpp", "lfd_sigma.hpp", "lfd_normals.hpp", "lfd_colour.hpp", "lfd_gain.hpp", "lfd_far.hpp", "lfd_audit.hpp", "lfd_pose.hpp", "lfd_consensus.hpp", "lfd_component.hpp", "lfd_undistort.hpp", "lfd_freespace.hpp", "lfd_depth.hpp", "lfd_fuse.hpp", "lfd_knn.hpp", "lfd_block.hpp", "lfd_cap.hpp", "lfd_head.hpp", "lfd_thin.hpp", "lfd_photo.hpp", os.path.join("..", "..", "include", "lfd_densify.h")]
# -amdgpu-sched-strategy=max-ilp: the dense kernel is bound by its vector arithmetic (long dependent f64 chains); the
# ILP-first machine scheduler is worth 3.5 % on it (profiles/history.md (r1/ablation.txt)), instruction semantics are unchanged
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
         "-fno-fast-math", "-Wall", "-Wno-unused-function", "-pthread"]
SCHED_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# ... except where it costs registers for nothing: the refiner-block kernels (lfd_block.hip) are bound by memory and by plain f32 FMAs on 25 + 32
# wave-uniform weights held in SGPRs; hoisting every scalar load to the top spills 40 and 46 SGPRs there, the default scheduler none.
# The refiner-head kernel (lfd_head.hip) streams z once and is bound by memory; max-ilp lifts its loads and the two f64 softplus evaluations per pixel
# over each other and costs 64 / 98 .. 108 VGPRs (2- / 4-pixel lanes) against 50 .. 52 / 96: one wave per SIMD less for the 4-pixel kernels.
# The pose kernel (lfd_pose.hip) holds up to 32 64-bit products for its folding reduction; max-ilp forms them all at once (179 .. 195 VGPRs, two
# waves per SIMD) where the default scheduler needs 138 .. 158 (three).
DEFAULT_SCHED = ("lfd_block.hip", "lfd_head.hip", "lfd_pose.hip")
# Flags of one source only.  lfd_kernels.hip without the SLP vectoriser: a v_pk_*_f32 is cheaper per operation than two scalar instructions only
# when both halves already sit in a register pair (profiles/r7/fma_f32_packing.txt); in the dense kernels the pairing costs more than it saves - moves to
# assemble the pairs, scalar instructions, SGPR spill reloads inside the geometry loop.  Same arithmetic, same bits; -1.7 % of the dense kernel's time
# (profiles/r7/ab_solver_stream.txt).  The other sources keep the default.
FILE_FLAGS = {"lfd_kernels.hip": ["-fno-slp-vectorize"]}
LINK_FLAGS = ["--offload-arch=gfx950", "-fPIC", "-shared", "-pthread"]


def compile_command(source: str, out: str, extra=()) -> list:
    """The hipcc command that compiles one source of SOURCES to an object (tests/test_dense_kernel_resources.py reuses it)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc] + FLAGS + ([] if source in DEFAULT_SCHED else SCHED_FLAGS) + FILE_FLAGS.get(source, []) + list(extra) + ["-c", os.path.join(HERE, source), "-o", out]


def needs_build() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SOURCES + HEADERS + ["build.py"])


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return OUT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    extra = ["-Rpass-analysis=kernel-resource-usage"] if verbose else []
    with tempfile.TemporaryDirectory(prefix="lfd_build_") as tmp:
        objs = [os.path.join(tmp, os.path.splitext(f)[0] + ".o") for f in SOURCES]
        cmds = [compile_command(f, o, extra) for f, o in zip(SOURCES, objs)]
        with ThreadPoolExecutor(max_workers=min(len(cmds), int(os.environ.get("MAX_JOBS", "8")))) as pool:
            results = list(pool.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds))
        link = [hipcc] + LINK_FLAGS + objs + ["-o", OUT]
        for cmd, res in zip(cmds, results):
            if verbose:
                print(" ".join(cmd))
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr)
                raise RuntimeError("hipcc failed building liblfd_densify.so (" + os.path.basename(cmd[-3]) + ")")
            if verbose:
                sys.stderr.write(res.stderr)
        res = subprocess.run(link, capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise RuntimeError("hipcc failed linking liblfd_densify.so")
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
