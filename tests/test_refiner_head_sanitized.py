"""The shared routine of the fused refiner head (csrc/lfd_head.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/abi/refiner_head_sanitize.cpp - a host program with its own main that drives the argument check and the per-pixel routine as the twin
does, on (1, 3, 4, 5), (1, 1, 2, 131) and (2, 32, 7, 9), from bf16 and f32 input, with every prev_dim, the previous state contiguous and through
strides, into arrays of exactly the needed size - is compiled with -fsanitize=address,undefined and run as a process of its own.  Nothing is
loaded into Python."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_head_routine_runs_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "refiner_head_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "refiner_head_sanitize.cpp"),
           "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    print(ran.stdout)
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
