"""The shared routines of the depth-map renderer (csrc/lfd_depth.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/abi/depth_sanitize.cpp - a host program with its own main that drives them as the twin does, on heap planes of exactly pw * ph words and
random clouds with non-finite points, and compares every cell with the two min-filter identities written as brute force - is compiled with
-fsanitize=address,undefined and run as a process of its own."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_shared_routines_run_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "depth_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "depth_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
