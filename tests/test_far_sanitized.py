"""The shared routines of the far-field shell (csrc/lfd_far.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/abi/far_sanitize.cpp - a host program with its own main that drives the per-cell decision, the direction cell, the sample and the emitted
record as the twins do, into arrays of exactly the documented sizes (a table of [6 S S][7], an image of [h_match * w_match * 3], exactly n_out
records), and compares every table with a second accumulation in the opposite order - is compiled with -fsanitize=address,undefined and run
as a process of its own."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_far_routines_run_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "far_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "far_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    print(ran.stdout)
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
