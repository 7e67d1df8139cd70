"""The shared routines of the per-image exposure gains (csrc/lfd_gain.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/abi/gain_sanitize.cpp - a host program with its own main that drives lfd_gain_sample, the quantisation and lfd_gain_value as the twins
do, into arrays of exactly the documented sizes (a table of [k][7], images of [h_match * w_match * 3], 3 n colour values), and compares every
sum and every value with a plain loop - is compiled with -fsanitize=address,undefined and run as a process of its own."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_gain_routines_run_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "gain_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "gain_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    print(ran.stdout)
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
