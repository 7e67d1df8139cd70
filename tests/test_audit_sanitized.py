"""The shared routines of the epipolar audit (csrc/lfd_audit.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/abi/audit_sanitize.cpp - a host program with its own main that drives the confidence test and the bin as the twin does, into arrays of
exactly the documented sizes (a table of [k][66], a cell map of [H W]), compares every table and map with a second accumulation in the
opposite order and every bin with the plain count of thresholds - is compiled with -fsanitize=address,undefined and run as a process of its
own."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_audit_routines_run_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "audit_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "audit_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    print(ran.stdout)
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
