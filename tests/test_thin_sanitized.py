"""The twin of the footprint-adaptive thinning (csrc/lfd_thin.hpp: lfd_thin_check and lfd_thin_walk, what lfd_thin_footprint_host runs behind its
context checks) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/abi/thin_sanitize.cpp - a host program with its own main that drives
it on clouds with duplicates, empty references, points behind their camera, identical points, a lattice with points on cell faces and footprints
that put everything on level 0 or level 20, into arrays of exactly the documented sizes, and compares every index, offset and statistic with a loop
that knows nothing of the sort - is compiled with -fsanitize=address,undefined and run as a process of its own."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_thinning_twin_runs_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "thin_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "thin_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    print(ran.stdout)
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
