"""The shared walk and union-find of the component filter (csrc/lfd_component.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/abi/component_sanitize.cpp - a host program with its own main that drives the routines as the twin does, on random clouds with NaN and
infinite coordinates, and compares every label and size with a brute-force partition - is compiled with -fsanitize=address,undefined and run
as a process of its own.  Nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

from helpers import ROOT


def test_the_walk_and_the_union_find_run_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = os.path.join(str(tmp_path), "component_sanitize")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "lichtfeld-densification-plugin_amd", "csrc"), os.path.join(ROOT, "tests", "abi", "component_sanitize.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.strip().endswith("ok (0 mismatches)") and "runtime error" not in ran.stderr and "AddressSanitizer" not in ran.stderr
