"""The range check that admits a pass to the lean wave-local kernels (wl_lean_ok, metalpathtracer_amd/csrc/mpt_wl_lean.h), on the CPU.

tests/wl_lean/wl_lean_check.cpp is a stand-alone program: it includes the header, checks every bound at its last accepted and its first
refused value and every refused mode, and for each accepted pass evaluates the lean kernels' index arithmetic with the instructions'
semantics (24-bit operands, 32-bit results) over the whole range of the pass against plain 64-bit arithmetic.  Built with the host
compiler and UndefinedBehaviorSanitizer; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_wl_lean_ok_bounds(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wl_lean_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc"), os.path.join(ROOT, "tests", "wl_lean", "wl_lean_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr
