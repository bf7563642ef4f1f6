"""The per-context (W, H) record behind the lean kernels' constant division (LeanCdivCache / lean_cdiv_ok,
metalpathtracer_amd/csrc/mpt_lean_cdiv.h), on the CPU.

tests/lean_math/lean_cdiv_cache_check.cpp is a stand-alone program: it includes the header and stubs the device check — the same pair
twice makes one check, a changed pair a new one, a failed check turns the lean dispatch off.  Built with the host compiler,
AddressSanitizer and UndefinedBehaviorSanitizer; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_lean_cdiv_cache(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lean_cdiv_cache_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc"), os.path.join(ROOT, "tests", "lean_math", "lean_cdiv_cache_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr
