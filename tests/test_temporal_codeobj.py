"""CPU-side check of the BUILT temporal kernels (libmpt_hip.so is cross-compiled for gfx950; no GPU needed): the code object's
metadata says k_tp_reproject (its three instantiations) and k_tp_pack use no scratch and spill no register, and their instruction
streams agree (extracted as tests/test_build_asm.py does)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
KERNELS = ("k_tp_reprojectILi0E", "k_tp_reprojectILi1E", "k_tp_reprojectILi2E", "k_tp_pack")


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("tp_codeobj")
    shutil.copy(LIB, d / "lib.so")                      # (--offloading writes the bundles next to its input)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(co) == 1, os.listdir(d)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co[0]], cwd=d, check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:      # one metadata entry per kernel, .agpr_count is its first key
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co[0]], cwd=d, check=True, capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.startswith("\t"):
            funcs[cur].append(line.split("//")[0].strip())
    return kernels, funcs


@pytest.mark.parametrize("key", KERNELS)
def test_temporal_kernels_use_no_scratch_and_spill_nothing(code_object, key):
    kernels, funcs = code_object
    names = [n for n in kernels if key in n and n.startswith("_Z")]
    assert len(names) == 1, (key, names)
    md = kernels[names[0]]
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["group_segment_fixed_size"] == 0, md                  # the taps are read through L2: no LDS
    assert md["vgpr_count"] <= 64, md                               # (8 waves per SIMD)
    ins = funcs[names[0]]
    assert ins and not [s for s in ins if s.startswith("scratch_")], key
    atomics = [s for s in ins if "atomic" in s]
    assert len(atomics) == (0 if key == "k_tp_pack" else 1), atomics   # one add per wave for the reset counter, nothing else
