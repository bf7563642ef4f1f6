"""CPU-side check of the BUILT SVGF kernels (libmpt_hip.so is cross-compiled for gfx950; no GPU needed): the code object's metadata
says that none of them uses scratch or spills a register; k_sv_reproject (its three instantiations) uses no LDS, at most 64 VGPRs
and exactly one atomic; k_sv_variance and k_sv_level use no atomic, at most 128 VGPRs (four waves per SIMD at the least) and an
LDS demand, static plus the largest dynamic one the library asks for, that lets two workgroups share a compute unit."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
REPROJECT = ("k_sv_reprojectILi0E", "k_sv_reprojectILi1E", "k_sv_reprojectILi2E")
LEVELS = ("k_sv_levelILb1ELb0E", "k_sv_levelILb1ELb1E", "k_sv_levelILb0ELb0E", "k_sv_levelILb0ELb1E")
OTHERS = ("k_sv_variance", "k_sv_modulate", "k_sv_pack")
LDS_PER_CU = 160 * 1024                      # gfx950
# the largest dynamic LDS sv_run asks for: step MPT_DN_LDS_MAX_STEP = 4, a tile of (16 + 4 * 4)^2 entries of 32 bytes
MAX_DYNAMIC_LDS = (16 + 4 * 4) ** 2 * 32


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("sv_codeobj")
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


def _kernel(code_object, key):
    kernels, funcs = code_object
    names = [n for n in kernels if key in n and n.startswith("_Z")]
    assert len(names) == 1, (key, names)
    md, ins = kernels[names[0]], funcs[names[0]]
    print(key, {k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert ins and not [s for s in ins if s.startswith("scratch_")], key
    return md, ins


@pytest.mark.parametrize("key", REPROJECT)
def test_reproject_uses_no_lds_and_one_atomic(code_object, key):
    md, ins = _kernel(code_object, key)
    assert md["group_segment_fixed_size"] == 0, md                  # the taps are read through L2: no LDS
    assert md["vgpr_count"] <= 64, md                               # (8 waves per SIMD)
    atomics = [s for s in ins if "atomic" in s]
    assert len(atomics) == 1, atomics                               # one add per wave for the reset counter, nothing else


@pytest.mark.parametrize("key", LEVELS + ("k_sv_variance",))
def test_filter_kernels_fit_four_waves_and_two_workgroups(code_object, key):
    md, ins = _kernel(code_object, key)
    assert md["vgpr_count"] <= 128, md
    assert not [s for s in ins if "atomic" in s], key
    dynamic = MAX_DYNAMIC_LDS if key.startswith("k_sv_levelILb1") else 0
    assert 2 * (md["group_segment_fixed_size"] + dynamic) <= LDS_PER_CU, md
    if key.startswith("k_sv_levelILb0"):
        assert md["group_segment_fixed_size"] == 0, md              # the large steps read through L2 / MALL


@pytest.mark.parametrize("key", ("k_sv_modulate", "k_sv_pack"))
def test_small_kernels(code_object, key):
    md, ins = _kernel(code_object, key)
    assert md["group_segment_fixed_size"] == 0 and not [s for s in ins if "atomic" in s], md
