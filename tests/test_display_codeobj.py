"""CPU-side check of the BUILT display kernels (libmpt_hip.so is cross-compiled for gfx950; no GPU needed): the code object's metadata
says every instantiation of k_dp_histogram, k_dp_exposure and k_dp_present uses no scratch, spills no register and keeps its static LDS
within 2 KB, and their instruction streams agree (extracted as tests/test_temporal_codeobj.py does); k_dp_present holds one atomic, the
clipped count's."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
# instantiations: histogram = 3 sources x (plain, aggregated); present = 3 sources x 3 tone curves x (1, 4 pixels per thread)
EXPECTED = {"k_dp_histogram": 6, "k_dp_exposure": 1, "k_dp_present": 18}


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("dp_codeobj")
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


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_display_kernels_use_no_scratch_spill_nothing_and_fit_their_lds(code_object, key):
    kernels, funcs = code_object
    names = sorted(n for n in kernels if key in n and n.startswith("_Z"))
    assert len(names) == EXPECTED[key], (key, names)
    for name in names:
        md = kernels[name]
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] <= 2048, (name, md)
        assert md["group_segment_fixed_size"] == (0 if key == "k_dp_exposure" else 1024), (name, md)   # 256 bins / 255 thresholds
        ins = funcs[name]
        assert ins and not [s for s in ins if s.startswith("scratch_")], name
        atomics = [s for s in ins if "atomic" in s or s.startswith("ds_add")]
        if key == "k_dp_present":
            assert len(atomics) == 1 and atomics[0].startswith("global_atomic_add_x2"), (name, atomics)   # the clipped count, once per wave
            assert md["vgpr_count"] <= 64, (name, md)                                                    # (8 waves per SIMD)
        elif key == "k_dp_exposure":
            assert not atomics, (name, atomics)                                                          # plain stores only
        else:
            assert [s for s in atomics if s.startswith("ds_add")] and [s for s in atomics if s.startswith("global_atomic_add")], (name, atomics)
