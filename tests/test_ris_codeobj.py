"""CPU-side check of the BUILT resampling kernels of metalpathtracer_amd/csrc/mpt_ris.h (libmpt_hip.so is cross-compiled for gfx950; no
GPU needed), from the code object's metadata alone (read as tests/test_nee_codeobj.py reads it): k_direct_ris, k_direct_ris_cone,
k_nee_ris and k_nee_ris_cone have exactly three instantiations each; each uses no scratch, spills no vector register and has dynamic LDS
only.  The scalar spills of the own-tree instantiations are printed and reported in DESIGN.md §19, not bounded here."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
OWN = "ILi2E"      # <MPT_AO_OWN>: the template argument in the mangled name
KERNELS = ("k_direct_ris", "k_direct_ris_cone", "k_nee_ris", "k_nee_ris_cone")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("ris_codeobj")
    shutil.copy(LIB, d / "lib.so")                      # (--offloading writes the bundles next to its input)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    co = [f for f in os.listdir(d) if "gfx950" in f]
    assert len(co) == 1, os.listdir(d)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co[0]], cwd=d, check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:      # one metadata entry per kernel, .agpr_count is its first key
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_ris_kernel_has_three_instantiations_without_scratch(kernels, kernel):
    prefix = "_Z%d%sILi" % (len(kernel), kernel)        # (the length in the mangled name keeps k_nee_ris apart from k_nee_ris_cone)
    names = sorted(n for n in kernels if n.startswith(prefix))
    assert len(names) == 3 and sum(OWN in n for n in names) == 1, names
    for name in names:
        md = kernels[name]
        print(name, {k: md[k] for k in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] == 0, (name, md)          # (dynamic LDS only: the scene image)
