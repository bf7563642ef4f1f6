"""CPU-side check of the BUILT next-event-estimation kernel (libmpt_hip.so is cross-compiled for gfx950; no GPU needed), from the code
object's metadata alone (read as tests/test_direct_codeobj.py reads it): k_nee has exactly three instantiations; each uses no scratch,
spills no vector register and has dynamic LDS only; the two reference-order ones spill no scalar register either.  The own-tree one
holds two closest-first walks' worth of scalars: its scalar spill count is reported in DESIGN.md §17, not bounded here."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
OWN = "ILi2E"      # k_nee<MPT_AO_OWN>: the template argument in the mangled name


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("nee_codeobj")
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


def test_nee_kernel_has_three_instantiations_without_scratch(kernels):
    names = sorted(n for n in kernels if n.startswith("_Z5k_nee"))
    assert len(names) == 3 and sum(OWN in n for n in names) == 1, names
    for name in names:
        md = kernels[name]
        print(name, {k: md[k] for k in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] == 0, (name, md)          # (dynamic LDS only: the scene image)
        if OWN not in name:
            assert md["sgpr_spill_count"] == 0, (name, md)
