"""CPU-side check of the BUILT shadow-ray kernels (libmpt_hip.so is cross-compiled for gfx950; no GPU needed), from the code object's
metadata alone (read as tests/test_display_codeobj.py reads it): every instantiation of k_occluded_ref, k_occluded_own and k_ao uses no
scratch and spills no register, and an any-hit kernel needs no more vector registers than the closest-hit kernel of the same tree."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
# instantiations: k_occluded_ref = (tree partly in LDS, all of it in LDS); k_ao = those two and the own tree
EXPECTED = {"k_occluded_ref": 2, "k_occluded_own": 1, "k_ao": 3}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("ao_codeobj")
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


def named(kernels, key):
    """Mangled names of the kernel `key` (_Z<length><name>...: k_ao is no prefix of another kernel's name this way)."""
    return sorted(n for n in kernels if n.startswith("_Z%d%s" % (len(key), key)))


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_shadow_ray_kernels_use_no_scratch_and_spill_nothing(kernels, key):
    names = named(kernels, key)
    assert len(names) == EXPECTED[key], (key, names)
    for name in names:
        md = kernels[name]
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] == 0, (name, md)          # (dynamic LDS only: the scene image)


def test_any_hit_kernels_need_no_more_vector_registers_than_closest_hit(kernels):
    (closest_ref,) = named(kernels, "k_trace_rays")
    (closest_own,) = named(kernels, "k_trace_rays_ordered")
    for name in named(kernels, "k_occluded_ref"):
        assert kernels[name]["vgpr_count"] <= kernels[closest_ref]["vgpr_count"], (name, kernels[name], kernels[closest_ref])
    (own,) = named(kernels, "k_occluded_own")
    assert kernels[own]["vgpr_count"] <= kernels[closest_own]["vgpr_count"], (own, kernels[own], kernels[closest_own])
