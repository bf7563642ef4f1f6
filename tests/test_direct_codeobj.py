"""CPU-side check of the BUILT direct-lighting kernels (libmpt_hip.so is cross-compiled for gfx950; no GPU needed), from the code
object's metadata alone (read as tests/test_ao_codeobj.py reads it): k_direct has exactly three instantiations, and each of them and the
light-table kernel uses no scratch, spills no register and has dynamic LDS only."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
# instantiations: k_direct = (reference-order tree partly in LDS, all of it in LDS, the own tree)
EXPECTED = {"k_direct": 3, "k_light_collect": 1}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("direct_codeobj")
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
    """Mangled names of the kernel `key` (_Z<length><name>...: k_direct is no prefix of another kernel's name this way)."""
    return sorted(n for n in kernels if n.startswith("_Z%d%s" % (len(key), key)))


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_direct_lighting_kernels_use_no_scratch_and_spill_nothing(kernels, key):
    names = named(kernels, key)
    assert len(names) == EXPECTED[key], (key, names)
    for name in names:
        md = kernels[name]
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] == 0, (name, md)          # (dynamic LDS only: the scene image; none for the table kernel)
