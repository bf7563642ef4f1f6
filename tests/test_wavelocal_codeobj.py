"""CPU-side checks of the BUILT wave-local trace kernels (libmpt_hip.so is cross-compiled for gfx950; no GPU needed).

The kernel sits on a register cliff: 6 waves/SIMD allow 80 VGPRs, and the hits a step keeps in its lanes (the carry, mpt_kernels.h)
take the last three.  test_build_asm.py watches the two k_wavelocal<false, ..> instantiations; this file adds the ones pipelined
renders run (bench.py's timed steps), k_wavelocal_corun<false> and <true>, and reads the kernels' metadata as well as their
instructions.  It also makes
sure that the push path of ring 0 is still there: the carry keeps hits in registers only when the next step pops them, every other
hit must still be written to its ring."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "metalpathtracer_amd", "lib", "libmpt_hip.so")
PRODUCT = ("k_wavelocal_corunILb0E", "k_wavelocal_corunILb1E", "k_wavelocalILb0ELb1E", "k_wavelocalILb0ELb0E")   # what mpt_render_async (k_wavelocal_corun<ALL_LDS>) and mpt_render (k_wavelocal<false, ALL_LDS>) launch without the counting flag


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not present")
    d = tmp_path_factory.mktemp("wl_codeobj")
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
    names = [n for n in funcs if key in n and n.startswith("_Z")]
    assert len(names) == 1, (key, names)
    return kernels[names[0]], funcs[names[0]]


@pytest.mark.parametrize("key", PRODUCT)
def test_product_trace_kernels_use_no_scratch(code_object, key):
    md, ins = _kernel(code_object, key)
    print(key, {k: md[k] for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
    assert ins and not [s for s in ins if s.startswith("scratch_")], (key, [s for s in ins if s.startswith("scratch_")][:4])
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 80, md                              # 6 waves per SIMD


def test_pipelined_trace_kernel_stays_inside_96_scalar_registers(code_object):
    """k_wavelocal_corun leaves a block of scalar registers free on every SIMD so that a resolve can run beside it (mpt_kernels.h)."""
    md, _ = _kernel(code_object, "k_wavelocal_corunILb0E")
    assert md["sgpr_count"] <= 96, md


@pytest.mark.parametrize("key", PRODUCT)
def test_ring_record_stores_are_still_there(code_object, key):
    """A record is 16-byte fields: a hit pushed to ring 0 writes od, dt, ia and (if it has gathered light) tl; a parked ray writes
    the same four and tv.  Those are the kernel's only plain 16-byte stores — the result slots are written non-temporally (`nt`),
    twice: a path that ends at a hit, a path that ends in the sky."""
    _, ins = _kernel(code_object, key)
    stores = [s for s in ins if s.startswith("global_store_dwordx4")]
    plain = [s for s in stores if not re.search(r"\bnt\b", s)]
    assert len(plain) >= 4 + 5, stores
    assert len(stores) - len(plain) >= 2, stores
