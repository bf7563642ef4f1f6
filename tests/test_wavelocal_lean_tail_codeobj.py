"""CPU-side checks of the BUILT lean wave-local kernels after the tail leaf moved behind the walk's loop (the tail leaf, mpt_lean_entry.h),
read from libmpt_hip.so the way test_wavelocal_codeobj.py reads the generic ones.  Registers and scratch only.

The epilogue adds a second copy of the leaf test to each of the three walks of the ALL_LDS kernels, and the guard's planes come from
LDS; the operating point must hold all the same: no scratch, <= 80 VGPRs (6 waves per SIMD), and the variant that runs beside a resolve
spills no more scalar registers than it did before the item (23)."""
import pytest

from test_wavelocal_codeobj import code_object, _kernel  # noqa: F401  (the fixture and the look-up of the generic kernels' test)
from test_wavelocal_lean_codeobj import LEAN

CORUN_ALL_LDS_SPILLS_BEFORE = 23


@pytest.mark.parametrize("key", LEAN)
def test_lean_kernels_with_the_tail_leaf_hold_the_operating_point(code_object, key):
    md, ins = _kernel(code_object, key)
    print(key, {k: md[k] for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
    assert ins and not [s for s in ins if s.startswith("scratch_")], (key, [s for s in ins if s.startswith("scratch_")][:4])
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 80, md
    if key.startswith("k_wavelocal_lean_corunILb1E"):
        assert md["sgpr_spill_count"] <= CORUN_ALL_LDS_SPILLS_BEFORE, md
