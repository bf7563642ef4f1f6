"""CPU-side checks of the BUILT lean wave-local trace kernels (k_wavelocal_lean<ALL_LDS>, k_wavelocal_lean_corun<ALL_LDS>: mpt_kernels.h),
read from libmpt_hip.so the way test_wavelocal_codeobj.py reads the generic ones.

The lean kernels are the step loop for Philox + Lambert with 24-bit index arithmetic.  They must hold the generic kernels' operating
point (<= 80 VGPRs, no scratch; <= 96 scalar registers for the variant that runs beside a resolve), spill no more scalar registers than
the generic kernel of the same shape, keep the ring-record and result-slot stores, and be free of the quarter-rate integer multiplies
the index arithmetic used to cost.

Quarter-rate multiplies, as built: the Philox block is 10 rounds x 2 products of 32 x 32 -> 64 bits per call, two calls per kernel (primary
ray, bounce): 40 products, which the specification pins.  The compiler emits a product as v_mad_u64_u32 when both halves are used and as
v_mul_hi_u32 / v_mul_lo_u32 when one half is dead (the last rounds: two v_mul_hi_u32 per call), so "no v_mul_hi_u32 at all" cannot hold
for a kernel that contains Philox.  What is asserted: at most 40 v_mad_u64_u32; v_mad_u64_u32 + v_mul_hi_u32 of the Philox chains
together at most 40; and NO v_mul_hi_u32 outside a Philox chain, with one exception that is not index arithmetic and runs once per wave:
the compiler's wave-aggregated 64-bit atomicAdd of note_wave_exit (ticks x lanes), right in front of its global_atomic_add_x2."""
import re

import pytest

from test_wavelocal_codeobj import code_object, _kernel  # noqa: F401  (the fixture and the look-up of the generic kernels' test)

LEAN = ("k_wavelocal_leanILb0E", "k_wavelocal_leanILb1E", "k_wavelocal_lean_corunILb0E", "k_wavelocal_lean_corunILb1E")
GENERIC_OF = {"k_wavelocal_leanILb0E": "k_wavelocalILb0ELb0E", "k_wavelocal_leanILb1E": "k_wavelocalILb0ELb1E",
              "k_wavelocal_lean_corunILb0E": "k_wavelocal_corunILb0E", "k_wavelocal_lean_corunILb1E": "k_wavelocal_corunILb1E"}


def _op(s):
    return re.sub(r"_e(32|64)$", "", s.split()[0])


@pytest.mark.parametrize("key", LEAN)
def test_lean_kernels_hold_the_operating_point(code_object, key):
    md, ins = _kernel(code_object, key)
    gmd, _ = _kernel(code_object, GENERIC_OF[key])
    print(key, {k: md[k] for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")},
          "generic sgpr_spill_count", gmd["sgpr_spill_count"])
    assert ins and not [s for s in ins if s.startswith("scratch_")], (key, [s for s in ins if s.startswith("scratch_")][:4])
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 80, md
    if "corun" in key:
        assert md["sgpr_count"] <= 96, md
    assert md["sgpr_spill_count"] <= gmd["sgpr_spill_count"], (md["sgpr_spill_count"], gmd["sgpr_spill_count"])


@pytest.mark.parametrize("key", LEAN)
def test_lean_kernels_have_no_quarter_rate_index_arithmetic(code_object, key):
    _, ins = _kernel(code_object, key)
    ops = [_op(s) for s in ins]
    mad = [i for i, o in enumerate(ops) if o == "v_mad_u64_u32"]
    hi = [i for i, o in enumerate(ops) if o == "v_mul_hi_u32"]
    philox_hi = [i for i in hi if any(abs(i - j) <= 16 for j in mad)]
    exit_hi = [i for i in hi if i not in philox_hi and any(s.startswith("global_atomic_add_x2") for s in ins[i:i + 12])]
    print(key, "v_mad_u64_u32", len(mad), "v_mul_hi_u32: philox", len(philox_hi), "exit timer", len(exit_hi), "other", len(hi) - len(philox_hi) - len(exit_hi),
          "v_mul_u32_u24", ops.count("v_mul_u32_u24"), "v_mad_u32_u24", ops.count("v_mad_u32_u24"))
    assert len(mad) <= 40, len(mad)
    assert len(mad) + len(philox_hi) <= 40, (len(mad), len(philox_hi))
    assert len(exit_hi) <= 1, [ins[i] for i in exit_hi]
    assert len(hi) == len(philox_hi) + len(exit_hi), [(i, ins[i]) for i in hi if i not in philox_hi and i not in exit_hi]
    assert ops.count("v_mul_u32_u24") + ops.count("v_mad_u32_u24") >= 4, "the 24-bit index arithmetic is gone"


@pytest.mark.parametrize("key", LEAN)
def test_lean_kernels_keep_the_ring_and_slot_stores(code_object, key):
    """As test_wavelocal_codeobj.test_ring_record_stores_are_still_there asks of the generic kernels: od, dt, ia, tl of a pushed hit and
    the same four plus tv of a parked ray as plain 16-byte stores, the two result-slot stores non-temporal."""
    _, ins = _kernel(code_object, key)
    stores = [s for s in ins if s.startswith("global_store_dwordx4")]
    plain = [s for s in stores if not re.search(r"\bnt\b", s)]
    assert len(plain) >= 4 + 5, stores
    assert len(stores) - len(plain) >= 2, stores
