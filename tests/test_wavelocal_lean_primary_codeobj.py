"""CPU-side checks of the BUILT lean wave-local kernels after the primary walk became an instantiation of its own (camera-relative
sphere terms, sphere_cam_terms: closest_hit_resume<.., LEAN, PRIMARY>, mpt_device.h), read from libmpt_hip.so the way
test_wavelocal_codeobj.py reads the generic ones.

A third walk in the step loop is more code and more live scalar values; the operating point must hold all the same: <= 80 VGPRs (6
waves per SIMD), no scratch and no VGPR spills, <= 96 scalar registers for the variants that run beside a resolve, and no more spilled
scalar registers than the generic kernel of the same shape.  The instruction counts of all eight kernels are printed (pytest -s)."""
import pytest

from test_wavelocal_codeobj import code_object, _kernel  # noqa: F401  (the fixture and the look-up of the generic kernels' test)
from test_wavelocal_lean_codeobj import GENERIC_OF, LEAN


@pytest.mark.parametrize("key", LEAN)
def test_lean_kernels_with_the_primary_walk_hold_the_operating_point(code_object, key):
    md, ins = _kernel(code_object, key)
    gmd, _ = _kernel(code_object, GENERIC_OF[key])
    print(key, {k: md[k] for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")},
          "generic sgpr_spill_count", gmd["sgpr_spill_count"])
    assert md["vgpr_count"] <= 80, md
    assert ins and not [s for s in ins if s.startswith("scratch_")], (key, [s for s in ins if s.startswith("scratch_")][:4])
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    if "corun" in key:
        assert md["sgpr_count"] <= 96, md
    assert md["sgpr_spill_count"] <= gmd["sgpr_spill_count"], (md["sgpr_spill_count"], gmd["sgpr_spill_count"])


def test_instruction_counts_of_the_eight_kernels(code_object):
    for key in LEAN + tuple(GENERIC_OF[k] for k in LEAN):
        _, ins = _kernel(code_object, key)
        assert ins
        print("%-32s %5d instructions, %5d vector, %5d scalar" % (key, len(ins), sum(s.startswith("v_") for s in ins), sum(s.startswith("s_") for s in ins)))
