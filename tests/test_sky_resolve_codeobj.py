"""CPU-side checks of the BUILT resolves (k_resolve_sum, k_resolve_sum_moments: mpt_kernels.h), read from libmpt_hip.so the way
test_wavelocal_codeobj.py reads the trace kernels.

With the sky tiles' samples computed in the resolve it still has to run BESIDE the next render's trace kernel, two waves per SIMD: inside
64 VGPRs (launch bound 256 x 8) without scratch or spilled vector registers, and inside the scalar registers k_wavelocal*_corun leaves
free — 128 per SIMD, allocated per wave in blocks of 16 after 6 more for the wave's own: at most 58 each (MPT_RESOLVE_SGPRS)."""
import pytest

from test_wavelocal_codeobj import code_object, _kernel  # noqa: F401  (the fixture and the look-up of the trace kernels' test)


@pytest.mark.parametrize("key", ["k_resolve_sum10PassParams", "k_resolve_sum_moments10PassParams"])
def test_resolves_fit_beside_the_trace_kernel(code_object, key):
    md, ins = _kernel(code_object, key)
    print(key, {k: md[k] for k in ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}, len(ins), "instructions")
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 64, md
    assert md["sgpr_count"] <= 58, md
    assert md["max_flat_workgroup_size"] == 256, md
