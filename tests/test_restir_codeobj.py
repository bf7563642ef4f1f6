"""CPU-side check of the BUILT reservoir-reuse kernels of metalpathtracer_amd/csrc/mpt_restir.h (libmpt_hip.so is cross-compiled for
gfx950; no GPU needed), from the code object's metadata alone (read as tests/test_ris_codeobj.py reads it): k_restir_initial has exactly
three instantiations and k_restir_merge six (three walks x two modes); each uses no scratch, spills no vector register and has dynamic
LDS only.  The scalar spills of the own-tree merge kernels are printed and reported in DESIGN.md §20, not bounded here."""
import pytest

from test_ris_codeobj import OWN, kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)


@pytest.mark.parametrize("kernel,count", [("k_restir_initial", 3), ("k_restir_merge", 6)])
def test_restir_kernel_instantiations_have_no_scratch(kernels, kernel, count):  # noqa: F811
    prefix = "_Z%d%sILi" % (len(kernel), kernel)
    names = sorted(n for n in kernels if n.startswith(prefix))
    assert len(names) == count and sum(OWN in n for n in names) == count // 3, names
    for name in names:
        md = kernels[name]
        print(name, {k: md[k] for k in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] == 0, (name, md)          # (dynamic LDS only: the scene image)
