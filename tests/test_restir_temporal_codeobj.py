"""CPU-side check of the BUILT temporal reservoir-reuse kernel of metalpathtracer_amd/csrc/mpt_restir_temporal.h (libmpt_hip.so is
cross-compiled for gfx950; no GPU needed), from the code object's metadata alone (read as tests/test_ris_codeobj.py reads it):
k_restir_temporal has exactly six instantiations (three walks x two modes); each uses no scratch, spills no vector register and has
dynamic LDS only.  The scalar spills are printed and reported in DESIGN.md §21, not bounded here."""
from test_ris_codeobj import OWN, kernels  # noqa: F401  (the module-scoped fixture that reads the metadata)


def test_restir_temporal_kernel_instantiations_have_no_scratch(kernels):  # noqa: F811
    kernel = "k_restir_temporal"
    prefix = "_Z%d%sILi" % (len(kernel), kernel)
    names = sorted(n for n in kernels if n.startswith(prefix))
    assert len(names) == 6 and sum(OWN in n for n in names) == 2, names
    for walk in range(3):                                                # two modes per walk
        assert [sum(n.startswith("%s%dELb%dE" % (prefix, walk, mode)) for n in names) for mode in (0, 1)] == [1, 1], names
    for name in names:
        md = kernels[name]
        print(name, {k: md[k] for k in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")})
        assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, (name, md)
        assert md["group_segment_fixed_size"] == 0, (name, md)          # (dynamic LDS only: the scene image)
