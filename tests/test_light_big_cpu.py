"""The conditions tests/test_gpu_light_big.py rests on, from the scene of tests/light_big_cases.py and the references alone (no GPU, host
tree): the reference tree exceeds the largest LDS image, the scene is large enough for MPT_WALK_AUTO to mean the own tree, more than 32
material rows with Lambert and emitter rows beyond the 32nd as first hits (by layout_scene's own numbering), 41 lights with gaps
between their ids, the duplicates patch over a quarter of the view, no flat leaf box, open and occluded shadow rays in every estimator
— and the two caps the GPU comparisons exempt pixels under: gap shadow rays touch at most 1 % of the pixels of every estimator under
both light samplings, ReSTIR's tainted pixels are at most 10 %.  The caps are conditions on the inputs: the reference alone decides
them."""
import os
import re

import numpy as np
import pytest

import light_big_cases as lb
import restir_ref
import scene_cases
from conftest import ROOT
from scene_cases import plain_dumper  # noqa: F401  (the fixture: layout_scene behind a stand-alone program)


def test_the_constants_are_the_products():
    text = open(os.path.join(ROOT, "include", "mpt.h")).read()
    assert int(re.search(r"#define MPT_AUTO_ORDERED_PRIMS (\d+)u", text).group(1)) == lb.AUTO_ORDERED_PRIMS
    text = open(os.path.join(ROOT, "metalpathtracer_amd", "csrc", "mpt_kernels.h")).read()
    assert int(re.search(r"#define MPT_LDS_MATS_N (\d+)u", text).group(1)) == lb.LDS_MATS
    assert lb.GAP_CAP == 0.01 and lb.TAINT_CAP == 0.10
    assert (lb.W, lb.H) == (24, 16)                                         # 3 x 2 tiles: two workgroups of four


def test_the_reference_tree_fits_no_lds_image():
    sc, (bvh, prims, mats, idx) = lb.scene()
    n_nodes, n_prims = bvh.shape[0], prims.shape[0]
    print("primitives", n_prims, "reference nodes", n_nodes, "bytes", n_nodes * 32, "lights", lb.host_refs().table.n)
    assert n_nodes * 32 > lb.LDS_MOST
    assert n_prims >= lb.AUTO_ORDERED_PRIMS
    assert n_prims == sc.getPrimitiveCount() == 4 + 2 * lb.N_TRI_LIGHTS + 2 * lb.FLOOR_N ** 2 + 2 * lb.PATCH_NX * lb.PATCH_NZ * lb.PATCH_COPIES
    kind = prims.reshape(-1, 12)[:, 3]
    n_sph = int((kind == 0).sum())
    assert 0 < n_sph <= 16 and (kind[:n_sph] == 0).all() and (kind[n_sph:] == 1).all()         # spheres first


def test_a_smaller_floor_would_fit(monkeypatch):
    """The triangle count is the smallest that gives the inequality: one row and column of cells fewer and the tree is below 160 KiB."""
    monkeypatch.setattr(lb, "FLOOR_N", lb.FLOOR_N - 1)
    sc = lb.big_scene()
    sc.buildBVH()
    assert sc.getBVHNodeCount() * 32 <= lb.LDS_MOST


def test_no_leaf_box_is_flat():
    bvh = lb.host_buffers()[0].reshape(-1, 2, 4)
    leaf = bvh[:, 1, 3].copy().view(np.int32) > 0
    assert leaf.sum() > 1000 and (bvh[leaf, 1, :3] > bvh[leaf, 0, :3]).all()


def test_lights_have_gaps_between_their_ids_and_one_is_a_sphere():
    t = lb.host_refs().table
    assert t.n == 1 + lb.N_TRI_LIGHTS and t.n & (t.n - 1) != 0              # no power of two
    assert t.rec[0, 0, 3] == 0 and (t.rec[1:, 0, 3] == 1).all()
    assert t.ids[0] == 0 and (np.diff(t.ids[1:]) == 2).all()


def test_rows_beyond_the_lds_table_are_first_hits(plain_dumper, tmp_path):  # noqa: F811
    """By the numbering mpt_upload_scene gives the rows (layout_scene's: first occurrence in leaf order)."""
    bvh, prims, mats, idx = lb.host_buffers()
    arrays, counts, ok = scene_cases.layout_dump(plain_dumper, tmp_path, bvh, prims, mats, idx)
    assert ok == 1                                                          # the scene qualifies for the own tree
    n_mats = counts["n_mats"]
    assert n_mats == np.unique(mats.reshape(-1, 8).view(np.uint32), axis=0).shape[0] > lb.LDS_MATS
    _, _, prim = lb.host_refs().guides()
    lambert, emitter = lb.material_rows_seen(prim, lb.rows_of_records(arrays["prims"]), mats)
    print("material rows", n_mats, "own nodes", counts["n_own"], "Lambert rows seen", lambert.size, "of them beyond the LDS table", int((lambert >= lb.LDS_MATS).sum()),
          "emitter rows seen", emitter.size, "beyond", int((emitter >= lb.LDS_MATS).sum()))
    assert (lambert >= lb.LDS_MATS).any() and (lambert < lb.LDS_MATS).any()
    assert (emitter >= lb.LDS_MATS).any()


def test_the_view_holds_the_patch_the_floor_lights_and_spheres():
    _, nc, prim = lb.host_refs().guides()
    patch = np.isin(prim, lb.patch_ids())
    print("pixels on the duplicates patch:", int(patch.sum()), "of", patch.size, "emitter pixels", int((nc[..., 3] == 1).sum()))
    assert 0.2 * patch.size <= patch.sum() <= 0.4 * patch.size              # roughly a quarter of the view
    assert (nc[..., 3] == 1).any() and (prim[nc[..., 3] == 1] == 0).any()   # emitters, the sphere light among them
    assert np.isin(prim, (1, 2, 3)).any()                                   # a dull sphere


@pytest.mark.parametrize("name,M,sampling", lb.DIRECT_FAMILIES)
def test_gap_rays_of_the_direct_pass(name, M, sampling):
    r = lb.host_refs()
    d = r.direct(M, sampling)
    rgba, traced, unocc = d["want"]
    on_patch = np.isin(r.guides()[2], lb.patch_ids())
    print(name, "gap pixels", int(d["gap"].sum()), "of", d["gap"].size, "traced", int(traced.sum()), "unoccluded", int(unocc.sum()))
    assert d["gap"].sum() <= lb.GAP_CAP * d["gap"].size
    assert traced.sum() > unocc.sum() > 0                                    # open and occluded shadow rays both occur
    assert (rgba[on_patch][:, :3] > 0).any()                                 # lit vertices lie on the duplicates patch


@pytest.mark.parametrize("name,M,sampling", lb.NEE_FAMILIES)
def test_gap_rays_of_the_render(name, M, sampling):
    """mpt_render_nee, and with it mpt_render_nee_adaptive's estimator."""
    d = lb.host_refs().nee(M, sampling)
    gap = d["gap"].any(-1)
    print(name, "gap pixels", int(gap.sum()), "of", gap.size, "rays", int(d["rays"].sum()), "shadow", int(d["shadow"].sum()), "occluded", int(d["occluded"].sum()))
    assert gap.sum() <= lb.GAP_CAP * gap.size
    assert d["shadow"].sum() > d["occluded"].sum() > 0


def test_tainted_pixels_of_restir():
    d = lb.host_refs().restir()
    for mode in restir_ref.MODES:
        tainted = d[mode]["tainted"]
        print("mode", mode, "tainted", int(tainted.sum()), "of", tainted.size, d[mode]["info"])
        assert tainted.sum() <= lb.TAINT_CAP * tainted.size
        assert d[mode]["traced"].sum() > d[mode]["unoccluded"].sum() > 0
    info = d[restir_ref.UNBIASED]["info"]
    assert info["neighbours_accepted"] > 0 and info["samples_from_neighbours"] > 0 and info["rays_correction"] > 0      # the merge does something
    assert d[restir_ref.BIASED]["info"]["rays_correction"] == 0
