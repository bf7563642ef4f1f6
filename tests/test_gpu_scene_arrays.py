"""The device scene arrays, read back (mpt_read_scene_array) and checked invariant by invariant by tests/scene_check.py — the threaded
tree, the primitive records, the materials, the own 4-wide tree, the leaf boxes and the always list — on both routes that write them:
mpt_upload_scene (layout_scene on the host, where the arrays must also be the CPU dump's bit for bit) and mpt_build_and_upload (the
kernels of mpt_devbuild.h, mpt_sah.h and mpt_lbvh.h) with every builder, both ways to the own tree, the sizes at the switches inside the
builders and the shapes that take a path of their own.  tests/test_scene_check_cpu.py shows that the checker notices; here every case
also shows that the read-back returns the device's words (their digest by mpt_scene_digest's formula is the device's) and leaves the
scene alone.  Nothing is rendered, nothing is timed."""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc
from conftest import host_scene
from scene_check import check_scene
from scene_cases import plain_dumper  # noqa: F401  (the fixture: layout_scene behind a stand-alone program, built without sanitizers)

pytestmark = pytest.mark.gpu

NAMES = ("nodes", "prims", "mats", "own", "refleaf", "refbox", "always", "ref_bvh", "ref_idx")


def digest_of(words):
    """mpt_scene_digest's formula (k_digest): the sum over i of splitmix64(i << 32 | word[i])"""
    with np.errstate(over="ignore"):
        z = (np.arange(words.size, dtype=np.uint64) << np.uint64(32) | words.astype(np.uint64)) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int((z ^ (z >> np.uint64(31))).sum(dtype=np.uint64))


def read_and_check(ctx, prims, mats, caller_tree=None):
    """Read the scene back, show the read-back changed nothing and returned the device's words, and run the checker against the
    reference-format tree: the caller's on the upload route, mpt_download_bvh's on the device route.  (report, arrays, counts)"""
    before = ctx.scene_digest()
    arrays, counts = ctx.read_scene()
    assert ctx.scene_digest() == before
    assert tuple(arrays) == NAMES and list(counts.values()) == before[9:]
    for k, name in enumerate(NAMES):
        assert digest_of(arrays[name]) == before[k], name
    if caller_tree is None:
        bvh, idx = ctx.download_bvh()
        np.testing.assert_array_equal(arrays["ref_bvh"], bvh.view(np.uint32).ravel())
        np.testing.assert_array_equal(arrays["ref_idx"].view(np.int32), idx)
    else:
        bvh, idx = caller_tree
        assert arrays["ref_bvh"].size == 0 and arrays["ref_idx"].size == 0
    rep = check_scene(arrays, counts, prims, mats, np.asarray(bvh, np.float32).reshape(-1, 8), idx, accel_info=ctx.accel_info())
    print(counts, rep)
    assert rep["leaf_boxes_bit_equal"]      # on both routes a leaf's box is its reference box moved out by the pad, one float32 operation per face
    return rep, arrays, counts


def set_builder(monkeypatch, builder):
    """"sah", "ploc", "lbvh" select the binary builder; "sah+refit" / "sah+sah" also force the way to the own tree (MPT_OWN_TREE), and
    "sah+walk" the bottom-up k_own_tree walk where the copy would do"""
    tree, _, own = builder.partition("+")
    monkeypatch.setenv("MPT_GPU_BUILD", tree)
    monkeypatch.delenv("MPT_OWN_TREE", raising=False)
    monkeypatch.delenv("MPT_OWN_TREE_WALK", raising=False)
    if own == "walk":
        monkeypatch.setenv("MPT_OWN_TREE_WALK", "1")
    elif own:
        monkeypatch.setenv("MPT_OWN_TREE", own)


BUILDERS = ["sah", "ploc", "lbvh", "sah+refit", "sah+sah", "sah+walk"]


@pytest.mark.parametrize("name", sc.ASSET_SCENES)
def test_upload_route_writes_the_cpu_layout_and_it_checks(gpu_ctx, plain_dumper, tmp_path, name):  # noqa: F811
    bvh, prims, mats, idx = host_scene(name)[1]
    gpu_ctx.upload_scene(bvh, prims, mats, idx)
    rep, arrays, counts = read_and_check(gpu_ctx, prims, mats, (bvh, idx))
    want, want_counts, ok = sc.layout_dump(plain_dumper, tmp_path, bvh, prims, mats, idx)
    assert counts == want_counts and gpu_ctx.accel_info()["ordered_ok"] == ok == 1
    for k in sc.ARRAYS:                                             # the upload itself (refbox: k_prim_refbox against its rule)
        np.testing.assert_array_equal(arrays[k], want[k], err_msg=k)
    assert rep["exempt_slots"] == 0


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", sc.ASSET_SCENES)
def test_device_route_on_the_asset_scenes(gpu_ctx, name, builder, monkeypatch):
    set_builder(monkeypatch, builder)
    _, prims, mats, _ = host_scene(name)[1]
    gpu_ctx.build_and_upload(prims, mats)
    rep, _, _ = read_and_check(gpu_ctx, prims, mats)
    assert rep["exempt_slots"] == 0 and rep["void_leaves"] == 0
    assert gpu_ctx.accel_info()["ordered_ok"] == 1


@pytest.mark.parametrize("builder", ["sah", "ploc", "lbvh"])
def test_device_route_at_the_switches_inside_the_builders(gpu_ctx, builder, monkeypatch):
    """5 ... 8300 primitives with 0 / 1 / 16 / 17 spheres and the ground sphere (scene_cases.BOUNDARY_CASES, 8191 and 8192 among them: the
    leaf limit goes from 6 to 2 and the leaf order from area-keyed to the builder's)"""
    set_builder(monkeypatch, builder)
    rng = np.random.default_rng(29)
    for n, n_sph in sc.BOUNDARY_CASES:
        prims, mats = sc.boundary_scene(rng, n, n_sph)
        gpu_ctx.build_and_upload(prims, mats)
        print(builder, n, n_sph)
        rep, _, counts = read_and_check(gpu_ctx, prims, mats)
        assert rep["exempt_slots"] == 0 and counts["n_always"] == (n_sph if n_sph <= 16 else 0)


def degenerate_257(variant):
    """the input of test_build_and_upload_survives_degenerate_input (test_gpu_lbvh.py)"""
    prims, mats = sc.degenerate_scene(np.random.default_rng(21), 257)
    if variant == "identical":
        prims[:] = prims[20]
    return prims, mats


def expected_exempt(bvh, idx, prims, arrays):
    """What the exemption rule gives for this input, worked out from the input itself: a leaf of the downloaded tree is exempt when the
    union of its primitives' boxes (min and max skip a NaN) is not finite; a slot of the own tree when it is such a leaf's or lies above
    one.  (leaves, slots) — the leaves are found through the tree's topology and the caller's rows, not through the boxes under test."""
    b = bvh.reshape(-1, 8)
    first, count = b[:, 3].copy().view(np.int32), b[:, 7].copy().view(np.int32)
    p = np.asarray(prims, np.float32).reshape(-1, 12)
    v = np.stack([p[:, 0:3], p[:, 4:7], p[:, 8:11]])
    tri = (p[:, 3] == 1.0)[:, None]
    with np.errstate(invalid="ignore"):
        plo = np.where(tri, np.fmin.reduce(v, axis=0, initial=np.inf), p[:, 0:3] - p[:, 4:5])
        phi = np.where(tri, np.fmax.reduce(v, axis=0, initial=-np.inf), p[:, 0:3] + p[:, 4:5])
    exempt_ids, leaves = set(), 0
    for n in np.flatnonzero(count > 0):
        ids = idx[first[n]:first[n] + count[n]]
        lo, hi = np.fmin.reduce(plo[ids], axis=0, initial=np.inf), np.fmax.reduce(phi[ids], axis=0, initial=-np.inf)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            leaves += 1
            exempt_ids.update(int(i) for i in ids)
    ref = arrays["own"].reshape(-1, 28)[:, 24:28]
    pid = arrays["prims"].reshape(-1, 12)[:, 11]
    slot = np.zeros(ref.shape, bool)
    for n in range(ref.shape[0] - 1, -1, -1):                       # breadth-first numbering: children come after their parent
        for k in range(4):
            r = int(ref[n, k])
            if r != 0xFFFFFFFF:
                slot[n, k] = int(pid[r & 0x7FFFFFF]) in exempt_ids if r & 0x80000000 else slot[r].any()
    return leaves, int(slot.sum())


def shape(name):
    """(prims, mats) of a shape that takes a path of its own"""
    rng = np.random.default_rng(31)
    if name == "spheres only":
        prims = np.stack([sc.sphere(rng.uniform(-3, 3, 3), 0.5) for _ in range(5)])
    elif name == "one triangle":
        prims = sc.triangles(rng, 1)
    elif name == "a sphere and two triangles":
        prims = sc.triangles(rng, 3)
        prims[0] = sc.sphere((0.5, 0.5, 0.5), 0.75)                 # (spheres first, as Scene::buildBVH sorts them)
    elif name == "a NaN-cornered triangle, no sphere":              # every corner NaN: its box is no box (Scalars::odd_leaf), and one NaN coordinate
        prims = sc.triangles(rng, 40)
        prims[8:20, 0:3] = prims[8:20, 4:7] = prims[8:20, 8:11] = np.nan   # (more than two leaves' worth: some leaf holds nothing else)
        prims[23, 5] = np.nan
    elif name == "a ground quad and 3 spheres":                     # items hoisted under the root: k_own_chain
        prims = sc.triangles(rng, 300)
        for k in (0, 1, 2):
            prims[k] = sc.sphere(rng.uniform(-3, 3, 3), 0.4 * (k + 1))
        prims[3, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = (-900, -1, -900, 900, -1, -900, 900, -1, 900)
        prims[4, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = (-900, -1, -900, 900, -1, 900, -900, -1, 900)
    elif name == "a primitive that is neither":                     # type 2: kept as a sphere of radius NaN, on the always list
        prims = sc.triangles(rng, 20)
        prims[0] = sc.sphere((0.0, 0.0, 0.0), 0.5)
        prims[0, 3] = 2.0
    elif name == "all primitives identical":
        prims = np.repeat(sc.triangles(rng, 1), 257, axis=0)
    elif name == "coplanar wall pairs":                             # the two halves of five axis-aligned walls of a box: the thickness rule
        quads = []
        for axis, at in ((0, -1.0), (0, 1.0), (1, -1.0), (1, 1.0), (2, -1.0)):
            u, v = [a for a in range(3) if a != axis]
            c = np.zeros((4, 3), np.float32)
            c[:, axis] = at
            c[:, u], c[:, v] = (-1, 1, 1, -1), (-1, -1, 1, 1)
            quads += [(c[0], c[1], c[2]), (c[0], c[2], c[3])]
        prims = np.zeros((len(quads), 12), np.float32)
        prims[:, 3] = 1.0
        for i, (a, b, c) in enumerate(quads):
            prims[i, 0:3], prims[i, 4:7], prims[i, 8:11] = a, b, c
    elif name in ("degenerate 257 mixed", "degenerate 257 identical"):
        return degenerate_257(name.split()[-1])
    else:
        raise KeyError(name)
    return prims, sc.materials(prims.shape[0])


SHAPES = ["spheres only", "one triangle", "a sphere and two triangles", "a primitive that is neither", "a NaN-cornered triangle, no sphere", "a ground quad and 3 spheres",
          "all primitives identical", "coplanar wall pairs", "degenerate 257 mixed", "degenerate 257 identical"]


@pytest.mark.parametrize("name", SHAPES)
def test_device_route_on_shapes_that_take_a_path_of_their_own(gpu_ctx, name, monkeypatch):
    prims, mats = shape(name)
    tight = 0
    for builder in BUILDERS:
        set_builder(monkeypatch, builder)
        gpu_ctx.build_and_upload(prims, mats)
        print(name, builder)
        rep, arrays, counts = read_and_check(gpu_ctx, prims, mats)
        tight += rep["tight_leaves"]
        # the exempt share is what the rule gives for this input, leaf for leaf and slot for slot
        bvh, idx = gpu_ctx.download_bvh()
        exempt, exempt_slots = expected_exempt(bvh, idx, prims, arrays)
        assert (rep["exempt_leaves"], rep["exempt_slots"]) == (exempt, exempt_slots)
        if name == "degenerate 257 mixed":                          # the two triangles with an infinite vertex, in one leaf or in two
            assert 1 <= exempt <= 2 and exempt <= exempt_slots <= exempt * counts["depth"]
        elif name == "a NaN-cornered triangle, no sphere":          # the leaves of all-NaN triangles alone: no box, left out of the own tree
            assert 1 <= exempt <= 12 and rep["void_leaves"] == exempt and rep["void_leaves_in_own_tree"] == 0 and exempt_slots == 0
        else:
            assert exempt == 0 and exempt_slots == 0
        if name == "a primitive that is neither":
            assert counts["n_always"] == 1 and np.isnan(arrays["always"].view(np.float32)[4])
        if name == "spheres only":
            assert counts["n_own"] == 1 and (arrays["own"][24:28] == 0xFFFFFFFF).all() and counts["n_always"] == 5
    # the host route over the tree the last builder made (mpt_upload_scene of the downloaded arrays): the same shape through layout_scene,
    # which keeps a leaf without a box as an item where the device route leaves it out
    bvh, idx = gpu_ctx.download_bvh()
    gpu_ctx.upload_scene(bvh, prims, mats, idx)
    print(name, "uploaded")
    up, _, _ = read_and_check(gpu_ctx, prims, mats, (bvh, idx))
    assert up["exempt_leaves"] == rep["exempt_leaves"] and up["void_leaves"] == rep["void_leaves"] == up["void_leaves_in_own_tree"]
    if name == "a sphere and two triangles":
        assert tight >= 1                                           # some builder puts the sphere in a leaf with a triangle: the tight box


def test_upload_route_with_a_chain_and_with_boxes_that_are_not_nested(gpu_ctx):
    bvh, prims, mats, idx = sc.hand_made("40-primitive leaf")
    gpu_ctx.upload_scene(bvh, prims, mats, idx)
    rep, _, counts = read_and_check(gpu_ctx, prims, mats, (bvh, idx))
    assert counts["n_nodes"] == 7 and counts["n_leaves"] == 3 and gpu_ctx.accel_info()["ordered_ok"] == 1
    bvh, prims, mats, idx = sc.hand_made("sphere with triangles")
    gpu_ctx.upload_scene(bvh, prims, mats, idx)
    rep, _, _ = read_and_check(gpu_ctx, prims, mats, (bvh, idx))
    assert rep["tight_leaves"] == 1 and gpu_ctx.accel_info()["ordered_ok"] == 1
    bvh = bvh.copy()
    bvh[1, 4] = np.nextafter(bvh[0, 4], np.float32(np.inf))         # the root's left child pokes out of the root by one ulp
    gpu_ctx.upload_scene(bvh, prims, mats, idx)
    assert gpu_ctx.accel_info()["ordered_ok"] == 0
    read_and_check(gpu_ctx, prims, mats, (bvh, idx))                # the own tree is made all the same, and its checks hold


def test_read_scene_array_argument_handling(gpu_ctx):
    from metalpathtracer_amd import capi
    L = gpu_ctx.L
    OK, INVALID, NOT_READY = 0, 1, 5
    fresh = capi.Context(0)
    try:
        n = C.c_uint64(77)
        assert L.mpt_read_scene_array(fresh.h, 0, None, 0, C.byref(n)) == NOT_READY and n.value == 0
    finally:
        fresh.close()
    bvh, prims, mats, idx = sc.hand_made("sphere with triangles")
    gpu_ctx.upload_scene(bvh, prims, mats, idx)
    before = gpu_ctx.scene_digest()
    n = C.c_uint64(77)
    assert L.mpt_read_scene_array(gpu_ctx.h, 1, None, 0, C.byref(n)) == OK and n.value == 12 * 7      # the size query
    buf = np.full(12 * 7 + 4, 0xA5A5A5A5, np.uint32)
    up = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    n = C.c_uint64(77)
    assert L.mpt_read_scene_array(gpu_ctx.h, 1, up, 12 * 7 - 1, C.byref(n)) == INVALID and n.value == 12 * 7   # too small: the size, nothing else
    assert (buf == 0xA5A5A5A5).all()
    assert L.mpt_read_scene_array(gpu_ctx.h, 1, None, 5, C.byref(n)) == INVALID
    for bad in (-1, 9, 1 << 20):
        n = C.c_uint64(77)
        assert L.mpt_read_scene_array(gpu_ctx.h, bad, up, buf.size, C.byref(n)) == INVALID and n.value == 0
    assert L.mpt_read_scene_array(gpu_ctx.h, 1, up, buf.size, None) == INVALID
    assert (buf == 0xA5A5A5A5).all()
    assert L.mpt_read_scene_array(gpu_ctx.h, 1, up, buf.size, C.byref(n)) == OK and n.value == 12 * 7   # a larger buffer: the tail stays
    assert (buf[12 * 7:] == 0xA5A5A5A5).all() and digest_of(buf[:12 * 7]) == before[1]
    for which in (7, 8):                                            # the reference-format tree: none after mpt_upload_scene
        n = C.c_uint64(77)
        assert L.mpt_read_scene_array(gpu_ctx.h, which, up, buf.size, C.byref(n)) == OK and n.value == 0
        assert gpu_ctx.read_scene_array(which).size == 0
    assert gpu_ctx.scene_digest() == before
