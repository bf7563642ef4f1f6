"""The conditions tests/test_gpu_materials.py rests on, checked on the CPU with the oracle: the scenes of tests/material_cases.py hold
the number of distinct material rows they claim, every row of the table cases is the first hit of a pixel (so the device's guide buffers
and renders see every entry of the table), the all-distinct cases show nearly every quad of the wall, and the crafted pair of rows does
collide in the upper half of the material hash and nowhere else."""
import numpy as np
import pytest

import material_cases as mc
from oracle import binding as ob

_hits = {}


def first_hit_prims(K):
    """[H, W] int32: the primitive the oracle hits first through every pixel centre (-1: none), on a one-leaf tree — once per geometry."""
    if K not in _hits:
        name = next(n for n, c in mc.CASES.items() if c[0] == K)
        prims = mc.geometry(K)
        bvh, idx = mc.flat_tree(prims)
        buffers = (bvh, np.ascontiguousarray(prims), None, idx)
        cam, d = mc.pixel_rays(mc.uniforms(name))
        out = np.full(d.shape[:2], -1, np.int32)
        for y in range(d.shape[0]):
            for x in range(d.shape[1]):
                out[y, x] = ob.first_hit(cam, d[y, x], buffers)[1]
        out.setflags(write=False)
        _hits[K] = out
    return _hits[K]


def rows_u32(mats):
    return np.ascontiguousarray(mats, np.float32).reshape(-1, 8).view(np.uint32)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_the_generator_delivers_the_distinct_rows_it_claims(name):
    prims, mats, n_mats = mc.scene(name)
    K, want, _ = mc.CASES[name]
    assert prims.shape == (5 + 2 * K * K, 12) and mats.shape == (prims.shape[0], 8)
    assert np.unique(rows_u32(mats), axis=0).shape[0] == n_mats == (want if want is not None else prims.shape[0])
    assert (prims[:3, 3] == 0).all() and (prims[3:, 3] == 1).all()              # spheres first, as the builders want them
    if n_mats >= 4:
        assert tuple(mats[:3, 3]) == (0.0, -1.0, 1.5)                           # Lambert, mirror, glass
    if want is not None:
        assert (rows_u32(mats[3]) == rows_u32(mats[4])).all()                   # the floor is one material
        same_as_next = (rows_u32(mats[5:-1]) == rows_u32(mats[6:])).all(1)
        assert n_mats == 1 or same_as_next.mean() < 0.1                         # equal rows are not neighbours in the array
    if name == "all40k":
        assert prims.shape[0] * 32 >= 1 << 20                                   # the size from which the helper thread uploads the materials


def test_sizes_pass_the_boundaries_they_are_meant_to_pass():
    n = {name: mc.geometry(c[0]).shape[0] for name, c in mc.CASES.items()}
    assert 1024 < n["m200"] < 2048                                              # just past one radix tile
    assert 4096 < n["all4k"] < 8192                                             # past a workgroup of four tiles, below the pipeline switch
    assert 8192 <= n["all8k"]                                                   # leaves of <= 2, MPT_PIPE_AUTO = k_ordered
    assert mc.W <= 128 and mc.H <= 96


def test_the_table_holds_the_rows_that_are_hard_to_tell_apart():
    _, mats, _ = mc.scene("m31")
    u = np.unique(rows_u32(mats), axis=0)
    f = u.view(np.float32)
    pairs = [(a, b) for a in range(len(u)) for b in range(a + 1, len(u)) if (u[a] != u[b]).sum() == 1]
    sign = [(a, b) for a, b in pairs if ((u[a] ^ u[b]) == 0x80000000).any() and (f[a, :3] == f[b, :3]).all()]
    mtype = [(a, b) for a, b in pairs if u[a, 3] != u[b, 3]]
    ulp = [(a, b) for a, b in pairs if u[a, 7] != u[b, 7] and abs(int(u[a, 7]) - int(u[b, 7])) == 1 and f[a, 7] > 0]
    assert len(sign) >= 3 and len(mtype) >= 6 and len(ulp) >= 3
    _, mats, _ = mc.scene("m200")
    em = np.unique(rows_u32(mats)[mats[:, 7] > 0], axis=0).view(np.float32)
    le = em[:, 4:7] * em[:, 7:8]
    assert em.shape[0] == mc.N_EMISSIVE and np.unique(le.view(np.uint32), axis=0).shape[0] == mc.N_EMISSIVE


@pytest.mark.parametrize("name", mc.TABLE_CASES)
def test_every_material_is_the_first_hit_of_a_pixel(name):
    prims, mats, n_mats = mc.scene(name)
    hit = first_hit_prims(mc.CASES[name][0])
    seen = np.unique(hit[hit >= 0])
    assert np.unique(rows_u32(mats)[seen], axis=0).shape[0] == n_mats
    if name == "collision":                                                     # both rows of the pair, each on many primitives
        pair = rows_u32(mc.colliding_pair())
        for r in pair:
            on = np.nonzero((rows_u32(mats) == r).all(1))[0]
            assert on.size == 32 and np.isin(on, seen).sum() >= 16
        a, b = [np.nonzero((rows_u32(mats) == r).all(1))[0] for r in pair]
        both = np.sort(np.concatenate([a, b]))
        assert (np.diff(both) == 16).all() and (np.isin(both[0::2], a)).all() and (np.isin(both[1::2], b)).all()   # dealt alternately, others between


@pytest.mark.parametrize("name", ["all4k", "all8k"])
def test_the_all_distinct_cases_show_the_wall(name):
    K = mc.CASES[name][0]
    hit = first_hit_prims(K)
    wall = hit[hit >= 5]
    quads = np.unique((wall - 5) // 2)
    print(name, "quads seen", quads.size, "of", K * K, "primitives seen", np.unique(hit[hit >= 0]).size)
    assert quads.size >= 0.9 * K * K
    assert {0, 1, 2}.issubset(set(hit[hit >= 0].tolist())) and (hit == 3).any() and (hit == 4).any()    # spheres and floor too


def test_the_pair_collides_in_the_upper_half_of_the_hash_only():
    pair = mc.colliding_pair()
    assert (rows_u32(pair[0]) != rows_u32(pair[1])).any()
    assert (pair[:, 3:] == 0).all() and ((pair[:, :3] >= 0.05) & (pair[:, :3] < 0.95)).all()
    h = mc.mat_hash(pair)
    assert h[0] >> np.uint64(32) == h[1] >> np.uint64(32) and h[0] != h[1]
    # the restatement against a plain-integer one
    for row, got in zip(rows_u32(pair), h):
        x = 0xcbf29ce484222325
        for w in row:
            x ^= int(w)
            x = (x * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
            x ^= x >> 29
        assert x == int(got)
    # no other row of the collision scene shares the pair's upper half: the pair's run of equal keys holds these two materials alone
    _, mats, _ = mc.scene("collision")
    hi = (mc.mat_hash(np.unique(rows_u32(mats), axis=0).view(np.float32)) >> np.uint64(32))
    assert (hi == h[0] >> np.uint64(32)).sum() == 2 and np.unique(hi).size == 201
