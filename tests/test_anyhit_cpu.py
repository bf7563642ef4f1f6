"""tests/anyhit_ref.py (the brute-force restatement of the any-hit walk) against the oracle's closest hit, without a GPU: two asset
scenes and four small adversarial families — slivers, needles, a height field with spheres inside, coplanar duplicates — shrunk from
the generators of tests/test_gpu_adversarial.py, every tree built by the oracle.  With t* = the oracle's closest t:
  * without a limit the reference-order answer is "the oracle found a hit", and t* is, bit for bit, one of the ray's accepted t;
  * for tmax at t*, one ulp either side and 0.5 / 0.999 / 1.001 / 2 times t*:  lower <= (t* < tmax) <= upper, where lower is the
    reference-order answer and upper the answer of the primitive tests alone; at t* and below both are empty;
  * upper & ~lower — the rays whose answer the own walk is free to choose, all of them the reference's artefact or one rounding of a
    leaf's slab entry against tmax — is at most 1 % of every set: the cap tests/test_gpu_anyhit_exact.py relies on."""
import numpy as np
import pytest

import anyhit_ref as ah
import ao_ref
from conftest import CORNELL_CAM, oracle_scene
from oracle import binding as ob
from test_gpu_adversarial import _grazing_rays, _grid_scene, _random_rays, _sliver_scene

F = np.float32
INF = F(np.inf)
GAP_CAP = 0.01
N_RAYS = 1024

# name -> (triangles(rng), spheres, grazing-ray recipe (angle range, distance range), spread of the random rays)
FAMILIES = {
    "slivers": (lambda r: _sliver_scene(r, 3000, 1.0, 30.0, 10.0, 1e4, 12.0), (), (1e-8, 1e-2, 1.0, 150.0), 20.0),
    "needles": (lambda r: _sliver_scene(r, 3000, 0.01, 2.0, 1e2, 1e5, 0.5), (), (1e-7, 1e-1, 0.1, 10.0), 0.8),
    "field+spheres": (lambda r: _grid_scene(r, 36, 0.5, 0.7),
                      tuple(((x, 0.0, z), 0.9) for x in (-6.0, -2.0, 2.0, 6.0) for z in (-6.0, -2.0, 2.0, 6.0)), (1e-6, 1e-1, 0.5, 40.0), 11.0),
    "duplicates": (lambda r: np.repeat(_sliver_scene(r, 1000, 0.5, 6.0, 1.0, 20.0, 4.0), 3, axis=0), (), (1e-6, 1.0, 0.5, 30.0), 6.0),
}
ASSETS = {"scene.xml": (None, (0.0, 10.0, 0.0), 20.0), "cornell.xml": (CORNELL_CAM, (0.0, 1.0, 0.0), 1.0)}   # camera, centre, spread

_family = {}


def family(name):
    """(triangles [n,3,3], spheres, grazing rays (o, d), random rays (o, d)) of a family: seeded by the name, computed once."""
    if name not in _family:
        make, spheres, (th_lo, th_hi, d_lo, d_hi), spread = FAMILIES[name]
        rng = np.random.default_rng(900 + sorted(FAMILIES).index(name))
        tris = make(rng)
        _family[name] = (tris, spheres, _grazing_rays(rng, tris, N_RAYS, th_lo, th_hi, d_lo, d_hi), _random_rays(rng, N_RAYS, spread))
    return _family[name]


def limits_around(tstar):
    """[(label, tmax [R], may_hit)]: the limits of the sandwich; may_hit = a ray with a finite t* has t* < tmax."""
    with np.errstate(invalid="ignore", over="ignore"):
        return [("t*", tstar, False), ("t* - 1 ulp", np.nextafter(tstar, F(0)), False), ("t* + 1 ulp", np.nextafter(tstar, INF), True),
                ("0.5 t*", F(0.5) * tstar, False), ("0.999 t*", F(0.999) * tstar, False), ("1.001 t*", F(1.001) * tstar, True),
                ("2 t*", F(2.0) * tstar, True)]


_tables = {}


def tables(name):
    """Per scene, computed once: [(set label, o, d, t*, T [R,P], no-limit (lower, upper), [(limit label, tmax, lower, upper)])]."""
    if name in _tables:
        return _tables[name]
    if name in FAMILIES:
        tris, spheres, grazing, rand = family(name)
        sc = ob.OracleScene()
        for c, r in spheres:
            sc.add_sphere(c, r)
        for t in tris:
            sc.add_triangle(t[0], t[1], t[2])
        sc.build_bvh()
        buf = sc.buffers()
        sets = [("grazing",) + grazing, ("random",) + rand]
    else:
        from test_gpu_occluded import camera_rays
        cam, centre, spread = ASSETS[name]
        sc, buf = oracle_scene(name)
        u = ob.make_uniforms(64, 36, sc.prim_count, sc.triangle_count, cam=cam)
        o, d = _random_rays(np.random.default_rng(77), N_RAYS, spread)
        sets = [("camera",) + camera_rays(u, N_RAYS, seed=5), ("random", o + np.asarray(centre, np.float32), d)]
    out = []
    for label, o, d in sets:
        ts = ao_ref.closest_t(o, d, buf, ob.first_hit)
        lims = limits_around(ts)
        res, T = ah.bounds(o, d, [INF] + [t for _, t, _ in lims], buf, want_t=True)
        out.append((label, o, d, ts, T, res[0], [(l, t, lo, up) for (l, t, _), (lo, up) in zip(lims, res[1:])]))
    _tables[name] = out
    return out


SCENES = sorted(FAMILIES) + sorted(ASSETS)


@pytest.mark.parametrize("name", SCENES)
def test_without_a_limit_the_walk_finds_what_the_oracle_finds(name):
    for label, o, d, ts, T, (lower, upper), _ in tables(name):
        hit = np.isfinite(ts)
        bad = np.flatnonzero(lower != hit)
        assert bad.size == 0, (name, label, bad[:4], o[bad[:4]], d[bad[:4]], ts[bad[:4]])
        assert not (lower & ~upper).any()
        assert 0.02 < hit.mean() < 0.98, (name, label, hit.mean())               # the set exercises both answers


@pytest.mark.parametrize("name", SCENES)
def test_the_closest_t_is_one_of_the_accepted_primitive_tests(name):
    for label, o, d, ts, T, _, _ in tables(name):
        hit = np.isfinite(ts)
        among = (T.view(np.uint32) == ts.view(np.uint32)[:, None]).any(1)
        bad = np.flatnonzero(hit & ~among)
        assert bad.size == 0, (name, label, bad[:4], o[bad[:4]], d[bad[:4]], ts[bad[:4]])


@pytest.mark.parametrize("name", SCENES)
def test_the_closest_hit_lies_between_the_two_bounds_around_tstar(name):
    for label, o, d, ts, T, _, lims in tables(name):
        hit = np.isfinite(ts)
        for lim, tmax, lower, upper in lims:
            with np.errstate(invalid="ignore"):
                mid = ao_ref.occluded(ts, d, tmax)
            where = "%s/%s/tmax = %s" % (name, label, lim)
            bad = np.flatnonzero(lower & ~mid)
            assert bad.size == 0, (where, "occluded in reference order although t* >= tmax", bad[:4], o[bad[:4]], d[bad[:4]], tmax[bad[:4]], ts[bad[:4]])
            bad = np.flatnonzero(mid & ~upper)
            assert bad.size == 0, (where, "t* < tmax although no primitive test is accepted below tmax", bad[:4], o[bad[:4]], d[bad[:4]], tmax[bad[:4]], ts[bad[:4]])
            if not mid.any():                                                    # tmax at t* and below: nothing is in the way
                assert not lower.any() and not upper.any(), (where, np.flatnonzero(upper)[:4])
            else:
                np.testing.assert_array_equal(mid, hit)
            gap = int((upper & ~lower).sum())
            print("%-45s gap %d of %d (t* < tmax: %d)" % (where, gap, ts.size, int(mid.sum())))
            assert gap <= GAP_CAP * ts.size, (where, gap)


def test_degenerate_restates_ot_degenerate():
    tiny, lim = F(2.0 ** -20), F(100.0)
    ok_d, ok_o = (0.5, -0.6, 0.7), (1.0, -2.0, 3.0)
    cases = [
        (ok_o, ok_d, False),
        (ok_o, (tiny, 0.5, 0.5), False), (ok_o, (0.5, -tiny, 0.5), False),                           # 2^-20 itself is taken
        (ok_o, (np.nextafter(tiny, F(0)), 0.5, 0.5), True), (ok_o, (0.5, 0.5, -np.nextafter(tiny, F(0))), True),
        (ok_o, (2.0, 0.5, 0.5), False), (ok_o, (0.5, -2.0, 0.5), False),                             # 2 itself is taken
        (ok_o, (np.nextafter(F(2), F(3)), 0.5, 0.5), True), (ok_o, (0.5, 0.5, -np.nextafter(F(2), F(3))), True),
        (ok_o, (0.0, 0.6, 0.8), True), (ok_o, (0.6, -0.0, 0.8), True),
        (ok_o, (np.nan, 0.6, 0.8), True), (ok_o, (0.6, np.inf, 0.8), True), (ok_o, (0.6, 0.8, -np.inf), True),
        ((lim, 0.0, 0.0), ok_d, False), ((0.0, -lim, 0.0), ok_d, False),                             # an origin at the limit is taken
        ((np.nextafter(lim, INF), 0.0, 0.0), ok_d, True), ((0.0, 0.0, -np.nextafter(lim, INF)), ok_d, True),
        ((np.nan, 0.0, 0.0), ok_d, True), ((0.0, np.inf, 0.0), ok_d, True),
    ]
    o = np.array([c[0] for c in cases], np.float32)
    d = np.array([c[1] for c in cases], np.float32)
    np.testing.assert_array_equal(ah.degenerate(o, d, lim), np.array([c[2] for c in cases]))
    assert not ah.degenerate(o[:1] * 1e30, d[:1], INF).any()                                         # a scene without triangles: no limit
    tri = np.zeros((2, 3, 4), np.float32)
    tri[0, 0] = (1000.0, 0, 0, 0)                                                                    # a sphere's centre does not count
    tri[1] = ((1, -3, 2, 1), (0.5, 0, 0, 0), (0, 0, 0, 0))
    assert ah.o_limit_of(tri) == F(192.0) and ah.o_limit_of(tri[:1]) == INF


def test_reach_does_not_depend_on_the_numbering_of_the_nodes():
    """The device builder of big scenes puts children in front of their parent: root 0 -> (3, 1), 3 -> (2, 4); leaves 1, 2, 4."""
    bvh = np.zeros((5, 2, 4), np.float32)
    w = bvh.view(np.int32)
    w[0, 0, 3], w[0, 1, 3] = 3, -1
    w[3, 0, 3], w[3, 1, 3] = 2, -4
    w[1, 0, 3], w[1, 1, 3] = 0, 1           # prim_idx[0:1]
    w[2, 0, 3], w[2, 1, 3] = 1, 1           # prim_idx[1:2]
    w[4, 0, 3], w[4, 1, 3] = 2, 2           # prim_idx[2:4]
    idx = np.array([3, 0, 2, 1], np.int32)
    levels, parent, leaf_of = ah.tree_tables(bvh, idx)
    assert [l.tolist() for l in levels] == [[3, 1], [2, 4]] and parent.tolist() == [-1, 0, 3, 0, 3] and leaf_of.tolist() == [2, 4, 4, 1]
    passed = np.array([[1, 1, 1, 0, 1], [1, 1, 1, 1, 1], [0, 1, 1, 1, 1], [1, 0, 1, 1, 0]], bool)
    np.testing.assert_array_equal(ah.reach(bvh, idx, passed), np.array([[0, 0, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 0]], bool))
    w[3, 0, 3] = 1                          # two parents for node 1
    with pytest.raises(AssertionError):
        ah.tree_tables(bvh, idx)
