"""GPU tests of the two any-hit walks (mpt_trace_occluded, mpt_ao_image) against tests/anyhit_ref.py, the brute-force restatement of
the any-hit walk itself — not against the closest hit, which cannot be asserted at the hit: with tmax one ulp above t* a ray may
correctly be NOT occluded in reference order (its leaf's slab entry rounds to >= tmax).  With
  lower = occluded_reference      (some accepted primitive with t < tmax whose boxes, root to leaf, all pass the slab test against tmax)
  upper = occluded_any_primitive  (some accepted primitive with t < tmax)
the contract of include/mpt.h is, with 0 mismatches:
  MPT_WALK_REFERENCE == lower, flags 0;   MPT_WALK_OWN / MPT_WALK_AUTO (where it is the own tree): lower <= answer <= upper, and == lower
  for every ray with a flag (1: direction or origin, 8: stack overflow — both re-traced in reference order); flags & 1 == ot_degenerate.
The limits sit where a walk goes wrong: at t*, one ulp either side, half and twice t*, +inf, 3e38, just above 1e-4; the scenes are the
adversarial families of tests/test_anyhit_cpu.py through the three host builders and the device builder, a scene that is wholly in
LDS, one with 17 spheres (no own tree) and one of exactly MPT_AUTO_ORDERED_PRIMS triangles (AUTO = the own tree, leaves of <= 2)."""
import numpy as np
import pytest

import anyhit_ref as ah
import ao_ref
from oracle import binding as ob
from test_anyhit_cpu import FAMILIES, GAP_CAP, family
from test_gpu_adversarial import _build, _grazing_rays, _grid_scene, _random_rays, _sliver_scene

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)
COUNTS = (1, 63, 64, 65, 255, 256, 257, 4096 + 3)      # the kernels use 256-thread blocks
N = COUNTS[-1]
N_PRIMARY = 1366                                       # grazing rays, and as many random ones; the rest: AO-style rays and the edge rays
SETS = ("grazing", "random", "ao", "edge")

# key -> (family of test_anyhit_cpu.py or None, tree: a host builder 0 / 1 / 2 or "device")
CASES = {
    "slivers/sweep": ("slivers", 0), "needles/binned": ("needles", 1), "field+spheres/lbvh": ("field+spheres", 2),
    "duplicates/binned": ("duplicates", 1), "slivers/device": ("slivers", "device"),
    "tiny/sweep": (None, 0), "17 spheres/sweep": (None, 0), "field 64x64/device": (None, "device"),
}


def _geometry(key):
    """(triangles, spheres, grazing recipe, spread, rng) of a case."""
    fam = CASES[key][0]
    rng = np.random.default_rng(4000 + sorted(CASES).index(key))
    if fam is not None:
        tris, spheres = family(fam)[:2]
        return tris, spheres, FAMILIES[fam][2], FAMILIES[fam][3], rng
    if key.startswith("tiny"):                                          # 40 triangles and 2 spheres: tree and primitives all in LDS
        return _sliver_scene(rng, 40, 0.5, 3.0, 1.0, 10.0, 1.0), (((0.5, 0.0, 0.0), 0.6), ((-1.0, 0.5, 0.3), 0.4)), (1e-6, 1e-1, 0.5, 10.0), 1.5, rng
    if key.startswith("17 spheres"):                                    # one more than the always list holds: no own tree
        spheres = tuple(((float(x), 1.0, float(z)), 0.8) for x, z in rng.uniform(-4.5, 4.5, (17, 2)))
        return _grid_scene(rng, 20, 0.5, 0.3), spheres, (1e-6, 1e-1, 0.5, 40.0), 6.0, rng
    return _grid_scene(rng, 64, 0.5, 0.7), (), (1e-6, 1e-1, 0.5, 60.0), 18.0, rng      # 8192 triangles = MPT_AUTO_ORDERED_PRIMS


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _far_direction(buf, oo, candidates):
    """The direction from the far origin oo to the first candidate point for which the two bounds agree (a hit, if there is one).  From
    10 x o_limit a sphere test is rounding noise (b * b - a * c cancels), so a ray that passes beside a sphere's box is a gap ray by
    chance; the choice is made from the reference alone."""
    dd = np.array([_unit(c - oo.astype(np.float64)) for c in candidates], np.float32)
    (lower, upper), = ah.bounds(np.broadcast_to(oo, dd.shape), dd, [INF], buf)
    same = np.flatnonzero(lower == upper)
    assert same.size, "no far ray without a gap"
    hit = np.flatnonzero(lower & upper)
    return dd[hit[0] if hit.size else same[0]]


def _edge_rays(buf, o_limit, centre, size, target, candidates):
    """The rays a walk treats specially: (origins, directions, limits; None = take the limit from t* like every other ray)."""
    box = np.asarray(buf[0], np.float32).reshape(-1, 2, 4)
    tiny = F(2.0 ** -20)
    o, d, tm = [], [], []

    def add(oo, dd, t=None):
        o.append(np.asarray(oo, np.float32)), d.append(np.asarray(dd, np.float32)), tm.append(t)

    base_o = (centre + size * np.array([0.23, 0.31, -0.27])).astype(np.float32)
    base_d = _unit(centre + size * np.array([-0.05, -0.1, 0.08]) - base_o).astype(np.float32)
    for axis in range(3):                                               # each direction component 0.0 and -0.0 in turn
        for zero in (0.0, -0.0):
            dd = base_d.copy()
            dd[axis] = zero
            add(base_o, dd, INF), add(base_o, dd)
    k = 0
    for node in (0, min(1, box.shape[0] - 1), box.shape[0] - 1):        # an origin ON a box plane with that component zero: 0 * inf = NaN
        for axis in range(3):
            for plane in (0, 1):
                oo = (0.5 * (box[node, 0, :3].astype(np.float64) + box[node, 1, :3])).astype(np.float32)
                oo[axis] = box[node, plane, axis]
                dd = np.array([0.6, -0.64, 0.48], np.float32)
                dd[axis] = (0.0, -0.0)[k & 1]
                add(oo, dd, INF)
                k += 1
    for axis in range(3):                                               # |d_i| at 2^-20 (taken by the own walk) and one ulp below (flag 1)
        for v in (tiny, -np.nextafter(tiny, F(0))):
            dd = base_d.copy()
            dd[axis] = v
            add(base_o, dd)
    for length in (0.5, 1.9):                                           # a non-unit direction: a != 1 in the sphere test
        for oo in (target + size * np.array([0.4, 0.5, 0.3]), target + np.array([0.05, -0.02, 0.03])):
            add(oo, (_unit(target - oo + 1e-3) * length), INF if length == 0.5 else None)
    add(base_o, (2.5, 0.3, -0.4), INF)                                  # a component beyond 2: flag 1
    add(base_o, (np.nan, -0.6, -0.8), INF)                              # a NaN direction: not occluded, no walk
    for t in (np.nan, 0.0, -1.0, 1e-4):                                 # !(tmax > 1e-4): not occluded, no walk
        add(base_o, base_d, F(t))
    for axis in range(3):                                               # origins at 10 x o_limit: flag 1
        oo = base_o.astype(np.float64)
        oo[axis] = 10.0 * float(o_limit) * (-1.0 if axis == 1 else 1.0)
        add(oo, _far_direction(buf, oo.astype(np.float32), candidates), INF)
    return np.array(o, np.float32), np.array(d, np.float32), tm


def _limits(tstar, explicit):
    """Per-ray limits, cycled over: around t* for a hit, {+inf, 1e30} for a miss; `explicit` entries that are not None win."""
    n = tstar.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        hit = np.stack([tstar, np.nextafter(tstar, F(0)), np.nextafter(tstar, INF), F(0.5) * tstar, F(2.0) * tstar, np.full(n, INF),
                        np.full(n, F(3e38)), np.full(n, np.nextafter(F(1e-4), F(1))), np.full(n, F(2e-4))])
    miss = np.array([INF, F(1e30)], np.float32)
    i = np.arange(n)
    tmax = np.where(np.isfinite(tstar), hit[i % 9, i], miss[i % 2]).astype(np.float32)
    for k, t in enumerate(explicit):
        if t is not None:
            tmax[k] = t
    return tmax


def _closest(o, d, buf):
    """The oracle's closest hit per ray: (t* [n], +inf for a miss; normal facing the ray [n,3])."""
    t = np.full(o.shape[0], INF, np.float32)
    nrm = np.zeros((o.shape[0], 3), np.float32)
    for i in range(o.shape[0]):
        ti, p, ni, _ = ob.first_hit(o[i], d[i], buf)
        if p >= 0:
            t[i], nrm[i] = ti, ni
    return t, nrm


_cases = {}


def case(ctx, key):
    """The case's scene on the context and, computed once per case and never modified: buffers in the reference's format, o_limit, the
    rays (shuffled, so that every prefix mixes the sets), their set, t*, the limits and both bounds for the limits and for no limit."""
    from metalpathtracer_amd import host
    tree = CASES[key][1]
    if key not in _cases:
        tris, spheres, (th_lo, th_hi, d_lo, d_hi), spread, rng = _geometry(key)
        if tree == "device":
            sc = host.Scene()
            for c, r in spheres:
                sc.addSphere([float(x) for x in c], float(r))
            for t in tris:
                sc.addTriangle([float(x) for x in t[0]], [float(x) for x in t[1]], [float(x) for x in t[2]])
            buf = host.make_ready(ctx, sc, host.BVH_DEVICE)            # the tree as it comes back from the device
        else:
            buf = _build(tris, spheres, tree)[1]
        o_limit = ah.o_limit_of(buf[1])
        assert o_limit == F(64.0) * np.abs(tris).max()
        centre = tris.reshape(-1, 3).mean(0)
        size = float(tris.reshape(-1, 3).std(0).max())
        target = np.asarray(spheres[0][0], np.float64) if spheres else tris[0].mean(0).astype(np.float64)
        og, dg = _grazing_rays(rng, tris, N_PRIMARY, th_lo, th_hi, d_lo, d_hi)
        orr, dr = _random_rays(rng, N_PRIMARY, spread)
        for k, (c, r) in enumerate(spheres[:16]):                       # origins inside the spheres
            orr[-1 - k] = np.asarray(c, np.float32) + F(0.4 * r) * _unit(rng.normal(size=3)).astype(np.float32)
        oe, de, explicit = _edge_rays(buf, o_limit, centre, size, target, tris[:: max(1, len(tris) // 24)].mean(1).astype(np.float64))
        # AO-style rays: from the hit points of the primaries, P + 1e-4 n, cosine-distributed about n
        op, dp = np.concatenate([og, orr]), np.concatenate([dg, dr])
        tp, nrm = _closest(op, dp, buf)
        n_ao = N - 2 * N_PRIMARY - oe.shape[0]
        pick = rng.choice(np.flatnonzero(np.isfinite(tp)), n_ao)
        P = op[pick] + tp[pick, None] * dp[pick]
        oa = (P + F(1e-4) * nrm[pick]).astype(np.float32)
        da = ao_ref.normalize(nrm[pick] + _unit(rng.normal(size=(n_ao, 3))).astype(np.float32)).astype(np.float32)
        o, d = np.concatenate([op, oa, oe]), np.concatenate([dp, da, de])
        kind = np.repeat(np.arange(4), (N_PRIMARY, N_PRIMARY, n_ao, oe.shape[0]))
        tstar = np.concatenate([tp, _closest(o[2 * N_PRIMARY:], d[2 * N_PRIMARY:], buf)[0]])
        tmax = _limits(tstar, [None] * (N - oe.shape[0]) + explicit)
        perm = np.random.default_rng(1).permutation(N)
        o, d, kind, tstar, tmax = (np.ascontiguousarray(a[perm]) for a in (o, d, kind, tstar, tmax))
        (lower, upper), (lower_inf, upper_inf) = ah.bounds(o, d, [tmax, INF], buf)
        c = dict(buf=buf, o_limit=o_limit, o=o, d=d, kind=kind, tstar=tstar, tmax=tmax, lower=lower, upper=upper, lower_inf=lower_inf,
                 upper_inf=upper_inf, degenerate=ah.degenerate(o, d, o_limit), n_spheres=len(spheres))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        # what the reference alone says about the inputs, before any walk is asked: the own walk's freedom is small, both answers occur
        assert o.shape == (N, 3) and not (lower & ~upper).any() and not (lower_inf & ~upper_inf).any()
        for s, label in enumerate(SETS):
            m = kind == s
            for lo, up in ((lower, upper), (lower_inf, upper_inf)):
                assert (up & ~lo & m).sum() <= GAP_CAP * m.sum(), (key, label, int((up & ~lo & m).sum()), int(m.sum()))
            if label != "edge":
                assert 0.02 < lower[m].mean() < 0.98, (key, label, lower[m].mean())
        _cases[key] = c
        if tree == "device":
            return c
    c = _cases[key]
    if tree == "device":
        ctx.build_and_upload(c["buf"][1], c["buf"][2])
        bvh, idx = ctx.download_bvh()                                   # the build is deterministic: the cached bounds are this tree's
        np.testing.assert_array_equal(bvh.view(np.uint32), c["buf"][0].view(np.uint32))
        np.testing.assert_array_equal(idx, c["buf"][3])
    else:
        ctx.upload_scene(*c["buf"])
    return c


def describe(c, i, got, flags, lower=None, upper=None):
    lower, upper = c["lower"] if lower is None else lower, c["upper"] if upper is None else upper
    return "\n".join("ray %d [%s] o=%r d=%r tmax=%r t*=%r lower=%d upper=%d answer=%d flags=%d" % (
        k, SETS[c["kind"][k]], c["o"][k].tolist(), c["d"][k].tolist(), float(c["tmax"][k]), float(c["tstar"][k]), lower[k], upper[k], got[k],
        flags[k]) for k in np.asarray(i)[:6])


def check_reference(c, where, got, flags, lower, n):
    bad = np.flatnonzero(got != lower[:n])
    assert bad.size == 0, "%s: the reference-order walk differs from the brute force on %d rays\n%s" % (where, bad.size, describe(c, bad, got, flags))
    assert not flags.any(), where


def check_own(c, where, got, flags, lower, upper, n):
    """The own tree answered: the sandwich, the flags, and the reference-order answer for every flagged ray."""
    bad = np.flatnonzero((lower[:n] & ~got) | (got & ~upper[:n]))
    assert bad.size == 0, "%s: the own walk leaves [lower, upper] on %d rays\n%s" % (where, bad.size, describe(c, bad, got, flags, lower, upper))
    bad = np.flatnonzero((flags != 0) & (got != lower[:n]))
    assert bad.size == 0, "%s: %d flagged rays differ from the reference-order answer\n%s" % (where, bad.size, describe(c, bad, got, flags, lower, upper))
    bad = np.flatnonzero(((flags & 1) != 0) != c["degenerate"][:n])
    assert bad.size == 0, "%s: flag 1 differs from ot_degenerate on %d rays\n%s" % (where, bad.size, describe(c, bad, got, flags, lower, upper))
    assert not (flags & ~np.uint32(1 | 8)).any(), where


@pytest.mark.parametrize("key", sorted(CASES))
def test_reference_walk_equals_the_brute_force(gpu_ctx, key):
    from metalpathtracer_amd import capi
    c = case(gpu_ctx, key)
    info = gpu_ctx.accel_info()
    walks = [capi.WALK_REFERENCE]
    if not info["ordered_ok"]:
        walks.append(capi.WALK_OWN)                                     # OWN without an own tree is REFERENCE
    if info["auto_pipeline"] != capi.PIPE_ORDERED:
        walks.append(capi.WALK_AUTO)                                    # AUTO below MPT_AUTO_ORDERED_PRIMS is REFERENCE
    assert info["ordered_ok"] == (0 if key.startswith("17 spheres") else 1), (key, info)
    for walk in walks:
        for n in COUNTS:
            got, flags = gpu_ctx.trace_occluded(c["o"][:n], c["d"][:n], c["tmax"][:n], walk=walk)
            check_reference(c, "%s/walk %d/%d rays" % (key, walk, n), got, flags, c["lower"], n)
        got, flags = gpu_ctx.trace_occluded(c["o"], c["d"], None, walk=walk)                          # tmax = NULL: +inf for every ray
        bad = np.flatnonzero(got != c["lower_inf"])
        assert bad.size == 0 and not flags.any(), "%s/walk %d/no limit\n%s" % (key, walk, describe(c, bad, got, flags, c["lower_inf"], c["upper_inf"]))


@pytest.mark.parametrize("key", sorted(k for k in CASES if not k.startswith("17 spheres")))
def test_own_walk_lies_between_the_two_bounds(gpu_ctx, key):
    from metalpathtracer_amd import capi
    c = case(gpu_ctx, key)
    info = gpu_ctx.accel_info()
    assert info["ordered_ok"] == 1 and info["always_spheres"] == c["n_spheres"], (key, info)
    big = key.startswith("field 64x64")
    assert (info["auto_pipeline"] == capi.PIPE_ORDERED) == big, (key, info)
    if big:
        assert gpu_ctx.build_info()["built_leaf_max"] == 2 and c["buf"][1].shape[0] == gpu_ctx.build_info()["auto_ordered_prims"]
    for walk in (capi.WALK_OWN, capi.WALK_AUTO) if big else (capi.WALK_OWN,):
        for n in COUNTS:
            got, flags = gpu_ctx.trace_occluded(c["o"][:n], c["d"][:n], c["tmax"][:n], walk=walk)
            check_own(c, "%s/walk %d/%d rays" % (key, walk, n), got, flags, c["lower"], c["upper"], n)
        gap = c["upper"] & ~c["lower"]                                  # (got, flags: the whole set)
        print("%-22s walk %d: flag 1 on %d rays, flag 8 on %d of %d; rays the own walk may answer either way: %d, answered occluded %s, not occluded %s"
              % (key, walk, int((flags & 1).astype(bool).sum()), int((flags & 8).astype(bool).sum()), N, int(gap.sum()),
                 np.flatnonzero(gap & got).tolist(), np.flatnonzero(gap & ~got).tolist()))
        got, flags = gpu_ctx.trace_occluded(c["o"], c["d"], None, walk=walk)
        check_own(c, "%s/walk %d/no limit" % (key, walk), got, flags, c["lower_inf"], c["upper_inf"], N)


def test_stack_overflow_is_answered_in_reference_order(gpu_ctx, monkeypatch):
    """MPT_OT_STACK=2 (the smallest stack a context accepts): any_hit_own pushes up to three children per node, so piles of overlapping
    slivers overflow it.  An overflow is an ordinary, handled path: the ray is traced again by the reference-order walk."""
    from metalpathtracer_amd import capi
    default = {}
    for key in ("slivers/sweep", "duplicates/binned"):
        c = case(gpu_ctx, key)
        default[key] = int((gpu_ctx.trace_occluded(c["o"], c["d"], c["tmax"], walk=capi.WALK_OWN)[1] & 8).astype(bool).sum())
    monkeypatch.setenv("MPT_OT_STACK", "2")
    ctx = capi.Context(0)
    try:
        for key in ("slivers/sweep", "duplicates/binned"):
            c = _cases[key]
            ctx.upload_scene(*c["buf"])
            assert ctx.accel_info()["ordered_ok"] == 1
            for tmax, lower, upper in ((c["tmax"], c["lower"], c["upper"]), (None, c["lower_inf"], c["upper_inf"])):
                got, flags = ctx.trace_occluded(c["o"], c["d"], tmax, walk=capi.WALK_OWN)
                over = (flags & 8) != 0
                print("%-20s %s: flag 8 on %d of %d rays with a stack of 2 (%d with the default 8, per-ray limits), flag 1 on %d"
                      % (key, "per-ray limits" if tmax is not None else "no limit", int(over.sum()), N, default[key], int((flags & 1).astype(bool).sum())))
                assert over.any(), key
                check_own(c, "%s/stack 2" % key, got, flags, lower, upper, N)
    finally:
        ctx.close()


# ---- ambient occlusion through the same walks --------------------------------------------------------------------------------------
AO_W, AO_H, AO_N = 24, 13, 65
AO_SEED = (0x51, 3)
AO_RADII = (0.5, 0.0)
AO_CAM = dict(pos=(0.5, 3.0, 8.0), fwd=(0.0, -0.33035, -0.94386), up=(0.0, 1.0, 0.0), vfov=60.0)
_ao = {}


def ao_case(ctx, name):
    """Per scene, once: (buffers, uniforms, guides, surface mask, per radius the (lower, upper) [H,W,65] of samples 0..64)."""
    from metalpathtracer_amd import capi, host
    if name == "scene.xml":
        from test_gpu_parity import setup
        buf, u = setup(ctx, name, AO_W, AO_H)
    else:
        buf = case(ctx, name)["buf"]
        P = buf[1].shape[0]
        u = host.make_uniforms(AO_W, AO_H, P, P - 16, cam=AO_CAM)
        ctx.resize(AO_W, AO_H)
        ctx.set_uniforms(u)
    if name not in _ao:
        ad, nc, _ = ctx.read_aovs()
        surface, o, d = ao_ref.sample_rays(ad, nc, u, 0, AO_N, AO_SEED)
        assert 0.2 < surface.mean() < 1.0, (name, surface.mean())
        oo = np.repeat(o[surface], AO_N, axis=0)
        dd = d[surface].reshape(-1, 3)
        res = ah.bounds(oo, dd, [F(r) if r > 0 else INF for r in AO_RADII], buf)
        per = {}
        for r, (lo, up) in zip(AO_RADII, res):
            full = np.zeros((2,) + surface.shape + (AO_N,), bool)
            full[0][surface] = lo.reshape(-1, AO_N)
            full[1][surface] = up.reshape(-1, AO_N)
            full.setflags(write=False)
            per[r] = full
        _ao[name] = (buf, u, ad, nc, surface, per)
    return _ao[name]


@pytest.mark.parametrize("radius", AO_RADII)
@pytest.mark.parametrize("n_samples", [3, 65])
@pytest.mark.parametrize("name", ["field+spheres/lbvh", "scene.xml"])
def test_ao_counts_are_the_sums_of_the_brute_force(gpu_ctx, name, n_samples, radius):
    """k_ao's counts are popcounts of ballots over a pixel's group of lanes: 3 samples sit in 2 lanes and 2 rounds, 65 in 64 lanes and 2
    rounds with one live lane in the second — a wrong `live` mask in the wave-uniform loops of either walk shows as a wrong count."""
    from metalpathtracer_amd import capi
    buf, u, ad, nc, surface, per = ao_case(gpu_ctx, name)
    assert gpu_ctx.accel_info()["ordered_ok"] == 1
    lower = per[radius][0][..., :n_samples].sum(-1).astype(np.uint32)
    upper = per[radius][1][..., :n_samples].sum(-1).astype(np.uint32)
    assert per[radius][0].any() and lower.sum() < surface.sum() * n_samples       # both answers occur among the 65 samples of the scene
    uu = capi.Uniforms.from_buffer_copy(bytes(u))
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        ao, occ = gpu_ctx.ao_image(ad, nc, uu, samples=n_samples, radius=radius, seed=AO_SEED, walk=walk)
        print("%s N %d radius %g walk %d: occluded %d, lower %d, upper %d" % (name, n_samples, radius, walk, int(occ.sum()), int(lower.sum()), int(upper.sum())))
        if walk == capi.WALK_REFERENCE:
            bad = np.argwhere(occ != lower)
            assert bad.size == 0, (name, walk, bad[:4].tolist(), occ[occ != lower][:4], lower[occ != lower][:4])
        else:
            bad = np.argwhere((occ < lower) | (occ > upper))
            assert bad.size == 0, (name, walk, bad[:4].tolist())
        want = np.where(surface, (F(n_samples) - occ.astype(np.float32)) / F(n_samples), F(1)).astype(np.float32)
        np.testing.assert_array_equal(ao.view(np.uint32), want.view(np.uint32))
        assert (occ[~surface] == 0).all()
