"""GPU tests of mpt_trace_occluded: both any-hit walks against the oracle's closest hit.  For every ray "occluded" must equal t* < tmax
(t* = the oracle's closest t): 0 mismatches.  A ray that is occluded with t* >= tmax breaks the exact direction of include/mpt.h and
is a bug, always; one with t* < tmax that is not occluded would be the reference's artefact (a hit in front of its own leaf's slab
entry, tmax between the two) or, with tmax within a rounding of t*, a leaf whose slab entry rounds to >= tmax although its hit lies
below (seen at tmax = nextafter(t*) and at 1.001 t* on sliver scenes), and is reported with the ray — the limits and scenes used here
keep tmax away from t* so that neither occurs.  tests/test_gpu_anyhit_exact.py puts the limit AT t* and checks both walks exactly,
against a brute-force restatement of the any-hit walk itself (tests/anyhit_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import ao_ref
from conftest import CORNELL_CAM, scene_path
from oracle import binding as ob
from test_gpu_parity import setup

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = (1, 63, 64, 65, 4096 + 3)
N = COUNTS[-1]
SCENES = {"cornell.xml": CORNELL_CAM, "scene.xml": None}       # everything in LDS / nodes and primitives partly in global memory
GUIDE_W, GUIDE_H = 48, 27


def camera_rays(u, n, seed):
    """n rays from the camera through uniformly drawn image positions."""
    rng = np.random.default_rng(seed)
    cam, first, vu, vv = ao_ref._cam(u)
    uv = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    d = ao_ref.normalize(((first + uv[:, :1] * vu) + uv[:, 1:] * vv) - cam).astype(np.float32)
    return np.broadcast_to(cam, d.shape).copy(), d


def limits_around(tstar, factors):
    """tmax = f * t*, f taken in turn from `factors`; +inf for a miss."""
    f = np.asarray(factors, np.float32)[np.arange(tstar.shape[0]) % len(factors)]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(tstar), f * tstar, F(np.inf)).astype(np.float32)


def edge_rays(u):
    """Set (c): zero direction components, a NaN direction, and the limits that ask for nothing."""
    cam = ao_ref._cam(u)[0]
    o, d, tmax = [], [], []
    for dirv in ((0, -1, 0), (0, 0, -1), (0, -0.6, -0.8), (0.6, 0, -0.8), (-0.6, -0.8, 0)):          # zero components, limits as set (a)
        for t in (np.inf, None, None):
            o.append(cam), d.append(dirv), tmax.append(t)
    o.append(cam), d.append((np.nan, -0.6, -0.8)), tmax.append(np.inf)                               # a NaN direction
    for t in (np.nan, 0.0, -1.0, 1e-4):                                                              # !(tmax > 1e-4)
        o.append(cam), d.append((0.01, -0.6, -0.8)), tmax.append(t)
    return np.array(o, np.float32), np.array(d, np.float32), tmax


_sets = {}


def ray_sets(ctx, name):
    """Per scene, computed once: [(label, origins, directions, tmax, t*)] for sets (a), (b), (c).  Leaves the scene uploaded."""
    buf, u = setup(ctx, name, GUIDE_W, GUIDE_H, cam=SCENES[name])
    if name in _sets:
        return _sets[name]
    out = []
    o, d = camera_rays(u, N, seed=21)                                                    # (a)
    ts = ao_ref.closest_t(o, d, buf, ob.first_hit)
    assert np.isfinite(ts).mean() > 0.3
    out.append(("camera", o, d, limits_around(ts, (0.5, 0.99, 1.01, 2.0)), ts))
    ad, nc, _ = ctx.read_aovs()                                                          # (b): AO-style rays from the guide pixels
    per_pixel = 8
    surface, po, pd = ao_ref.sample_rays(ad, nc, u, 0, per_pixel, seed=(3, 1))
    assert surface.sum() * per_pixel >= N, (name, int(surface.sum()))
    d = pd[surface].reshape(-1, 3)[:N]
    o = np.repeat(po[surface], per_pixel, axis=0)[:N]
    ts = ao_ref.closest_t(o, d, buf, ob.first_hit)
    out.append(("ao", o, d, np.asarray((0.25, 1.0, np.inf), np.float32)[np.arange(N) % 3], ts))
    o, d, tm = edge_rays(u)                                                              # (c)
    ts = ao_ref.closest_t(o, d, buf, ob.first_hit)
    fill = limits_around(ts, (0.99, 1.01))
    tmax = np.array([fill[i] if t is None else t for i, t in enumerate(tm)], np.float32)
    out.append(("edge", o, d, tmax, ts))
    _sets[name] = out
    return out


def check(label, got, o, d, tmax, tstar):
    want = ao_ref.occluded(tstar, d, tmax)
    wrong = np.flatnonzero(got & ~want)
    assert wrong.size == 0, "%s: occluded although t* >= tmax (the exact direction): rays %s, o %s d %s tmax %s t* %s" % (
        label, wrong[:4], o[wrong[:4]], d[wrong[:4]], tmax[wrong[:4]], tstar[wrong[:4]])
    missed = np.flatnonzero(want & ~got)
    assert missed.size == 0, "%s: not occluded although t* < tmax: rays %s, o %s d %s tmax %s t* %s" % (
        label, missed[:4], o[missed[:4]], d[missed[:4]], tmax[missed[:4]], tstar[missed[:4]])


@pytest.mark.parametrize("walk", ["reference", "own"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_occluded_equals_closest_hit_below_the_limit(gpu_ctx, name, walk):
    from metalpathtracer_amd import capi
    sets = ray_sets(gpu_ctx, name)
    assert gpu_ctx.accel_info()["ordered_ok"] == 1
    w = capi.WALK_OWN if walk == "own" else capi.WALK_REFERENCE
    for label, o, d, tmax, tstar in sets:
        for n in COUNTS:
            n = min(n, o.shape[0])
            got, flags = gpu_ctx.trace_occluded(o[:n], d[:n], tmax[:n], walk=w)
            check("%s/%s/%s/%d" % (name, walk, label, n), got, o[:n], d[:n], tmax[:n], tstar[:n])
            if walk == "reference":
                assert not flags.any()
            elif label == "edge":
                assert (flags[:15] & 1).all()            # zero direction components go to the reference-order walk
            assert not (flags & ~np.uint32(1 | 8)).any() # (1: direction or origin, 8: stack overflow; both answered in reference order)
        want = ao_ref.occluded(tstar, d, tmax)
        if label != "edge":
            assert 0.02 < want.mean() < 0.98, (name, label, want.mean())      # both answers are exercised
    label, o, d, tmax, tstar = sets[0]                  # tmax = NULL: +inf for every ray
    got, _ = gpu_ctx.trace_occluded(o[:65], d[:65], None, walk=w)
    np.testing.assert_array_equal(got, np.isfinite(tstar[:65]))


def test_three_walks_agree_on_a_scene_of_the_closest_first_pipeline(gpu_ctx):
    """bunny20.xml through mpt_build_and_upload (>= MPT_AUTO_ORDERED_PRIMS primitives): MPT_WALK_AUTO is the own tree, and the three
    walks agree with each other and with mpt_trace_rays' t < tmax (the oracle's tree build is too slow for a test here)."""
    from metalpathtracer_amd import capi, host
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(scene_path("bunny20.xml"), sc)
    assert st == 0, log
    prims, mats = sc.packed_primitives()
    gpu_ctx.build_and_upload(prims, mats)
    info = gpu_ctx.accel_info()
    assert info["ordered_ok"] == 1 and info["auto_pipeline"] == capi.PIPE_ORDERED
    assert sc.getPrimitiveCount() >= gpu_ctx.build_info()["auto_ordered_prims"]
    u = host.make_uniforms(160, 90, sc.getPrimitiveCount(), sc.getTriangleCount())
    o, d = camera_rays(u, N, seed=33)
    d[-3:, 0] = 0.0                                     # three rays only the reference-order walk takes: the flags tell the walks apart
    tstar, prim, _, _ = gpu_ctx.trace_rays(o, d)
    tstar = np.where(prim >= 0, tstar, F(np.inf)).astype(np.float32)
    assert (prim >= 0).mean() > 0.3
    tmax = limits_around(tstar, (0.5, 0.99, 1.01, 2.0))
    res = {w: gpu_ctx.trace_occluded(o, d, tmax, walk=w) for w in (capi.WALK_REFERENCE, capi.WALK_OWN, capi.WALK_AUTO)}
    for w, (got, flags) in res.items():
        check("bunny20/walk %d" % w, got, o, d, tmax, tstar)
    np.testing.assert_array_equal(res[capi.WALK_AUTO][1], res[capi.WALK_OWN][1])
    assert (res[capi.WALK_AUTO][1][-3:] & 1).all() and not res[capi.WALK_REFERENCE][1].any()


def test_argument_errors_and_not_ready(gpu_ctx):
    from metalpathtracer_amd import capi
    setup(gpu_ctx, "cornell.xml", 16, 16, cam=CORNELL_CAM)
    L, h = gpu_ctx.L, gpu_ctx.h
    o = np.zeros((2, 3), np.float32)
    d = np.ones((2, 3), np.float32)
    occ = np.zeros(2, np.uint8)
    fp, bp = capi._fp, lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    INVALID, NOT_READY = 1, 5
    assert L.mpt_trace_occluded(h, None, fp(d), None, 2, 0, bp(occ), None) == INVALID
    assert L.mpt_trace_occluded(h, fp(o), None, None, 2, 0, bp(occ), None) == INVALID
    assert L.mpt_trace_occluded(h, fp(o), fp(d), None, 2, 0, None, None) == INVALID
    assert L.mpt_trace_occluded(h, fp(o), fp(d), None, 0, 0, bp(occ), None) == INVALID
    for walk in (-1, 3):
        assert L.mpt_trace_occluded(h, fp(o), fp(d), None, 2, walk, bp(occ), None) == INVALID
    assert L.mpt_trace_occluded(h, fp(o), fp(d), None, 2, capi.WALK_AUTO, bp(occ), None) == 0      # flags_out may be NULL
    fresh = capi.Context(0)
    try:
        assert fresh.L.mpt_trace_occluded(fresh.h, fp(o), fp(d), None, 2, 0, bp(occ), None) == NOT_READY
    finally:
        fresh.close()
