"""GPU tests of the ray queries' host side (csrc/mpt_query.h): what a call returns must not depend on how many rays it was given —
the first n results of a 257-ray call, bit for bit, at the counts where a wave or workgroup boundary, a rounded-up grid or a misplaced
output pointer would show; the codes and texts of the argument and state errors of mpt_trace_rays and mpt_trace_rays_ordered; and
mpt_time_trace's result block.  What the kernels answer is checked against the oracle in test_gpu_parity.py, test_gpu_ordered.py and
test_gpu_occluded.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import CORNELL_CAM
from test_gpu_occluded import camera_rays, limits_around
from test_gpu_parity import setup

pytestmark = pytest.mark.gpu

N = 257
COUNTS = (1, 63, 64, 65, 256, 257)
INVALID, BAD_SCENE, NOT_READY = 1, 4, 5


def bits(a):
    """Floats as their 32-bit patterns (NaNs and signed zeros count); everything else as it is."""
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(label, got, full, n):
    for k, (g, f) in enumerate(zip(got, full)):
        assert g.dtype == f.dtype and g.shape == f[:n].shape, (label, k, g.dtype, g.shape)
        np.testing.assert_array_equal(bits(g), bits(f[:n]), err_msg="%s, output %d" % (label, k))


def cornell_rays(ctx):
    """The Cornell box at 16 x 16 (left uploaded) and 257 camera rays into it."""
    _, u = setup(ctx, "cornell.xml", 16, 16, cam=CORNELL_CAM)
    assert ctx.accel_info()["ordered_ok"] == 1
    return camera_rays(u, N, seed=5)


def forty_spheres(ctx):
    """The scene of test_ordered_falls_back_when_the_scene_does_not_qualify: more than 16 spheres, no closest-first walk."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    rng = np.random.default_rng(2)
    for k in range(40):
        c = rng.uniform(-8, 8, 3).astype(np.float32) + np.array([0, 20, 20], np.float32)
        sc.addSphere([float(x) for x in c], 1.0 + 0.05 * k, albedo=(0.7, 0.6, 0.5))
    sc.buildBVH()
    ctx.upload_scene(*sc.buffers())
    assert ctx.accel_info()["ordered_ok"] == 0


def test_closest_hit_of_the_first_n_rays_is_the_first_n_of_the_batch(gpu_ctx):
    o, d = cornell_rays(gpu_ctx)
    for name, call in (("trace_rays", gpu_ctx.trace_rays), ("trace_rays_ordered", gpu_ctx.trace_rays_ordered)):
        full = call(o, d)
        assert (full[1] >= 0).mean() > 0.3, name                    # hits and misses
        for n in COUNTS:
            same_bits("%s/%d" % (name, n), call(o[:n], d[:n]), full, n)


def test_occlusion_of_the_first_n_rays_is_the_first_n_of_the_batch(gpu_ctx):
    from metalpathtracer_amd import capi
    o, d = cornell_rays(gpu_ctx)
    t, prim, _, _ = gpu_ctx.trace_rays(o, d)
    tmax = limits_around(np.where(prim >= 0, t, np.float32(np.inf)).astype(np.float32), (0.5, 2.0))
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN, capi.WALK_AUTO):
        for limit in (tmax, None):
            full = gpu_ctx.trace_occluded(o, d, limit, walk=walk)
            if limit is not None:
                assert 0.02 < full[0].mean() < 0.98, walk           # both answers
            for n in COUNTS:
                got = gpu_ctx.trace_occluded(o[:n], d[:n], None if limit is None else limit[:n], walk=walk)
                same_bits("trace_occluded/walk %d/%s/%d" % (walk, "inf" if limit is None else "tmax", n), got, full, n)


def test_closest_hit_argument_errors_not_ready_and_bad_scene(gpu_ctx):
    from metalpathtracer_amd import capi
    setup(gpu_ctx, "cornell.xml", 16, 16, cam=CORNELL_CAM)
    L, h = gpu_ctx.L, gpu_ctx.h
    o, d = np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32)
    t, nrm, prim, front, flags = np.zeros(2, np.float32), np.zeros((2, 3), np.float32), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.uint32)
    fp, ip, up = capi._fp, capi._ip, capi._up

    def err(ctx):
        return (ctx.L.mpt_last_error(ctx.h) or b"").decode()

    calls = {"mpt_trace_rays": (L.mpt_trace_rays, [fp(o), fp(d), 2, fp(t), ip(prim), fp(nrm), ip(front)], 1 << 30, "bad argument"),
             "mpt_trace_rays_ordered": (L.mpt_trace_rays_ordered, [fp(o), fp(d), 2, fp(t), ip(prim), fp(nrm), ip(front), up(flags)], 1 << 22,
                                        "bad argument (at most 2^22 rays per call)")}
    fresh = capi.Context(0)
    try:
        for name, (fn, args, n_max, text) in calls.items():
            assert fn(h, *args) == 0, name
            bad = [args[:k] + [None] + args[k + 1:] for k in range(len(args)) if k != 2]       # each null pointer
            bad += [args[:2] + [n] + args[3:] for n in (0, n_max + 1)]                         # no rays, too many rays
            for a in bad:
                assert fn(h, *a) == INVALID and err(gpu_ctx) == text, (name, a)
            assert fn(None, *args) == INVALID, name
            assert getattr(fresh.L, name)(fresh.h, *args) == NOT_READY and err(fresh) == "no scene", name
            assert getattr(fresh.L, name)(fresh.h, None, *args[1:]) == INVALID and err(fresh) == text, name     # INVALID_ARG before NOT_READY
    finally:
        fresh.close()
    forty_spheres(gpu_ctx)
    fn, args, _, _ = calls["mpt_trace_rays_ordered"]
    assert fn(h, *args) == BAD_SCENE
    assert err(gpu_ctx) == "closest-first walk unavailable for this scene: more than 16 spheres"
    assert fn(h, None, *args[1:]) == INVALID                                                   # ... and before BAD_SCENE
    fn, args, _, _ = calls["mpt_trace_rays"]
    assert fn(h, *args) == 0                                                                   # the reference-order walk takes any scene


def test_time_trace_fills_reps_by_four_and_leaves_the_queries_as_they_were(gpu_ctx):
    from metalpathtracer_amd import capi
    o, d = cornell_rays(gpu_ctx)
    o, d = o[:65], d[:65]
    before = gpu_ctx.trace_rays(o, d)
    for tmax in (None, np.float32(2.0)):
        ms = gpu_ctx.time_trace(o, d, tmax, warmup=0, reps=2)
        assert ms.shape == (2, 4) and ms.dtype == np.float64
        assert np.isfinite(ms).all() and (ms > 0).all(), ms        # four kernels ran, every launch between its own pair of events
    for reps in (0, 1001):
        with pytest.raises(capi.MptError) as e:
            gpu_ctx.time_trace(o, d, None, warmup=0, reps=reps)
        assert e.value.status == INVALID
    ms = np.zeros((2, 4), np.float64)
    mp = ms.ctypes.data_as(C.POINTER(C.c_double))
    assert gpu_ctx.L.mpt_time_trace(gpu_ctx.h, capi._fp(o), capi._fp(d), None, 65, 1001, 2, mp) == INVALID      # warmup > 1000
    assert gpu_ctx.L.mpt_time_trace(gpu_ctx.h, capi._fp(o), capi._fp(d), None, 65, 0, 2, None) == INVALID
    same_bits("trace_rays after time_trace", gpu_ctx.trace_rays(o, d), before, 65)
    forty_spheres(gpu_ctx)                                         # no own tree: its two columns stay 0
    ms = gpu_ctx.time_trace(o, d, None, warmup=0, reps=2)
    assert ms.shape == (2, 4) and np.isfinite(ms).all() and (ms[:, :2] > 0).all(), ms
    assert (ms[:, 2:] == 0.0).all(), ms
