"""The device against the oracle on the cases of tests/optics_cases.py, which tests/test_optics_cpu.py holds to ray optics bounce by bounce:
mirrors seen from both sides, refraction in and out, Schlick reflection outside and inside, total internal reflection, a glass sphere (entered,
never left: the near root alone), and the refraction at the critical angle whose direction is NaN — the ray closest_hit_resume
(mpt_device.h) answers without a walk.  Every case runs in every pipeline, through mpt_upload_scene with the host's tree and through
mpt_build_and_upload, where the oracle renders the tree mpt_download_bvh returns.  Everything is compared exactly: the sum bit for bit, paths
and rays, and with MPT_FLAG_COUNT_WORK the work of the reference-order pipelines test for test — except on the critical cases, where the
device leaves out the walk of the NaN ray that the oracle makes.

One check has no oracle in between: the mirror quad at depth 2 against albedo * sky(reflect(d, n)) in float64.  The oracle is within 4.5e-7
of that closed form (tests/test_optics_cpu.py measures and asserts it); the device is allowed 4 x that, 1.8e-6, on a sum of four samples."""
import numpy as np
import pytest

import optics_cases as oc
from oracle import binding as ob

pytestmark = pytest.mark.gpu

PIPES = (0, 1, 2, 3, 4)                 # wavefront, megakernel, wave-local, closest-first (or its fallback), auto
ROUTES = ("host tree", "device build")
BUILD_ENV = ("MPT_GPU_BUILD", "MPT_BUILD_ONE_STREAM", "MPT_BUILD_NO_HELPER", "MPT_DEBUG_MAT_KEY_BITS")
_oracle = {}


def put_scene(ctx, name, route):
    """The case's scene, image size and camera on the context; returns the (bvh, prims, mats, prim_idx) the oracle is to walk."""
    _, buf = oc.scene_of(name)
    c = oc.CASES[name]
    ctx.resize(c.W, c.H)
    ctx.set_uniforms(oc.uniforms_of(name))
    if route == "host tree":
        ctx.upload_scene(*buf)
        return buf
    ctx.build_and_upload(buf[1], buf[2])
    bvh, idx = ctx.download_bvh()
    return bvh, buf[1], buf[2], idx


def oracle_on(name, buffers):
    """(sum, counters) of the oracle over `buffers`: once per case and tree."""
    key = (name, buffers[0].tobytes(), buffers[3].tobytes())
    if key not in _oracle:
        ref, ct = oc.oracle_render(name, buffers)
        ref.setflags(write=False)
        _oracle[key] = (ref, ct)
    return _oracle[key]


def device_kwargs(name):
    from metalpathtracer_amd import capi
    c = oc.CASES[name]
    return dict(rng_mode=capi.RNG_PHILOX, bsdf_mode=c.bsdf, max_depth=c.depth, sample_count=c.spp, seed=oc.SEED)


def same_sum(ctx, ref, what):
    got = ctx.read_sum()
    bad = (got.view(np.uint32) != ref.view(np.uint32)).any(-1)
    assert not bad.any(), "%s: %d pixels differ from the oracle's, the first at %s: %s against %s" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], ref[bad][0])


@pytest.mark.parametrize("name,route,pipe", [(n, r, p) for n in oc.CASES for r in ROUTES for p in PIPES])
def test_device_renders_the_oracles_sum(gpu_ctx, name, route, pipe, monkeypatch):
    from metalpathtracer_amd import capi
    for env in BUILD_ENV:
        monkeypatch.delenv(env, raising=False)
    buffers = put_scene(gpu_ctx, name, route)
    ref, ct = oracle_on(name, buffers)
    info = gpu_ctx.accel_info()
    what = "%s, %s, pipeline %d (closest-first tree: %d, auto: %d)" % (name, route, pipe, info["ordered_ok"], info["auto_pipeline"])
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.render(pipeline=pipe, **device_kwargs(name))
    same_sum(gpu_ctx, ref, what)
    st = gpu_ctx.stats()
    assert (st["paths"], st["rays"]) == (ct["paths"], ct["rays"]), what
    if pipe not in capi.REFERENCE_ORDER_PIPELINES:
        return
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.render(pipeline=pipe, flags=capi.FLAG_COUNT_WORK, **device_kwargs(name))
    same_sum(gpu_ctx, ref, what + ", counting")
    st = gpu_ctx.stats()
    assert (st["paths"], st["rays"]) == (ct["paths"], ct["rays"]), what
    work = (st["node_visits"], st["aabb_hits"], st["prim_tests"])
    print(what, "work", work, "oracle", (ct["node_pops"], ct["aabb_pass"], ct["prim_tests"]))
    if name in oc.CRITICAL:               # the walk of a NaN ray passes every box and hits nothing: the device does not make it
        assert st["node_visits"] < ct["node_pops"], what
    else:
        assert work == (ct["node_pops"], ct["aabb_pass"], ct["prim_tests"]), what


@pytest.mark.parametrize("route", ROUTES)
def test_nan_directions_through_async_renders_and_moments(gpu_ctx, route, monkeypatch):
    """The critical case whose paths go on after a NaN sample's neighbours: two mpt_render_async of half the samples each and one mpt_wait,
    then one render with MPT_FLAG_MOMENTS.  The sum is the oracle's both times; the moments are finite."""
    from metalpathtracer_amd import capi
    for env in BUILD_ENV:
        monkeypatch.delenv(env, raising=False)
    name = "critical 1.5 deep"
    buffers = put_scene(gpu_ctx, name, route)
    ref, ct = oracle_on(name, buffers)
    kw = device_kwargs(name)
    half = kw.pop("sample_count") // 2
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.render_async(sample_begin=0, sample_count=half, **kw)
    gpu_ctx.render_async(sample_begin=half, sample_count=half, **kw)
    gpu_ctx.wait()
    same_sum(gpu_ctx, ref, "%s, %s, two asynchronous renders" % (name, route))
    st = gpu_ctx.stats()
    assert (st["paths"], st["rays"]) == (ct["paths"], ct["rays"])
    gpu_ctx.clear_sum()
    gpu_ctx.render(flags=capi.FLAG_MOMENTS, **device_kwargs(name))
    same_sum(gpu_ctx, ref, "%s, %s, with moments" % (name, route))
    m2 = gpu_ctx.read_moments()
    assert np.isfinite(m2).all() and (m2 >= 0).all() and m2.max() > 0
    # a sample's colours are clamped to [0, 1]: the squares add up to no more than the values
    assert (m2[..., :3] <= gpu_ctx.read_sum()[..., :3] * (1 + 1e-6)).all()


@pytest.mark.parametrize("pipe", PIPES)
def test_mirror_quad_against_the_closed_form(gpu_ctx, pipe):
    """albedo * sky(reflect(d, n)) per sample in float64 (tests/optics_ref.py:plane_mirror_under_sky), on the pixels whose footprint lies
    inside the quad.  The oracle's own deviation from it is 4.5e-7 (asserted on the CPU); the device is allowed 4 x that = 1.8e-6."""
    name = oc.PHYSICS
    put_scene(gpu_ctx, name, "host tree")
    pred, inside, edge, _ = oc.mirror_quad_prediction()
    assert edge.sum() <= 0.10 * (edge.sum() + inside.sum())
    gpu_ctx.clear_sum()
    gpu_ctx.render(pipeline=pipe, **device_kwargs(name))
    dev = np.abs(gpu_ctx.read_sum().astype(np.float64) - pred)[inside]
    print("pipeline", pipe, "pixels", int(inside.sum()), "largest deviation from the closed form", dev.max())
    assert dev.max() <= 4 * oc.PHYSICS_ORACLE_DEVIATION
