"""GPU tests of the material tables the device holds, with 1 .. 40,000 distinct materials (tests/material_cases.py): through
mpt_build_and_upload (hash, radix sort, run heads, numbering: mpt_devbuild.h) and through mpt_upload_scene of the tree that build
downloaded (the host's de-duplication, whose ids come in another order).  Everything is compared exactly and nothing is left out: the
table's size, per pixel the albedo bits and emitter class against the caller's own rows, the light table against tests/direct_ref.py, and
renders with mirror and glass in play against the oracle on the downloaded tree, in all four pipelines.  Tables of more than 32 rows are
served from global memory by shade_bounce (mpt_device.h), the first 32 from LDS: 31, 32 and 33 rows bracket that.  One scene holds two
different rows whose hashes agree in their upper halves, interleaved in the array: the build's 32-bit keys must notice and fall back.
tests/test_materials_cpu.py asserts what these tests rest on: every row of a table case is some pixel's first hit."""
import ctypes as C

import numpy as np
import pytest

import direct_ref as dr
import material_cases as mc
from oracle import binding as ob
from test_gpu_radix import harness

pytestmark = pytest.mark.gpu

SPP, DEPTH, SEED = 2, 8, (4, 2)
RENDERED = [n for n, c in mc.CASES.items() if c[2]]
_lights = {}


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def lights_of(name):
    if name not in _lights:
        prims, mats, _ = mc.scene(name)
        _lights[name] = dr.light_table(prims, mats)
    return _lights[name]


def frame(ctx, name):
    """The case's image size and camera on the context; returns the uniforms."""
    u = mc.uniforms(name)
    ctx.resize(mc.W, mc.H)
    ctx.set_uniforms(u)
    return u


def check_table(ctx, name, lights=True):
    """The scene in place holds the case's materials: table size, guide buffers, light table."""
    prims, mats, n_mats = mc.scene(name)
    assert ctx.build_info()["materials"] == n_mats
    ad, nc, prim = ctx.read_aovs()
    hit = prim >= 0
    assert hit.any() and prim.max() < prims.shape[0]
    same(ad[hit][:, :3], mats[prim[hit], 0:3])                                   # bits: +0 and -0 are two materials
    np.testing.assert_array_equal(nc[hit][:, 3], np.where(mats[prim[hit], 7] > 0, 1.0, 0.0).astype(np.float32))
    assert (nc[~hit][:, 3] == 2).all()
    if name in mc.TABLE_CASES:                                                   # every entry of the table has been looked up
        assert np.unique(mats[np.unique(prim[hit])].view(np.uint32), axis=0).shape[0] == n_mats
    if lights:
        want = lights_of(name)
        ids, rec, cdf = ctx.read_lights()
        np.testing.assert_array_equal(ids, want.ids)
        same(rec, want.rec)
        same(cdf, want.cdf)
        assert ctx.light_info() == dict(lights=want.n, emissive_prims=want.seen, triangle_lights=int((want.rec[:, 0, 3] == 1).sum()),
                                        sphere_lights=int((want.rec[:, 0, 3] == 0).sum()))
        assert want.n == (0 if n_mats == 1 else int((mats[:, 7] > 0).sum()))


def check_renders(ctx, name, ref, rays, pipes, what):
    from metalpathtracer_amd import capi
    for pipe in pipes:
        ctx.clear_sum()
        ctx.reset_stats()
        ctx.render(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_SCATTER, max_depth=DEPTH, sample_count=SPP, seed=SEED, pipeline=pipe)
        got = ctx.read_sum()
        bad = int((got.view(np.uint32) != ref.view(np.uint32)).any(-1).sum())
        assert bad == 0, "%s %s pipeline %d: %d pixels differ from the oracle's" % (name, what, pipe, bad)
        assert ctx.stats()["rays"] == rays, (name, what, pipe)


def oracle_render(name, u, buffers):
    ref, ct = ob.render(ob.Uniforms.from_buffer_copy(bytes(u)), buffers, rng_mode=ob.RNG_PHILOX, bsdf_mode=ob.BSDF_SCATTER, max_depth=DEPTH,
                        accumulate=1, sample_count=SPP, seed=SEED, threads=8)
    return ref, ct["rays"]


def both_routes(ctx, name, render=True, lights=True, pipes=None):
    """mpt_build_and_upload twice (one digest), its table; mpt_upload_scene of the downloaded tree, its table; the renders of both."""
    from metalpathtracer_amd import capi
    pipes = pipes or (capi.PIPE_WAVELOCAL, capi.PIPE_ORDERED, capi.PIPE_MEGAKERNEL, capi.PIPE_WAVEFRONT)
    prims, mats, n_mats = mc.scene(name)
    u = frame(ctx, name)
    ctx.build_and_upload(prims, mats)
    first = ctx.scene_digest()
    ctx.build_and_upload(prims, mats)
    assert ctx.scene_digest() == first, "%s: a second build of the same arrays wrote other arrays" % name
    bvh, idx = ctx.download_bvh()
    buffers = (bvh, np.ascontiguousarray(prims).reshape(-1, 3, 4), np.ascontiguousarray(mats).reshape(-1, 2, 4), idx)
    check_table(ctx, name, lights)
    if render:
        ref, rays = oracle_render(name, u, buffers)
        check_renders(ctx, name, ref, rays, pipes, "device build")
    ctx.upload_scene(*buffers)
    check_table(ctx, name, lights)
    if render:
        check_renders(ctx, name, ref, rays, pipes, "host upload")
    return first


@pytest.mark.parametrize("name", RENDERED)
def test_tables_guides_lights_and_renders_are_exact(gpu_ctx, name, monkeypatch):
    for env in ("MPT_GPU_BUILD", "MPT_BUILD_ONE_STREAM", "MPT_BUILD_NO_HELPER", "MPT_DEBUG_MAT_KEY_BITS"):
        monkeypatch.delenv(env, raising=False)
    both_routes(gpu_ctx, name)
    if name == "all8k":
        assert gpu_ctx.build_info()["prims"] >= gpu_ctx.build_info()["auto_ordered_prims"]      # MPT_PIPE_AUTO is the closest-first pipeline here


def test_forty_thousand_materials(gpu_ctx, monkeypatch):
    """n * 32 >= 1 MiB: the helper thread uploads the materials and runs their chain, 40 radix tiles.  Table size and guides alone."""
    for env in ("MPT_GPU_BUILD", "MPT_BUILD_ONE_STREAM", "MPT_BUILD_NO_HELPER", "MPT_DEBUG_MAT_KEY_BITS"):
        monkeypatch.delenv(env, raising=False)
    both_routes(gpu_ctx, "all40k", render=False, lights=False)


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
@pytest.mark.parametrize("name", ["m200", "collision"])
def test_the_other_builders_give_the_same(gpu_ctx, name, builder, monkeypatch):
    from metalpathtracer_amd import capi
    monkeypatch.setenv("MPT_GPU_BUILD", builder)
    both_routes(gpu_ctx, name, pipes=(capi.PIPE_WAVELOCAL, capi.PIPE_ORDERED))


def test_the_build_fallbacks_give_the_same(gpu_ctx, monkeypatch):
    """One stream, the material upload by the calling thread and the 64-bit material sort (forced by keeping 2 bits of the key) write the
    arrays the default build writes, 200 materials in the table."""
    from metalpathtracer_amd import capi
    for env in ("MPT_GPU_BUILD", "MPT_BUILD_ONE_STREAM", "MPT_BUILD_NO_HELPER", "MPT_DEBUG_MAT_KEY_BITS"):
        monkeypatch.delenv(env, raising=False)
    prims, mats, n_mats = mc.scene("m200")
    frame(gpu_ctx, "m200")
    gpu_ctx.build_and_upload(prims, mats)
    want = gpu_ctx.scene_digest()
    for env, val in (("MPT_BUILD_ONE_STREAM", "1"), ("MPT_BUILD_NO_HELPER", "1"), ("MPT_DEBUG_MAT_KEY_BITS", "2")):
        monkeypatch.setenv(env, val)
        got = both_routes(gpu_ctx, "m200", pipes=(capi.PIPE_WAVELOCAL,))
        monkeypatch.delenv(env)
        assert got == want, env


def test_the_crafted_collision_is_one_on_the_device(gpu_ctx):
    """k_mat_hash over the candidates of the collision search is the numpy restatement, bit for bit: were the hash to change, the pair of
    tests/material_cases.py would stop colliding and the collision case would test nothing — this fails first, and says so."""
    rows = mc.collision_candidates()
    got = np.zeros(rows.shape[0], np.uint64)
    rc = harness().radix_harness_mat_hash(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], got.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0
    want = mc.mat_hash(rows)
    assert (got == want).all(), "k_mat_hash is no longer what material_cases.mat_hash restates: %d of %d hashes differ" % ((got != want).sum(), got.size)
    h = mc.mat_hash(mc.colliding_pair())
    assert h[0] >> np.uint64(32) == h[1] >> np.uint64(32) and h[0] != h[1]
