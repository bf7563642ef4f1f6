"""GPU tests of mpt_ambient_occlusion / mpt_ao_image against tests/ao_ref.py: the counts are compared exactly and ao bit for bit (the
rays are restated in float32, their occlusion is the oracle's closest t below the limit), for both any-hit walks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_ref
from conftest import CORNELL_CAM, ROOT, scene_path
from oracle import binding as ob
from test_gpu_parity import setup

pytestmark = pytest.mark.gpu

SEED = (0x1234, 7)
CASES = {"scene.xml": (48, 27, None), "cornell.xml": (32, 32, CORNELL_CAM)}
N_MAX = 65
INVALID, NOT_READY = 1, 5

_ref = {}


def reference(ctx, name):
    """Per scene, computed once and never modified: (buffers, uniforms, albedo_depth, normal_class, t* of samples [0, 65) of every
    surface pixel).  Leaves the scene, the size and the uniforms of the case on the context."""
    W, H, cam = CASES[name]
    buf, u = setup(ctx, name, W, H, cam=cam)
    if name not in _ref:
        ad, nc, _ = ctx.read_aovs()
        ts = ao_ref.closest_t_of_pass(ad, nc, u, buf, ob.first_hit, 0, N_MAX, SEED)
        for a in (ad, nc, ts):
            a.setflags(write=False)
        _ref[name] = (buf, u, ad, nc, ts)
    return _ref[name]


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("radius", [0.5, 0.0])
@pytest.mark.parametrize("N", [1, 3, 16, 65])
@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_are_exact_with_both_walks(gpu_ctx, name, N, radius):
    from metalpathtracer_amd import capi
    buf, u, ad, nc, ts = reference(gpu_ctx, name)
    ao_want, occ_want = ao_ref.ambient_occlusion(ad, nc, u, 0, N, radius, SEED, tstar=ts[..., :N])
    surface = nc[..., 3] == 0
    assert surface.any() and not surface.all()
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        info = gpu_ctx.ambient_occlusion(samples=N, radius=radius, seed=SEED, walk=walk)
        ao, occ = gpu_ctx.read_ao()
        print(name, N, radius, walk, "pixels that differ:", int((occ != occ_want).sum()), "occluded rays", int(occ.sum()), "of", info["rays"])
        np.testing.assert_array_equal(occ, occ_want)
        same(ao, ao_want)
        assert info["pixels_surface"] == surface.sum() and info["rays"] == surface.sum() * N and info["rays_occluded"] == occ_want.sum()
        assert info["device_ms"] > 0
    if N == 16:
        assert 0 < occ_want.sum() < surface.sum() * N            # both answers occur
        assert (ao[~surface] == 1).all() and (occ[~surface] == 0).all()


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3)])
def test_small_image_sizes(gpu_ctx, W, H):
    from metalpathtracer_amd import capi
    buf, u = setup(gpu_ctx, "scene.xml", W, H)
    ad, nc, _ = gpu_ctx.read_aovs()
    for N, radius in ((16, 0.0), (5, 2.0)):
        ao_want, occ_want = ao_ref.ambient_occlusion(ad, nc, u, 0, N, radius, SEED, buffers=buf, first_hit=ob.first_hit)
        for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
            gpu_ctx.ambient_occlusion(samples=N, radius=radius, seed=SEED, walk=walk)
            ao, occ = gpu_ctx.read_ao()
            np.testing.assert_array_equal(occ, occ_want)
            same(ao, ao_want)


def test_sample_begin_splits_a_pass(gpu_ctx):
    buf, u, ad, nc, ts = reference(gpu_ctx, "scene.xml")
    parts = []
    for begin, count in ((0, 8), (8, 8), (0, 16)):
        gpu_ctx.ambient_occlusion(samples=count, sample_begin=begin, radius=0.0, seed=SEED)
        parts.append(gpu_ctx.read_ao()[1])
    np.testing.assert_array_equal(parts[0] + parts[1], parts[2])
    _, want = ao_ref.ambient_occlusion(ad, nc, u, 8, 8, 0.0, SEED, tstar=ts[..., 8:16])
    np.testing.assert_array_equal(parts[1], want)


def test_ao_image_on_hand_made_guides(gpu_ctx):
    """mpt_ao_image: an emitter pixel, a miss, a surface pixel whose normal is 0 (its directions are the drawn unit vectors themselves)
    and real surface pixels, at a size the context does not have; the context's own AO result is not touched."""
    from metalpathtracer_amd import capi
    buf, u, ad0, nc0, _ = reference(gpu_ctx, "scene.xml")
    info = gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    before = gpu_ctx.read_ao()
    H, W = 3, 5
    ys, xs = np.nonzero(nc0[..., 3] == 0)
    pick = np.linspace(0, ys.size - 1, H * W).astype(int)
    ad = ad0[ys[pick], xs[pick]].reshape(H, W, 4).copy()
    nc = nc0[ys[pick], xs[pick]].reshape(H, W, 4).copy()
    nc[0, 0, 3] = 1                                                  # class 1: an emitter
    ad[0, 1] = (0, 0, 0, np.inf)                                     # class 2: a miss
    nc[0, 1] = (0, 0, 0, 2)
    nc[0, 2, :3] = 0                                                 # a surface without a normal
    uu = capi.Uniforms.from_buffer_copy(bytes(u))
    for N, radius, walk in ((8, 0.0, capi.WALK_REFERENCE), (8, 30.0, capi.WALK_OWN)):
        ao_want, occ_want = ao_ref.ambient_occlusion(ad, nc, u, 2, N, radius, SEED, buffers=buf, first_hit=ob.first_hit)
        ao, occ = gpu_ctx.ao_image(ad, nc, uu, samples=N, sample_begin=2, radius=radius, seed=SEED, walk=walk)
        np.testing.assert_array_equal(occ, occ_want)
        same(ao, ao_want)
        assert ao[0, 0] == 1 and ao[0, 1] == 1 and occ[0, 0] == 0 and occ[0, 1] == 0
    after = gpu_ctx.read_ao()
    same(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    assert info["rays"] > 0


def test_the_pass_has_no_side_effects(gpu_ctx):
    from metalpathtracer_amd import capi
    reference(gpu_ctx, "scene.xml")
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(1, 0))
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    s0, d0, st0 = gpu_ctx.read_sum(), gpu_ctx.read_denoised(), gpu_ctx.stats()
    gpu_ctx.render_async(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_begin=2, sample_count=2, seed=(1, 0))   # the pass waits for it
    info = gpu_ctx.ambient_occlusion(samples=8, radius=1.5, seed=SEED)
    st1 = gpu_ctx.stats()
    gpu_ctx.ambient_occlusion(samples=3, seed=SEED, walk=capi.WALK_OWN)
    assert gpu_ctx.stats() == st1 and info["rays"] > 0
    assert st1["rays"] > st0["rays"]                                 # (the queued render was counted, the pass was not)
    same(gpu_ctx.read_denoised(), d0)
    s1 = gpu_ctx.read_sum()
    gpu_ctx.ambient_occlusion(samples=8, radius=1.5, seed=SEED)
    same(gpu_ctx.read_sum(), s1)
    assert not np.array_equal(s0, s1)


def test_lifetime_and_errors(gpu_ctx):
    from metalpathtracer_amd import capi
    W, H, _ = CASES["scene.xml"]
    buf, u, ad, nc, ts = reference(gpu_ctx, "scene.xml")            # (setup() resizes: whatever result there was is gone)
    L, h = gpu_ctx.L, gpu_ctx.h
    ao = np.zeros((H, W), np.float32)
    ptr, nbytes = C.c_void_p(), C.c_uint64()
    assert L.mpt_read_ao(h, capi._fp(ao), None) == NOT_READY
    assert L.mpt_ao_buffer(h, C.byref(ptr), C.byref(nbytes)) == NOT_READY
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    want = gpu_ctx.read_ao()
    assert L.mpt_read_ao(h, capi._fp(ao), None) == 0                 # the counts are optional
    same(ao, want[0])
    p, n = gpu_ctx.ao_buffer()
    assert p and n == W * H * 4
    # invalid arguments change nothing
    assert L.mpt_ambient_occlusion(h, None, None) == INVALID
    for kw in (dict(samples=0), dict(samples=capi.AO_MAX_SAMPLES + 1), dict(radius=float("nan")), dict(walk=3), dict(walk=-1)):
        q = capi.ao_params(**kw)
        assert L.mpt_ambient_occlusion(h, C.byref(q), None) == INVALID, kw
        assert L.mpt_ao_image(h, W, H, capi._fp(ad), capi._fp(nc), C.byref(capi.Uniforms.from_buffer_copy(bytes(u))), C.byref(q), capi._fp(ao), None) == INVALID
    assert L.mpt_read_ao(h, None, None) == INVALID
    got = gpu_ctx.read_ao()
    same(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    q = capi.ao_params(samples=capi.AO_MAX_SAMPLES, radius=0.25)
    assert L.mpt_ambient_occlusion(h, C.byref(q), None) == 0         # the cap itself is allowed, info may be NULL
    _, occ = gpu_ctx.read_ao()
    assert occ.max() <= capi.AO_MAX_SAMPLES
    # dropped by mpt_resize and by the scene calls
    gpu_ctx.resize(W, H)
    assert L.mpt_read_ao(h, capi._fp(ao), None) == NOT_READY
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    same(gpu_ctx.read_ao()[0], want[0])
    gpu_ctx.upload_scene(*buf)
    assert L.mpt_read_ao(h, capi._fp(ao), None) == NOT_READY
    assert L.mpt_ao_buffer(h, C.byref(ptr), C.byref(nbytes)) == NOT_READY
    # before scene, uniforms and size
    fresh = capi.Context(0)
    try:
        q = capi.ao_params(samples=4)
        assert fresh.L.mpt_ambient_occlusion(fresh.h, C.byref(q), None) == NOT_READY
        fresh.upload_scene(*buf)
        assert fresh.L.mpt_ambient_occlusion(fresh.h, C.byref(q), None) == NOT_READY
        fresh.resize(W, H)
        assert fresh.L.mpt_ambient_occlusion(fresh.h, C.byref(q), None) == NOT_READY
        assert fresh.L.mpt_read_ao(fresh.h, capi._fp(ao), None) == NOT_READY
        fresh.set_uniforms(capi.Uniforms.from_buffer_copy(bytes(u)))
        assert fresh.L.mpt_ambient_occlusion(fresh.h, C.byref(q), None) == 0
    finally:
        fresh.close()


EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def test_cli_writes_the_python_paths_bytes(tmp_path):
    """mpt_render --ao 8 --ao-radius 0.5 writes what Renderer.renderAmbientOcclusion gives through the same .ppm writer, and a run
    without --ao writes what it wrote before: the radiance through that writer."""
    import json
    from metalpathtracer_amd import capi, host
    W, H, spp = 64, 48, 4
    base = [EXE, "--scene", scene_path("cornell.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", "8", "--seed", "1",
            "--bvh", "reference"]
    a, b = str(tmp_path / "ao.ppm"), str(tmp_path / "plain.ppm")
    r = subprocess.run(base + ["--out", a, "--ao", "8", "--ao-radius", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.splitlines()[-1])
    r = subprocess.run(base + ["--out", b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for bad in (["--out", str(tmp_path / "c.pfm"), "--ao", "8"], ["--out", a, "--ao", "0"], ["--out", a, "--ao", "8", "--denoise"],
                ["--out", a, "--ao-radius", "1"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--ao" in r.stderr, (bad, r.stderr[-500:])
    rr = host.Renderer(0, scene_path("cornell.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        ao, info = rr.renderAmbientOcclusion(8, 0.5)
        assert ao.shape == (H, W) and 0 < info["rays_occluded"] < info["rays"] == info["pixels_surface"] * 8
        assert line["ao"]["rays"] == info["rays"] and line["ao"]["rays_occluded"] == info["rays_occluded"] and line["paths"] == 0
        grey = np.stack([ao, ao, ao, np.ones_like(ao)], -1)
        mine = str(tmp_path / "mine.ppm")
        assert host.write_ppm(mine, grey) == 0
        assert open(mine, "rb").read() == open(a, "rb").read()
        rr.clearSum()
        rr.renderBatch(0, spp)
        today = str(tmp_path / "today.ppm")
        assert host.write_ppm(today, rr.readSum(), scale=1.0 / spp) == 0
        assert open(today, "rb").read() == open(b, "rb").read()
        assert open(a, "rb").read() != open(b, "rb").read()
    finally:
        rr.close()
