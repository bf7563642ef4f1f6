"""GPU tests of the light table and of mpt_direct_lighting / mpt_direct_image against tests/direct_ref.py: the table and the image are
compared bit for bit and the counts exactly.  The samples are restated in float32; their occlusion is tests/anyhit_ref.py's `lower`, what
MPT_WALK_REFERENCE must answer, and MPT_WALK_OWN is held to the same on every pixel without a gap ray (tests/test_direct_cpu.py caps
those pixels at 1 % of the surface pixels of each case)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import anyhit_ref
import direct_cases as dcs
import direct_ref as dr
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

SEED = dcs.SEED
INVALID, BAD_SCENE, NOT_READY = 1, 4, 5


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def put(ctx, name, W=None, H=None):
    """The case's scene (through mpt_upload_scene with the host's tree), size and uniforms on the context; returns the uniforms."""
    from metalpathtracer_amd import capi
    _, buf = dcs.scene_of(name)
    ctx.upload_scene(*buf)
    u = dcs.uniforms_of(name, W, H)
    ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    ctx.set_uniforms(u)
    return capi.Uniforms.from_buffer_copy(bytes(u))


def reference(ctx, name):
    """dcs.reference(name) with the case on the context; the device's guides are the reference's, bit for bit."""
    put(ctx, name)
    r = dcs.reference(name)
    ad, nc, _ = ctx.read_aovs()
    same(ad, r["ad"])
    same(nc, r["nc"])
    return r


def check_pass(ctx, r, begin, N, sampled, lower, upper, walks=None):
    """One pass per walk against the reference; returns the last (rgba, traced, unoccluded)."""
    from metalpathtracer_amd import capi
    want = dr.direct(r["ad"], r["nc"], r["u"], r["table"], begin, N, SEED, lower, sampled=sampled)
    surface = r["nc"][..., 3] == 0
    gap = (upper & ~lower).any(-1)
    assert gap.sum() <= dcs.GAP_CAP * surface.sum()
    got = None
    for walk in walks or (capi.WALK_REFERENCE, capi.WALK_OWN):
        info = ctx.direct_lighting(samples=N, sample_begin=begin, seed=SEED, walk=walk)
        got = ctx.read_direct()
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        print("walk", walk, "N", N, "pixels that differ:", int((got[0].view(np.uint32) != want[0].view(np.uint32)).any(-1).sum()), "traced",
              info["rays"], "occluded", info["rays_occluded"], "gap pixels", int(gap.sum()), "ms", info["device_ms"])
        same(got[0][keep], want[0][keep])
        np.testing.assert_array_equal(got[1], want[1])                      # (what is traced does not depend on the walk)
        np.testing.assert_array_equal(got[2][keep], want[2][keep])
        assert info["pixels_surface"] == surface.sum() and info["rays"] == want[1].sum() and info["lights"] == r["table"].n
        if not gap.any():
            assert info["rays_occluded"] == want[1].sum() - want[2].sum()
        assert info["device_ms"] > 0
        assert (got[0][~surface] == (0, 0, 0, 1)).all() and (got[1][~surface] == 0).all() and (got[2][~surface] == 0).all()
    return got, want


@pytest.mark.parametrize("N", [1, 3, 16, 65])
@pytest.mark.parametrize("name", ["scene.xml", "cornell.xml"])
def test_the_pass_is_exact_with_both_walks(gpu_ctx, name, N):
    r = reference(gpu_ctx, name)
    sampled, lower, upper = dcs.sliced(r, 0, N)
    got, want = check_pass(gpu_ctx, r, 0, N, sampled, lower, upper)
    surface = r["nc"][..., 3] == 0
    assert surface.any() and not surface.all()
    if N == 16:
        skipped = sampled[4] & surface[..., None]
        assert lower.any() and (want[2] > 0).any() and skipped.any()      # occluded, open and skipped samples all occur
        assert (want[0][..., :3] > 0).any()


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3)])
def test_small_image_sizes(gpu_ctx, W, H):
    put(gpu_ctx, "scene.xml", W, H)
    r = dcs.guides_and_bounds("scene.xml", W, H, 0, 16)
    ad, nc, _ = gpu_ctx.read_aovs()
    same(ad, r["ad"])
    same(nc, r["nc"])
    for N in (16, 5):
        sampled, lower, upper = dcs.sliced(r, 0, N)
        check_pass(gpu_ctx, r, 0, N, sampled, lower, upper)


def read_table(ctx):
    ids, rec, cdf = ctx.read_lights()
    return ids, rec, cdf, ctx.light_info()


@pytest.mark.parametrize("name", ["cornell.xml", "scene.xml", "handmade"])
def test_light_table_on_the_device(gpu_ctx, name):
    """mpt_read_lights is direct_ref.light_table bit for bit, through mpt_upload_scene and through mpt_build_and_upload."""
    sc, buf = dcs.scene_of(name)
    want = dr.light_table(buf[1], buf[2])
    gpu_ctx.upload_scene(*buf)
    a = read_table(gpu_ctx)
    prims, mats = sc.packed_primitives()
    gpu_ctx.build_and_upload(prims, mats)
    b = read_table(gpu_ctx)
    for ids, rec, cdf, info in (a, b):
        np.testing.assert_array_equal(ids, want.ids)
        same(rec, want.rec)
        same(cdf, want.cdf)
        assert info == dict(lights=want.n, emissive_prims=want.seen, triangle_lights=int((want.rec[:, 0, 3] == 1).sum()),
                            sphere_lights=int((want.rec[:, 0, 3] == 0).sum()))
    if name == "handmade":
        assert a[3]["lights"] == 4 and a[3]["emissive_prims"] == 6
    # a capacity below n fills what fits and still reports n
    n = C.c_uint32()
    one = np.full(3, -1, np.int32)
    assert gpu_ctx.L.mpt_read_lights(gpu_ctx.h, 1, one.ctypes.data_as(C.POINTER(C.c_int32)), None, None, C.byref(n)) == 0
    assert n.value == want.n and one[0] == want.ids[0] and (one[1:] == -1).all()


def test_the_table_is_rebuilt_after_a_new_scene(gpu_ctx):
    _, cornell = dcs.scene_of("cornell.xml")
    _, dark = dcs.scene_of("dark")
    gpu_ctx.upload_scene(*cornell)
    assert gpu_ctx.light_info()["lights"] == 2
    gpu_ctx.upload_scene(*dark)
    assert gpu_ctx.light_info() == dict(lights=0, emissive_prims=0, triangle_lights=0, sphere_lights=0)
    ids, rec, cdf = gpu_ctx.read_lights()
    assert ids.size == 0 and rec.shape == (0, 4, 4) and cdf.size == 0
    gpu_ctx.upload_scene(*cornell)
    assert gpu_ctx.light_info()["lights"] == 2


def test_hand_made_scene_is_exact(gpu_ctx):
    r = reference(gpu_ctx, "handmade")
    assert r["table"].n == 4
    for N in (16, 65):
        sampled, lower, upper = dcs.sliced(r, 0, N)
        got, want = check_pass(gpu_ctx, r, 0, N, sampled, lower, upper)
    assert (r["nc"][..., 3] == 1).any()                                   # an emitter is in view, and black
    assert (want[0][..., :3] > 0).any()


def test_scene_without_an_emitter(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "dark")
    ad, nc, _ = gpu_ctx.read_aovs()
    assert (nc[..., 3] == 0).any()
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        info = gpu_ctx.direct_lighting(samples=7, seed=SEED, walk=walk)
        rgba, traced, unocc = gpu_ctx.read_direct()
        assert info["lights"] == 0 and info["rays"] == 0 and info["rays_occluded"] == 0 and info["pixels_surface"] == (nc[..., 3] == 0).sum()
        assert (rgba == (0, 0, 0, 1)).all() and not traced.any() and not unocc.any()


def test_sample_begin_splits_a_pass(gpu_ctx):
    r = reference(gpu_ctx, "scene.xml")
    parts = []
    for begin, count in ((0, 8), (8, 8), (0, 16)):
        gpu_ctx.direct_lighting(samples=count, sample_begin=begin, seed=SEED)
        parts.append(gpu_ctx.read_direct())
    np.testing.assert_array_equal(parts[0][1] + parts[1][1], parts[2][1])
    np.testing.assert_array_equal(parts[0][2] + parts[1][2], parts[2][2])
    sampled, lower, upper = dcs.sliced(r, 8, 8)
    check_pass(gpu_ctx, r, 8, 8, sampled, lower, upper)


def test_direct_image_on_hand_made_guides(gpu_ctx):
    """mpt_direct_image: an emitter pixel, a miss, a surface pixel whose normal is 0 (every sample skipped) and real surface pixels, at a
    size the context does not have; the context's own result is not touched."""
    from metalpathtracer_amd import capi
    r0 = reference(gpu_ctx, "scene.xml")
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    before = gpu_ctx.read_direct()
    H, W = 3, 5
    ys, xs = np.nonzero(r0["nc"][..., 3] == 0)
    pick = np.linspace(0, ys.size - 1, H * W).astype(int)
    ad = r0["ad"][ys[pick], xs[pick]].reshape(H, W, 4).copy()
    nc = r0["nc"][ys[pick], xs[pick]].reshape(H, W, 4).copy()
    nc[0, 0, 3] = 1                                                  # class 1: an emitter
    ad[0, 1] = (0, 0, 0, np.inf)                                     # class 2: a miss
    nc[0, 1] = (0, 0, 0, 2)
    nc[0, 2, :3] = 0                                                 # a surface without a normal: cos_s = 0, every sample skipped
    u = r0["u"]
    uu = capi.Uniforms.from_buffer_copy(bytes(u))
    table = r0["table"]
    for N, begin, walk in ((8, 2, capi.WALK_REFERENCE), (8, 2, capi.WALK_OWN)):
        sampled = dr.samples(ad, nc, u, table, begin, N, SEED)
        lower, upper = dr.occlusion_bounds(sampled, r0["buf"], anyhit_ref.bounds)
        assert not (upper & ~lower).any()
        want = dr.direct(ad, nc, u, table, begin, N, SEED, lower, sampled=sampled)
        got = gpu_ctx.direct_image(ad, nc, uu, samples=N, sample_begin=begin, seed=SEED, walk=walk)
        same(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        assert (got[0][0, :3] == (0, 0, 0, 1)).all() and (got[1][0, :3] == 0).all()
        assert got[1].any()
    after = gpu_ctx.read_direct()
    same(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])
    np.testing.assert_array_equal(before[2], after[2])


def test_the_pass_has_no_side_effects(gpu_ctx):
    from metalpathtracer_amd import capi
    reference(gpu_ctx, "scene.xml")
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(1, 0))
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    s0, d0, st0, ao0 = gpu_ctx.read_sum(), gpu_ctx.read_denoised(), gpu_ctx.stats(), gpu_ctx.read_ao()
    gpu_ctx.render_async(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_begin=2, sample_count=2, seed=(1, 0))   # the pass waits for it
    info = gpu_ctx.direct_lighting(samples=8, seed=SEED)
    st1 = gpu_ctx.stats()
    gpu_ctx.direct_lighting(samples=3, seed=SEED, walk=capi.WALK_OWN)
    assert gpu_ctx.stats() == st1 and info["rays"] > 0
    assert st1["rays"] > st0["rays"]                                 # (the queued render was counted, the pass was not)
    same(gpu_ctx.read_denoised(), d0)
    ao1 = gpu_ctx.read_ao()
    same(ao1[0], ao0[0])
    np.testing.assert_array_equal(ao1[1], ao0[1])
    s1 = gpu_ctx.read_sum()
    gpu_ctx.direct_lighting(samples=8, seed=SEED)
    same(gpu_ctx.read_sum(), s1)
    assert not np.array_equal(s0, s1)


def test_lifetime_and_errors(gpu_ctx):
    from metalpathtracer_amd import capi
    W, H, _ = dcs.CASES["scene.xml"]
    r = reference(gpu_ctx, "scene.xml")                              # (put() resizes: whatever result there was is gone)
    buf, u, ad, nc = r["buf"], r["u"], r["ad"], r["nc"]
    L, h = gpu_ctx.L, gpu_ctx.h
    rgba = np.zeros((H, W, 4), np.float32)
    ptr, nbytes = C.c_void_p(), C.c_uint64()
    assert L.mpt_read_direct(h, capi._fp(rgba), None, None) == NOT_READY
    assert L.mpt_direct_buffer(h, C.byref(ptr), C.byref(nbytes)) == NOT_READY
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    want = gpu_ctx.read_direct()
    assert L.mpt_read_direct(h, capi._fp(rgba), None, None) == 0     # the counts are optional
    same(rgba, want[0])
    p, n = gpu_ctx.direct_buffer()
    assert p and n == W * H * 16
    # invalid arguments change nothing
    assert L.mpt_direct_lighting(h, None, None) == INVALID
    uu = capi.Uniforms.from_buffer_copy(bytes(u))
    for kw in (dict(samples=0), dict(samples=capi.DIRECT_MAX_SAMPLES + 1), dict(walk=3), dict(walk=-1)):
        q = capi.direct_params(**kw)
        assert L.mpt_direct_lighting(h, C.byref(q), None) == INVALID, kw
        assert L.mpt_direct_image(h, W, H, capi._fp(ad), capi._fp(nc), C.byref(uu), C.byref(q), capi._fp(rgba), None, None) == INVALID
    assert L.mpt_read_direct(h, None, None, None) == INVALID
    got = gpu_ctx.read_direct()
    same(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    q = capi.direct_params(samples=capi.DIRECT_MAX_SAMPLES)
    assert L.mpt_direct_lighting(h, C.byref(q), None) == 0           # the cap itself is allowed, info may be NULL
    _, traced, unocc = gpu_ctx.read_direct()
    assert traced.max() <= capi.DIRECT_MAX_SAMPLES and (unocc <= traced).all()
    # dropped by mpt_resize and by the scene calls
    gpu_ctx.resize(W, H)
    assert L.mpt_read_direct(h, capi._fp(rgba), None, None) == NOT_READY
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    same(gpu_ctx.read_direct()[0], want[0])
    gpu_ctx.upload_scene(*buf)
    assert L.mpt_read_direct(h, capi._fp(rgba), None, None) == NOT_READY
    assert L.mpt_direct_buffer(h, C.byref(ptr), C.byref(nbytes)) == NOT_READY
    # before scene, uniforms and size
    fresh = capi.Context(0)
    try:
        q = capi.direct_params(samples=4, seed=SEED)
        out4 = (C.c_uint64 * 4)()
        n = C.c_uint32()
        assert fresh.L.mpt_direct_lighting(fresh.h, C.byref(q), None) == NOT_READY
        assert fresh.L.mpt_light_info(fresh.h, out4) == NOT_READY
        assert fresh.L.mpt_read_lights(fresh.h, 0, None, None, None, C.byref(n)) == NOT_READY
        assert fresh.L.mpt_direct_image(fresh.h, W, H, capi._fp(ad), capi._fp(nc), C.byref(uu), C.byref(q), capi._fp(rgba), None, None) == NOT_READY
        fresh.upload_scene(*buf)
        assert fresh.L.mpt_direct_lighting(fresh.h, C.byref(q), None) == NOT_READY
        fresh.resize(W, H)
        assert fresh.L.mpt_direct_lighting(fresh.h, C.byref(q), None) == NOT_READY
        assert fresh.L.mpt_read_direct(fresh.h, capi._fp(rgba), None, None) == NOT_READY
        fresh.set_uniforms(uu)
        assert fresh.L.mpt_direct_lighting(fresh.h, C.byref(q), None) == 0
        assert fresh.L.mpt_read_direct(fresh.h, capi._fp(rgba), None, None) == 0
        same(rgba, want[0])
    finally:
        fresh.close()


def test_too_many_lights_is_a_bad_scene(gpu_ctx):
    """MPT_LIGHTS_MAX + 1 tiny emissive triangles: MPT_ERR_BAD_SCENE with a message from the call that needs the table, nothing kept;
    MPT_LIGHTS_MAX of them are a table."""
    from metalpathtracer_amd import capi
    n = capi.LIGHTS_MAX + 1
    k = np.arange(n, dtype=np.float32)
    v0 = np.stack([(k % 256) * 0.01, np.floor(k / 256) * 0.01, np.zeros(n, np.float32)], -1).astype(np.float32)
    prims = np.zeros((n, 3, 4), np.float32)
    prims[:, 0, :3] = v0
    prims[:, 1, :3] = v0 + np.array([0.005, 0.0, 0.001], np.float32)
    prims[:, 2, :3] = v0 + np.array([0.0, 0.005, 0.002], np.float32)
    prims[:, 0, 3] = 1
    mats = np.zeros((n, 2, 4), np.float32)
    mats[:, 0, :3] = 0.5
    mats[:, 1] = (1.0, 1.0, 1.0, 2.0)
    gpu_ctx.build_and_upload(prims, mats)
    out4 = (C.c_uint64 * 4)()
    assert gpu_ctx.L.mpt_light_info(gpu_ctx.h, out4) == BAD_SCENE
    assert b"MPT_LIGHTS_MAX" in gpu_ctx.L.mpt_last_error(gpu_ctx.h)
    cnt = C.c_uint32(7)
    assert gpu_ctx.L.mpt_read_lights(gpu_ctx.h, 0, None, None, None, C.byref(cnt)) == BAD_SCENE and cnt.value == 7
    gpu_ctx.resize(4, 4)
    gpu_ctx.set_uniforms(dcs.uniforms_of("handmade", 4, 4))
    q = capi.direct_params(samples=1)
    assert gpu_ctx.L.mpt_direct_lighting(gpu_ctx.h, C.byref(q), None) == BAD_SCENE
    gpu_ctx.build_and_upload(prims[:-1], mats[:-1])
    info = gpu_ctx.light_info()
    assert info["lights"] == capi.LIGHTS_MAX and info["triangle_lights"] == capi.LIGHTS_MAX
    ids, rec, cdf = gpu_ctx.read_lights()
    np.testing.assert_array_equal(ids, np.arange(capi.LIGHTS_MAX))
    assert cdf[-1] == 1 and (np.diff(cdf) >= 0).all()


EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def test_cli_writes_the_python_paths_bytes(tmp_path):
    """mpt_render --direct 8 writes what Renderer.renderDirectLighting gives through the same .ppm writer, a run without --direct writes
    what it wrote before (the radiance through that writer), and the combinations that make no sense are refused."""
    import json
    from metalpathtracer_amd import capi, host
    W, H, spp = 64, 48, 4
    base = [EXE, "--scene", scene_path("cornell.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", "8", "--seed", "1",
            "--bvh", "reference"]
    a, b = str(tmp_path / "direct.ppm"), str(tmp_path / "plain.ppm")
    r = subprocess.run(base + ["--out", a, "--direct", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.splitlines()[-1])
    r = subprocess.run(base + ["--out", b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "direct" not in json.loads(r.stdout.splitlines()[-1])
    for bad in (["--out", str(tmp_path / "c.pfm"), "--direct", "8"], ["--out", a, "--direct", "0"], ["--out", a, "--direct", "8", "--denoise"],
                ["--out", a, "--direct", "8", "--ao", "4"], ["--out", a, "--direct", "8", "--adaptive", "0.05"], ["--out", a, "--direct", "8", "--temporal"],
                ["--out", a, "--direct", "8", "--svgf"], ["--out", a, "--direct-walk", "own"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--direct" in r.stderr, (bad, r.stderr[-500:])
    rr = host.Renderer(0, scene_path("cornell.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        rgba, info = rr.renderDirectLighting(8)
        # (Camera::reset() sees the box from far away: a handful of surface pixels, which is all this comparison of bytes needs)
        assert rgba.shape == (H, W, 4) and 0 < info["rays"] <= info["pixels_surface"] * 8 and info["lights"] == 2
        assert (rgba[..., :3] > 0).any()
        for key in ("pixels_surface", "rays", "rays_occluded", "lights"):
            assert line["direct"][key] == info[key], key
        assert line["paths"] == 0
        mine = str(tmp_path / "mine.ppm")
        assert host.write_ppm(mine, rgba) == 0
        assert open(mine, "rb").read() == open(a, "rb").read()
        rr.clearSum()
        rr.renderBatch(0, spp)
        today = str(tmp_path / "today.ppm")
        assert host.write_ppm(today, rr.readSum(), scale=1.0 / spp) == 0
        assert open(today, "rb").read() == open(b, "rb").read()
        assert open(a, "rb").read() != open(b, "rb").read()
    finally:
        rr.close()
