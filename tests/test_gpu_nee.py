"""GPU tests of mpt_render_nee against tests/nee_ref.py: the HDR sum is compared bit for bit and the counts exactly.  The estimator is
restated in float32; closest hits are the oracle's, occlusion is tests/anyhit_ref.py's `lower` — what MPT_WALK_REFERENCE must answer —
and MPT_WALK_OWN is held to the same on every pixel without a gap ray (tests/test_nee_cpu.py caps those pixels at 1 % of each case).
Then identities against mpt_render that need no reference, order and state, the errors, the CLI, and a statistical comparison with the
plain path tracer: same expectation, less variance."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import nee_cases as ncs
import nee_ref
from conftest import CORNELL_CAM, ROOT, scene_path

pytestmark = pytest.mark.gpu

SEED = ncs.SEED
INVALID, BAD_SCENE, NOT_READY = 1, 4, 5
EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def put(ctx, name, W=None, H=None):
    """The case's scene (through mpt_upload_scene with the host's tree), size and uniforms on the context; returns the uniforms."""
    _, buf = ncs.scene_of(name)
    ctx.upload_scene(*buf)
    u = ncs.uniforms_of(name, W, H)
    ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    ctx.set_uniforms(u)
    return u


def nee(ctx, name, **kw):
    from metalpathtracer_amd import capi
    kw.setdefault("seed", SEED)
    return ctx.render_nee(rng_mode=capi.RNG_PHILOX, bsdf_mode=ncs.CASES[name][4], **kw)


def check_exact(ctx, name, r, spp, depth):
    """samples [0, spp) of the reference r with both walks: the sum bit for bit, the counts exactly."""
    from metalpathtracer_amd import capi
    want = nee_ref.accumulate(r["value"][:, :, :spp])
    gap = r["gap"][:, :, :spp].any(-1)
    assert gap.sum() <= ncs.GAP_CAP * gap.size
    rays, shadow, occluded = (int(r[k][:, :, :spp].sum()) for k in ("rays", "shadow", "occluded"))
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        ctx.clear_sum()
        ctx.reset_stats()
        info = nee(ctx, name, walk=walk, clamp=0.0, max_depth=depth, sample_count=spp)
        got = ctx.read_sum()
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        print(name, "spp", spp, "depth", depth, "walk", walk, "pixels that differ:", int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()),
              "rays", info["rays"], "shadow", info["shadow_rays"], "occluded", info["shadow_rays_occluded"], "gap pixels", int(gap.sum()),
              "ms", info["device_ms"])
        same(got[keep], want[keep])
        assert info["paths"] == gap.size * spp and info["rays"] == rays and info["shadow_rays"] == shadow
        if not gap.any():
            assert info["shadow_rays_occluded"] == occluded
        assert info["lights"] == ncs.table_of(name).n and info["device_ms"] > 0
        st = ctx.stats()
        assert st["paths"] == info["paths"] and st["rays"] == info["rays"] and st["trace_launches"] == 1
        assert st["trace_kernel_ms"] > 0 and st["total_ms"] >= st["trace_kernel_ms"]


@pytest.mark.parametrize("depth", ncs.DEPTHS)
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", sorted(ncs.CASES))
def test_the_sum_is_exact_with_both_walks(gpu_ctx, name, spp, depth):
    put(gpu_ctx, name)
    r = ncs.reference(name, depth)
    check_exact(gpu_ctx, name, r, spp, depth)
    if name != "dark" and depth > 1 and spp == 3:
        assert r["shadow"].sum() > r["occluded"].sum() > 0                   # open and occluded shadow rays both occur
        assert (r["value"][..., :3] > 1).any()                                # (no clamp: values above mpt_render's 1 occur)


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3)])
def test_small_image_sizes(gpu_ctx, W, H):
    put(gpu_ctx, "scene.xml", W, H)
    r = ncs.render_ref("scene.xml", 4, W, H)
    check_exact(gpu_ctx, "scene.xml", r, 3, 4)


# ---- identities against mpt_render: no reference needed -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth", [("dark", 1), ("dark", 3), ("dark", 8), ("cornell.xml", 1), ("scene.xml", 1)])
def test_without_a_light_sample_the_call_adds_what_mpt_render_adds(gpu_ctx, name, depth):
    """An empty light table at any depth, or max_depth = 1 (no vertex may draw a light sample), with clamp = 1: all four channels."""
    from metalpathtracer_amd import capi
    put(gpu_ctx, name)
    kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=depth, sample_begin=2, sample_count=3, seed=SEED)
    gpu_ctx.clear_sum()
    gpu_ctx.render(**kw)
    want = gpu_ctx.read_sum()
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN, capi.WALK_AUTO):
        gpu_ctx.clear_sum()
        info = gpu_ctx.render_nee(walk=walk, clamp=1.0, **kw)
        same(gpu_ctx.read_sum(), want)
        assert info["shadow_rays"] == 0 and info["lights"] == (0 if name == "dark" else ncs.table_of(name).n)
    assert want[..., :3].any() and want[..., 3].any()


# ---- order and state ----------------------------------------------------------------------------------------------------------------
def test_sample_ranges_add_up_in_order_and_onto_what_the_sum_holds(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "cornell.xml")
    kw = dict(walk=capi.WALK_REFERENCE, max_depth=4)
    gpu_ctx.clear_sum()
    nee(gpu_ctx, "cornell.xml", sample_begin=0, sample_count=3, **kw)
    whole = gpu_ctx.read_sum()
    gpu_ctx.clear_sum()
    nee(gpu_ctx, "cornell.xml", sample_begin=0, sample_count=2, **kw)
    first = gpu_ctx.read_sum()
    nee(gpu_ctx, "cornell.xml", sample_begin=2, sample_count=1, **kw)                 # a second call adds onto the first
    same(gpu_ctx.read_sum(), whole)
    assert not np.array_equal(first, whole)
    r = ncs.reference("cornell.xml", 4)
    same(whole, nee_ref.accumulate(r["value"]))
    same(first, nee_ref.accumulate(r["value"][:, :, :2]))
    # ... and onto whatever the sum held: a plain render first
    gpu_ctx.clear_sum()
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(5, 5))
    start = gpu_ctx.read_sum()
    nee(gpu_ctx, "cornell.xml", sample_begin=0, sample_count=3, **kw)
    same(gpu_ctx.read_sum(), nee_ref.accumulate(r["value"], start=start))


def test_the_callers_sum_buffer_is_honoured(gpu_ctx):
    from metalpathtracer_amd import capi
    u = put(gpu_ctx, "handmade")
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    other = capi.Context(0)                                          # its sum buffer is device memory this context knows nothing about
    try:
        other.resize(W, H)
        ptr, nbytes = other.sum_buffer()
        assert nbytes == W * H * 16
        gpu_ctx.clear_sum()
        inside = gpu_ctx.read_sum()
        gpu_ctx.set_sum_buffer(ptr)
        try:
            nee(gpu_ctx, "handmade", walk=capi.WALK_REFERENCE, max_depth=4, sample_count=3)
            same(gpu_ctx.read_sum(), other.read_sum())
        finally:
            gpu_ctx.set_sum_buffer(None)
        same(other.read_sum(), nee_ref.accumulate(ncs.reference("handmade", 4)["value"]))
        same(gpu_ctx.read_sum(), inside)                             # the internal buffer was not written
    finally:
        other.close()


def test_the_call_touches_only_the_sum_and_the_stats(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "scene.xml")
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.draw(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(1, 0))
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(1, 0), flags=capi.FLAG_MOMENTS)
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.display(source=capi.DISPLAY_SUM, samples=2)
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    read = lambda: (gpu_ctx.read_frame(), gpu_ctx.read_moments(), gpu_ctx.read_denoised(), gpu_ctx.read_temporal(), gpu_ctx.read_svgf(),
                    gpu_ctx.read_display(), gpu_ctx.read_ao()[0], gpu_ctx.read_ao()[1], gpu_ctx.read_direct()[0], gpu_ctx.read_direct()[1])
    before, s0, st0 = read(), gpu_ctx.read_sum(), gpu_ctx.stats()
    gpu_ctx.render_async(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_begin=2, sample_count=2, seed=(1, 0))    # the call waits for it
    info = nee(gpu_ctx, "scene.xml", walk=capi.WALK_AUTO, max_depth=4, sample_begin=4, sample_count=2)
    st1 = gpu_ctx.stats()
    for a, b in zip(before, read()):
        np.testing.assert_array_equal(a, b)
    assert st1["paths"] == st0["paths"] + 2 * s0.shape[0] * s0.shape[1] + info["paths"]      # the queued render was collected and counted
    assert st1["rays"] > st0["rays"] + info["rays"] and st1["trace_launches"] == 1
    s1 = gpu_ctx.read_sum()
    assert (s1[..., 3] >= s0[..., 3]).all() and not np.array_equal(s0, s1)
    # the result is a sum like any other: the denoiser reads it
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=6)
    assert np.isfinite(gpu_ctx.read_denoised()).all()


def test_both_scene_calls_give_the_same_image_for_the_same_tree(gpu_ctx):
    from metalpathtracer_amd import capi
    sc, buf = ncs.scene_of("handmade")
    u = ncs.uniforms_of("handmade")
    gpu_ctx.build_and_upload(buf[1], buf[2])
    gpu_ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    gpu_ctx.set_uniforms(u)
    gpu_ctx.clear_sum()
    a_info = nee(gpu_ctx, "handmade", walk=capi.WALK_REFERENCE, max_depth=4, sample_count=3)
    a = gpu_ctx.read_sum()
    bvh, idx = gpu_ctx.download_bvh()
    gpu_ctx.upload_scene(bvh, buf[1], buf[2], idx)
    gpu_ctx.clear_sum()
    b_info = nee(gpu_ctx, "handmade", walk=capi.WALK_REFERENCE, max_depth=4, sample_count=3)
    same(gpu_ctx.read_sum(), a)
    for k in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights"):
        assert a_info[k] == b_info[k], k
    assert a_info["shadow_rays"] > 0 and a[..., :3].any()


def test_errors_leave_the_sum_untouched(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "cornell.xml")
    gpu_ctx.clear_sum()
    nee(gpu_ctx, "cornell.xml", max_depth=2, sample_count=1)
    want, st = gpu_ctx.read_sum(), gpu_ctx.stats()
    L, h = gpu_ctx.L, gpu_ctx.h
    good_p = gpu_ctx.params(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=1, seed=SEED)
    good_n = capi.NeeParams(capi.WALK_AUTO, 0.0)
    assert L.mpt_render_nee(h, None, C.byref(good_n), None) == INVALID
    assert L.mpt_render_nee(h, C.byref(good_p), None, None) == INVALID
    bad_params = (dict(rng_mode=capi.RNG_LITERAL), dict(bsdf_mode=capi.BSDF_SCATTER_ALL), dict(shard_count=2), dict(shard_count=2, shard_rank=1),
                  dict(flags=capi.FLAG_MOMENTS), dict(flags=capi.FLAG_COUNT_WORK), dict(sample_count=0), dict(max_depth=0), dict(max_depth=-1))
    for kw in bad_params:
        q = gpu_ctx.params(**{**dict(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=1, seed=SEED), **kw})
        assert L.mpt_render_nee(h, C.byref(q), C.byref(good_n), None) == INVALID, kw
    for walk, clamp in ((3, 0.0), (-1, 0.0), (capi.WALK_AUTO, float("nan"))):
        n = capi.NeeParams(walk, clamp)
        assert L.mpt_render_nee(h, C.byref(good_p), C.byref(n), None) == INVALID, (walk, clamp)
    same(gpu_ctx.read_sum(), want)
    assert gpu_ctx.stats() == st
    # pipeline and slots_per_iter are ignored; info may be NULL; a negative clamp is "none"
    q = gpu_ctx.params(rng_mode=capi.RNG_PHILOX, max_depth=2, sample_count=1, seed=SEED, pipeline=77, slots_per_iter=5)
    gpu_ctx.clear_sum()
    n = capi.NeeParams(capi.WALK_AUTO, -1.0)
    assert L.mpt_render_nee(h, C.byref(q), C.byref(n), None) == 0
    same(gpu_ctx.read_sum(), want)
    # before scene, uniforms and size
    _, buf = ncs.scene_of("cornell.xml")
    u = ncs.uniforms_of("cornell.xml")
    fresh = capi.Context(0)
    try:
        assert fresh.L.mpt_render_nee(fresh.h, C.byref(good_p), C.byref(good_n), None) == NOT_READY
        fresh.upload_scene(*buf)
        assert fresh.L.mpt_render_nee(fresh.h, C.byref(good_p), C.byref(good_n), None) == NOT_READY
        fresh.resize(int(u.screenSize[0]), int(u.screenSize[1]))
        assert fresh.L.mpt_render_nee(fresh.h, C.byref(good_p), C.byref(good_n), None) == NOT_READY
        fresh.set_uniforms(u)
        assert fresh.L.mpt_render_nee(fresh.h, C.byref(q), C.byref(n), None) == 0
        same(fresh.read_sum(), want)
    finally:
        fresh.close()


def test_too_many_lights_is_a_bad_scene_and_nothing_is_rendered(gpu_ctx):
    """MPT_LIGHTS_MAX + 1 tiny emissive triangles (the scene of tests/test_gpu_direct.py): MPT_ERR_BAD_SCENE from the light table, with
    the sum and the statistics as they were; one light fewer renders."""
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
    gpu_ctx.resize(8, 8)
    cam = dict(pos=(1.28, 1.28, 4.0), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
    from metalpathtracer_amd import host
    gpu_ctx.set_uniforms(host.make_uniforms(8, 8, n, n, cam=cam))
    rng = np.random.default_rng(3)
    start = rng.uniform(0.0, 2.0, (8, 8, 4)).astype(np.float32)
    gpu_ctx.write_sum(start)
    gpu_ctx.reset_stats()
    st = gpu_ctx.stats()
    p = gpu_ctx.params(rng_mode=capi.RNG_PHILOX, max_depth=3, sample_count=2, seed=SEED)
    q = capi.NeeParams(capi.WALK_AUTO, 0.0)
    info = capi.NeeInfo()
    assert gpu_ctx.L.mpt_render_nee(gpu_ctx.h, C.byref(p), C.byref(q), C.byref(info)) == BAD_SCENE
    assert b"MPT_LIGHTS_MAX" in gpu_ctx.L.mpt_last_error(gpu_ctx.h)
    same(gpu_ctx.read_sum(), start)
    assert gpu_ctx.stats() == st
    gpu_ctx.build_and_upload(prims[:-1], mats[:-1])
    gpu_ctx.set_uniforms(host.make_uniforms(8, 8, n - 1, n - 1, cam=cam))
    gpu_ctx.write_sum(start)
    assert gpu_ctx.L.mpt_render_nee(gpu_ctx.h, C.byref(p), C.byref(q), C.byref(info)) == 0
    assert info.lights == capi.LIGHTS_MAX and info.paths == 8 * 8 * 2 and info.shadow_rays > 0
    assert not np.array_equal(gpu_ctx.read_sum(), start)


def test_cli_renders_with_nee(tmp_path):
    """mpt_render --nee writes what Renderer.renderNee gives through the same writer; without --nee the file is what it was; the
    combinations that make no sense are refused."""
    from metalpathtracer_amd import capi, host
    W, H, spp, depth = 48, 48, 4, 4
    base = [EXE, "--scene", scene_path("cornell.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth), "--seed", "1",
            "--bvh", "reference"]
    a, b, c = str(tmp_path / "nee.pfm"), str(tmp_path / "plain.pfm"), str(tmp_path / "nee_dn.ppm")
    r = subprocess.run(base + ["--out", a, "--nee", "--nee-walk", "reference"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.splitlines()[-1])
    r = subprocess.run(base + ["--out", b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "nee" not in json.loads(r.stdout.splitlines()[-1])
    r = subprocess.run(base + ["--out", c, "--nee", "--nee-clamp", "4", "--denoise"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.getsize(c) > W * H * 3, r.stderr[-2000:]
    for bad in (["--nee", "--adaptive", "0.05"], ["--nee", "--gpus", "2"], ["--nee", "--ao", "4"], ["--nee", "--direct", "4"], ["--nee", "--rng", "literal"],
                ["--nee", "--bsdf", "scatter-all"], ["--nee", "--frames", "2"], ["--nee-walk", "own"], ["--nee-clamp", "2"],
                ["--nee", "--camera-path", str(tmp_path / "path.txt")], ["--nee", "--camera-path", str(tmp_path / "path.txt"), "--temporal"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "x.ppm")] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--nee" in r.stderr, (bad, r.stderr[-500:])
    # checkpoints: two --nee runs of spp / 2 give the whole render's file; an --nee sum and a plain one never continue each other, nor
    # two --nee sums of different clamps; a plain checkpoint is the file it was
    ck, ck2, ckp, d = str(tmp_path / "nee.ck"), str(tmp_path / "nee2.ck"), str(tmp_path / "plain.ck"), str(tmp_path / "resumed.pfm")
    half = list(base)
    half[half.index("--spp") + 1] = str(spp // 2)
    r = subprocess.run(half + ["--out", d, "--nee", "--nee-walk", "reference", "--checkpoint", ck], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(ck, "rb").read(8) == b"MPTNEE1 ", r.stderr[-2000:]
    r = subprocess.run(half + ["--out", d, "--nee", "--nee-walk", "reference", "--resume", ck, "--checkpoint", ck2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(d, "rb").read() == open(a, "rb").read()
    r = subprocess.run(half + ["--out", d, "--checkpoint", ckp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(ckp, "rb").read(8) == b"MPTSUM2 ", r.stderr[-2000:]
    for bad in (["--resume", ck], ["--nee", "--resume", ckp], ["--nee", "--nee-clamp", "2", "--resume", ck]):
        r = subprocess.run(half + ["--out", d] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "checkpoint" in r.stderr, (bad, r.stderr[-500:])
    rr = host.Renderer(0, scene_path("cornell.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=depth, seed=(1, 0))
        rr.clearSum()
        info = rr.renderNee(spp, depth, walk=capi.WALK_REFERENCE)
        assert info["paths"] == W * H * spp and info["lights"] == 2 and info["rays"] >= info["paths"]
        for key in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights"):
            assert line["nee"][key] == info[key], key
        assert line["paths"] == info["paths"] and line["rays"] == info["rays"]
        mine = str(tmp_path / "mine.pfm")
        assert host.write_pfm(mine, rr.readSum(), scale=1.0 / spp) == 0
        assert open(mine, "rb").read() == open(a, "rb").read()
        rr.clearSum()
        rr.renderBatch(0, spp)
        today = str(tmp_path / "today.pfm")
        assert host.write_pfm(today, rr.readSum(), scale=1.0 / spp) == 0
        assert open(today, "rb").read() == open(b, "rb").read()
        assert open(a, "rb").read() != open(b, "rb").read()
    finally:
        rr.close()


# ---- the same expectation as the path tracer, and less variance -----------------------------------------------------------------------
B, SPP_B, STAT_W, STAT_DEPTH = 64, 64, 32, 4
_stat = {}


def statistics(ctx):
    """Batch means of mpt_render and of mpt_render_nee(clamp = +inf) on the Cornell box with the light's emissionPower 1 and albedo 0, so
    that mpt_render's per-sample clamp can never bite (thr <= 1, the first emitter hit zeroes thr, sky <= 1): [B, H, W, 3] each, B = 64
    batches of 64 spp with different seeds (and different ones for the two estimators: they are independent).  Computed once."""
    from metalpathtracer_amd import capi, host
    if not _stat:
        sc, buf = ncs.scene_of("cornell.xml")
        mats = np.array(buf[2], np.float32).reshape(-1, 2, 4)
        lights = mats[:, 1, 3] > 0
        assert lights.sum() == 2 and (mats[lights, 1, :3] <= 1).all()
        mats[lights, 1, 3] = 1.0
        mats[lights, 0, :3] = 0.0
        assert (mats[:, 0, :3] <= 1).all()
        ctx.upload_scene(buf[0], buf[1], mats, buf[3])
        u = host.make_uniforms(STAT_W, STAT_W, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=CORNELL_CAM)
        ctx.resize(STAT_W, STAT_W)
        ctx.set_uniforms(u)
        pt = np.empty((B, STAT_W, STAT_W, 3), np.float64)
        ne = np.empty_like(pt)
        ms = [0.0, 0.0]
        shadow = 0
        for b in range(B):
            ctx.clear_sum()
            ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=STAT_DEPTH, sample_count=SPP_B, seed=(b, 1))
            ms[0] += ctx.stats()["trace_kernel_ms"]
            pt[b] = ctx.read_sum()[..., :3].astype(np.float64) / SPP_B
            ctx.clear_sum()
            info = ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=STAT_DEPTH, sample_count=SPP_B, seed=(b, 2), walk=capi.WALK_AUTO, clamp=0.0)
            ms[1] += info["device_ms"]
            shadow += info["shadow_rays"]
            ne[b] = ctx.read_sum()[..., :3].astype(np.float64) / SPP_B
        print("trace ms, %d batches of %d spp at %dx%d: mpt_render %.2f, mpt_render_nee %.2f (%d shadow rays)" % (B, SPP_B, STAT_W, STAT_W, ms[0], ms[1], shadow))
        _stat.update(pt=pt, ne=ne)
    return _stat["pt"], _stat["ne"]


def test_nee_has_the_expectation_of_the_path_tracer(gpu_ctx):
    """Per pixel the scalar is the mean of the three channels.  z = (m_nee - m_pt) / sqrt((s2_nee + s2_pt) / B) over the pixels with a
    positive variance: |mean z| <= 5 / sqrt(n), mean z^2 <= 1.3 (under the null about 1.03 +- 0.05 over ~1000 independent pixels);
    the image mean per channel within 5 of its standard errors, and that standard error at most 1 % of the mean."""
    pt, ne = statistics(gpu_ctx)
    x_pt, x_ne = pt.mean(-1), ne.mean(-1)                            # [B, H, W]
    m_pt, m_ne = x_pt.mean(0), x_ne.mean(0)
    v_pt, v_ne = x_pt.var(0, ddof=1), x_ne.var(0, ddof=1)
    still = (v_pt == 0) & (v_ne == 0)
    print("pixels with both variances 0:", int(still.sum()), "of", still.size)
    assert still.sum() <= still.size // 2
    np.testing.assert_allclose(m_ne[still], m_pt[still], rtol=1e-6)
    z = (m_ne - m_pt)[~still] / np.sqrt((v_ne + v_pt)[~still] / B)
    print("pixels:", z.size, "mean z:", z.mean(), "bound", 5 / np.sqrt(z.size), "mean z^2:", (z * z).mean(), "max |z|:", np.abs(z).max())
    assert abs(z.mean()) <= 5 / np.sqrt(z.size)
    assert (z * z).mean() <= 1.3
    i_pt, i_ne = pt.mean((1, 2)), ne.mean((1, 2))                    # [B, 3]: the image mean of every batch
    se = np.sqrt((i_pt.var(0, ddof=1) + i_ne.var(0, ddof=1)) / B)
    print("image mean pt", i_pt.mean(0), "nee", i_ne.mean(0), "standard error", se, "difference in units of it", (i_ne.mean(0) - i_pt.mean(0)) / se,
          "relative", se / i_pt.mean(0))
    assert (np.abs(i_ne.mean(0) - i_pt.mean(0)) <= 5 * se).all()
    assert (se <= 0.01 * i_pt.mean(0)).all()


def test_nee_has_less_variance_than_the_path_tracer(gpu_ctx):
    pt, ne = statistics(gpu_ctx)
    v_pt, v_ne = pt.mean(-1).var(0, ddof=1), ne.mean(-1).var(0, ddof=1)
    both = (v_pt > 0) & (v_ne > 0)
    ratio = v_pt[both] / v_ne[both]
    print("pixels:", int(both.sum()), "mean of s2_pt / s2_nee:", ratio.mean(), "median:", np.median(ratio), "ratio of the summed variances:",
          v_pt[both].sum() / v_ne[both].sum())
    assert ratio.mean() > 1
