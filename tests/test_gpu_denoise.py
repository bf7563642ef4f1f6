"""The denoiser on the MI355X: guide buffers against the oracle's first hit, the filter kernels against the numpy restatement
(tests/denoise_ref.py), the end-to-end entry points against the unit hook, no side effects, staleness, quality, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
from conftest import CORNELL_CAM, ROOT, oracle_scene, scene_path

pytestmark = pytest.mark.gpu

TOL = 1e-4
# with sigma_luminance 0.05 and sigma_normal 1024 the weights amplify the ulp differences of exp / pow between the device and numpy
# level by level: 1920x1080 measured 2.7e-4 at N = 5 and 1.0e-3 at N = 8 (the default sigmas stay within 1e-4 at every size and N)
TOL_EXTREME = 5e-3


def _ctx_for(name, W, H, cam=None):
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    sc, buf = oracle_scene(name)
    ctx = capi.Context(0)
    ctx.upload_scene(*buf)
    ctx.resize(W, H)
    u = ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=cam)
    ctx.set_uniforms(capi.Uniforms.from_buffer_copy(bytes(u)))
    return ctx, u, buf


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name,cam,W,H", [("scene.xml", None, 96, 54), ("cornell.xml", CORNELL_CAM, 64, 64),
                                          ("bunny20.xml", None, 96, 54)])
def test_guides_match_oracle_first_hit(name, cam, W, H):
    from oracle import binding as ob
    ctx, u, buf = _ctx_for(name, W, H, cam)
    try:
        ad, nc, prim = ctx.read_aovs()
    finally:
        ctx.close()
    rad, rnc, rprim = dr.first_hit_guides(u, buf, ob.first_hit)
    same = prim == rprim
    assert same.mean() >= 0.999, same.mean()
    assert (prim >= 0).any() and (prim < 0).any() or name == "cornell.xml"
    np.testing.assert_array_equal(ad[same][:, :3], rad[same][:, :3])
    np.testing.assert_array_equal(nc[same][:, 3], rnc[same][:, 3])
    hit = same & (prim >= 0)
    assert np.abs(nc[hit][:, :3] - rnc[hit][:, :3]).max() <= 1e-6
    assert (np.abs(ad[hit][:, 3] - rad[hit][:, 3]) <= 1e-6 * rad[hit][:, 3]).all()


def _random_case(rng, H, W):
    c = rng.random((H, W, 4), np.float32) * np.float32(2)
    alb = rng.random((H, W, 3), np.float32) * np.float32(0.9) + np.float32(0.05)
    t = rng.random((H, W), np.float32) * np.float32(5) + np.float32(0.5)
    n = rng.normal(size=(H, W, 3)).astype(np.float32)
    n[: H // 2] = (0, 0, 1)                                  # a flat region, so that weights are not all tiny
    n /= np.linalg.norm(n, axis=-1, keepdims=True).astype(np.float32)
    cls = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2], np.float32), size=(H, W))
    ad = np.concatenate([alb, t[..., None]], -1).astype(np.float32)
    nc = np.concatenate([n, cls[..., None]], -1).astype(np.float32)
    return c, ad, nc


SIGMAS = [dict(), dict(sigma_luminance=0.05, sigma_normal=1024.0, sigma_depth=0.01),
          dict(sigma_luminance=1000.0, sigma_normal=0.5, sigma_depth=1000.0)]


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (65, 33), (1920, 1080)])
def test_denoise_image_matches_restatement(gpu_ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    c, ad, nc = _random_case(rng, H, W)
    passthru = nc[..., 3] != 0
    iters = range(0, 9) if W * H < 10000 else (0, 1, 3, 5, 8)
    for sg in SIGMAS if W * H < 10000 else SIGMAS[:2]:
        for N in iters:
            got = gpu_ctx.denoise_image(c, ad, nc, iterations=N, **sg)
            want = dr.denoise(c, ad, nc, iterations=N, **sg)
            assert np.array_equal(_bits(got[passthru]), _bits(c[passthru])), (N, sg)
            assert np.array_equal(_bits(got[..., 3]), _bits(c[..., 3]))
            if N == 0:
                assert np.array_equal(_bits(got), _bits(c))
            tol = TOL if sg is not SIGMAS[1] else TOL_EXTREME
            assert np.abs(got - want).max() <= tol, (N, sg, float(np.abs(got - want).max()))


def test_denoise_image_real_render_matches_restatement(gpu_ctx):
    ctx, u, buf = _ctx_for("cornell.xml", 64, 64, CORNELL_CAM)
    try:
        ctx.render(sample_count=4, max_depth=8)
        c = ctx.read_sum() / 4
        ad, nc, _ = ctx.read_aovs()
    finally:
        ctx.close()
    for N in (0, 1, 5, 8):
        got = gpu_ctx.denoise_image(c, ad, nc, iterations=N)
        want = dr.denoise(c, ad, nc, iterations=N)
        assert np.abs(got - want).max() <= TOL * max(1.0, float(np.abs(want).max())), N


def test_end_to_end_sum_frame_async_and_no_side_effects():
    from metalpathtracer_amd import capi
    ctx, u, buf = _ctx_for("cornell.xml", 80, 48, CORNELL_CAM)
    try:
        ctx.render(sample_count=4, max_depth=8)
        s0, f0, st0 = ctx.read_sum(), ctx.read_frame(), ctx.stats()
        ad, nc, prim = ctx.read_aovs()
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        got = ctx.read_denoised()
        assert np.array_equal(_bits(ctx.read_sum()), _bits(s0)) and np.array_equal(_bits(ctx.read_frame()), _bits(f0))
        assert ctx.stats() == st0
        want = ctx.denoise_image(s0 / 4, ad, nc)
        assert np.array_equal(_bits(got), _bits(want))
        ptr, nbytes = ctx.denoised_buffer()
        assert ptr and nbytes == 80 * 48 * 16
        # asynchronous renders, denoised without an explicit wait: the same bits as with one
        ctx.clear_sum()
        ctx.render_async(sample_count=2, max_depth=8)
        ctx.render_async(sample_begin=2, sample_count=2, max_depth=8)
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        a = ctx.read_denoised()
        ctx.wait()
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        assert np.array_equal(_bits(a), _bits(ctx.read_denoised()))
        assert np.array_equal(_bits(a), _bits(want))
        # FRAME after a few draws
        for f in range(3):
            u.frameCount = f
            ctx.set_uniforms(capi.Uniforms.from_buffer_copy(bytes(u)))
            ctx.draw(max_depth=8, sample_begin=f)
        fr = ctx.read_frame()
        ctx.denoise(source=capi.DENOISE_FRAME)
        assert np.array_equal(_bits(ctx.read_denoised()), _bits(ctx.denoise_image(fr, ad, nc)))
    finally:
        ctx.close()


def test_argument_errors_and_not_ready():
    from metalpathtracer_amd import capi
    ctx = capi.Context(0)
    try:
        with pytest.raises(capi.MptError) as e:
            ctx.denoise(source=capi.DENOISE_FRAME)
        assert e.value.status == 5   # MPT_ERR_NOT_READY: no scene
        for kw in (dict(source=capi.DENOISE_SUM, samples=0), dict(source=2, samples=1), dict(source=0, samples=1, iterations=9)):
            with pytest.raises(capi.MptError) as e:
                ctx.denoise(**kw)
            assert e.value.status == 1, kw
    finally:
        ctx.close()


def test_guides_follow_the_camera():
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    ctx, u, buf = _ctx_for("scene.xml", 64, 36)
    try:
        _, _, p0 = ctx.read_aovs()
        cam = ob.camera_reset()
        cam["pos"] = (8.0, 20.0, 45.0)
        u2 = ob.make_uniforms(64, 36, u.primitiveCount, u.triangleCount, cam=cam)
        ctx.set_uniforms(capi.Uniforms.from_buffer_copy(bytes(u2)))
        _, _, p1 = ctx.read_aovs()
        assert (p0 != p1).mean() > 0.05
        _, _, r1 = dr.first_hit_guides(u2, buf, ob.first_hit)
        assert (p1 == r1).mean() >= 0.999
    finally:
        ctx.close()


def test_quality_cornell_256():
    """Denoised 4 spp against 1024 spp (another seed) on the device: at least the calibrated factor (tests/test_denoise_cpu.py)."""
    from metalpathtracer_amd import capi
    from test_denoise_cpu import MIN_FACTOR
    ctx, u, buf = _ctx_for("cornell.xml", 256, 256, CORNELL_CAM)
    try:
        ctx.render(sample_count=1024, max_depth=8, seed=(7, 0))
        ref = ctx.read_sum() / 1024
        ctx.clear_sum()
        ctx.render(sample_count=4, max_depth=8)
        noisy = ctx.read_sum() / 4
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        out = ctx.read_denoised()
    finally:
        ctx.close()
    m0 = float(((noisy[..., :3] - ref[..., :3]).astype(np.float64) ** 2).mean())
    m1 = float(((out[..., :3] - ref[..., :3]).astype(np.float64) ** 2).mean())
    print("cornell 256: mse %.3e -> %.3e, factor %.2f" % (m0, m1, m0 / m1))
    assert m0 / m1 >= MIN_FACTOR["cornell.xml"], m0 / m1


def test_cli_denoise_matches_python(tmp_path):
    from metalpathtracer_amd import capi, host
    exe = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
    out = str(tmp_path / "d.pfm")
    W, H, spp = 96, 54, 4
    r = subprocess.run([exe, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp),
                        "--depth", "8", "--seed", "1", "--bvh", "reference", "--denoise", "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hdr = ("PF\n%d %d\n-1.0\n" % (W, H)).encode()
    raw = open(out, "rb").read()
    assert raw.startswith(hdr)
    img = np.frombuffer(raw[len(hdr):], np.float32).reshape(H, W, 3)[::-1]
    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        rr.clearSum()
        rr.renderBatch(0, spp)
        want = rr.denoise()
    finally:
        rr.close()
    np.testing.assert_array_equal(img, want[..., :3])
