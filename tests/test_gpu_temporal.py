"""Temporal accumulation on the MI355X: the kernels against the numpy restatement (tests/temporal_ref.py) bit for bit, the context's
entry point against the unit hook, the still and the moving camera end to end, drops, no side effects, the filtered history, and the
CLI against the Python host layer."""
import json
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as tr
from conftest import CORNELL_CAM, ROOT, oracle_scene, scene_path

pytestmark = pytest.mark.gpu
F = np.float32
PARAM_SETS = [dict(), dict(max_history=8, depth_tolerance=0.3, normal_threshold=0.1, min_weight=0.3),
              dict(max_history=1000, depth_tolerance=0.001, normal_threshold=0.99, min_weight=0.9)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(u):
    from metalpathtracer_amd import capi
    return capi.Uniforms.from_buffer_copy(bytes(u))


def _cam(pos, fwd, W, H, vfov=50.0):
    from oracle import binding as ob
    return ob.make_uniforms(W, H, 1, 0, cam=dict(pos=pos, fwd=fwd, up=(0.0, 1.0, 0.0), vfov=vfov))


def _ctx_for(name, W, H):
    from metalpathtracer_amd import capi
    sc, buf = oracle_scene(name)
    ctx = capi.Context(0)
    ctx.upload_scene(*buf)
    ctx.resize(W, H)
    return ctx, sc, buf


def _check_image(gpu_ctx, c, ad, nc, u, hist, adp, ncp, up, what, **params):
    if hist is None:
        got, info = gpu_ctx.temporal_image(c, ad, nc, _cu(u), **params)
        want, n_reset = tr.accumulate(c, ad, nc, u, **params)
    else:
        got, info = gpu_ctx.temporal_image(c, ad, nc, _cu(u), hist, adp, ncp, _cu(up), **params)
        want, n_reset = tr.accumulate(c, ad, nc, u, hist, adp, ncp, up, **params)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, params, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert info == dict(pixels_reprojected=c.shape[0] * c.shape[1] - n_reset, pixels_reset=n_reset), (what, params)
    return n_reset


def _random_guides(rng, H, W, t_lo=2.0, t_hi=9.0):
    n = rng.normal(size=(H, W, 3)).astype(np.float32)
    n[: H // 2] = (0.0, 0.0, 1.0)
    n /= np.linalg.norm(n, axis=-1, keepdims=True).astype(np.float32)
    cls = rng.choice(np.array([0, 0, 0, 0, 1, 2], np.float32), size=(H, W))
    t = (rng.random((H, W), np.float32) * F(t_hi - t_lo) + F(t_lo)).astype(np.float32)
    t = np.where(cls == 2, F(np.inf), t).astype(np.float32)
    ad = np.concatenate([rng.random((H, W, 3), np.float32), t[..., None]], -1).astype(np.float32)
    nc = np.concatenate([n, cls[..., None]], -1).astype(np.float32)
    return ad, nc


def _plane_guides(u, W, H, depth, rng):
    """The plane z = -depth seen from u (float64 construction, then float32), with patches of sky and of light."""
    k = tr.camera_key(u).astype(np.float64)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    dv = k[9:12] + ((px + 0.5) / W)[..., None] * k[3:6] + ((py + 0.5) / H)[..., None] * k[6:9] - k[0:3]
    d = dv / np.linalg.norm(dv, axis=-1, keepdims=True)
    t = depth / np.maximum(-d[..., 2], 1e-3)
    ad = np.concatenate([rng.random((H, W, 3)), t[..., None]], -1).astype(np.float32)
    nc = np.zeros((H, W, 4), np.float32)
    nc[..., 2] = 1
    cls = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2], np.float32), size=((H + 3) // 4, (W + 3) // 4))
    nc[..., 3] = np.repeat(np.repeat(cls, 4, axis=0), 4, axis=1)[:H, :W]
    ad[..., 3] = np.where(nc[..., 3] == 2, F(np.inf), ad[..., 3])
    return ad, nc


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (65, 33), (1920, 1080)])
def test_temporal_image_matches_restatement_bit_for_bit(gpu_ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    u0 = _cam((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H)
    cams = [_cam((0.05, -0.02, 0.03), (0.02, 0.01, -1.0), W, H), _cam((0.4, 0.1, -0.3), (-0.2, 0.05, -1.0), W, H),
            _cam((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), W, H), u0]
    big = W * H > 10000
    kinds = 0
    for ci, u1 in enumerate(cams):
        for geometry in ("random", "plane"):
            if geometry == "random":
                ad0, nc0 = _random_guides(rng, H, W)
                ad1, nc1 = _random_guides(rng, H, W)
            else:
                ad0, nc0 = _plane_guides(u0, W, H, 5.0, rng)
                ad1, nc1 = _plane_guides(u1, W, H, 5.0, rng)
            c = rng.random((H, W, 4), np.float32) * F(2)
            hist = rng.random((H, W, 4), np.float32) * F(2)
            hist[..., 3] = rng.integers(1, 40, size=(H, W)).astype(np.float32)
            for params in PARAM_SETS[:1] if big else PARAM_SETS:
                n_reset = _check_image(gpu_ctx, c, ad1, nc1, u1, hist, ad0, nc0, u0, (W, H, ci, geometry), **params)
                kinds |= 1 if n_reset == 0 else 2 if n_reset == W * H else 4
    _check_image(gpu_ctx, c, ad1, nc1, u1, None, None, None, None, (W, H, "no history"))
    assert kinds == 7 or W * H < 100, kinds    # nothing reset (same camera), everything reset, and a mixture were all seen


@pytest.mark.parametrize("name,cam,W,H", [("cornell.xml", CORNELL_CAM, 64, 64), ("scene.xml", None, 96, 54), ("bunny20.xml", None, 96, 54)])
def test_temporal_image_real_guides_match_restatement(gpu_ctx, name, cam, W, H):
    from oracle import binding as ob
    ctx, sc, buf = _ctx_for(name, W, H)
    cam0 = cam or ob.camera_reset()
    P = tr.PATHS[name]
    try:
        views = []
        for f in (0, 3):
            u = ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=tr.path_camera(cam0, f, P["step"], yaw_deg=1.0))
            ctx.set_uniforms(_cu(u))
            ad, nc, _ = ctx.read_aovs()
            ctx.clear_sum()
            ctx.render(sample_begin=f, sample_count=1, max_depth=8)
            views.append((u, ctx.read_sum(), ad, nc))
    finally:
        ctx.close()
    (u0, c0, ad0, nc0), (u1, c1, ad1, nc1) = views
    hist, _ = tr.accumulate(c0, ad0, nc0, u0)
    for params in PARAM_SETS:
        n_reset = _check_image(gpu_ctx, c1, ad1, nc1, u1, hist, ad0, nc0, u0, name, **params)
        assert n_reset < W * H and (n_reset > 0 or params), (name, params, n_reset)   # (the strip that came into view has no history)


@pytest.mark.parametrize("source", ["sum", "frame"])
def test_accumulate_equals_the_unit_hook(gpu_ctx, source):
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    W, H, spp = 80, 48, 2
    ctx, sc, buf = _ctx_for("scene.xml", W, H)
    cam0 = ob.camera_reset()
    try:
        prev = None
        for f, pf in enumerate((0, 2, 2, 5)):     # three cameras, the second one twice (the same-camera rule)
            u = ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=tr.path_camera(cam0, pf, (0.3, 0.0, 0.1), yaw_deg=0.4))
            u.frameCount = f
            ctx.set_uniforms(_cu(u))
            if source == "sum":
                ctx.clear_sum()
                ctx.render(sample_begin=f * spp, sample_count=spp, max_depth=8)
                info = ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=spp)
                c = ctx.read_sum() / F(spp)
            else:
                ctx.draw(max_depth=8, sample_begin=f)
                info = ctx.temporal_accumulate(source=capi.DENOISE_FRAME)
                c = ctx.read_frame()
            got = ctx.read_temporal()
            ad, nc, _ = ctx.read_aovs()
            if prev is None:
                want, winfo = gpu_ctx.temporal_image(c, ad, nc, _cu(u))
            else:
                want, winfo = gpu_ctx.temporal_image(c, ad, nc, _cu(u), prev[0], prev[1], prev[2], _cu(prev[3]))
            assert np.array_equal(_bits(got), _bits(want)), (source, f)
            assert info == winfo and info["pixels_reprojected"] + info["pixels_reset"] == W * H, (source, f, info, winfo)
            if f == 0:
                assert info["pixels_reset"] == W * H
            elif pf == 2 and f == 2:
                assert info["pixels_reset"] == 0
            else:
                assert info["pixels_reset"] < W * H // 4
            prev = (got, ad, nc, u)
        ptr, nbytes = ctx.temporal_buffer()
        assert ptr and nbytes == W * H * 16
    finally:
        ctx.close()


def test_still_camera_is_the_running_mean():
    """K = 8 frames of 1 spp: n = 8 everywhere and the colour within 2^-19 of sum / 8 of one 8-spp render (per-sample colours are
    clamped to [0, 1]: eight updates of three roundings of at most 2^-25 each, plus the seven additions of the sum of at most 2^-22
    each divided by 8, stay below 2^-19).  With max_history = 4, n = 4."""
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    W, H, K = 96, 54, 8
    ctx, sc, buf = _ctx_for("scene.xml", W, H)
    try:
        ctx.set_uniforms(_cu(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count)))
        for maxh in (8, 32, 4):
            ctx.temporal_reset()
            for f in range(K):
                ctx.clear_sum()
                ctx.render(sample_begin=f, sample_count=1, max_depth=8)
                info = ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=1, max_history=maxh)
                assert info["pixels_reset"] == (W * H if f == 0 else 0)
            hist = ctx.read_temporal()
            assert (hist[..., 3] == min(K, maxh)).all(), maxh
            if maxh >= K:
                ctx.clear_sum()
                ctx.render(sample_begin=0, sample_count=K, max_depth=8)
                mean = ctx.read_sum() / F(K)
                err = float(np.abs(hist[..., :3].astype(np.float64) - mean[..., :3].astype(np.float64)).max())
                print("still camera, max_history %d: max |history - sum / 8| = %.3e (2^-19 = %.3e)" % (maxh, err, 2.0 ** -19))
                assert err <= 2.0 ** -19, (maxh, err)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(tr.PATHS))
def test_moving_camera_end_to_end(name):
    """The three calibration paths on the device: F >= 0.9 x the restatement's (the renders are bit-identical to the oracle's; the
    margin is for the guides, which may differ from the oracle's first hit in up to 0.1 % of the pixels)."""
    from metalpathtracer_amd import capi
    from test_temporal_cpu import HELD_F, MAX_RESET
    P = tr.PATHS[name]
    W, H = P["W"], P["H"]
    ctx, sc, buf = _ctx_for(name, W, H)
    try:
        for f, u in enumerate(tr.path_uniforms(name, sc)):
            ctx.set_uniforms(_cu(u))
            ctx.clear_sum()
            ctx.render(sample_begin=f, sample_count=1, max_depth=8, seed=(1, 0))
            info = ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=1)
        raw, hist = ctx.read_sum(), ctx.read_temporal()
        ctx.clear_sum()
        ctx.render(sample_count=1024, max_depth=8, seed=(7, 0))
        hi = ctx.read_sum() / F(1024)
    finally:
        ctx.close()
    f_dev = tr.mse(raw, hi) / tr.mse(hist, hi)
    share = info["pixels_reset"] / float(W * H)
    print("%s on the device: F %.3f (restatement %.2f), %.2f %% of the last frame reset" % (name, f_dev, HELD_F[name], 100 * share))
    assert f_dev >= 0.9 * HELD_F[name], (name, f_dev)
    assert share <= MAX_RESET, (name, share)


def test_drops_and_not_ready():
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    W, H = 64, 36
    ctx, sc, buf = _ctx_for("scene.xml", W, H)
    try:
        u = _cu(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count))
        for call in (ctx.read_temporal, ctx.temporal_buffer, ctx.denoise_temporal):
            with pytest.raises(capi.MptError) as e:
                call()
            assert e.value.status == 5, call     # MPT_ERR_NOT_READY: no history
        with pytest.raises(capi.MptError) as e:
            ctx.temporal_accumulate(source=capi.DENOISE_FRAME)
        assert e.value.status == 5                # no uniforms yet
        ctx.set_uniforms(u)

        def frame(f):
            ctx.clear_sum()
            ctx.render(sample_begin=f, sample_count=1, max_depth=8)
            return ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=1)["pixels_reset"]

        assert frame(0) == W * H and frame(1) == 0
        ctx.clear_sum()                           # mpt_clear_sum does not touch the history
        assert ctx.read_temporal()[..., 3].min() == 2 and frame(2) == 0
        for kw in (dict(source=capi.DENOISE_SUM, samples=0), dict(source=2, samples=1), dict(samples=1, depth_tolerance=float("nan")),
                   dict(samples=1, min_weight=float("nan"))):
            before = ctx.read_temporal()
            with pytest.raises(capi.MptError) as e:
                ctx.temporal_accumulate(**kw)
            assert e.value.status == 1, kw
            assert np.array_equal(_bits(ctx.read_temporal()), _bits(before))      # refused with nothing changed
        drops = [("resize", lambda: ctx.resize(W, H)), ("upload_scene", lambda: ctx.upload_scene(*buf)),
                 ("build_and_upload", lambda: ctx.build_and_upload(buf[1], buf[2])), ("temporal_reset", ctx.temporal_reset)]
        for i, (what, drop) in enumerate(drops):
            assert frame(10 + 2 * i) == 0, what
            drop()
            with pytest.raises(capi.MptError) as e:
                ctx.read_temporal()
            assert e.value.status == 5, what
            assert frame(11 + 2 * i) == W * H, what
        ctx.resize(W // 2, H // 2)                # another size: new buffers
        ctx.set_uniforms(_cu(ob.make_uniforms(W // 2, H // 2, sc.prim_count, sc.triangle_count)))
        assert frame(30) == (W // 2) * (H // 2) and frame(31) == 0
        assert ctx.read_temporal().shape == (H // 2, W // 2, 4)
    finally:
        ctx.close()


def test_no_side_effects_async_and_filtered_history():
    """(A queued render that FAILS is reported by mpt_temporal_accumulate through the same drain-then-wait path as mpt_denoise; it is
    not exercised here: only a HIP error or a ring overflow makes a queued render fail, and neither can be had harmlessly.)"""
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    W, H = 80, 48
    ctx, sc, buf = _ctx_for("cornell.xml", W, H)
    try:
        u0 = ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=CORNELL_CAM)
        u1 = ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=tr.path_camera(CORNELL_CAM, 20, (0.01, 0.0, 0.0)))
        ctx.set_uniforms(_cu(u0))
        ctx.draw(max_depth=8)
        ctx.render(sample_count=4, max_depth=8)
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        s0, f0, d0, st0 = ctx.read_sum(), ctx.read_frame(), ctx.read_denoised(), ctx.stats()
        ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=4)
        ctx.set_uniforms(_cu(u1))
        info = ctx.temporal_accumulate(source=capi.DENOISE_FRAME)
        assert 0 < info["pixels_reset"] < W * H
        assert np.array_equal(_bits(ctx.read_sum()), _bits(s0)) and np.array_equal(_bits(ctx.read_frame()), _bits(f0))
        assert np.array_equal(_bits(ctx.read_denoised()), _bits(d0))
        assert ctx.stats() == st0
        # the filtered history: the a-trous kernels over the history with the current guides
        hist = ctx.read_temporal()
        ad, nc, _ = ctx.read_aovs()
        for N in (0, 3):
            ctx.denoise_temporal(iterations=N)
            assert np.array_equal(_bits(ctx.read_denoised()), _bits(ctx.denoise_image(hist, ad, nc, iterations=N))), N
        assert np.array_equal(_bits(ctx.read_temporal()), _bits(hist))
        # asynchronous renders, accumulated without an explicit wait: the same bits as with one
        ctx.temporal_reset()
        ctx.clear_sum()
        ctx.render_async(sample_count=2, max_depth=8)
        ctx.render_async(sample_begin=2, sample_count=2, max_depth=8)
        ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=4)
        a = ctx.read_temporal()
        ctx.wait()
        ctx.temporal_reset()
        ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=4)
        assert np.array_equal(_bits(a), _bits(ctx.read_temporal()))
        assert np.array_equal(_bits(a[..., :3]), _bits((ctx.read_sum() / F(4))[..., :3]))
    finally:
        ctx.close()


CAMERA_PATH = "2\n3 d mouse 4 0\n2 w\n"


@pytest.mark.parametrize("denoise", [False, True])
def test_cli_temporal_matches_the_python_host_layer(tmp_path, denoise):
    from metalpathtracer_amd import capi, host
    exe = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
    path = tmp_path / "path.txt"
    path.write_text(CAMERA_PATH)
    out_dir = tmp_path / "runs"
    W, H, spp = 96, 54, 2
    r = subprocess.run([exe, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--depth", "8", "--seed", "1",
                        "--bvh", "reference", "--camera-path", str(path), "--out-dir", str(out_dir), "--temporal", "--temporal-spp", str(spp),
                        "--temporal-history", "16"] + (["--denoise"] if denoise else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    frames = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"frame"')]
    assert [f["frame"] for f in frames] == list(range(7))
    assert all(f["reprojected"] + f["reset"] == W * H for f in frames)
    assert frames[0]["reset"] == W * H and frames[1]["reset"] == 0 and frames[2]["reset"] < W * H
    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        inputs = [dict()] * 2 + [dict(move=(1, 0, 0), rotate=(4, 0))] * 3 + [dict(move=(0, 0, 1))] * 2
        for f, inp in enumerate(inputs):
            rr.input(**inp)
            info = rr.drawTemporal(spp, max_history=16)
            assert info == dict(pixels_reprojected=frames[f]["reprojected"], pixels_reset=frames[f]["reset"]), f
            img = rr.denoiseTemporal() if denoise else rr.readTemporal()
            want = str(tmp_path / "want.ppm")
            assert host.write_ppm(want, img) == 0
            assert open(want, "rb").read() == open(out_dir / ("frame_%04d.ppm" % f), "rb").read(), f
        assert rr.readTemporal()[..., 3].max() <= 7 + 1e-5     # (seven frames; the bilinear mean of the lengths rounds a few ulps)
    finally:
        rr.close()
