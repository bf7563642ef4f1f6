"""SVGF on the MI355X: the kernels against the numpy restatement (tests/svgf_ref.py) — step A bit for bit, steps B and C within the
tolerance of tests/test_gpu_denoise.py —, the context's entry point against the unit hook, the still and the moving camera end to
end, drops, no side effects, and the CLI against the Python host layer."""
import json
import os
import subprocess

import numpy as np
import pytest

import svgf_ref as sr
import temporal_ref as tr
from conftest import CORNELL_CAM, ROOT, oracle_scene, scene_path

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-4      # tests/test_gpu_denoise.py: max |device - restatement| <= TOL * max(1, max |restatement|); exp / pow differ by an ulp or so
A_SETS = [dict(), dict(max_history=8, depth_tolerance=0.3, normal_threshold=0.1, min_weight=0.3)]


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


def _close(got, want, what):
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    scale = max(1.0, float(np.abs(want).max()))
    assert np.isfinite(want).all() and err <= TOL * scale, (what, err, scale)
    return err / scale


def _check_image(gpu_ctx, c, ad, nc, u, prev, what, worst, **params):
    """The unit hook against the restatement.  prev: None or (history, moments, albedo_depth, normal_class, uniforms)."""
    if prev is None:
        got = gpu_ctx.svgf_image(c, ad, nc, _cu(u), **params)
        want = sr.svgf_image(c, ad, nc, u, **params)
    else:
        got = gpu_ctx.svgf_image(c, ad, nc, _cu(u), prev[0], prev[1], prev[2], prev[3], _cu(prev[4]), **params)
        want = sr.svgf_image(c, ad, nc, u, *prev, **params)
    (gh, gmv, gf, info), (wh, wmv, wf, n_reset) = got, want
    assert info == dict(pixels_reprojected=c.shape[0] * c.shape[1] - n_reset, pixels_reset=n_reset), (what, params)
    diff = _bits(gmv[..., :2]) != _bits(wmv[..., :2])
    assert not diff.any(), (what, params, "moments", int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert np.array_equal(_bits(gh[..., 3]), _bits(wh[..., 3])) and np.array_equal(_bits(gf[..., 3]), _bits(wh[..., 3])), (what, params)
    assert (gmv[..., 3] == 0).all() and (gmv[..., 2][nc[..., 3] != 0] == 0).all()
    feedback = params.get("feedback", -1) > 0 and params.get("iterations", -1) != 0
    if feedback:
        worst[0] = max(worst[0], _close(gh[..., :3], wh[..., :3], (what, params, "history with feedback")))
    else:
        diff = _bits(gh) != _bits(wh)
        assert not diff.any(), (what, params, "history", int(diff.sum()), np.argwhere(diff)[:4].tolist())
    worst[0] = max(worst[0], _close(gmv[..., 2], wmv[..., 2], (what, params, "V_0")), _close(gf[..., :3], wf[..., :3], (what, params, "filtered")))
    other = nc[..., 3] != 0
    assert np.array_equal(_bits(gf[other]), _bits(wf[other])), (what, params)     # (X, n) of step A, untouched
    return n_reset


def _random_guides(rng, H, W, t_lo=2.0, t_hi=9.0):
    """Depth steps and creases at every pixel in the lower half, one normal and smooth depth in the upper; sky and emitters in 4 x 4
    blocks so that surfaces have surface neighbours."""
    n = rng.normal(size=(H, W, 3)).astype(np.float32)
    n[: H // 2] = (0.0, 0.0, 1.0)
    n /= np.linalg.norm(n, axis=-1, keepdims=True).astype(np.float32)
    cls = rng.choice(np.array([0, 0, 0, 0, 1, 2], np.float32), size=((H + 3) // 4, (W + 3) // 4))
    cls = np.repeat(np.repeat(cls, 4, axis=0), 4, axis=1)[:H, :W]
    t = (rng.random((H, W), np.float32) * F(t_hi - t_lo) + F(t_lo)).astype(np.float32)
    px, py = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    t[: H // 2] = (F(4) + F(0.01) * px + F(0.02) * py)[: H // 2]
    t = np.where(cls == 2, F(np.inf), t).astype(np.float32)
    ad = np.concatenate([F(0.2) + F(0.8) * rng.random((H, W, 3), np.float32), t[..., None]], -1).astype(np.float32)
    nc = np.concatenate([n, cls[..., None]], -1).astype(np.float32)
    return ad, nc


def _plane_guides(u, W, H, depth, rng):
    """The plane z = -depth seen from u (float64 construction, then float32), with patches of sky and of light."""
    k = tr.camera_key(u).astype(np.float64)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    dv = k[9:12] + ((px + 0.5) / W)[..., None] * k[3:6] + ((py + 0.5) / H)[..., None] * k[6:9] - k[0:3]
    d = dv / np.linalg.norm(dv, axis=-1, keepdims=True)
    t = depth / np.maximum(-d[..., 2], 1e-3)
    ad = np.concatenate([0.2 + 0.8 * rng.random((H, W, 3)), t[..., None]], -1).astype(np.float32)
    nc = np.zeros((H, W, 4), np.float32)
    nc[..., 2] = 1
    cls = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2], np.float32), size=((H + 3) // 4, (W + 3) // 4))
    nc[..., 3] = np.repeat(np.repeat(cls, 4, axis=0), 4, axis=1)[:H, :W]
    ad[..., 3] = np.where(nc[..., 3] == 2, F(np.inf), ad[..., 3])
    return ad, nc


def _random_state(rng, H, W):
    """A plausible history: n from 1 to 39 (some below 4), M2 >= M1^2."""
    hist = rng.random((H, W, 4), np.float32) * F(2)
    hist[..., 3] = rng.integers(1, 40, size=(H, W)).astype(np.float32)
    m1 = sr.lum(hist[..., :3])
    mom = np.stack([m1, m1 * m1 + F(0.2) * rng.random((H, W), np.float32)], -1).astype(np.float32)
    return hist, mom


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (37, 29), (96, 54), (130, 70), (333, 190)])
def test_svgf_image_matches_restatement(gpu_ctx, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    u0 = _cam((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), W, H)
    cams = [_cam((0.05, -0.02, 0.03), (0.02, 0.01, -1.0), W, H), _cam((0.4, 0.1, -0.3), (-0.2, 0.05, -1.0), W, H),
            _cam((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), W, H), u0]
    kinds, worst = 0, [0.0]
    for ci, u1 in enumerate(cams):
        for geometry in ("random", "plane"):
            if geometry == "random":
                ad0, nc0 = _random_guides(rng, H, W)
                ad1, nc1 = _random_guides(rng, H, W)
            else:
                ad0, nc0 = _plane_guides(u0, W, H, 5.0, rng)
                ad1, nc1 = _plane_guides(u1, W, H, 5.0, rng)
            if ci == 3:
                ad1, nc1 = ad0, nc0                                       # the same camera sees the same guides
            c = rng.random((H, W, 4), np.float32) * F(2)
            hist, mom = _random_state(rng, H, W)
            prev = (hist, mom, ad0, nc0, u0)
            for N in range(6):
                pa = A_SETS[N % 2]
                n_reset = _check_image(gpu_ctx, c, ad1, nc1, u1, prev, (W, H, ci, geometry), worst, iterations=N, **pa)
                kinds |= 1 if n_reset == 0 else 2 if n_reset == W * H else 4
            _check_image(gpu_ctx, c, ad1, nc1, u1, prev, (W, H, ci, geometry), worst, iterations=3, feedback=1)
            _check_image(gpu_ctx, c, ad1, nc1, u1, prev, (W, H, ci, geometry), worst, sigma_luminance=0.5, sigma_normal=4.0, sigma_depth=2.0)
    for N in (0, 2, 5):
        _check_image(gpu_ctx, c, ad1, nc1, u1, None, (W, H, "no history"), worst, iterations=N)
    _check_image(gpu_ctx, c, ad1, nc1, u1, prev, (W, H, "defaults"), worst)
    print("%d x %d: worst error of V_0 / the filtered frame / the fed-back history, relative to max(1, max |want|): %.3e" % (W, H, worst[0]))
    assert kinds == 7 or W * H < 100, kinds    # nothing reset (same camera), everything reset, and a mixture were all seen


@pytest.mark.parametrize("name,cam,W,H", [("cornell.xml", CORNELL_CAM, 64, 64), ("scene.xml", None, 96, 54), ("bunny20.xml", None, 96, 54)])
def test_svgf_image_real_guides_match_restatement(gpu_ctx, name, cam, W, H):
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
    worst = [0.0]
    hist, mv, _, _ = sr.svgf_image(c0, ad0, nc0, u0, iterations=0)
    _check_image(gpu_ctx, c0, ad0, nc0, u0, None, name, worst)
    prev = (hist, mv[..., :2], ad0, nc0, u0)
    for N in range(6):
        for fb in (0, 1):
            n_reset = _check_image(gpu_ctx, c1, ad1, nc1, u1, prev, name, worst, iterations=N, feedback=fb)
            assert 0 < n_reset < W * H, (name, n_reset)       # (the strip that came into view has no history)
    print("%s: worst relative error %.3e" % (name, worst[0]))


@pytest.mark.parametrize("source", ["sum", "frame"])
@pytest.mark.parametrize("feedback", [0, 1])
def test_accumulate_equals_the_unit_hook(gpu_ctx, source, feedback):
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    W, H, spp = 80, 48, 2
    ctx, sc, buf = _ctx_for("scene.xml", W, H)
    cam0 = ob.camera_reset()
    kw = dict(iterations=3, feedback=feedback)
    try:
        prev = None
        for f, pf in enumerate((0, 2, 2, 5, 7)):     # four cameras, the second one twice (the same-camera rule)
            u = ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=tr.path_camera(cam0, pf, (0.3, 0.0, 0.1), yaw_deg=0.4))
            u.frameCount = f
            ctx.set_uniforms(_cu(u))
            if source == "sum":
                ctx.clear_sum()
                ctx.render(sample_begin=f * spp, sample_count=spp, max_depth=8)
                info = ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=spp, **kw)
                c = ctx.read_sum() / F(spp)
            else:
                ctx.draw(max_depth=8, sample_begin=f)
                info = ctx.svgf_accumulate(source=capi.DENOISE_FRAME, **kw)
                c = ctx.read_frame()
            got, (hist, mv) = ctx.read_svgf(), ctx.read_svgf_state()
            ad, nc, _ = ctx.read_aovs()
            if prev is None:
                wh, wmv, wf, winfo = gpu_ctx.svgf_image(c, ad, nc, _cu(u), **kw)
            else:
                wh, wmv, wf, winfo = gpu_ctx.svgf_image(c, ad, nc, _cu(u), prev[0], prev[1], prev[2], prev[3], _cu(prev[4]), **kw)
            assert np.array_equal(_bits(got), _bits(wf)) and np.array_equal(_bits(hist), _bits(wh)) and np.array_equal(_bits(mv), _bits(wmv)), (source, f)
            assert info == winfo and info["pixels_reprojected"] + info["pixels_reset"] == W * H, (source, f, info, winfo)
            if f == 0:
                assert info["pixels_reset"] == W * H
            elif pf == 2 and f == 2:
                assert info["pixels_reset"] == 0
            else:
                assert info["pixels_reset"] < W * H // 4
            prev = (hist, mv[..., :2], ad, nc, u)
        ptr, nbytes = ctx.svgf_buffer()
        assert ptr and nbytes == W * H * 16
    finally:
        ctx.close()


def test_still_camera_state_is_the_running_mean():
    """K = 8 frames of 1 spp: n = 8 everywhere; X, M1 and M2 are the means of x, l and l^2 over the frames to 1e-6 — the bound of
    tests/test_svgf_cpu.py, in the convention of tests/test_gpu_denoise.py: relative to max(1, the largest x), and to its square for
    M2, a mean of squares; N = 0 returns X * a."""
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    W, H, K = 96, 54, 8
    ctx, sc, buf = _ctx_for("scene.xml", W, H)
    try:
        ctx.set_uniforms(_cu(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count)))
        ad, nc, _ = ctx.read_aovs()
        a = sr.albedo(ad, nc)
        for maxh in (8, 4):
            ctx.svgf_reset()
            xs = []
            for f in range(K):
                ctx.clear_sum()
                ctx.render(sample_begin=f, sample_count=1, max_depth=8)
                info = ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=1, max_history=maxh, iterations=0)
                assert info["pixels_reset"] == (W * H if f == 0 else 0)
                xs.append((ctx.read_sum()[..., :3] / a).astype(np.float64))
            hist, mv = ctx.read_svgf_state()
            assert (hist[..., 3] == min(K, maxh)).all(), maxh
            assert np.array_equal(_bits(ctx.read_svgf()[..., :3]), _bits(hist[..., :3] * a))
            if maxh >= K:
                ls = [0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2] for x in xs]
                scale = max(1.0, float(np.max(xs)))
                errs = (float(np.abs(hist[..., :3] - np.mean(xs, axis=0)).max()) / scale, float(np.abs(mv[..., 0] - np.mean(ls, axis=0)).max()) / scale,
                        float(np.abs(mv[..., 1] - np.mean(np.square(ls), axis=0)).max()) / (scale * scale))
                print("still camera: errors of X, M1, M2 relative to the largest value: %.2e %.2e %.2e" % errs)
                assert max(errs) <= 1e-6, errs
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(tr.PATHS))
def test_moving_camera_end_to_end(name):
    """The three calibration paths on the device: F >= 0.9 x the restatement's (the renders are bit-identical to the oracle's; the
    margin is for the ulps of exp / pow and for the guides, which may differ from the oracle's first hit in up to 0.1 % of the pixels)."""
    from metalpathtracer_amd import capi
    from test_svgf_cpu import HELD_F, MAX_RESET
    P = tr.PATHS[name]
    W, H = P["W"], P["H"]
    ctx, sc, buf = _ctx_for(name, W, H)
    try:
        for f, u in enumerate(tr.path_uniforms(name, sc)):
            ctx.set_uniforms(_cu(u))
            ctx.clear_sum()
            ctx.render(sample_begin=f, sample_count=1, max_depth=8, seed=(1, 0))
            info = ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=1)
        raw, out = ctx.read_sum(), ctx.read_svgf()
        ctx.clear_sum()
        ctx.render(sample_count=1024, max_depth=8, seed=(7, 0))
        hi = ctx.read_sum() / F(1024)
    finally:
        ctx.close()
    f_dev = tr.mse(raw, hi) / tr.mse(out, hi)
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
        for call in (ctx.read_svgf, ctx.svgf_buffer, ctx.read_svgf_state):
            with pytest.raises(capi.MptError) as e:
                call()
            assert e.value.status == 5, call     # MPT_ERR_NOT_READY: no state
        with pytest.raises(capi.MptError) as e:
            ctx.svgf_accumulate(source=capi.DENOISE_FRAME)
        assert e.value.status == 5                # no uniforms yet
        ctx.set_uniforms(u)

        def frame(f):
            ctx.clear_sum()
            ctx.render(sample_begin=f, sample_count=1, max_depth=8)
            return ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=1)["pixels_reset"]

        assert frame(0) == W * H and frame(1) == 0
        ctx.clear_sum()                           # mpt_clear_sum does not touch the state
        assert ctx.read_svgf()[..., 3].min() == 2 and frame(2) == 0
        nan = float("nan")
        for kw in (dict(source=capi.DENOISE_SUM, samples=0), dict(source=2, samples=1), dict(samples=1, depth_tolerance=nan),
                   dict(samples=1, min_weight=nan), dict(samples=1, sigma_luminance=nan), dict(samples=1, sigma_normal=nan),
                   dict(samples=1, sigma_depth=nan), dict(samples=1, iterations=capi.DENOISE_MAX_ITERATIONS + 1)):
            before = ctx.read_svgf(), ctx.read_svgf_state()
            with pytest.raises(capi.MptError) as e:
                ctx.svgf_accumulate(**kw)
            assert e.value.status == 1, kw
            after = ctx.read_svgf(), ctx.read_svgf_state()                         # refused with nothing changed
            assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[1][0]), _bits(before[1][0]))
            assert np.array_equal(_bits(after[1][1]), _bits(before[1][1]))
        drops = [("resize", lambda: ctx.resize(W, H)), ("upload_scene", lambda: ctx.upload_scene(*buf)),
                 ("build_and_upload", lambda: ctx.build_and_upload(buf[1], buf[2])), ("svgf_reset", ctx.svgf_reset)]
        for i, (what, drop) in enumerate(drops):
            assert frame(10 + 2 * i) == 0, what
            drop()
            for call in (ctx.read_svgf, ctx.read_svgf_state, ctx.svgf_buffer):
                with pytest.raises(capi.MptError) as e:
                    call()
                assert e.value.status == 5, what
            assert frame(11 + 2 * i) == W * H, what
        ctx.resize(W // 2, H // 2)                # another size: new buffers
        ctx.set_uniforms(_cu(ob.make_uniforms(W // 2, H // 2, sc.prim_count, sc.triangle_count)))
        assert frame(30) == (W // 2) * (H // 2) and frame(31) == 0
        assert ctx.read_svgf().shape == (H // 2, W // 2, 4)
    finally:
        ctx.close()


def test_no_side_effects_and_async():
    """The HDR sum, the frame target, mpt_stats, the mpt_temporal_* history and an mpt_denoise result are what they were, whichever
    of the stages ran last.  (A queued render that FAILS is reported through the same drain-then-wait path as mpt_denoise; it is not
    exercised here: only a HIP error or a ring overflow makes a queued render fail, and neither can be had harmlessly.)"""
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
        ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=4)
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        s0, f0, d0, t0, st0 = ctx.read_sum(), ctx.read_frame(), ctx.read_denoised(), ctx.read_temporal(), ctx.stats()
        ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=4, iterations=5)
        ctx.set_uniforms(_cu(u1))
        info = ctx.svgf_accumulate(source=capi.DENOISE_FRAME, iterations=5, feedback=1)
        assert 0 < info["pixels_reset"] < W * H
        assert np.array_equal(_bits(ctx.read_sum()), _bits(s0)) and np.array_equal(_bits(ctx.read_frame()), _bits(f0))
        assert np.array_equal(_bits(ctx.read_denoised()), _bits(d0)) and np.array_equal(_bits(ctx.read_temporal()), _bits(t0))
        assert ctx.stats() == st0
        # interleaved with the other two stages: neither disturbs this one's frame or state, nor the other way round
        before = ctx.read_svgf(), ctx.read_svgf_state()
        ctx.denoise(source=capi.DENOISE_FRAME, iterations=5)
        d1 = ctx.read_denoised()
        ctx.temporal_accumulate(source=capi.DENOISE_FRAME)
        ctx.denoise_temporal(iterations=4)
        d2, t2 = ctx.read_denoised(), ctx.read_temporal()
        after = ctx.read_svgf(), ctx.read_svgf_state()
        assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[1][0]), _bits(before[1][0]))
        assert np.array_equal(_bits(after[1][1]), _bits(before[1][1]))
        ctx.svgf_accumulate(source=capi.DENOISE_FRAME, iterations=5)
        assert np.array_equal(_bits(ctx.read_denoised()), _bits(d2)) and np.array_equal(_bits(ctx.read_temporal()), _bits(t2))
        assert not np.array_equal(_bits(d1), _bits(d2))
        # asynchronous renders, accumulated without an explicit wait: the same bits as with one
        ctx.svgf_reset()
        ctx.clear_sum()
        ctx.render_async(sample_count=2, max_depth=8)
        ctx.render_async(sample_begin=2, sample_count=2, max_depth=8)
        ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=4)
        a = ctx.read_svgf(), ctx.read_svgf_state()
        ctx.wait()
        ctx.svgf_reset()
        ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=4)
        b = ctx.read_svgf(), ctx.read_svgf_state()
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1][0]), _bits(b[1][0])) and np.array_equal(_bits(a[1][1]), _bits(b[1][1]))
        ad, nc, _ = ctx.read_aovs()
        assert np.array_equal(_bits(a[1][0][..., :3]), _bits((ctx.read_sum() / F(4))[..., :3] / sr.albedo(ad, nc)))
    finally:
        ctx.close()


CAMERA_PATH = "2\n3 d mouse 4 0\n2 w\n"


@pytest.mark.parametrize("iterations", [None, 4])
def test_cli_svgf_matches_the_python_host_layer(tmp_path, iterations):
    from metalpathtracer_amd import capi, host
    exe = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
    path = tmp_path / "path.txt"
    path.write_text(CAMERA_PATH)
    out_dir = tmp_path / "runs"
    W, H, spp = 96, 54, 2
    r = subprocess.run([exe, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--depth", "8", "--seed", "1",
                        "--bvh", "reference", "--camera-path", str(path), "--out-dir", str(out_dir), "--svgf", "--temporal-spp", str(spp),
                        "--temporal-history", "16"] + (["--svgf-iterations", str(iterations)] if iterations is not None else []),
                       capture_output=True, text=True, timeout=300)
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
            info = rr.drawSvgf(spp, max_history=16, iterations=-1 if iterations is None else iterations)
            assert info == dict(pixels_reprojected=frames[f]["reprojected"], pixels_reset=frames[f]["reset"]), f
            want = str(tmp_path / "want.ppm")
            assert host.write_ppm(want, rr.readSvgf()) == 0
            assert open(want, "rb").read() == open(out_dir / ("frame_%04d.ppm" % f), "rb").read(), f
        assert rr.readSvgf()[..., 3].max() <= 7 + 1e-5     # (seven frames; the bilinear mean of the lengths rounds a few ulps)
    finally:
        rr.close()
