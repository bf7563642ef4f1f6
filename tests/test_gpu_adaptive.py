"""Adaptive sampling on the MI355X (philox): the moments against single-sample renders, every tile of an adaptive render against a
plain mpt_render of the same sample range (bit for bit), the stopping rule against the numpy restatement (tests/adaptive_ref.py),
the limits, the refused arguments, and the CLI / host layer against the C ABI."""
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
from conftest import CORNELL_CAM, ROOT, host_scene, oracle_scene, scene_path

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def _ctx(name, W, H, cam=None, device_tree=False):
    from metalpathtracer_amd import capi, host
    ctx = capi.Context(0)
    if device_tree:
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(scene_path(name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        u = host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)
    else:
        from oracle import binding as ob
        sc, buf = oracle_scene(name)
        ctx.upload_scene(*buf)
        u = capi.Uniforms.from_buffer_copy(bytes(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=cam)))
    ctx.resize(W, H)
    ctx.set_uniforms(u)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _plain(ctx, begin, count, **kw):
    ctx.clear_sum()
    ctx.render(sample_begin=begin, sample_count=count, **kw)
    return ctx.read_sum()


def _check_tiles_exact(ctx, counts, got, begin, min_distinct=3, **kw):
    """Every tile holding n samples equals, bit for bit, a plain render of [begin, begin + n)."""
    from metalpathtracer_amd import capi
    per_px = capi.expand_tile_counts(counts, ctx.height, ctx.width)
    distinct = np.unique(counts)
    assert len(distinct) >= min_distinct, distinct
    for n in distinct:
        ref = _plain(ctx, begin, int(n), **kw)
        m = per_px == n
        assert np.array_equal(_bits(got[m]), _bits(ref[m])), "tiles at %d samples differ from a plain render" % n
    return distinct


def _threshold_for(ctx, begin, n0, quantile, **kw):
    """A threshold that stops part of the tiles at n0 (the quantile of their errors there), so that the counts spread."""
    from metalpathtracer_amd import capi
    ctx.clear_sum()
    ctx.render(sample_begin=begin, sample_count=n0, flags=capi.FLAG_MOMENTS, **kw)
    e = ar.tile_errors(ctx.read_sum(), ctx.read_moments(), n0)
    return float(np.float32(np.quantile(e, quantile)))


def test_moments_against_single_sample_renders():
    from metalpathtracer_amd import capi
    ctx = _ctx("cornell.xml", 64, 64, CORNELL_CAM)
    kw = dict(max_depth=8)
    try:
        vs = np.stack([_plain(ctx, s, 1, **kw) for s in range(8)])   # 0 + v is exact: the per-sample values
        ctx.clear_sum()
        ctx.render(sample_count=8, flags=capi.FLAG_MOMENTS, **kw)
        s_m, m2 = ctx.read_sum(), ctx.read_moments()
        want = np.empty_like(m2)
        want[..., :3] = (vs[..., :3].astype(np.float64) ** 2).sum(0)
        want[..., 3] = (ar.lum32(vs).astype(np.float64) ** 2).sum(0)
        assert (want > 0).any()
        np.testing.assert_allclose(m2, want, rtol=1e-5, atol=1e-30)
        # a render without the flag leaves the moments as they are; mpt_clear_sum zeroes them
        ctx.render(sample_begin=8, sample_count=2, **kw)
        assert np.array_equal(_bits(ctx.read_moments()), _bits(m2))
        ctx.clear_sum()
        assert not ctx.read_moments().any()
        # the sum is bit-identical with and without the flag: mpt_render, and two overlapped mpt_render_async
        s_p = _plain(ctx, 0, 8, **kw)
        assert np.array_equal(_bits(s_p), _bits(s_m))
        ctx.clear_sum()
        ctx.render_async(sample_begin=0, sample_count=4, flags=capi.FLAG_MOMENTS, **kw)
        ctx.render_async(sample_begin=4, sample_count=4, flags=capi.FLAG_MOMENTS, **kw)
        ctx.wait()
        assert np.array_equal(_bits(ctx.read_sum()), _bits(s_m))
        np.testing.assert_allclose(ctx.read_moments(), m2, rtol=1e-6, atol=1e-30)
    finally:
        ctx.close()


def test_moments_zero_before_use_and_not_ready_before_resize():
    from metalpathtracer_amd import capi
    ctx = capi.Context(0)
    try:
        with pytest.raises(capi.MptError) as e:
            ctx.read_moments()
        assert e.value.status == 5
        with pytest.raises(capi.MptError) as e:
            ctx.read_tile_samples()
        assert e.value.status == 5
        ctx.resize(20, 12)
        assert not ctx.read_moments().any() and ctx.read_moments().shape == (12, 20, 4)
        assert not ctx.read_tile_samples().any() and ctx.read_tile_samples().shape == (2, 3)
    finally:
        ctx.close()


@pytest.mark.parametrize("pipe", [0, 1, 2, 3, 4])
def test_tiles_exact_cornell_partial_edges(pipe):
    ctx = _ctx("cornell.xml", 250, 186, CORNELL_CAM)
    kw = dict(max_depth=8, pipeline=pipe)
    b = 5
    try:
        thr = _threshold_for(ctx, b, 4, 0.3, **kw)
        info = ctx.render_adaptive(thr, min_samples=4, batch_samples=4, sample_begin=b, sample_count=24, **kw)
        counts, got = ctx.read_tile_samples(), ctx.read_sum()
        assert info["passes"] >= 3
        _check_tiles_exact(ctx, counts, got, b, **kw)
    finally:
        ctx.close()


@pytest.mark.parametrize("bsdf", [1, 2])
def test_tiles_exact_scatter_modes(bsdf):
    ctx = _ctx("glass.xml", 96, 64)
    kw = dict(max_depth=8, bsdf_mode=bsdf)
    try:
        thr = _threshold_for(ctx, 2, 4, 0.3, **kw)
        ctx.render_adaptive(thr, min_samples=4, batch_samples=4, sample_begin=2, sample_count=24, **kw)
        _check_tiles_exact(ctx, ctx.read_tile_samples(), ctx.read_sum(), 2, min_distinct=2, **kw)
    finally:
        ctx.close()


def test_tiles_exact_device_built_bunny_ordered():
    from metalpathtracer_amd import capi
    ctx = _ctx("bunny20.xml", 480, 272, device_tree=True)
    kw = dict(max_depth=8, pipeline=capi.PIPE_ORDERED)
    try:
        assert ctx.accel_info()["ordered_ok"] == 1
        thr = _threshold_for(ctx, 7, 8, 0.3, **kw)
        ctx.render_adaptive(thr, min_samples=8, batch_samples=8, sample_begin=7, sample_count=40, **kw)
        _check_tiles_exact(ctx, ctx.read_tile_samples(), ctx.read_sum(), 7, **kw)
    finally:
        ctx.close()


def test_stopping_rule_matches_restatement():
    from metalpathtracer_amd import capi
    ctx = _ctx("cornell.xml", 250, 186, CORNELL_CAM)
    kw = dict(max_depth=8)
    b, N, m, bt = 3, 30, 4, 6
    try:
        sched = ar.schedule(N, m, bt)
        errs = []
        for n in sched:
            ctx.clear_sum()
            ctx.render(sample_begin=b, sample_count=n, flags=capi.FLAG_MOMENTS, **kw)
            errs.append(ar.tile_errors(ctx.read_sum(), ctx.read_moments(), n))
        thr = float(np.float32(np.quantile(errs[0], 0.3)))
        ctx.render_adaptive(thr, min_samples=m, batch_samples=bt, sample_begin=b, sample_count=N, **kw)
        counts = ctx.read_tile_samples()
    finally:
        ctx.close()
    want = ar.stop_counts(errs, sched, np.float64(np.float32(thr)), N)
    near = np.zeros(counts.shape, bool)
    for e, n in zip(errs, sched):
        near |= (np.abs(e - thr) <= 1e-6 * thr) & (n <= want)
    ok = ~near
    assert ok.mean() > 0.9
    assert np.array_equal(counts[ok], want[ok])
    assert len(np.unique(counts)) >= 3


def test_limits_stats_and_determinism():
    from metalpathtracer_amd import capi
    ctx = _ctx("cornell.xml", 100, 60, CORNELL_CAM)
    kw = dict(max_depth=8)
    tiles = 13 * 8
    try:
        info = ctx.render_adaptive(0.0, min_samples=4, batch_samples=5, sample_begin=2, sample_count=16, **kw)
        assert info["tiles_at_max"] == tiles and info["tiles_converged"] == 0
        assert info["passes"] == len(ar.schedule(16, 4, 5))
        assert (ctx.read_tile_samples() == 16).all()
        got = ctx.read_sum()
        assert np.array_equal(_bits(got), _bits(_plain(ctx, 2, 16, **kw)))
        info = ctx.render_adaptive(1e30, min_samples=6, sample_count=64, **kw)
        assert info["passes"] == 1 and info["tiles_converged"] == tiles and info["tiles_at_max"] == 0
        assert (ctx.read_tile_samples() == 6).all()
        assert info["samples"] == 100 * 60 * 6
        runs = []
        for _ in range(2):
            ctx.reset_stats()
            info = ctx.render_adaptive(0.08, min_samples=4, batch_samples=4, sample_count=32, **kw)
            st = ctx.stats()
            counts = ctx.read_tile_samples()
            per_px = capi.expand_tile_counts(counts, 60, 100)
            assert st["paths"] == info["samples"] == int(per_px.astype(np.int64).sum())
            assert st["trace_launches"] >= info["passes"]
            assert info["tiles_converged"] + info["tiles_at_max"] == tiles
            assert info["tiles_at_max"] == int((counts == 32).sum())
            runs.append((info, counts, ctx.read_sum(), ctx.read_moments()))
        assert runs[0][0] == runs[1][0]
        assert np.array_equal(runs[0][1], runs[1][1])
        assert np.array_equal(_bits(runs[0][2]), _bits(runs[1][2])) and np.array_equal(_bits(runs[0][3]), _bits(runs[1][3]))
    finally:
        ctx.close()


def test_headline_size_scene_exact_per_tile():
    ctx = _ctx("scene.xml", 1920, 1080)
    kw = dict(max_depth=32)
    try:
        info = ctx.render_adaptive(0.05, sample_begin=11, sample_count=256, **kw)
        counts, got = ctx.read_tile_samples(), ctx.read_sum()
        print("scene.xml 1080p: %s, mean spp %.1f" % (info, info["samples"] / (1920 * 1080)))
        assert info["tiles_converged"] > 0
        _check_tiles_exact(ctx, counts, got, 11, **kw)
    finally:
        ctx.close()


def test_refused_arguments_and_not_ready():
    from metalpathtracer_amd import capi
    ctx = capi.Context(0)
    try:
        with pytest.raises(capi.MptError) as e:   # no scene, uniforms or size
            ctx.render_adaptive(0.1, sample_count=8)
        assert e.value.status == 5
    finally:
        ctx.close()
    ctx = _ctx("cornell.xml", 40, 24, CORNELL_CAM)
    try:
        bad = [dict(rng_mode=capi.RNG_LITERAL), dict(shard_count=2), dict(shard_count=2, shard_rank=1), dict(min_samples=1),
               dict(threshold=-0.5), dict(threshold=float("nan")), dict(sample_count=1), dict(sample_count=0)]
        for b in bad:
            kw = dict(threshold=0.1, sample_count=8, max_depth=4)
            kw.update(b)
            with pytest.raises(capi.MptError) as e:
                ctx.render_adaptive(**kw)
            assert e.value.status == 1, b
        assert not ctx.read_sum().any()   # nothing rendered
        info = ctx.render_adaptive(0.1, sample_count=8, max_depth=4)
        assert info["passes"] == 1 and info["samples"] == 40 * 24 * 8
    finally:
        ctx.close()


def _read_pfm(path, W, H):
    hdr = ("PF\n%d %d\n-1.0\n" % (W, H)).encode()
    raw = open(path, "rb").read()
    assert raw.startswith(hdr)
    return np.frombuffer(raw[len(hdr):], np.float32).reshape(H, W, 3)[::-1]


def test_cli_and_host_layer_match_capi(tmp_path):
    from metalpathtracer_amd import capi, host
    W, H, spp, thr = 96, 54, 32, 0.1
    args = [CLI, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", "8",
            "--seed", "1", "--bvh", "reference", "--adaptive", str(thr), "--adaptive-min", "4", "--adaptive-batch", "4"]
    r = subprocess.run(args + ["--out", str(tmp_path / "a.pfm")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    cli_img = _read_pfm(tmp_path / "a.pfm", W, H)
    r = subprocess.run(args + ["--denoise", "--out", str(tmp_path / "d.pfm")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cli_dn = _read_pfm(tmp_path / "d.pfm", W, H)

    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        hinfo = rr.renderAdaptive(0, spp, thr, min_samples=4, batch_samples=4)
        hcounts = rr.readTileSamples()
        hmean = rr.readSum() / capi.expand_tile_counts(hcounts, H, W).astype(np.float32)[..., None]
        u = rr.uniforms()
    finally:
        rr.close()
    _, buf = host_scene("scene.xml")
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(*buf)
        ctx.resize(W, H)
        ctx.set_uniforms(u)
        info = ctx.render_adaptive(thr, min_samples=4, batch_samples=4, sample_count=spp, max_depth=8, seed=(1, 0))
        mean = ctx.read_adaptive_mean()
        counts = ctx.read_tile_samples()
        ad, nc, _ = ctx.read_aovs()
        want_dn = ctx.denoise_image(mean, ad, nc)
    finally:
        ctx.close()
    assert hinfo == info and np.array_equal(hcounts, counts)
    assert np.array_equal(_bits(hmean), _bits(mean))
    assert np.array_equal(_bits(cli_img), _bits(mean[..., :3]))
    assert np.array_equal(_bits(cli_dn), _bits(want_dn[..., :3]))
    a = line["adaptive"]
    assert (a["passes"], a["samples"], a["tiles_converged"], a["tiles_at_max"]) == (
        info["passes"], info["samples"], info["tiles_converged"], info["tiles_at_max"])
    assert abs(a["mean_spp"] - info["samples"] / (W * H)) < 1e-3
    assert line["paths"] == info["samples"]
