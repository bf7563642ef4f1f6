"""GPU tests of mpt_render_nee_adaptive (include/mpt.h).  The reference is code that was there before the call: the per-sample values
v_s of every pixel from single-sample mpt_render_nee calls on a cleared sum (0 + v is exact), joined in numpy float32 in sample order
into running sums and running moments (tests/nee_adaptive_ref.py), and the stopping rule of tests/adaptive_ref.py over them.  Every
tile must hold the running sum and the running moments at its own count bit for bit, the counts must be the rule's, and the limits,
the determinism, the state the call leaves alone, the refusals and the CLI / host layer are checked against the C ABI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import display_ref as dr
import nee_adaptive_ref as nar
import nee_cases as ncs
import nee_ref
from conftest import ROOT, host_scene, scene_path

pytestmark = pytest.mark.gpu

SEED = ncs.SEED
INVALID, NOT_READY = 1, 5
EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
DEPTH, B, N, MIN, BATCH = 4, 5, 16, 4, 4
SCHED = ar.schedule(N, MIN, BATCH)
AREA, CONE = 0, 1
REF, OWN = 0, 1
LAMBERT, SCATTER = 0, 1

_values = {}   # case -> the per-sample values [N, H, W, 4] of samples [B, B + N), computed once and never modified


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def put(ctx, name, W, H, sampling=AREA):
    _, buf = ncs.scene_of(name)
    ctx.upload_scene(*buf)
    u = ncs.uniforms_of(name, W, H)
    ctx.resize(W, H)
    ctx.set_uniforms(u)
    ctx.set_light_sampling(sampling)
    return u


def kw_of(walk, bsdf, **more):
    from metalpathtracer_amd import capi
    return dict(walk=walk, clamp=0.0, rng_mode=capi.RNG_PHILOX, bsdf_mode=bsdf, max_depth=DEPTH, seed=SEED, **more)


def reference(ctx, case):
    """(running sums, running moments) [N + 1, H, W, 4] of the case; the context holds the case's scene, size and sampling afterwards."""
    name, W, H, walk, sampling, bsdf = case
    put(ctx, name, W, H, sampling)
    if case not in _values:
        vs = []
        for s in range(B, B + N):
            ctx.clear_sum()
            ctx.render_nee(sample_begin=s, sample_count=1, **kw_of(walk, bsdf))
            vs.append(ctx.read_sum())
        v = np.stack(vs)
        v.setflags(write=False)
        _values[case] = v
    return nar.running(_values[case])


def threshold_for(sums, moms):
    """_threshold_for of tests/test_gpu_adaptive.py over the reference: the 0.3 quantile of the tile errors at n_0."""
    return float(np.float32(np.quantile(ar.tile_errors(sums[MIN], moms[MIN], MIN), 0.3)))


def adaptive(ctx, case, thr, **more):
    name, W, H, walk, sampling, bsdf = case
    kw = dict(min_samples=MIN, batch_samples=BATCH, sample_begin=B, sample_count=N)
    kw.update(more)
    return ctx.render_nee_adaptive(thr, **kw_of(walk, bsdf, **kw))


CORNELL = [("cornell.xml", W, H, walk, sampling, LAMBERT) for (W, H) in ((40, 24), (37, 21)) for walk in (REF, OWN) for sampling in (AREA, CONE)]
SPECULAR = [("specular", 37, 21, walk, AREA, bsdf) for walk in (REF, OWN) for bsdf in (LAMBERT, SCATTER)]
SPHERE_LIGHT = [("manylights", 37, 21, REF, CONE, LAMBERT)]   # (beyond the issue's cases: a sphere light, which the cone changes)


@pytest.mark.parametrize("case", CORNELL + SPECULAR + SPHERE_LIGHT, ids=lambda c: "-".join(str(x) for x in c))
def test_every_tile_holds_the_running_sum_and_moments_at_its_count(gpu_ctx, case):
    from metalpathtracer_amd import capi
    name, W, H = case[:3]
    sums, moms = reference(gpu_ctx, case)
    thr = threshold_for(sums, moms)
    out = adaptive(gpu_ctx, case, thr)
    counts, got_s, got_m = gpu_ctx.read_tile_samples(), gpu_ctx.read_sum(), gpu_ctx.read_moments()
    per_px = capi.expand_tile_counts(counts, H, W)
    want_s, want_m = nar.at_counts(sums, per_px), nar.at_counts(moms, per_px)
    print(case, "threshold", thr, "counts", dict(zip(*np.unique(counts, return_counts=True))), "pixels that differ: sum",
          int((bits(got_s) != bits(want_s)).any(-1).sum()), "moments", int((bits(got_m) != bits(want_m)).any(-1).sum()), out)
    assert np.isin(counts, SCHED).all()
    same(got_s, want_s)
    same(got_m, want_m)
    assert want_m[..., 3].any()
    assert len(np.unique(counts)) >= 3, np.unique(counts)
    a = out["adaptive"]
    assert a["samples"] == int(per_px.astype(np.int64).sum()) == out["nee"]["paths"]
    assert a["tiles_at_max"] == int((counts == N).sum()) and a["tiles_converged"] == int((counts != N).sum())
    assert a["passes"] == max(nar.steps_taken(int(c), MIN, BATCH) for c in counts.ravel())


@pytest.mark.parametrize("case", [c for c in CORNELL if c[3] == REF and c[4] == AREA], ids=lambda c: "%dx%d" % c[1:3])
def test_the_counts_are_the_stopping_rules(gpu_ctx, case):
    sums, moms = reference(gpu_ctx, case)
    errs = nar.schedule_errors(sums, moms, SCHED)
    thr = threshold_for(sums, moms)
    want = ar.stop_counts(errs, SCHED, np.float64(np.float32(thr)), N)
    near = np.zeros(want.shape, bool)
    for e, n in zip(errs, SCHED):
        near |= (np.abs(e - thr) <= 1e-6 * thr) & (n <= want)
    ok = ~near
    assert ok.mean() > 0.9                                 # (of the reference alone: the inputs are fit for the comparison)
    adaptive(gpu_ctx, case, thr)
    counts = gpu_ctx.read_tile_samples()
    print(case, "threshold", thr, "near", int(near.sum()), "of", near.size, "tiles that differ", int((counts != want)[ok].sum()))
    assert np.array_equal(counts[ok], want[ok])
    assert len(np.unique(counts)) >= 3, np.unique(counts)


def test_limits(gpu_ctx):
    case = ("cornell.xml", 37, 21, REF, AREA, LAMBERT)
    name, W, H, walk, sampling, bsdf = case
    put(gpu_ctx, name, W, H, sampling)
    tiles = 5 * 3
    gpu_ctx.reset_stats()
    out = adaptive(gpu_ctx, case, 0.0)
    a, st = out["adaptive"], gpu_ctx.stats()
    got = gpu_ctx.read_sum()
    assert (gpu_ctx.read_tile_samples() == N).all()
    assert a["tiles_at_max"] == tiles and a["tiles_converged"] == 0 and a["passes"] == len(SCHED)
    assert a["samples"] == W * H * N == out["nee"]["paths"] == st["paths"]
    assert st["rays"] == out["nee"]["rays"] and st["trace_launches"] == 1 and st["trace_kernel_ms"] > 0
    assert out["nee"]["device_ms"] > 0 and out["nee"]["shadow_rays"] > 0
    gpu_ctx.clear_sum()
    plain = gpu_ctx.render_nee(sample_begin=B, sample_count=N, **kw_of(walk, bsdf))
    same(got, gpu_ctx.read_sum())
    for k in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights"):
        assert out["nee"][k] == plain[k], k
    # a threshold nothing misses: every tile stops at n_0, one step; N below min_samples: one step at N
    out = adaptive(gpu_ctx, case, 1e30)
    assert (gpu_ctx.read_tile_samples() == MIN).all()
    assert out["adaptive"] == dict(out["adaptive"], passes=1, tiles_converged=tiles, tiles_at_max=0, samples=W * H * MIN)
    out = adaptive(gpu_ctx, case, 1e30, sample_count=3)
    assert (gpu_ctx.read_tile_samples() == 3).all() and out["adaptive"]["passes"] == 1 and out["adaptive"]["tiles_at_max"] == tiles
    # the defaults of mpt_adaptive_params (16, 16) and a batch that would overflow 32 bits
    out = adaptive(gpu_ctx, case, 0.0, min_samples=0, batch_samples=0, sample_count=40)
    assert (gpu_ctx.read_tile_samples() == 40).all() and out["adaptive"]["passes"] == 3
    out = adaptive(gpu_ctx, case, 0.0, min_samples=2, batch_samples=0xFFFFFFFF, sample_count=9)
    assert (gpu_ctx.read_tile_samples() == 9).all() and out["adaptive"]["passes"] == 2


def test_two_calls_give_the_same(gpu_ctx):
    case = ("specular", 37, 21, OWN, AREA, SCATTER)
    sums, moms = reference(gpu_ctx, case)
    thr = threshold_for(sums, moms)
    runs = []
    for _ in range(2):
        out = adaptive(gpu_ctx, case, thr)
        out["nee"].pop("device_ms")
        runs.append((out, gpu_ctx.read_tile_samples(), gpu_ctx.read_sum(), gpu_ctx.read_moments()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1])
    same(runs[0][2], runs[1][2])
    same(runs[0][3], runs[1][3])


def test_the_call_leaves_the_other_state_alone(gpu_ctx):
    from metalpathtracer_amd import capi
    case = ("cornell.xml", 40, 24, REF, AREA, LAMBERT)
    name, W, H, walk, sampling, bsdf = case
    sums, moms = reference(gpu_ctx, case)
    thr = threshold_for(sums, moms)
    gpu_ctx.clear_sum()
    gpu_ctx.reset_stats()
    gpu_ctx.draw(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(1, 0))
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(1, 0))
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.display(source=capi.DISPLAY_SUM, samples=2)
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    read = lambda: (gpu_ctx.read_frame(), gpu_ctx.read_denoised(), gpu_ctx.read_temporal(), gpu_ctx.read_svgf(), gpu_ctx.read_display(),
                    gpu_ctx.read_ao()[0], gpu_ctx.read_ao()[1], gpu_ctx.read_direct()[0], gpu_ctx.read_direct()[1])
    before, st0 = read(), gpu_ctx.stats()
    gpu_ctx.render_async(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_begin=2, sample_count=2, seed=(1, 0))    # the call waits for it
    out = adaptive(gpu_ctx, case, thr)
    st1 = gpu_ctx.stats()
    for a, b in zip(before, read()):
        np.testing.assert_array_equal(a, b)
    assert st1["paths"] == st0["paths"] + 2 * W * H + out["nee"]["paths"] and st1["trace_launches"] == 1
    counts = gpu_ctx.read_tile_samples()
    per_px = capi.expand_tile_counts(counts, H, W)
    total = gpu_ctx.read_sum()
    same(total, nar.at_counts(sums, per_px))               # (the queued render's samples were cleared away with the rest)
    # MPT_DISPLAY_ADAPTIVE reads the same buffers
    kw = dict(tone=1, transfer=0, auto_exposure=True)
    gpu_ctx.display_reset()
    info = gpu_ctx.display(source=capi.DISPLAY_ADAPTIVE, **kw)
    want = dr.display(dr.source_adaptive(total, per_px), **kw)
    assert np.array_equal(gpu_ctx.read_display(), want[0]) and np.array_equal(gpu_ctx.read_display_histogram(), want[1])
    assert dr.same_info(info, want[2])
    same(gpu_ctx.read_adaptive_mean()[..., :3], dr.source_adaptive(total, per_px))
    # the caller's sum buffer is honoured: cleared, written, and the internal one left alone
    other = capi.Context(0)
    try:
        other.resize(W, H)
        ptr, _ = other.sum_buffer()
        other.write_sum(np.full((H, W, 4), 7.0, np.float32))
        gpu_ctx.set_sum_buffer(ptr)
        try:
            adaptive(gpu_ctx, case, thr)
            assert np.array_equal(gpu_ctx.read_tile_samples(), counts)
        finally:
            gpu_ctx.set_sum_buffer(None)
        same(other.read_sum(), total)
        same(gpu_ctx.read_sum(), total)                    # (what the call before left there)
    finally:
        other.close()
    # mpt_render_adaptive and mpt_render_nee afterwards, each held to its own exactness once
    plain_kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, seed=SEED)
    gpu_ctx.render_adaptive(0.3, min_samples=2, batch_samples=2, sample_begin=1, sample_count=6, **plain_kw)
    c2, got = capi.expand_tile_counts(gpu_ctx.read_tile_samples(), H, W), gpu_ctx.read_sum()
    for n in np.unique(c2):
        gpu_ctx.clear_sum()
        gpu_ctx.render(sample_begin=1, sample_count=int(n), **plain_kw)
        same(got[c2 == n], gpu_ctx.read_sum()[c2 == n])
    r = ncs.reference("cornell.xml", DEPTH)                 # (the case at its own size, samples [0, 3), as tests/test_gpu_nee.py)
    _, w, h = ncs.CASES["cornell.xml"][:3]
    put(gpu_ctx, "cornell.xml", w, h)
    gpu_ctx.clear_sum()
    gpu_ctx.render_nee(sample_count=ncs.SPP_MAX, **kw_of(REF, LAMBERT))
    same(gpu_ctx.read_sum(), nee_ref.accumulate(r["value"]))


def test_refusals_leave_everything_as_it_was(gpu_ctx):
    from metalpathtracer_amd import capi
    case = ("cornell.xml", 40, 24, REF, AREA, LAMBERT)
    name, W, H = case[:3]
    put(gpu_ctx, name, W, H)
    adaptive(gpu_ctx, case, 0.2)
    want = (gpu_ctx.read_sum(), gpu_ctx.read_moments(), gpu_ctx.read_tile_samples())
    assert all(w.any() for w in want)
    st = gpu_ctx.stats()
    L, h = gpu_ctx.L, gpu_ctx.h
    base = dict(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=8, seed=SEED)
    good_p, good_n, good_a = gpu_ctx.params(**base), capi.NeeParams(capi.WALK_AUTO, 0.0), capi.AdaptiveParams(4, 4, 0.1, 0.0)

    def call(p=good_p, n=good_n, a=good_a):
        ref = lambda x: None if x is None else C.byref(x)
        return L.mpt_render_nee_adaptive(h, ref(p), ref(n), ref(a), None, None)

    assert call(p=None) == INVALID and call(n=None) == INVALID and call(a=None) == INVALID
    bad_params = (dict(rng_mode=capi.RNG_LITERAL), dict(bsdf_mode=capi.BSDF_SCATTER_ALL), dict(shard_count=2), dict(shard_count=2, shard_rank=1),
                  dict(flags=capi.FLAG_MOMENTS), dict(flags=capi.FLAG_COUNT_WORK), dict(max_depth=0), dict(max_depth=-1), dict(max_depth=33),
                  dict(sample_begin=(1 << 27) - 4, sample_count=8), dict(sample_count=1), dict(sample_count=0))
    for kw in bad_params:
        assert call(p=gpu_ctx.params(**{**base, **kw})) == INVALID, kw
    for walk, clamp in ((3, 0.0), (-1, 0.0), (capi.WALK_AUTO, float("nan"))):
        assert call(n=capi.NeeParams(walk, clamp)) == INVALID, (walk, clamp)
    for a in (capi.AdaptiveParams(1, 4, 0.1, 0.0), capi.AdaptiveParams(4, 4, -0.5, 0.0), capi.AdaptiveParams(4, 4, float("nan"), 0.0)):
        assert call(a=a) == INVALID, (a.min_samples, a.threshold)
    for got, w in zip((gpu_ctx.read_sum(), gpu_ctx.read_moments(), gpu_ctx.read_tile_samples()), want):
        same(got, w)
    assert gpu_ctx.stats() == st
    assert call() == 0                                      # both infos may be NULL
    assert (gpu_ctx.read_tile_samples() >= 4).all()
    # before scene, uniforms and size
    _, buf = ncs.scene_of(name)
    u = ncs.uniforms_of(name, W, H)
    fresh = capi.Context(0)
    try:
        f = lambda: fresh.L.mpt_render_nee_adaptive(fresh.h, C.byref(good_p), C.byref(good_n), C.byref(good_a), None, None)
        assert f() == NOT_READY
        fresh.upload_scene(*buf)
        assert f() == NOT_READY
        fresh.resize(W, H)
        assert f() == NOT_READY
        assert not fresh.read_sum().any() and not fresh.read_tile_samples().any()
        fresh.set_uniforms(u)
        assert f() == 0
        same(fresh.read_sum(), gpu_ctx.read_sum())
    finally:
        fresh.close()


def _read_pfm(path, W, H):
    hdr = ("PF\n%d %d\n-1.0\n" % (W, H)).encode()
    raw = open(path, "rb").read()
    assert raw.startswith(hdr)
    return np.frombuffer(raw[len(hdr):], np.float32).reshape(H, W, 3)[::-1]


def test_cli_and_host_layer_match_capi(tmp_path):
    from metalpathtracer_amd import capi, host
    W, H, spp, thr = 96, 54, 24, 0.1
    base = [EXE, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", "4", "--seed", "1",
            "--bvh", "reference"]
    args = base + ["--nee-adaptive", str(thr), "--adaptive-min", "4", "--adaptive-batch", "4", "--nee-walk", "reference", "--light-sampling", "cone"]
    r = subprocess.run(args + ["--out", str(tmp_path / "a.pfm")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    cli_img = _read_pfm(tmp_path / "a.pfm", W, H)

    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(1, 0))
        rr.setLightSampling(capi.LIGHT_SAMPLING_CONE)
        hout = rr.renderNeeAdaptive(spp, 4, thr, min_samples=4, batch_samples=4, walk=capi.WALK_REFERENCE)
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
        ctx.set_light_sampling(capi.LIGHT_SAMPLING_CONE)
        out = ctx.render_nee_adaptive(thr, min_samples=4, batch_samples=4, walk=capi.WALK_REFERENCE, sample_count=spp, max_depth=4, seed=(1, 0))
        mean, counts = ctx.read_adaptive_mean(), ctx.read_tile_samples()
    finally:
        ctx.close()
    for o in (out, hout):
        o["nee"].pop("device_ms")
    assert hout == out and np.array_equal(hcounts, counts) and len(np.unique(counts)) >= 2
    same(hmean, mean)
    same(cli_img, mean[..., :3])
    a, n = line["adaptive"], line["nee"]
    assert {k: a[k] for k in ("passes", "samples", "tiles_converged", "tiles_at_max")} == {k: out["adaptive"][k] for k in
                                                                                           ("passes", "samples", "tiles_converged", "tiles_at_max")}
    assert abs(a["mean_spp"] - out["adaptive"]["samples"] / (W * H)) < 1e-3
    assert {k: n[k] for k in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights")} == {k: out["nee"][k] for k in
                                                                                                   ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights")}
    assert n["light_sampling"] == "cone" and line["paths"] == out["adaptive"]["samples"]
    # --denoise and the display flags run over the adaptive mean
    r = subprocess.run(args + ["--denoise", "--tonemap", "reinhard", "--out", str(tmp_path / "d.ppm")], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.getsize(tmp_path / "d.ppm") > W * H * 3, r.stderr
    # every refused combination: exit code 2, and the message names the flag
    path = tmp_path / "path.txt"
    path.write_text("0 0 1 3.4 0 0 -1\n")
    for extra in (["--nee"], ["--adaptive", "0.05"], ["--gpus", "2"], ["--camera-path", str(path)], ["--frames", "2"],
                  ["--checkpoint", str(tmp_path / "c.sum")], ["--resume", str(tmp_path / "c.sum")], ["--ao", "4"], ["--direct", "4"],
                  ["--rng", "literal"]):
        r = subprocess.run(base + ["--nee-adaptive", "0.1", "--out", str(tmp_path / "x.pfm")] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--nee-adaptive" in r.stderr, (extra, r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "x.pfm")
    r = subprocess.run(base + ["--nee", "--adaptive", "0.05", "--out", str(tmp_path / "x.pfm")], capture_output=True, text=True)
    assert r.returncode == 2 and "--nee-adaptive" not in r.stderr and "--nee" in r.stderr, r.stderr
