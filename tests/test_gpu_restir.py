"""GPU tests of mpt_direct_restir (include/mpt.h: spatial reservoir reuse in the direct pass) against tests/restir_ref.py: the image, the
counts, the info totals and both reservoir read-backs are compared bit for bit.  Occlusion is tests/anyhit_ref.py's `lower` — what
MPT_WALK_REFERENCE must answer — and MPT_WALK_OWN is held to the same on every pixel that is not tainted (tests/test_restir_cpu.py caps
those at 10 % of each case's pixels; measured, none of the cases has one).  Then the small sizes, K = 0 against mpt_direct_lighting,
identities that need no reference, the state and its life, the refusals, the expectation on the device and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import restir_cases as rsc
import restir_ref
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

SEED = rsc.SEED
INVALID, NOT_READY = 1, 5
EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
INFO_KEYS = ("pixels_surface", "rays_initial", "rays_final", "rays_correction", "rays_occluded", "neighbours_accepted", "samples_from_neighbours",
             "lights")


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(autouse=True)
def _settings_restored(request):
    """One candidate and area sampling again after every test, whatever it did (other files share the session's context)."""
    ctx = request.getfixturevalue("gpu_ctx") if "gpu_ctx" in request.fixturenames else None
    yield
    if ctx is not None:
        from metalpathtracer_amd import capi
        ctx.set_light_candidates(1)
        ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)


def put(ctx, name, W=None, H=None):
    """The case's scene (through mpt_upload_scene with the host's tree), size and uniforms on the context; returns the uniforms."""
    _, buf = rsc.scene_of(name)
    ctx.upload_scene(*buf)
    u = rsc.uniforms_of(name, W, H)
    ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    ctx.set_uniforms(u)
    return u


def guides_match(ctx, g):
    ad, nc, _ = ctx.read_aovs()
    same(ad, g["ad"])
    same(nc, g["nc"])


def check(ctx, ref, K, R, begin, N, image=True):
    """mpt_direct_restir in both modes with both walks, and mpt_restir_image, against the reference `ref` of the same arguments."""
    from metalpathtracer_amd import capi
    g = ref["g"]
    surface = g["nc"][..., 3] == 0
    for mode in restir_ref.MODES:
        want = ref[mode]
        kw = dict(samples=N, sample_begin=begin, seed=SEED, neighbours=K, radius=R, mode=mode)
        for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
            info = ctx.direct_restir(walk=walk, **kw)
            rgba, traced, unocc = ctx.read_restir()
            initial, pick = ctx.read_restir_reservoirs(0), ctx.read_restir_reservoirs(1)
            keep = np.ones_like(surface) if walk == capi.WALK_REFERENCE else ~want["tainted"]
            print("K", K, "R", R, "rounds", (begin, N), "mode", mode, "walk", walk, "pixels that differ:",
                  int((rgba.view(np.uint32) != want["rgba"].view(np.uint32)).any(-1).sum()), {k: info[k] for k in INFO_KEYS}, "tainted",
                  int(want["tainted"].sum()), "ms", info["device_ms"])
            same(rgba[keep], want["rgba"][keep])
            np.testing.assert_array_equal(traced[keep], want["traced"][keep])
            np.testing.assert_array_equal(unocc[keep], want["unoccluded"][keep])
            np.testing.assert_array_equal(initial[keep], ref["initial"][keep])
            np.testing.assert_array_equal(pick[keep], want["pick"][keep])
            if keep.all():
                assert {k: info[k] for k in INFO_KEYS} == want["info"]
            assert traced.sum() == info["rays_initial"] + info["rays_final"] + info["rays_correction"]
            assert traced.sum() - unocc.sum() == info["rays_occluded"]
            assert (rgba[~surface] == (0, 0, 0, 1)).all() and (traced[~surface] == 0).all() and (unocc[~surface] == 0).all()
            assert not initial[~surface].any() and not pick[~surface].any()
        if image:
            img = ctx.restir_image(g["ad"], g["nc"], g["u"], walk=capi.WALK_REFERENCE, **kw)
            for a, b in zip(img, (want["rgba"], want["traced"], want["unoccluded"])):
                same(a, b)


# ---- exactness ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", rsc.MS)
@pytest.mark.parametrize("name", rsc.CASES)
def test_the_pass_is_exact(gpu_ctx, name, M):
    put(gpu_ctx, name)
    guides_match(gpu_ctx, rsc.guides(name))
    gpu_ctx.set_light_candidates(M)
    merged = 0
    for K, R, begin, N in rsc.grid():
        ref = rsc.reference(name, M, K, R, begin, N)
        check(gpu_ctx, ref, K, R, begin, N)
        merged += ref[restir_ref.UNBIASED]["info"]["samples_from_neighbours"]
    assert merged > 0                                                            # neighbours' samples were taken
    assert (ref[0]["rgba"][..., :3] > 0).any() and (ref[0]["traced"] > ref[0]["unoccluded"]).any()


@pytest.mark.parametrize("W,H,R", rsc.SMALL_SIZES)
@pytest.mark.parametrize("name", rsc.CASES)
def test_the_pass_at_small_sizes(gpu_ctx, name, W, H, R):
    """1 x 1: no neighbour can be inside, the result is K = 0's.  7 x 3 with R = 64: the radius exceeds the image."""
    put(gpu_ctx, name, W, H)
    guides_match(gpu_ctx, rsc.guides(name, W, H))
    gpu_ctx.set_light_candidates(rsc.SMALL_M)
    ref = rsc.reference(name, rsc.SMALL_M, rsc.SMALL_K, R, 7, 3, W, H)
    check(gpu_ctx, ref, rsc.SMALL_K, R, 7, 3)
    if (W, H) == (1, 1):
        none = rsc.reference(name, rsc.SMALL_M, 0, R, 7, 3, W, H)
        for mode in restir_ref.MODES:
            same(ref[mode]["rgba"], none[mode]["rgba"])
            assert ref[mode]["info"] == none[mode]["info"] and ref[mode]["info"]["neighbours_accepted"] == 0


# ---- K = 0 is the resampled direct pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (2, 32))
@pytest.mark.parametrize("name", rsc.CASES)
def test_without_neighbours_it_is_mpt_direct_lighting(gpu_ctx, name, M):
    from metalpathtracer_amd import capi
    put(gpu_ctx, name)
    gpu_ctx.set_light_candidates(M)
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        for begin, N in ((0, 1), (7, 3)):
            d = gpu_ctx.direct_lighting(samples=N, sample_begin=begin, seed=SEED, walk=walk)
            want = gpu_ctx.read_direct()
            for mode in restir_ref.MODES:
                info = gpu_ctx.direct_restir(samples=N, sample_begin=begin, seed=SEED, walk=walk, neighbours=0, mode=mode)
                for a, b in zip(gpu_ctx.read_restir(), want):
                    same(a, b)
                assert info["rays_final"] == info["rays_correction"] == info["neighbours_accepted"] == info["samples_from_neighbours"] == 0
                assert info["rays_initial"] == d["rays"] and info["rays_occluded"] == d["rays_occluded"] and info["pixels_surface"] == d["pixels_surface"]
    assert want[0][..., :3].any()


# ---- identities that need no reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell.xml", "manylights"])
def test_identities(gpu_ctx, name):
    """traced sums to the three kinds of ray; BIASED traces no correction ray and starts from the same reservoirs; twice the same bits."""
    from metalpathtracer_amd import capi
    put(gpu_ctx, name, 40, 24)
    gpu_ctx.set_light_candidates(4)
    kw = dict(samples=5, sample_begin=2, seed=SEED, neighbours=6, radius=5, walk=capi.WALK_AUTO)
    state = lambda: gpu_ctx.read_restir() + (gpu_ctx.read_restir_reservoirs(0), gpu_ctx.read_restir_reservoirs(1))
    iu = gpu_ctx.direct_restir(mode=capi.RESTIR_UNBIASED, **kw)
    u = state()
    ib = gpu_ctx.direct_restir(mode=capi.RESTIR_BIASED, **kw)
    b = state()
    for info, s in ((iu, u), (ib, b)):
        assert s[1].sum() == info["rays_initial"] + info["rays_final"] + info["rays_correction"]
        assert s[1].sum() - s[2].sum() == info["rays_occluded"]
    assert ib["rays_correction"] == 0 and iu["rays_correction"] > 0 and iu["samples_from_neighbours"] > 0
    assert ib["rays_initial"] == iu["rays_initial"] and ib["rays_final"] == iu["rays_final"] and ib["neighbours_accepted"] == iu["neighbours_accepted"]
    np.testing.assert_array_equal(u[3], b[3])                                    # the same initial reservoirs ...
    np.testing.assert_array_equal(u[4], b[4])                                    # ... and the same picks: the modes part at step D
    assert not np.array_equal(u[0], b[0])
    gpu_ctx.direct_restir(mode=capi.RESTIR_UNBIASED, **kw)
    for x, y in zip(u, state()):
        same(x, y)
    lum = lambda s: float(s[0][..., :3].astype(np.float64).mean())
    print(name, "image mean unbiased", lum(u), "biased", lum(b), iu, ib)


# ---- state ------------------------------------------------------------------------------------------------------------------------------------
def test_the_call_touches_no_other_stage_and_no_other_touches_it(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "scene.xml")
    gpu_ctx.clear_sum()
    gpu_ctx.draw(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(1, 0))
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(1, 0), flags=capi.FLAG_MOMENTS)
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.display(source=capi.DISPLAY_SUM, samples=2)
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    gpu_ctx.reset_stats()
    others = lambda: (gpu_ctx.read_frame(), gpu_ctx.read_moments(), gpu_ctx.read_denoised(), gpu_ctx.read_temporal(), gpu_ctx.read_svgf(),
                      gpu_ctx.read_display(), gpu_ctx.read_ao()[0], gpu_ctx.read_ao()[1], gpu_ctx.read_sum()) + gpu_ctx.read_direct()
    before, stats = others(), gpu_ctx.stats()
    gpu_ctx.set_light_candidates(4)
    gpu_ctx.direct_restir(samples=4, seed=SEED, neighbours=4)
    for a, b in zip(before, others()):
        np.testing.assert_array_equal(a, b)
    assert gpu_ctx.stats() == stats
    mine = gpu_ctx.read_restir() + (gpu_ctx.read_restir_reservoirs(0), gpu_ctx.read_restir_reservoirs(1))
    assert mine[0][..., :3].any()
    gpu_ctx.direct_lighting(samples=3, seed=(5, 5))                              # ... and the direct pass leaves this result alone
    for a, b in zip(mine, gpu_ctx.read_restir() + (gpu_ctx.read_restir_reservoirs(0), gpu_ctx.read_restir_reservoirs(1))):
        same(a, b)
    ptr, nbytes = gpu_ctx.restir_buffer()
    assert ptr and nbytes == mine[0].size * 4 and ptr != gpu_ctx.direct_buffer()[0]


def test_the_result_is_dropped_by_resize_and_by_both_scene_calls(gpu_ctx):
    name = "handmade"
    sc, buf = rsc.scene_of(name)
    u = put(gpu_ctx, name)
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    L, h = gpu_ctx.L, gpu_ctx.h
    out = np.empty((H, W, 4), np.float32)
    words = np.empty((H, W, 6), np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    def gone():
        p, n = C.c_void_p(), C.c_uint64()
        return (L.mpt_read_restir(h, out.ctypes.data_as(fp), None, None) == NOT_READY and L.mpt_restir_buffer(h, C.byref(p), C.byref(n)) == NOT_READY
                and L.mpt_read_restir_reservoirs(h, 0, words.ctypes.data_as(up)) == NOT_READY)

    assert gone()                                                                # (put has made a scene and a size anew)
    for drop in (lambda: (gpu_ctx.resize(W + 1, H), gpu_ctx.resize(W, H)), lambda: gpu_ctx.upload_scene(*buf),
                 lambda: gpu_ctx.build_and_upload(*sc.packed_primitives())):
        gpu_ctx.direct_restir(samples=2, seed=SEED, neighbours=2)
        assert not gone() and gpu_ctx.read_restir()[0][..., :3].any()
        drop()
        assert gone()


def test_every_refusal_leaves_the_previous_result(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "cornell.xml")
    gpu_ctx.set_light_candidates(3)
    gpu_ctx.direct_restir(samples=2, seed=SEED, neighbours=3)
    state = lambda: gpu_ctx.read_restir() + (gpu_ctx.read_restir_reservoirs(0), gpu_ctx.read_restir_reservoirs(1))
    before = state()
    L, h = gpu_ctx.L, gpu_ctx.h
    nan = float("nan")
    bad = [dict(samples=0), dict(samples=capi.DIRECT_MAX_SAMPLES + 1), dict(walk=3), dict(walk=-1), dict(mode=2), dict(mode=-1), dict(neighbours=17),
           dict(radius=65), dict(normal_threshold=nan), dict(depth_tolerance=nan)]
    for kw in bad:
        p = capi.restir_params(**dict(dict(samples=2, seed=SEED, neighbours=3), **kw))
        assert L.mpt_direct_restir(h, C.byref(p), None) == INVALID, kw
        assert b"restir" in L.mpt_last_error(h), kw
    assert L.mpt_direct_restir(h, None, None) == INVALID
    g = rsc.guides("cornell.xml")
    with pytest.raises(capi.MptError):
        gpu_ctx.restir_image(g["ad"], g["nc"], g["u"], samples=2, neighbours=17)
    gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_CONE)                          # cone sampling in effect: refused, K = 0 too
    for K in (0, 3):
        p = capi.restir_params(samples=2, seed=SEED, neighbours=K)
        assert L.mpt_direct_restir(h, C.byref(p), None) == INVALID and b"area" in L.mpt_last_error(h)
    gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)
    words = np.empty(before[3].shape, np.uint32)
    assert L.mpt_read_restir_reservoirs(h, 2, words.ctypes.data_as(C.POINTER(C.c_uint32))) == INVALID
    for a, b in zip(before, state()):
        same(a, b)
    gpu_ctx.direct_restir(samples=2, seed=SEED, neighbours=3)                     # ... and the call works as before
    for a, b in zip(before, state()):
        same(a, b)


# ---- the expectation on the device ------------------------------------------------------------------------------------------------------------
B, ROUNDS_B, STAT_K = 48, 32, 4


@pytest.mark.parametrize("name", ["manylights", "cornell.xml"])
def test_unbiased_reuse_has_the_expectation_of_the_direct_pass(gpu_ctx, name):
    """tests/test_gpu_ris.py's scenes at 32 x 32; B batches of ROUNDS_B rounds per estimator under different seeds.  The pixels of one
    ReSTIR image share samples, so the image mean is the unit: D_b = the image mean of (restir - direct) of batch b and
    |mean_b D_b| <= 5 std_b(D_b) / sqrt(B).  Per pixel mean z^2 <= 1.3 as there: a pixel's marginal is not affected by the sharing.
    The same two figures are printed for BIASED and not asserted."""
    from metalpathtracer_amd import capi
    from test_gpu_ris import stat_scene
    stat_scene(gpu_ctx, name)
    gpu_ctx.set_light_candidates(1)
    x = {k: np.empty((B, 32, 32)) for k in ("direct", "unbiased", "biased")}
    ms = dict.fromkeys(x, 0.0)
    for b in range(B):
        info = gpu_ctx.direct_lighting(samples=ROUNDS_B, seed=(b, 1), walk=capi.WALK_AUTO)
        x["direct"][b] = gpu_ctx.read_direct()[0][..., :3].astype(np.float64).mean(-1)
        ms["direct"] += info["device_ms"]
        for key, mode in (("unbiased", capi.RESTIR_UNBIASED), ("biased", capi.RESTIR_BIASED)):
            info = gpu_ctx.direct_restir(samples=ROUNDS_B, seed=(b, 2 + mode), walk=capi.WALK_AUTO, neighbours=STAT_K, mode=mode)
            x[key][b] = gpu_ctx.read_restir()[0][..., :3].astype(np.float64).mean(-1)
            ms[key] += info["device_ms"]
    m1, v1 = x["direct"].mean(0), x["direct"].var(0, ddof=1)
    figures = {}
    for key in ("unbiased", "biased"):
        D = (x[key] - x["direct"]).reshape(B, -1).mean(-1)
        m, v = x[key].mean(0), x[key].var(0, ddof=1)
        still = (v1 == 0) & (v == 0)
        z = (m - m1)[~still] / np.sqrt((v + v1)[~still] / B)
        both = (v1 > 0) & (v > 0)
        figures[key] = (D.mean(), 5 * D.std(ddof=1) / np.sqrt(B), (z * z).mean(), still, m)
        print(name, key, "mean D", D.mean(), "bound", 5 * D.std(ddof=1) / np.sqrt(B), "pixels", z.size, "mean z^2", (z * z).mean(), "max |z|",
              np.abs(z).max(), "image means", m1.mean(), m.mean(), "sum var(direct) / sum var:", v1[both].sum() / v[both].sum(), "device ms",
              ms["direct"], ms[key])
    mean, bound, z2, still, m = figures["unbiased"]
    assert (~still).sum() >= still.size // 4
    np.testing.assert_allclose(m[still], m1[still], rtol=1e-6)
    assert bound > 0 and abs(mean) <= bound
    assert z2 <= 1.3


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------
def run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


W_CLI, H_CLI = 48, 32


def cli_base():
    return [EXE, "--scene", scene_path("scene.xml"), "--width", str(W_CLI), "--height", str(H_CLI), "--spp", "4", "--depth", "4", "--seed", "1", "--bvh",
            "reference"]


def test_cli_restir(tmp_path):
    """mpt_render --direct 4 --restir 4 writes what the host layer returns through the same writer; --restir 0 writes the file of
    --light-candidates alone; each refusal prints its message and exits non-zero.  (Without --restir the files are the parent's:
    tests/test_gpu_ris.py::test_cli_light_candidates and tests/test_gpu_direct.py hold them to the host layer, unchanged.)"""
    from metalpathtracer_amd import capi, host
    p = lambda name: str(tmp_path / name)
    read = lambda name: open(p(name), "rb").read()
    lines = {}
    for key, extra in (("r4", ["--direct", "4", "--restir", "4"]), ("r4b", ["--direct", "4", "--restir", "4", "--restir-radius", "3", "--restir-biased"]),
                       ("r0", ["--direct", "4", "--restir", "0", "--light-candidates", "4"]), ("d4", ["--direct", "4", "--light-candidates", "4"]),
                       ("d", ["--direct", "4"])):
        r = run(cli_base() + ["--out", p(key + ".ppm")] + extra)
        assert r.returncode == 0, (key, r.stderr[-2000:])
        lines[key] = json.loads(r.stdout.splitlines()[-1])
    assert "restir" not in lines["d"] and "restir" not in lines["d4"] and "direct" not in lines["r4"]
    assert lines["r4"]["restir"]["neighbours"] == 4 and lines["r4"]["restir"]["radius"] == capi.RESTIR_DEFAULTS["radius"] == 4 and lines["r4"]["restir"]["mode"] == "unbiased"
    assert lines["r4b"]["restir"]["radius"] == 3 and lines["r4b"]["restir"]["mode"] == "biased" and lines["r4b"]["restir"]["rays_correction"] == 0
    assert lines["r4"]["restir"]["samples_from_neighbours"] > 0 and lines["r4"]["restir"]["rays_correction"] > 0
    assert read("r0.ppm") == read("d4.ppm") and read("r4.ppm") != read("d.ppm")
    assert lines["r0"]["restir"]["light_candidates"] == 4 and lines["r0"]["restir"]["rays_initial"] == lines["d4"]["direct"]["rays"]
    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W_CLI, H_CLI)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(1, 0))
        for key, kw in (("r4", dict(neighbours=4)), ("r4b", dict(neighbours=4, radius=3, mode=capi.RESTIR_BIASED))):
            rgba, info = rr.renderDirectRestir(4, **kw)
            for k in INFO_KEYS:
                assert lines[key]["restir"][k] == info[k], (key, k)
            assert host.write_ppm(p("mine.ppm"), rgba) == 0
            assert read("mine.ppm") == read(key + ".ppm")
        with pytest.raises(Exception):
            rr.renderDirectRestir(4, 17)
    finally:
        rr.close()
    for bad, word in ((["--restir", "4"], "--direct"), (["--nee", "--restir", "4"], "--direct"), (["--direct", "4", "--restir-radius", "4"], "--restir K"),
                      (["--direct", "4", "--restir-biased"], "--restir K"), (["--direct", "4", "--restir", "17"], "0..16"),
                      (["--direct", "4", "--restir", "-1"], "0..16"), (["--direct", "4", "--restir", "4", "--restir-radius", "0"], "1..64"),
                      (["--direct", "4", "--restir", "4", "--restir-radius", "65"], "1..64"),
                      (["--direct", "4", "--restir", "4", "--light-sampling", "cone"], "cone")):
        r = run(cli_base() + ["--out", p("x.ppm")] + bad)
        assert r.returncode == 2 and "--restir" in r.stderr and word in r.stderr, (bad, r.stderr[-500:])
