"""GPU tests of mpt_set_light_candidates (include/mpt.h: resampled light sampling) against tests/ris_ref.py: with m >= 2 the direct
pass's image and counts and mpt_render_nee's sum and counts are compared bit for bit, under both light samplings.  Occlusion is
tests/anyhit_ref.py's `lower` — what MPT_WALK_REFERENCE must answer — and MPT_WALK_OWN is held to the same on every pixel without a gap
ray (tests/test_ris_cpu.py caps those at 1 % of each case's pixels).  Then identities that need no reference, the setting and its life,
the expectation on the device (m = 8 against m = 1 under different seeds) and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ris_cases as rcs
import ris_ref
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

SEED = rcs.SEED
INVALID = 1
EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


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
    _, buf = rcs.scene_of(name)
    ctx.upload_scene(*buf)
    u = rcs.uniforms_of(name, W, H)
    ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    ctx.set_uniforms(u)
    return u


def setting(ctx, M, sampling):
    ctx.set_light_candidates(M)
    ctx.set_light_sampling(sampling)               # (rcs.AREA, rcs.CONE are the C API's values)


# ---- the direct pass ------------------------------------------------------------------------------------------------------------------
def check_direct(ctx, r, begin, N):
    """mpt_direct_lighting with both walks and mpt_direct_image against samples [begin, begin + N) of the reference r."""
    from metalpathtracer_amd import capi
    sampled, lower, upper = rcs.direct_sliced(r, begin, N)
    want = ris_ref.direct(r["ad"], r["nc"], r["u"], r["table"], begin, N, SEED, lower, sampled=sampled)
    surface = r["nc"][..., 3] == 0
    gap = (upper & ~lower).any(-1)
    assert gap.sum() <= rcs.GAP_CAP * gap.size
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        info = ctx.direct_lighting(samples=N, sample_begin=begin, seed=SEED, walk=walk)
        got = ctx.read_direct()
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        print("walk", walk, "begin", begin, "N", N, "pixels that differ:", int((got[0].view(np.uint32) != want[0].view(np.uint32)).any(-1).sum()),
              "traced", info["rays"], "occluded", info["rays_occluded"], "gap pixels", int(gap.sum()), "ms", info["device_ms"])
        same(got[0][keep], want[0][keep])
        np.testing.assert_array_equal(got[1], want[1])                      # (what is traced does not depend on the walk)
        np.testing.assert_array_equal(got[2][keep], want[2][keep])
        assert info["pixels_surface"] == surface.sum() and info["rays"] == want[1].sum() and info["lights"] == r["table"].n
        if not gap.any():
            assert info["rays_occluded"] == want[1].sum() - want[2].sum()
        assert (got[0][~surface] == (0, 0, 0, 1)).all() and (got[1][~surface] == 0).all() and (got[2][~surface] == 0).all()
    img = ctx.direct_image(r["ad"], r["nc"], r["u"], samples=N, sample_begin=begin, seed=SEED, walk=capi.WALK_REFERENCE)
    for a, b in zip(img, want):
        same(a, b)
    return want


@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("M", rcs.DIRECT_MS)
@pytest.mark.parametrize("name", rcs.DIRECT_CASES)
def test_the_direct_pass_is_exact(gpu_ctx, name, M, sampling):
    put(gpu_ctx, name)
    r = rcs.direct_reference(name, M, sampling)
    ad, nc, _ = gpu_ctx.read_aovs()
    same(ad, r["ad"])
    same(nc, r["nc"])
    setting(gpu_ctx, M, sampling)
    for begin in (0, 7):
        for N in (1, 3):
            want = check_direct(gpu_ctx, r, begin, N)
    assert (want[0][..., :3] > 0).any() and (want[1] > want[2]).any()            # lit pixels and occluded samples occur


@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("W,H", rcs.SMALL_SIZES)
@pytest.mark.parametrize("name", rcs.DIRECT_CASES)
def test_the_direct_pass_at_small_sizes(gpu_ctx, name, W, H, sampling):
    put(gpu_ctx, name, W, H)
    r = rcs.direct_reference(name, rcs.SMALL_M, sampling, W, H)
    ad, nc, _ = gpu_ctx.read_aovs()
    same(ad, r["ad"])
    same(nc, r["nc"])
    setting(gpu_ctx, rcs.SMALL_M, sampling)
    check_direct(gpu_ctx, r, 7, 3)


# ---- mpt_render_nee -------------------------------------------------------------------------------------------------------------------
def nee(ctx, name, **kw):
    from metalpathtracer_amd import capi
    kw.setdefault("seed", SEED)
    return ctx.render_nee(rng_mode=capi.RNG_PHILOX, bsdf_mode=rcs.bsdf_mode(name), **kw)


def check_nee(ctx, name, r, spp, depth):
    """samples [0, spp) of the reference r with both walks: the sum bit for bit, the counts exactly."""
    from metalpathtracer_amd import capi
    want = ris_ref.accumulate(r["value"][:, :, :spp])
    gap = r["gap"][:, :, :spp].any(-1)
    assert gap.sum() <= rcs.GAP_CAP * gap.size
    rays, shadow, occluded = (int(r[k][:, :, :spp].sum()) for k in ("rays", "shadow", "occluded"))
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        ctx.clear_sum()
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
        assert info["lights"] == rcs.table_of(name).n


@pytest.mark.parametrize("depth", rcs.DEPTHS)
@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("name", rcs.NEE_CASES)
def test_the_sum_is_exact(gpu_ctx, name, sampling, depth):
    put(gpu_ctx, name)
    for M in rcs.nee_ms(name):
        setting(gpu_ctx, M, sampling)
        r = rcs.nee_reference(name, depth, M, sampling)
        for spp in (1, 3):
            check_nee(gpu_ctx, name, r, spp, depth)
        if depth > 1:
            assert r["shadow"].sum() > r["occluded"].sum() > 0               # open and occluded shadow rays both occur


@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("W,H", rcs.SMALL_SIZES)
@pytest.mark.parametrize("name", rcs.NEE_CASES)
def test_the_sum_at_small_sizes(gpu_ctx, name, W, H, sampling):
    put(gpu_ctx, name, W, H)
    setting(gpu_ctx, rcs.SMALL_M, sampling)
    check_nee(gpu_ctx, name, rcs.nee_reference(name, 4, rcs.SMALL_M, sampling, W, H), 3, 4)


# ---- identities that need no reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,depth", [("manylights", 1), ("scene.xml", 1), ("dark", 4)])
def test_without_a_light_sample_the_call_adds_what_mpt_render_adds(gpu_ctx, name, depth):
    """max_depth = 1 (no vertex may draw a light sample), or an empty light table at any depth, with clamp = 1: all four channels."""
    from metalpathtracer_amd import capi
    import direct_cases
    if name == "dark":
        _, buf = direct_cases.scene_of("dark")
        gpu_ctx.upload_scene(*buf)
        u = direct_cases.uniforms_of("dark")
        gpu_ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
        gpu_ctx.set_uniforms(u)
    else:
        put(gpu_ctx, name)
    kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=depth, sample_begin=2, sample_count=3, seed=SEED)
    gpu_ctx.clear_sum()
    gpu_ctx.render(**kw)
    want = gpu_ctx.read_sum()
    for sampling in rcs.SAMPLINGS:
        setting(gpu_ctx, 4, sampling)
        for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
            gpu_ctx.clear_sum()
            info = gpu_ctx.render_nee(walk=walk, clamp=1.0, **kw)
            same(gpu_ctx.read_sum(), want)
            assert info["shadow_rays"] == 0
        if name == "dark":                                                       # ... and the direct pass of a scene without lights is black
            info = gpu_ctx.direct_lighting(samples=3, seed=SEED)
            rgba, traced, unocc = gpu_ctx.read_direct()
            assert info["rays"] == 0 and not rgba[..., :3].any() and not traced.any() and not unocc.any()
    assert want[..., :3].any() and want[..., 3].any()


def outputs(ctx, name):
    """(direct rgba, traced, unoccluded, the sum of a render) under the context's settings."""
    from metalpathtracer_amd import capi
    ctx.direct_lighting(samples=3, sample_begin=1, seed=SEED, walk=capi.WALK_REFERENCE)
    d = ctx.read_direct()
    ctx.clear_sum()
    nee(ctx, name, walk=capi.WALK_REFERENCE, max_depth=4, sample_count=3)
    return d + (ctx.read_sum(),)


def test_the_setting(gpu_ctx):
    """The default is 1 and get / set round-trip; 8 survives mpt_resize, both scene calls and mpt_clear_sum; 0, 33 and a null pointer
    are MPT_ERR_INVALID_ARG and change neither the getter nor the next result; after set(8), set(1) the output is an untouched
    context's — today's kernels, whose bits tests/test_gpu_direct.py and tests/test_gpu_nee.py pin."""
    from metalpathtracer_amd import capi
    name = "manylights"
    sc, buf = rcs.scene_of(name)
    L, h = gpu_ctx.L, gpu_ctx.h
    fresh = capi.Context(0)
    try:
        assert fresh.get_light_candidates() == 1 and gpu_ctx.get_light_candidates() == 1
        put(fresh, name)
        untouched = outputs(fresh, name)
        put(gpu_ctx, name)
        for m in (32, 2, 8):
            gpu_ctx.set_light_candidates(m)
            assert gpu_ctx.get_light_candidates() == m
        eight = outputs(gpu_ctx, name)
        assert not np.array_equal(eight[0], untouched[0]) and not np.array_equal(eight[3], untouched[3])
        W, H = int(rcs.uniforms_of(name).screenSize[0]), int(rcs.uniforms_of(name).screenSize[1])
        gpu_ctx.resize(W + 1, H)
        gpu_ctx.resize(W, H)
        gpu_ctx.upload_scene(*buf)
        prims, mats = sc.packed_primitives()
        gpu_ctx.build_and_upload(prims, mats)
        gpu_ctx.clear_sum()
        assert gpu_ctx.get_light_candidates() == 8
        put(gpu_ctx, name)
        for m in (0, 33, 0xFFFFFFFF):
            assert L.mpt_set_light_candidates(h, m) == INVALID, m
            assert b"mpt_set_light_candidates" in L.mpt_last_error(h)
            assert gpu_ctx.get_light_candidates() == 8
        assert L.mpt_get_light_candidates(h, None) == INVALID and L.mpt_set_light_candidates(None, 2) == INVALID
        for a, b in zip(eight, outputs(gpu_ctx, name)):                          # a second call gives the same bits
            same(a, b)
        gpu_ctx.set_light_candidates(1)
        for a, b in zip(untouched, outputs(gpu_ctx, name)):
            same(a, b)
    finally:
        fresh.close()


def test_sample_ranges_compose_and_the_callers_sum_buffer_is_honoured(gpu_ctx):
    from metalpathtracer_amd import capi
    name = "handmade"
    u = put(gpu_ctx, name)
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    setting(gpu_ctx, 5, rcs.AREA)
    r = rcs.nee_reference(name, 4, 5, rcs.AREA)
    kw = dict(walk=capi.WALK_REFERENCE, max_depth=4)
    gpu_ctx.clear_sum()
    nee(gpu_ctx, name, sample_begin=0, sample_count=2, **kw)
    first = gpu_ctx.read_sum()
    nee(gpu_ctx, name, sample_begin=2, sample_count=1, **kw)                   # a second call adds onto the first: [0, 2) + [2, 3) = [0, 3)
    whole = gpu_ctx.read_sum()
    same(first, ris_ref.accumulate(r["value"][:, :, :2]))
    same(whole, ris_ref.accumulate(r["value"]))
    other = capi.Context(0)                                                     # its sum buffer is device memory this context knows nothing about
    try:
        other.resize(W, H)
        ptr, nbytes = other.sum_buffer()
        assert nbytes == W * H * 16
        gpu_ctx.clear_sum()
        inside = gpu_ctx.read_sum()
        gpu_ctx.set_sum_buffer(ptr)
        try:
            nee(gpu_ctx, name, sample_count=3, **kw)
        finally:
            gpu_ctx.set_sum_buffer(None)
        same(other.read_sum(), whole)
        same(gpu_ctx.read_sum(), inside)                                        # the internal buffer was not written
    finally:
        other.close()


def test_the_calls_touch_no_other_stage(gpu_ctx):
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
    others = lambda: (gpu_ctx.read_frame(), gpu_ctx.read_moments(), gpu_ctx.read_denoised(), gpu_ctx.read_temporal(), gpu_ctx.read_svgf(),
                      gpu_ctx.read_display(), gpu_ctx.read_ao()[0], gpu_ctx.read_ao()[1])
    before, d0, s0 = others(), gpu_ctx.read_direct(), gpu_ctx.read_sum()
    setting(gpu_ctx, 4, rcs.CONE)
    nee(gpu_ctx, "scene.xml", walk=capi.WALK_AUTO, max_depth=4, sample_begin=2, sample_count=2)
    for a, b in zip(before + d0, others() + gpu_ctx.read_direct()):            # the render touched the sum alone
        np.testing.assert_array_equal(a, b)
    s1 = gpu_ctx.read_sum()
    assert not np.array_equal(s0, s1)
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    for a, b in zip(before + (s1,), others() + (gpu_ctx.read_sum(),)):         # the pass touched its own result alone
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(d0[0], gpu_ctx.read_direct()[0])


def test_the_adaptive_render_refuses_more_than_one_candidate(gpu_ctx):
    """MPT_ERR_INVALID_ARG with the sum, the moments and the tile counts untouched; it works again with one candidate."""
    from metalpathtracer_amd import capi
    put(gpu_ctx, "manylights")
    kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=8, seed=SEED)
    gpu_ctx.render_nee_adaptive(0.05, min_samples=4, batch_samples=4, **kw)
    state = lambda: (gpu_ctx.read_sum(), gpu_ctx.read_moments(), gpu_ctx.read_tile_samples())
    before = state()
    assert before[0].any() and before[2].any()
    gpu_ctx.set_light_candidates(4)
    p, n = gpu_ctx.params(**kw), capi.NeeParams(capi.WALK_AUTO, 0.0)
    a = capi.AdaptiveParams(4, 4, 0.05, 0.0)
    assert gpu_ctx.L.mpt_render_nee_adaptive(gpu_ctx.h, C.byref(p), C.byref(n), C.byref(a), None, None) == INVALID
    assert b"candidates" in gpu_ctx.L.mpt_last_error(gpu_ctx.h)
    for x, y in zip(before, state()):
        same(x, y)
    gpu_ctx.set_light_candidates(1)
    gpu_ctx.render_nee_adaptive(0.05, min_samples=4, batch_samples=4, **kw)
    for x, y in zip(before, state()):
        same(x, y)


# ---- the expectation on the device: m = 8 against m = 1 ---------------------------------------------------------------------------------
B, SPP_B, STAT_W, STAT_DEPTH = 64, 64, 32, 4


def stat_scene(ctx, name):
    """manylights, or the Cornell box of tests/test_gpu_nee.py's statistical test (the lights' emissionPower 1 and albedo 0), at 32 x 32."""
    from metalpathtracer_amd import host
    sc, buf = rcs.scene_of(name)
    mats = np.array(buf[2], np.float32).reshape(-1, 2, 4)
    cam = rcs.nee_cases.CASES[name][3]
    if name == "cornell.xml":
        lights = mats[:, 1, 3] > 0
        assert lights.sum() == 2
        mats[lights, 1, 3] = 1.0
        mats[lights, 0, :3] = 0.0
    ctx.upload_scene(buf[0], buf[1], mats, buf[3])
    u = host.make_uniforms(STAT_W, STAT_W, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)
    ctx.resize(STAT_W, STAT_W)
    ctx.set_uniforms(u)


@pytest.mark.parametrize("what", ["direct", "nee"])
@pytest.mark.parametrize("name", ["manylights", "cornell.xml"])
def test_eight_candidates_have_the_expectation_of_one(gpu_ctx, name, what):
    """The batch design and the two bounds of tests/test_gpu_nee.py: 64 batches of 64 samples per pixel and estimator, different seeds
    for the two; per pixel the scalar is the mean of the three channels, z = (m_8 - m_1) / sqrt((s2_8 + s2_1) / B) over the pixels with
    a variance; |mean z| <= 5 / sqrt(n), mean z^2 <= 1.3."""
    from metalpathtracer_amd import capi
    stat_scene(gpu_ctx, name)
    x = {1: np.empty((B, STAT_W, STAT_W)), 8: np.empty((B, STAT_W, STAT_W))}
    ms = {1: 0.0, 8: 0.0}
    for M in (1, 8):
        gpu_ctx.set_light_candidates(M)
        for b in range(B):
            if what == "direct":
                info = gpu_ctx.direct_lighting(samples=SPP_B, seed=(b, M), walk=capi.WALK_AUTO)
                x[M][b] = gpu_ctx.read_direct()[0][..., :3].astype(np.float64).mean(-1)
            else:
                gpu_ctx.clear_sum()
                info = gpu_ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=STAT_DEPTH, sample_count=SPP_B, seed=(b, M), walk=capi.WALK_AUTO, clamp=0.0)
                x[M][b] = gpu_ctx.read_sum()[..., :3].astype(np.float64).mean(-1) / SPP_B
            ms[M] += info["device_ms"]
    m1, m8 = x[1].mean(0), x[8].mean(0)
    v1, v8 = x[1].var(0, ddof=1), x[8].var(0, ddof=1)
    still = (v1 == 0) & (v8 == 0)
    assert (~still).sum() >= still.size // 4                            # (the many-light case shows the sky in its upper half)
    np.testing.assert_allclose(m8[still], m1[still], rtol=1e-6)
    z = (m8 - m1)[~still] / np.sqrt((v8 + v1)[~still] / B)
    both = (v1 > 0) & (v8 > 0)
    print(name, what, "pixels:", z.size, "mean z:", z.mean(), "bound", 5 / np.sqrt(z.size), "mean z^2:", (z * z).mean(), "max |z|:", np.abs(z).max(),
          "image means", m1.mean(), m8.mean(), "sum var(1) / sum var(8):", v1[both].sum() / v8[both].sum(), "device ms", ms[1], ms[8])
    assert abs(z.mean()) <= 5 / np.sqrt(z.size)
    assert (z * z).mean() <= 1.3


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


W_CLI, H_CLI, SPP_CLI, DEPTH_CLI = 48, 32, 4, 4


def cli_base(spp=SPP_CLI):
    return [EXE, "--scene", scene_path("scene.xml"), "--width", str(W_CLI), "--height", str(H_CLI), "--spp", str(spp), "--depth", str(DEPTH_CLI),
            "--seed", "1", "--bvh", "reference"]


def test_cli_light_candidates(tmp_path):
    """mpt_render --direct 4 / --nee with --light-candidates 4 writes what the host layer gives through the same writer; with
    --light-candidates 1 and without the flag the files are the same and the JSON keys without it are what they were; the refusals."""
    from metalpathtracer_amd import capi, host
    p = lambda name: str(tmp_path / name)
    lines = {}
    for key, extra in (("d_4", ["--out", p("d_4.ppm"), "--direct", "4", "--light-candidates", "4"]),
                       ("d_1", ["--out", p("d_1.ppm"), "--direct", "4", "--light-candidates", "1"]),
                       ("d_none", ["--out", p("d_none.ppm"), "--direct", "4"]),
                       ("n_4", ["--out", p("n_4.pfm"), "--nee", "--nee-walk", "reference", "--light-candidates", "4", "--light-sampling", "cone"]),
                       ("n_1", ["--out", p("n_1.pfm"), "--nee", "--nee-walk", "reference", "--light-candidates", "1"]),
                       ("n_none", ["--out", p("n_none.pfm"), "--nee", "--nee-walk", "reference"]),
                       ("a_1", ["--out", p("a_1.pfm"), "--nee-adaptive", "0.05", "--light-candidates", "1"])):
        r = run(cli_base() + extra)
        assert r.returncode == 0, (key, r.stderr[-2000:])
        lines[key] = json.loads(r.stdout.splitlines()[-1])
    assert lines["d_4"]["direct"]["light_candidates"] == 4 and lines["d_1"]["direct"]["light_candidates"] == 1
    assert lines["n_4"]["nee"]["light_candidates"] == 4 and lines["n_4"]["nee"]["light_sampling"] == "cone" and lines["n_1"]["nee"]["light_candidates"] == 1
    assert "light_candidates" not in lines["d_none"]["direct"] and "light_candidates" not in lines["n_none"]["nee"]
    assert sorted(lines["d_1"]["direct"]) == sorted(list(lines["d_none"]["direct"]) + ["light_candidates"])
    read = lambda name: open(p(name), "rb").read()
    assert read("d_1.ppm") == read("d_none.ppm") and read("n_1.pfm") == read("n_none.pfm")
    assert read("d_4.ppm") != read("d_none.ppm") and read("n_4.pfm") != read("n_none.pfm")
    for bad in (["--light-candidates", "4"], ["--light-candidates", "4", "--ao", "4"], ["--nee", "--light-candidates", "0"],
                ["--nee", "--light-candidates", "33"], ["--direct", "4", "--light-candidates", "-2"], ["--nee-adaptive", "0.05", "--light-candidates", "2"]):
        r = run(cli_base() + ["--out", p("x.ppm")] + bad)
        assert r.returncode == 2 and "--light-candidates" in r.stderr, (bad, r.stderr[-500:])
    # the host layer through the same writers
    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W_CLI, H_CLI)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH_CLI, seed=(1, 0))
        assert rr.lightCandidates() == 1
        for m, sampling, d_name, n_name, d_key, n_key in ((4, capi.LIGHT_SAMPLING_AREA, "d_4.ppm", None, "d_4", None),
                                                          (4, capi.LIGHT_SAMPLING_CONE, None, "n_4.pfm", None, "n_4"),
                                                          (1, capi.LIGHT_SAMPLING_AREA, "d_none.ppm", "n_none.pfm", "d_none", "n_none")):
            rr.setLightCandidates(m)
            rr.setLightSampling(sampling)
            assert rr.lightCandidates() == m
            if d_name:
                rgba, info = rr.renderDirectLighting(4)
                for key in ("pixels_surface", "rays", "rays_occluded", "lights"):
                    assert lines[d_key]["direct"][key] == info[key], (m, key)
                assert host.write_ppm(p("mine.ppm"), rgba) == 0
                assert read("mine.ppm") == read(d_name)
            if n_name:
                rr.clearSum()
                info = rr.renderNee(SPP_CLI, DEPTH_CLI, walk=capi.WALK_REFERENCE)
                for key in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights"):
                    assert lines[n_key]["nee"][key] == info[key], (m, key)
                assert host.write_pfm(p("mine.pfm"), rr.readSum(), scale=1.0 / SPP_CLI) == 0
                assert read("mine.pfm") == read(n_name)
        for m in (0, 33):
            with pytest.raises(Exception):
                rr.setLightCandidates(m)
        assert rr.lightCandidates() == 1
    finally:
        rr.close()


def test_cli_checkpoints_of_different_candidate_counts_do_not_mix(tmp_path):
    """A run with M > 1 writes the header MPTNEE3 (its last fields the sampling and M) and two halves give the whole render's file; with
    --light-candidates 1 the header stays MPTNEE1; neither resumes the other's file, nor one of another M or another sampling."""
    p = lambda name: str(tmp_path / name)
    read = lambda name: open(p(name), "rb").read()
    nee_flags = ["--nee", "--nee-walk", "reference"]
    four = nee_flags + ["--light-candidates", "4"]
    r = run(cli_base() + ["--out", p("whole.pfm")] + four)
    assert r.returncode == 0, r.stderr[-2000:]
    half = cli_base(SPP_CLI // 2)
    r = run(half + ["--out", p("h.pfm")] + four + ["--checkpoint", p("four.ck")])
    assert r.returncode == 0 and read("four.ck")[:8] == b"MPTNEE3 ", r.stderr[-2000:]
    assert read("four.ck").split(b"\n", 1)[0].split()[-2:] == [b"0", b"4"]
    r = run(half + ["--out", p("resumed.pfm")] + four + ["--resume", p("four.ck"), "--checkpoint", p("four2.ck")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert read("resumed.pfm") == read("whole.pfm")
    r = run(half + ["--out", p("h.pfm")] + nee_flags + ["--light-candidates", "1", "--checkpoint", p("one.ck")])
    assert r.returncode == 0 and read("one.ck")[:8] == b"MPTNEE1 ", r.stderr[-2000:]
    r = run(half + ["--out", p("h1.pfm")] + nee_flags + ["--checkpoint", p("none.ck")])
    assert r.returncode == 0 and read("none.ck") == read("one.ck") and read("h1.pfm") == read("h.pfm")
    for bad in (four + ["--resume", p("one.ck")], nee_flags + ["--resume", p("four.ck")], nee_flags + ["--light-candidates", "1", "--resume", p("four.ck")],
                nee_flags + ["--light-candidates", "5", "--resume", p("four.ck")], four + ["--light-sampling", "cone", "--resume", p("four.ck")],
                ["--resume", p("four.ck")]):
        r = run(half + ["--out", p("x.pfm")] + bad)
        assert r.returncode == 1 and "checkpoint" in r.stderr, (bad, r.stderr[-500:])
