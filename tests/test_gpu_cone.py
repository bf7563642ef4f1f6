"""GPU tests of MPT_LIGHT_SAMPLING_CONE (mpt_set_light_sampling, include/mpt.h) against tests/cone_ref.py: under CONE the direct pass's
image and mpt_render_nee's HDR sum are compared bit for bit and the counts exactly, with both walks.  Occlusion is tests/anyhit_ref.py's
`lower` — what MPT_WALK_REFERENCE must answer — and MPT_WALK_OWN is held to the same on every pixel without a gap ray
(tests/test_cone_cpu.py caps those pixels at 1 % of each case).  Then identities that need no reference, the setting itself, a
statistical comparison with the plain path tracer and with the area rule, and the CLI."""
import json
import os
import subprocess

import numpy as np
import pytest

import cone_cases as ccs
import cone_ref
import nee_cases as ncs
from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

SEED = ccs.SEED
INVALID = 1
EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture
def cone_ctx(gpu_ctx):
    """The session's context with CONE set; AREA again afterwards, whatever the test did (other files share the context)."""
    from metalpathtracer_amd import capi
    gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_CONE)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)


def put(ctx, name, W=None, H=None):
    """The case's scene (through mpt_upload_scene with the host's tree), size and uniforms on the context; returns the uniforms."""
    _, buf = ccs.scene_of(name)
    ctx.upload_scene(*buf)
    u = ccs.uniforms_of(name, W, H)
    ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    ctx.set_uniforms(u)
    return u


# ---- the direct pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("size", [None] + list(ccs.SMALL_SIZES))
@pytest.mark.parametrize("name", ccs.DIRECT_CASES)
def test_the_direct_pass_is_exact_with_both_walks(cone_ctx, name, size, N):
    from metalpathtracer_amd import capi
    W, H = size or (None, None)
    u = put(cone_ctx, name, W, H)
    assert cone_ctx.light_sampling == capi.LIGHT_SAMPLING_CONE          # (the scene upload and the resize left the setting alone)
    r = ccs.direct_reference(name, W, H)
    ad, nc, _ = cone_ctx.read_aovs()
    same(ad, r["ad"])
    same(nc, r["nc"])
    sampled, lower, upper = ccs.direct_sliced(r, N)
    want = cone_ref.direct(r["ad"], r["nc"], r["u"], r["table"], 0, N, SEED, lower, sampled=sampled)
    surface = r["nc"][..., 3] == 0
    gap = (upper & ~lower).any(-1)
    assert gap.sum() <= ccs.GAP_CAP * gap.size
    uu = capi.Uniforms.from_buffer_copy(bytes(u))
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        info = cone_ctx.direct_lighting(samples=N, seed=SEED, walk=walk)
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        for got in (cone_ctx.read_direct(), cone_ctx.direct_image(r["ad"], r["nc"], uu, samples=N, seed=SEED, walk=walk)):
            print(name, size, "walk", walk, "N", N, "pixels that differ:", int((got[0].view(np.uint32) != want[0].view(np.uint32)).any(-1).sum()), "traced",
                  info["rays"], "occluded", info["rays_occluded"], "gap pixels", int(gap.sum()), "ms", info["device_ms"])
            same(got[0][keep], want[0][keep])
            np.testing.assert_array_equal(got[1], want[1])                  # (what is traced does not depend on the walk)
            np.testing.assert_array_equal(got[2][keep], want[2][keep])
        assert info["pixels_surface"] == surface.sum() and info["rays"] == want[1].sum() and info["lights"] == r["table"].n
        if not gap.any():
            assert info["rays_occluded"] == want[1].sum() - want[2].sum()
    if size is None and N == 3:
        assert (want[0][..., :3] > 0).any() and (want[2] < want[1]).any()   # lit pixels and occluded samples both occur


# ---- mpt_render_nee -------------------------------------------------------------------------------------------------------------------
def nee(ctx, name, **kw):
    from metalpathtracer_amd import capi
    kw.setdefault("seed", SEED)
    return ctx.render_nee(rng_mode=capi.RNG_PHILOX, bsdf_mode=ccs.CASES[name][3], **kw)


def check_nee(ctx, name, r, spp, depth):
    """samples [0, spp) of the reference r with both walks: the sum bit for bit, the counts exactly."""
    from metalpathtracer_amd import capi
    want = cone_ref.accumulate(r["value"][:, :, :spp])
    gap = r["gap"][:, :, :spp].any(-1)
    assert gap.sum() <= ccs.GAP_CAP * gap.size
    rays, shadow, occluded = (int(r[k][:, :, :spp].sum()) for k in ("rays", "shadow", "occluded"))
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        ctx.clear_sum()
        info = nee(ctx, name, walk=walk, clamp=0.0, max_depth=depth, sample_count=spp)
        got = ctx.read_sum()
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        print(name, "spp", spp, "depth", depth, "walk", walk, "pixels that differ:", int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()),
              "rays", info["rays"], "shadow", info["shadow_rays"], "occluded", info["shadow_rays_occluded"], "gap pixels", int(gap.sum()), "ms", info["device_ms"])
        same(got[keep], want[keep])
        assert info["paths"] == gap.size * spp and info["rays"] == rays and info["shadow_rays"] == shadow
        if not gap.any():
            assert info["shadow_rays_occluded"] == occluded
        assert info["lights"] == ccs.table_of(name).n


@pytest.mark.parametrize("depth", ccs.DEPTHS)
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", sorted(ccs.CASES))
def test_the_sum_is_exact_with_both_walks(cone_ctx, name, spp, depth):
    put(cone_ctx, name)
    check_nee(cone_ctx, name, ccs.nee_reference(name, depth), spp, depth)


@pytest.mark.parametrize("W,H", ccs.SMALL_SIZES)
def test_small_image_sizes_of_the_render(cone_ctx, W, H):
    put(cone_ctx, "scene.xml", W, H)
    check_nee(cone_ctx, "scene.xml", ccs.nee_reference("scene.xml", 4, W, H), 3, 4)


# ---- identities that need no reference ------------------------------------------------------------------------------------------------
def test_triangle_lights_alone_give_the_area_rules_bits(gpu_ctx):
    """The Cornell box has two triangle lights and no sphere light: CONE output is AREA output, in the direct pass and in the render."""
    from metalpathtracer_amd import capi
    _, buf = ncs.scene_of("cornell.xml")
    u = ncs.uniforms_of("cornell.xml")
    gpu_ctx.upload_scene(*buf)
    gpu_ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    gpu_ctx.set_uniforms(u)
    out = {}
    try:
        for mode in (capi.LIGHT_SAMPLING_AREA, capi.LIGHT_SAMPLING_CONE):
            gpu_ctx.set_light_sampling(mode)
            for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
                d_info = gpu_ctx.direct_lighting(samples=5, seed=SEED, walk=walk)
                direct = gpu_ctx.read_direct()
                gpu_ctx.clear_sum()
                n_info = gpu_ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=3, seed=SEED, walk=walk, clamp=0.0)
                out[mode, walk] = (direct, gpu_ctx.read_sum(), {k: d_info[k] for k in ("rays", "rays_occluded")},
                                   {k: n_info[k] for k in ("paths", "rays", "shadow_rays", "shadow_rays_occluded")})
    finally:
        gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        a, c = out[capi.LIGHT_SAMPLING_AREA, walk], out[capi.LIGHT_SAMPLING_CONE, walk]
        same(a[0][0], c[0][0])
        np.testing.assert_array_equal(a[0][1], c[0][1])
        np.testing.assert_array_equal(a[0][2], c[0][2])
        same(a[1], c[1])
        assert a[2] == c[2] and a[3] == c[3]
        assert a[3]["shadow_rays"] > 0 and a[1][..., :3].any() and a[0][0][..., :3].any()


def test_depth_one_adds_what_mpt_render_adds(cone_ctx):
    from metalpathtracer_amd import capi
    put(cone_ctx, "scene.xml")
    kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=1, sample_begin=2, sample_count=3, seed=SEED)
    cone_ctx.clear_sum()
    cone_ctx.render(**kw)
    want = cone_ctx.read_sum()
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        cone_ctx.clear_sum()
        info = cone_ctx.render_nee(walk=walk, clamp=1.0, **kw)
        same(cone_ctx.read_sum(), want)
        assert info["shadow_rays"] == 0 and info["lights"] == 1
    assert want[..., :3].any()


def outputs(ctx, name):
    """(direct rgba, traced, unoccluded, the render's sum) of a case with the reference-order walk."""
    from metalpathtracer_amd import capi
    ctx.direct_lighting(samples=3, seed=SEED, walk=capi.WALK_REFERENCE)
    d = ctx.read_direct()
    ctx.clear_sum()
    nee(ctx, name, walk=capi.WALK_REFERENCE, clamp=0.0, max_depth=4, sample_count=2)
    return d[0], d[1], d[2], ctx.read_sum()


def test_the_setting(gpu_ctx):
    """The default is AREA; CONE survives mpt_resize, both scene calls and mpt_clear_sum; a bad mode is MPT_ERR_INVALID_ARG and changes
    neither the getter nor the next render; after set(CONE), set(AREA) the output is an untouched context's."""
    from metalpathtracer_amd import capi
    sc, buf = ccs.scene_of("conehand")
    L, h = gpu_ctx.L, gpu_ctx.h
    fresh = capi.Context(0)
    try:
        assert fresh.light_sampling == capi.LIGHT_SAMPLING_AREA
        put(fresh, "conehand")
        untouched = outputs(fresh, "conehand")
        put(gpu_ctx, "conehand")
        assert gpu_ctx.light_sampling == capi.LIGHT_SAMPLING_AREA
        gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_CONE)
        cone = outputs(gpu_ctx, "conehand")
        assert not np.array_equal(cone[0], untouched[0]) and not np.array_equal(cone[3], untouched[3])
        W, H = ccs.CASES["conehand"][:2]
        gpu_ctx.resize(W + 1, H)
        gpu_ctx.resize(W, H)
        gpu_ctx.upload_scene(*buf)
        prims, mats = sc.packed_primitives()
        gpu_ctx.build_and_upload(prims, mats)
        gpu_ctx.clear_sum()
        assert gpu_ctx.light_sampling == capi.LIGHT_SAMPLING_CONE
        put(gpu_ctx, "conehand")
        for mode in (2, -1, 1 << 20):
            assert L.mpt_set_light_sampling(h, mode) == INVALID, mode
            assert b"mpt_set_light_sampling" in L.mpt_last_error(h)
            assert gpu_ctx.light_sampling == capi.LIGHT_SAMPLING_CONE
        assert L.mpt_get_light_sampling(h, None) == INVALID and L.mpt_set_light_sampling(None, 0) == INVALID
        again = outputs(gpu_ctx, "conehand")
        for a, b in zip(cone, again):
            same(a, b)
        gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)
        assert gpu_ctx.light_sampling == capi.LIGHT_SAMPLING_AREA
        for a, b in zip(untouched, outputs(gpu_ctx, "conehand")):
            same(a, b)
    finally:
        gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)
        fresh.close()


def test_a_point_inside_an_emissive_sphere_gets_nothing(cone_ctx):
    """mpt_direct_image on hand-made guides: pixel 0 lies at the centre of an emissive sphere (no sample, nothing traced: as under AREA),
    pixel 1 outside it, facing it (every sample traced and open)."""
    from metalpathtracer_amd import capi, host
    sc = host.Scene()
    sc.addSphere((0.0, 0.0, 0.0), 5.0, emission=(1.0, 1.0, 1.0), emissionPower=2.0)
    sc.addTriangle((-30.0, -20.0, -30.0), (0.0, -19.5, 30.0), (30.0, -20.2, -30.0), albedo=(0.5, 0.5, 0.5))
    sc.buildBVH()
    cone_ctx.upload_scene(*sc.buffers())
    cam = dict(pos=(0.0, 0.0, 20.0), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=0.5)
    u = host.make_uniforms(2, 1, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)
    uu = capi.Uniforms.from_buffer_copy(bytes(u))
    ad = np.array([[[0.8, 0.8, 0.8, 20.0], [0.8, 0.8, 0.8, 5.0]]], np.float32)
    nc = np.array([[[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0]]], np.float32)
    for mode in (capi.LIGHT_SAMPLING_CONE, capi.LIGHT_SAMPLING_AREA):
        cone_ctx.set_light_sampling(mode)
        for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
            rgba, traced, unocc = cone_ctx.direct_image(ad, nc, uu, samples=16, seed=SEED, walk=walk)
            assert (rgba[0, 0] == (0, 0, 0, 1)).all() and traced[0, 0] == 0 and unocc[0, 0] == 0, (mode, walk)
            if mode == capi.LIGHT_SAMPLING_CONE:
                assert traced[0, 1] == 16 and unocc[0, 1] == 16 and (rgba[0, 1, :3] > 0).all()


# ---- the same expectation as the path tracer, and less variance than the area rule ----------------------------------------------------
B, SPP_B, STAT_W, STAT_DEPTH = 64, 64, 32, 4
_stat = {}


def statistics(ctx):
    """Batch means of mpt_render, of mpt_render_nee under CONE and under AREA (clamp = +inf) on the lit box of tests/cone_cases.py —
    a sphere light of emissionPower 1 and albedo 0 inside a closed box, so that mpt_render's per-sample clamp can never bite:
    [B, H, W, 3] each, B = 64 batches of 64 spp, every estimator with seeds of its own (they are independent).  Computed once."""
    from metalpathtracer_amd import capi, host
    if not _stat:
        sc, buf = ccs.scene_of("lit_box")
        mats = np.asarray(buf[2], np.float32).reshape(-1, 2, 4)
        assert (mats[:, 0, :3] <= 1).all() and (mats[:, 1, 3] > 0).sum() == 1
        ctx.upload_scene(*buf)
        ctx.resize(STAT_W, STAT_W)
        ctx.set_uniforms(host.make_uniforms(STAT_W, STAT_W, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=ccs.BOX_CAM))
        assert ctx.light_info() == dict(lights=1, emissive_prims=1, triangle_lights=0, sphere_lights=1)
        out = {k: np.empty((B, STAT_W, STAT_W, 3), np.float64) for k in ("pt", "cone", "area")}
        ms = dict(pt=0.0, cone=0.0, area=0.0)
        try:
            for b in range(B):
                ctx.clear_sum()
                ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=STAT_DEPTH, sample_count=SPP_B, seed=(b, 1))
                ms["pt"] += ctx.stats()["trace_kernel_ms"]
                out["pt"][b] = ctx.read_sum()[..., :3].astype(np.float64) / SPP_B
                for k, mode, s in (("cone", capi.LIGHT_SAMPLING_CONE, 2), ("area", capi.LIGHT_SAMPLING_AREA, 3)):
                    ctx.set_light_sampling(mode)
                    ctx.clear_sum()
                    info = ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=STAT_DEPTH, sample_count=SPP_B, seed=(b, s), walk=capi.WALK_AUTO, clamp=0.0)
                    ms[k] += info["device_ms"]
                    out[k][b] = ctx.read_sum()[..., :3].astype(np.float64) / SPP_B
        finally:
            ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)
        print("trace ms, %d batches of %d spp at %dx%d:" % (B, SPP_B, STAT_W, STAT_W), ms)
        _stat.update(out)
    return _stat["pt"], _stat["cone"], _stat["area"]


def test_cone_sampling_has_the_expectation_of_the_path_tracer(gpu_ctx):
    """The z-statistics and bounds of tests/test_gpu_nee.py.  Per pixel the scalar is the mean of the three channels.
    z = (m_nee - m_pt) / sqrt((s2_nee + s2_pt) / B) over the pixels with a positive variance: |mean z| <= 5 / sqrt(n), mean z^2 <= 1.3;
    the image mean per channel within 5 of its standard errors, and that standard error at most 1 % of the mean."""
    pt, ne, _ = statistics(gpu_ctx)
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
    print("image mean pt", i_pt.mean(0), "nee (cone)", i_ne.mean(0), "standard error", se, "difference in units of it", (i_ne.mean(0) - i_pt.mean(0)) / se,
          "relative", se / i_pt.mean(0))
    assert (np.abs(i_ne.mean(0) - i_pt.mean(0)) <= 5 * se).all()
    assert (se <= 0.01 * i_pt.mean(0)).all()


def test_cone_sampling_has_less_variance_than_area_sampling(gpu_ctx):
    pt, cone, area = statistics(gpu_ctx)
    v_pt, v_cone, v_area = (x.mean(-1).var(0, ddof=1) for x in (pt, cone, area))
    print("summed over the image: s2_area / s2_cone", v_area.sum() / v_cone.sum(), "s2_pt / s2_cone", v_pt.sum() / v_cone.sum(), "s2_pt / s2_area",
          v_pt.sum() / v_area.sum())
    assert v_area.sum() / v_cone.sum() > 1


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------
def run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def test_cli_light_sampling(tmp_path):
    """mpt_render --direct 4 / --nee with --light-sampling cone writes what the host layer gives through the same writer; without the
    flag the files and the JSON keys are what they were; the flag alone is refused."""
    from metalpathtracer_amd import capi, host
    W, H, spp, depth = 48, 32, 4, 4
    base = [EXE, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth), "--seed", "1",
            "--bvh", "reference"]
    p = lambda name: str(tmp_path / name)
    lines = {}
    for key, extra in (("d_cone", ["--out", p("d_cone.ppm"), "--direct", "4", "--light-sampling", "cone"]),
                       ("d_area", ["--out", p("d_area.ppm"), "--direct", "4", "--light-sampling", "area"]),
                       ("d_none", ["--out", p("d_none.ppm"), "--direct", "4"]),
                       ("n_cone", ["--out", p("n_cone.pfm"), "--nee", "--nee-walk", "reference", "--light-sampling", "cone"]),
                       ("n_area", ["--out", p("n_area.pfm"), "--nee", "--nee-walk", "reference", "--light-sampling", "area"]),
                       ("n_none", ["--out", p("n_none.pfm"), "--nee", "--nee-walk", "reference"]),
                       ("plain", ["--out", p("plain.pfm")])):
        r = run(base + extra)
        assert r.returncode == 0, (key, r.stderr[-2000:])
        lines[key] = json.loads(r.stdout.splitlines()[-1])
    assert lines["d_cone"]["direct"]["light_sampling"] == "cone" and lines["d_area"]["direct"]["light_sampling"] == "area"
    assert lines["n_cone"]["nee"]["light_sampling"] == "cone" and lines["n_area"]["nee"]["light_sampling"] == "area"
    assert "light_sampling" not in lines["d_none"]["direct"] and "light_sampling" not in lines["n_none"]["nee"]
    assert "nee" not in lines["plain"] and "direct" not in lines["plain"]
    read = lambda name: open(p(name), "rb").read()
    assert read("d_area.ppm") == read("d_none.ppm") and read("n_area.pfm") == read("n_none.pfm")
    assert read("d_cone.ppm") != read("d_none.ppm") and read("n_cone.pfm") != read("n_none.pfm")
    # the flag alone, or with a value it does not know
    for bad in (["--light-sampling", "cone"], ["--light-sampling", "area"], ["--nee", "--light-sampling", "sphere"], ["--light-sampling", "cone", "--ao", "4"]):
        r = run(base + ["--out", p("x.ppm")] + bad)
        assert r.returncode == 2 and "--light-sampling" in r.stderr, (bad, r.stderr[-500:])
    # the host layer through the same writers
    rr = host.Renderer(0, scene_path("scene.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=depth, seed=(1, 0))
        for mode, d_name, n_name, d_key, n_key in ((capi.LIGHT_SAMPLING_CONE, "d_cone.ppm", "n_cone.pfm", "d_cone", "n_cone"),
                                                   (capi.LIGHT_SAMPLING_AREA, "d_none.ppm", "n_none.pfm", "d_none", "n_none")):
            rr.setLightSampling(mode)
            rgba, info = rr.renderDirectLighting(4)
            for key in ("pixels_surface", "rays", "rays_occluded", "lights"):
                assert lines[d_key]["direct"][key] == info[key], (mode, key)
            assert host.write_ppm(p("mine.ppm"), rgba) == 0
            assert read("mine.ppm") == read(d_name)
            rr.clearSum()
            info = rr.renderNee(spp, depth, walk=capi.WALK_REFERENCE)
            for key in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights"):
                assert lines[n_key]["nee"][key] == info[key], (mode, key)
            assert host.write_pfm(p("mine.pfm"), rr.readSum(), scale=1.0 / spp) == 0
            assert read("mine.pfm") == read(n_name)
        with pytest.raises(Exception):
            rr.setLightSampling(7)
        rr.clearSum()
        rr.renderBatch(0, spp)
        assert host.write_pfm(p("today.pfm"), rr.readSum(), scale=1.0 / spp) == 0
        assert read("today.pfm") == read("plain.pfm")
    finally:
        rr.close()


def test_cli_checkpoints_of_the_two_samplings_do_not_mix(tmp_path):
    """A cone run writes the header MPTNEE2 (its last field the sampling) and two halves give the whole render's file; an area run
    with the flag given keeps MPTNEE1 (tests/test_gpu_nee.py pins it without the flag); neither resumes the other's file, nor does a plain run resume either."""
    W, H, spp, depth = 48, 32, 4, 4
    base = [EXE, "--scene", scene_path("scene.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", str(depth), "--seed", "1",
            "--bvh", "reference"]
    p = lambda name: str(tmp_path / name)
    read = lambda name: open(p(name), "rb").read()
    cone_flags = ["--nee", "--nee-walk", "reference", "--light-sampling", "cone"]
    area_flags = ["--nee", "--nee-walk", "reference"]
    r = run(base + ["--out", p("whole.pfm")] + cone_flags)
    assert r.returncode == 0, r.stderr[-2000:]
    half = list(base)
    half[half.index("--spp") + 1] = str(spp // 2)
    r = run(half + ["--out", p("h.pfm")] + cone_flags + ["--checkpoint", p("cone.ck")])
    assert r.returncode == 0 and read("cone.ck")[:8] == b"MPTNEE2 ", r.stderr[-2000:]
    assert read("cone.ck").split(b"\n", 1)[0].split()[-1] == b"1"
    r = run(half + ["--out", p("resumed.pfm")] + cone_flags + ["--resume", p("cone.ck"), "--checkpoint", p("cone2.ck")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert read("resumed.pfm") == read("whole.pfm")
    r = run(half + ["--out", p("h.pfm")] + area_flags + ["--light-sampling", "area", "--checkpoint", p("area.ck")])
    assert r.returncode == 0 and read("area.ck")[:8] == b"MPTNEE1 ", r.stderr[-2000:]
    for bad in (cone_flags + ["--resume", p("area.ck")], area_flags + ["--resume", p("cone.ck")], area_flags + ["--light-sampling", "area", "--resume", p("cone.ck")],
                ["--resume", p("cone.ck")], ["--resume", p("area.ck")]):
        r = run(half + ["--out", p("h.pfm")] + bad)
        assert r.returncode == 1 and "checkpoint" in r.stderr, (bad, r.stderr[-500:])
