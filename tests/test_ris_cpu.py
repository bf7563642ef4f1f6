"""tests/ris_ref.py (the numpy restatement of mpt_set_light_candidates: resampled light sampling) without a GPU:
  * with M = 1 it picks the sample of tests/direct_ref.py, tests/cone_ref.py and tests/nee_ref.py: directions, tmax and the counts bit for
    bit, the values within 4 ulp (the l * fac / l round trip — the reason m = 1 launches the old kernels);
  * the estimator against closed forms (not against the code under test), in the setup of tests/test_nee_cpu.py: a Lambert point of
    albedo 1 under one triangle light, and under one sphere light (area and cone), in a black enclosure, max_depth = 2, M = 4 — the mean
    of 16384 samples is irradiance / pi within 5 standard errors;
  * the direct pass of `manylights` with M = 8 has the expectation of M = 1 under different seeds (4096 samples; the bounds of
    tests/test_gpu_nee.py: |mean z| <= 5 / sqrt(pixels), mean z^2 <= 1.3) ...
  * ... and less variance: sum var(M = 1) / sum var(M = 8) > 3 at 256 samples with reference-order occlusion.  Measured here: 8.4,
    with 99.96 % of the samples traced against 78 % (the prototype of the rule measured 6.8 with other seeds; a resampler that ignores
    its weights gives 1);
  * the gap shadow rays of the GPU cases touch at most 1 % of each case's pixels, bounce-vertex rays included, for every M of the GPU grid,
    both samplings and max_depth 1, 2 and 4;
  * the setting's entry points refuse a null context or renderer (everything else about the setting needs a context: tests/test_gpu_ris.py)."""
import ctypes as C

import numpy as np
import pytest

import anyhit_ref
import cone_ref
import direct_ref
import nee_ref
import ris_cases as rcs
import ris_ref
from oracle import binding as ob
from test_direct_cpu import sphere_irradiance, triangle_irradiance
from test_nee_cpu import N_MC, SPH_C, SPH_LE, SPH_R, TRI, TRI_LE, closed_form_scene

F = np.float32
ULP = 2.0 ** -23


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def close_in_ulp(a, b, ulps):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) <= ulps * ULP * np.maximum(np.abs(a), np.abs(b))).all()


# ---- M = 1 is the sample of the existing references ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("name", rcs.DIRECT_CASES)
def test_one_candidate_is_the_direct_pass_sample(name, sampling):
    g = rcs.guides(name)
    mod = cone_ref if sampling == rcs.CONE else direct_ref
    o, wi, tmax, contrib, skipped = mod.samples(g["ad"], g["nc"], g["u"], g["table"], 0, rcs.N_MAX, rcs.SEED)
    o1, wi1, tmax1, contrib1, skipped1 = ris_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, rcs.N_MAX, 1, rcs.SEED, cone=sampling == rcs.CONE)
    live = ~skipped
    assert live.any() and (skipped & (g["nc"][..., 3] == 0)[..., None]).any()          # traced and skipped samples both occur
    # (a sample that the M = 1 rule traces is skipped by the resampling rule only if its weight is not in (0, +inf): none here)
    np.testing.assert_array_equal(skipped1, skipped)
    np.testing.assert_array_equal(bits(o1), bits(o))
    np.testing.assert_array_equal(bits(wi1[live]), bits(wi[live]))
    np.testing.assert_array_equal(bits(tmax1[live]), bits(tmax[live]))
    assert close_in_ulp(contrib1[live], contrib[live], 4)
    print(name, sampling, "samples", int(live.sum()), "values that differ in a bit:", int((bits(contrib1[live]) != bits(contrib[live])).any(-1).sum()))


@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("name", ["manylights", "specular", "scene.xml"])
def test_one_candidate_is_the_render_sample(name, sampling):
    _, buf = rcs.scene_of(name)
    u = rcs.uniforms_of(name)
    kw = dict(bsdf_mode=rcs.bsdf_mode(name), max_depth=4, begin=0, count=rcs.SPP_MAX, seed=rcs.SEED)
    mod = cone_ref if sampling == rcs.CONE else nee_ref
    a = mod.render(u, buf, rcs.table_of(name), rcs.first_hit, anyhit_ref.bounds, **kw)
    b = ris_ref.render(u, buf, rcs.table_of(name), rcs.first_hit, anyhit_ref.bounds, 1, cone=sampling == rcs.CONE, **kw)
    for key in ("rays", "shadow", "occluded", "gap", "mis_lights"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["shadow"].sum() > 0
    np.testing.assert_array_equal(bits(a["value"][..., 3]), bits(b["value"][..., 3]))
    assert close_in_ulp(a["value"][..., :3], b["value"][..., :3], 4)                    # (no clamp: a sample's terms are all >= 0)


# ---- the estimator against closed forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,sampling", [("triangle", rcs.AREA), ("sphere", rcs.AREA), ("sphere", rcs.CONE)])
def test_estimator_matches_the_analytic_direct_light(which, sampling):
    buf, u, X, n = closed_form_scene(which)
    table = direct_ref.light_table(buf[1], buf[2])
    assert table.n == 1
    if which == "triangle":
        want = triangle_irradiance(X, n, TRI, TRI_LE) / np.pi
    else:
        want = sphere_irradiance(X, n, SPH_C, SPH_R, SPH_LE) / np.pi
    r = ris_ref.render(u, buf, table, ob.first_hit, anyhit_ref.bounds, 4, cone=sampling == rcs.CONE, max_depth=2, count=N_MC, seed=(78, 2))
    v = r["value"][0, 0].astype(np.float64)
    assert r["rays"].sum() == 2 * N_MC and not r["gap"].any() and r["occluded"].sum() == 0
    mean = v[:, :3].mean(0)
    se = v[:, :3].std(0, ddof=1) / np.sqrt(N_MC)
    print(which, sampling, "analytic", want, "mean", mean, "standard error", se, "in units of it", (mean - want) / se, "shadow rays", int(r["shadow"].sum()))
    assert (se > 0).all() and (np.abs(mean - want) <= 5 * se).all()
    assert r["shadow"].sum() > 0.3 * N_MC


# ---- the direct pass of the many-light case: the same expectation, less variance ---------------------------------------------------------------
def pixel_values(g, sampled, lower):
    """[H, W, N] float64: the per-sample value of every pixel with the reference-order occlusion, the mean of its three channels."""
    _, _, _, contrib, skipped = sampled
    open_ = ~skipped & ~lower
    with np.errstate(all="ignore"):
        rgb = ((g["ad"][..., None, :3] * direct_ref.INV_PI) * contrib).astype(np.float64)
    return np.where(open_, rgb.mean(-1), 0.0)


def many_light_values(M, N, seed):
    g = rcs.guides("manylights")
    if M == 1:
        sampled = direct_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, N, seed)
    else:
        sampled = ris_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, N, M, seed)
    lower, upper = direct_ref.occlusion_bounds(sampled, g["buf"], anyhit_ref.bounds)
    skipped = sampled[4]
    surface = g["nc"][..., 3] == 0
    return pixel_values(g, sampled, lower), float((~skipped).sum()) / (surface.sum() * N), int((upper & ~lower).sum())


def test_eight_candidates_have_the_expectation_of_one():
    """Over the 99 lit pixels of the case mean z^2 has a standard deviation of about sqrt(2 / 99) = 0.14 under the null, so the bound
    1.3 sits two of them above 1: measured over 16 pairs of seeds, M = 1 against M = 8 gave 0.76 .. 1.39 with a mean of 1.02, and M = 8
    against M = 8 (the null itself) 0.86 .. 1.41; mean z stayed within +-0.15 of 0 (bound 0.50).  The seeds below are fixed."""
    N = 4096
    v1, _, _ = many_light_values(1, N, (1000, 1))
    v8, _, _ = many_light_values(8, N, (8000, 1))
    m1, m8 = v1.mean(-1), v8.mean(-1)
    s1, s8 = v1.var(-1, ddof=1), v8.var(-1, ddof=1)
    lit = (s1 > 0) | (s8 > 0)
    assert lit.sum() > lit.size // 2
    np.testing.assert_array_equal(m8[~lit], m1[~lit])
    z = (m8 - m1)[lit] / np.sqrt((s8 + s1)[lit] / N)
    print("pixels:", z.size, "mean z:", z.mean(), "bound", 5 / np.sqrt(z.size), "mean z^2:", (z * z).mean(), "max |z|:", np.abs(z).max(),
          "image means", m1.mean(), m8.mean())
    assert abs(z.mean()) <= 5 / np.sqrt(z.size)
    assert (z * z).mean() <= 1.3


def test_eight_candidates_have_less_variance_than_one():
    N = 256
    v1, traced1, gap1 = many_light_values(1, N, rcs.SEED)
    v8, traced8, gap8 = many_light_values(8, N, rcs.SEED)
    ratio = v1.var(-1, ddof=1).sum() / v8.var(-1, ddof=1).sum()
    print("sum var(M=1) / sum var(M=8):", ratio, "traced fraction", traced1, traced8, "gap rays", gap1, gap8)
    assert traced8 > traced1
    assert ratio > 3


# ---- the gap rays of the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("name", rcs.DIRECT_CASES)
def test_direct_gap_rays_touch_at_most_one_percent_of_the_pixels(name, sampling):
    sizes = [(None, None, M) for M in rcs.DIRECT_MS] + [(W, H, rcs.SMALL_M) for W, H in rcs.SMALL_SIZES]
    for W, H, M in sizes:
        r = rcs.direct_reference(name, M, sampling, W, H)
        skipped = r["sampled"][4]
        gap = (r["upper"] & ~r["lower"]).any(-1)
        print(name, sampling, (W, H), "M", M, "samples", int((~skipped).sum()), "occluded", int(r["lower"].sum()), "pixels with a gap ray", int(gap.sum()))
        assert gap.sum() <= rcs.GAP_CAP * gap.size
        if W is None:
            assert r["lower"].any() and (~skipped & ~r["lower"]).any()        # occluded and open samples both occur


@pytest.mark.parametrize("depth", rcs.DEPTHS)
@pytest.mark.parametrize("sampling", rcs.SAMPLINGS)
@pytest.mark.parametrize("name", rcs.NEE_CASES)
def test_nee_gap_rays_touch_at_most_one_percent_of_the_pixels(name, sampling, depth):
    sizes = [(None, None, M) for M in rcs.nee_ms(name)] + ([(W, H, rcs.SMALL_M) for W, H in rcs.SMALL_SIZES] if depth == 4 else [])
    for W, H, M in sizes:
        r = rcs.nee_reference(name, depth, M, sampling, W, H)
        gap = r["gap"].any(-1)
        print(name, sampling, (W, H), "M", M, "depth", depth, "rays", int(r["rays"].sum()), "shadow rays", int(r["shadow"].sum()), "occluded",
              int(r["occluded"].sum()), "pixels with a gap ray", int(gap.sum()))
        assert gap.sum() <= rcs.GAP_CAP * gap.size
        assert (r["occluded"] <= r["shadow"]).all() and (r["shadow"] <= r["rays"]).all()
        if depth == 1:
            assert r["shadow"].sum() == 0
        elif W is None:
            assert r["shadow"].sum() > r["occluded"].sum() > 0


# ---- the setting without a device -----------------------------------------------------------------------------------------------------------
def test_the_setting_refuses_a_null_context_or_renderer():
    from metalpathtracer_amd import capi, host
    L, Lh = capi.load(), host.load()
    m = C.c_uint32(7)
    assert capi.LIGHT_CANDIDATES_MAX == ris_ref.M_MAX == 32
    assert L.mpt_set_light_candidates(None, 4) == 1                  # MPT_ERR_INVALID_ARG, no crash
    assert L.mpt_get_light_candidates(None, C.byref(m)) == 1 and m.value == 7
    assert Lh.mpt_renderer_set_light_candidates(None, 4) == 1
    assert Lh.mpt_renderer_get_light_candidates(None, C.byref(m)) == 1 and m.value == 7
