"""tests/direct_ref.py (the numpy restatement of the light table and of the direct-lighting pass) without a GPU:
  * the table on Cornell, scene.xml and the hand-made scene of tests/direct_cases.py: ids ascending, cdf non-decreasing and ending in
    exactly 1, inv_pdf * pmf = area to float32 rounding, and the hand-made scene's four lights;
  * the estimator against closed forms (not against the code under test): the mean of 16384 per-sample contributions at a point that
    sees all of the light is the analytic irradiance, within 5 standard errors of those same contributions;
  * the gap rays of the GPU cases (the samples the own-tree walk may answer either way) touch at most 1 % of the surface pixels."""
import numpy as np
import pytest

import direct_cases as dcs
import direct_ref as dr

F = np.float32


@pytest.mark.parametrize("name", ["cornell.xml", "scene.xml", "handmade", "dark"])
def test_light_table(name):
    _, buf = dcs.scene_of(name)
    t = dr.light_table(buf[1], buf[2])
    mats = np.asarray(buf[2]).reshape(-1, 2, 4)
    print(name, "lights", t.n, "emissive primitives", t.seen, "ids", t.ids[:8], "cdf", t.cdf[:8])
    assert t.seen == (mats[:, 1, 3] > 0).sum()
    if name == "dark":
        assert t.n == 0 and t.seen == 0
        return
    assert t.n > 0 and (np.diff(t.ids) > 0).all() and (mats[t.ids, 1, 3] > 0).all()
    assert (np.diff(t.cdf) >= 0).all() and t.cdf[-1] == F(1) and t.cdf[0] > 0
    assert t.rec.dtype == np.float32 and t.cdf.dtype == np.float32
    # inv_pdf = A / pmf: one rounding of the float64 quotient to float32 (2^-24 relative), and the product with pmf one more in float64
    np.testing.assert_allclose(t.rec[:, 3, 3].astype(np.float64) * t.pmf, t.A, rtol=2.0 ** -23)
    np.testing.assert_allclose(t.pmf.sum(), 1.0, rtol=1e-12)
    Le = mats[t.ids, 1, :3] * mats[t.ids, 1, 3:4]
    np.testing.assert_array_equal(t.rec[:, 3, :3].view(np.uint32), Le.astype(np.float32).view(np.uint32))
    if name == "handmade":
        assert t.n == 4 and t.seen == 6
        np.testing.assert_array_equal(t.ids, [0, 1, 3, 4])
        np.testing.assert_array_equal(t.rec[:, 0, 3], [0, 0, 1, 1])
        np.testing.assert_allclose(t.A[:2], [4 * np.pi * 0.25, 4 * np.pi], rtol=1e-12)
        assert not (t.rec[0, 3, :3] == t.rec[1, 3, :3]).any()
    if name == "cornell.xml":
        assert t.n == 2 and (t.rec[:, 0, 3] == 1).all()          # the two ceiling triangles


# ---- the estimator against closed forms -----------------------------------------------------------------------------------------
N_MC = 16384
X = np.array([0.3, 0.1, -0.2], np.float32)
NRM = np.array([0.0, 1.0, 0.0], np.float32)
TRI = np.array([[-1.0, 3.0, -0.5], [1.5, 2.5, 0.0], [0.2, 3.5, 1.8]], np.float32)      # wholly above the horizon of X
TRI_LE = (3.0, 2.0, 1.0)
SPH_C, SPH_R = np.array([1.0, 4.0, 2.0], np.float32), 0.75
SPH_LE = (0.5, 1.5, 4.0)


def table_of(tri=False, sphere=False):
    prims, mats = [], []
    if sphere:
        prims.append([[*SPH_C, 0], [SPH_R, 0, 0, 0], [0, 0, 0, 0]])
        mats.append([[0, 0, 0, 0], [*SPH_LE, 1.0]])
    if tri:
        prims.append([[*TRI[0], 1], [*TRI[1], 0], [*TRI[2], 0]])
        mats.append([[0, 0, 0, 0], [*TRI_LE, 1.0]])
    return dr.light_table(np.array(prims, np.float32), np.array(mats, np.float32))


def triangle_irradiance(x, n, tri, Le):
    """Le * 1/2 * |sum_i theta_i (n . Gamma_i)| (Lambert's formula for a polygon wholly above the horizon), in float64."""
    r = tri.astype(np.float64) - x.astype(np.float64)
    total = 0.0
    for i in range(3):
        a, b = r[i], r[(i + 1) % 3]
        theta = np.arccos(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
        g = np.cross(a, b)
        total += theta * np.dot(n.astype(np.float64), g / np.linalg.norm(g))
    return np.array(Le, np.float64) * 0.5 * abs(total)


def sphere_irradiance(x, n, c, r, Le):
    """Le * pi (r / D)^2 cos(theta) for a sphere wholly above the horizon (D cos(theta) >= r), in float64."""
    v = c.astype(np.float64) - x.astype(np.float64)
    D = np.linalg.norm(v)
    cos_t = np.dot(n.astype(np.float64), v) / D
    assert D * cos_t >= r
    return np.array(Le, np.float64) * np.pi * (r / D) ** 2 * cos_t


@pytest.mark.parametrize("which", ["triangle", "sphere", "both"])
def test_estimator_matches_the_analytic_irradiance(which):
    tri, sph = which in ("triangle", "both"), which in ("sphere", "both")
    t = table_of(tri=tri, sphere=sph)
    assert t.n == int(tri) + int(sph)
    assert ((TRI - X) @ NRM > 0).all()
    want = np.zeros(3)
    if tri:
        want += triangle_irradiance(X, NRM, TRI, TRI_LE)
    if sph:
        want += sphere_irradiance(X, NRM, SPH_C, SPH_R, SPH_LE)
    _, _, contrib, valid = dr.sample_lights(X, NRM, np.uint32(5), t, 0, N_MC, seed=(77, 1))
    c = np.where(valid[:, None], contrib, 0).astype(np.float64)      # a skipped sample adds nothing (the far side of the sphere)
    mean = c.mean(0)
    se = c.std(0, ddof=1) / np.sqrt(N_MC)
    print(which, "analytic", want, "mean", mean, "standard error", se, "in units of it", (mean - want) / se, "skipped", int((~valid).sum()))
    assert (se > 0).all() and (np.abs(mean - want) <= 5 * se).all()
    if sph and not tri:
        assert 0.3 < (~valid).mean() < 0.7                            # about half of a sphere faces away
    if tri and not sph:
        assert valid.all()


# ---- the gap rays of the GPU cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene.xml", "cornell.xml", "handmade"])
def test_gap_rays_touch_at_most_one_percent_of_the_surface_pixels(name):
    r = dcs.reference(name)
    surface = r["nc"][..., 3] == 0
    o, wi, tmax, contrib, skipped = r["sampled"]
    lower, upper = r["lower"], r["upper"]
    gap = dcs.gap_pixels(r)
    live = ~skipped
    print(name, "surface pixels", int(surface.sum()), "samples", int(live.sum()), "skipped", int((skipped & surface[..., None]).sum()),
          "occluded (reference order)", int(lower.sum()), "gap rays", int((upper & ~lower).sum()), "pixels with a gap ray", int(gap.sum()))
    assert surface.any() and not (lower & ~upper).any() and not (lower & skipped).any()
    assert gap.sum() <= dcs.GAP_CAP * surface.sum()
    # the cases are worth running: occluded, open and skipped samples all occur among the first 16
    l16, s16 = lower[..., :16], skipped[..., :16] & surface[..., None]
    assert l16.any() and (live[..., :16] & ~upper[..., :16]).any() and s16.any()
