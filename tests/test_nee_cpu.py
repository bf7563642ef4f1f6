"""tests/nee_ref.py (the numpy restatement of mpt_render_nee's estimator) without a GPU:
  * the two MIS weights of one geometry — the light sample's wl and the weight w of the same light found by the bounce — sum to 1 within
    4 ulp of 1 (4 * 2^-23);
  * the estimator against closed forms (not against the code under test): a Lambert point of albedo 1 under one triangle light, and under
    one sphere light, inside a black enclosure (no sky), max_depth = 2 — the mean of 16384 reference samples (light sample + the
    emission the bounce finds) is irradiance / pi within 5 standard errors of those same samples;
  * the gap shadow rays of the GPU cases (upper & ~lower of tests/anyhit_ref.py: rays the own-tree walk may answer either way) touch at
    most 1 % of each case's pixels, bounce-vertex rays included."""
import numpy as np
import pytest

import anyhit_ref
import direct_ref
import nee_cases as ncs
import nee_ref
from oracle import binding as ob
from test_direct_cpu import sphere_irradiance, triangle_irradiance

F = np.float32


def test_mis_weights_of_one_geometry_sum_to_one():
    rng = np.random.default_rng(20261019)
    n = 200000
    cos_s = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    cos_l = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    d2 = np.exp(rng.uniform(np.log(1e-2), np.log(1e4), n)).astype(np.float32)
    inv_pdf = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)).astype(np.float32)
    wl, _ = nee_ref.light_weight(cos_s, cos_l, d2, inv_pdf)
    # the same geometry met by the bounce: t = the distance, the bounce's pdf = the cosine pdf at cos_s
    w = nee_ref.bsdf_weight(np.sqrt(d2), cos_l, inv_pdf, cos_s * direct_ref.INV_PI)
    assert wl.dtype == np.float32 and w.dtype == np.float32
    err = np.abs((wl.astype(np.float64) + w.astype(np.float64)) - 1.0) / 2.0 ** -23
    print("largest |wl + w - 1| in ulp of 1:", err.max(), "mean:", err.mean(), "wl range", wl.min(), wl.max())
    assert wl.min() < 0.01 and wl.max() > 0.99                       # both techniques dominate somewhere
    assert err.max() <= 4.0


# ---- the estimator against closed forms -----------------------------------------------------------------------------------------------
N_MC = 16384
CAM_POS = np.array([0.0, 5.0, 8.0])
FLOOR = np.array([[-9.0, -0.4, -9.0], [0.0, 0.3, 12.0], [9.0, 0.1, -9.0]], np.float32)      # (not flat: a flat leaf box is never hit)
TRI = np.array([[-1.0, 3.0, -0.5], [1.5, 2.5, 0.0], [0.2, 3.5, 1.8]], np.float32)
TRI_LE = (3.0, 2.0, 1.0)
SPH_C, SPH_R = np.array([1.0, 4.0, 2.0], np.float32), 0.75
SPH_LE = (0.5, 1.5, 4.0)
S = 60.0
ENCLOSURE = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * F(S)     # a tetrahedron, inradius 34: black walls


def closed_form_scene(which):
    """(buffers, uniforms, X, n): the light, the floor and the black enclosure; a 1 x 1 image whose pixel is 0.02 degrees wide and looks
    at the floor point X (float64) with the normal n facing the camera."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    if which == "sphere":
        sc.addSphere(tuple(SPH_C), SPH_R, albedo=(0.0, 0.0, 0.0), emission=SPH_LE, emissionPower=1.0)
    else:
        sc.addTriangle(*map(tuple, TRI), albedo=(0.0, 0.0, 0.0), emission=TRI_LE, emissionPower=1.0)
    sc.addTriangle(*map(tuple, FLOOR), albedo=(1.0, 1.0, 1.0))
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        sc.addTriangle(tuple(ENCLOSURE[a]), tuple(ENCLOSURE[b]), tuple(ENCLOSURE[c]), albedo=(0.0, 0.0, 0.0))
    sc.buildBVH()
    fl = FLOOR.astype(np.float64)
    n = np.cross(fl[1] - fl[0], fl[2] - fl[0])
    n /= np.linalg.norm(n)
    target = np.array([0.3, 0.0, -0.2])
    fwd = (target - CAM_POS) / np.linalg.norm(target - CAM_POS)
    t = np.dot(fl[0] - CAM_POS, n) / np.dot(fwd, n)
    X = CAM_POS + t * fwd
    if np.dot(n, fwd) > 0:
        n = -n
    cam = dict(pos=tuple(CAM_POS), fwd=tuple(fwd), up=(0.0, 1.0, 0.0), vfov=0.02)
    u = host.make_uniforms(1, 1, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)
    return sc.buffers(), u, X, n


@pytest.mark.parametrize("which", ["triangle", "sphere"])
def test_estimator_matches_the_analytic_direct_light(which):
    buf, u, X, n = closed_form_scene(which)
    table = direct_ref.light_table(buf[1], buf[2])
    assert table.n == 1
    if which == "triangle":
        assert ((TRI.astype(np.float64) - X) @ n > 0).all()
        want = triangle_irradiance(X, n, TRI, TRI_LE) / np.pi
    else:
        want = sphere_irradiance(X, n, SPH_C, SPH_R, SPH_LE) / np.pi
    r = nee_ref.render(u, buf, table, ob.first_hit, anyhit_ref.bounds, max_depth=2, count=N_MC, seed=(77, 1))
    v = r["value"][0, 0].astype(np.float64)
    found = v[:, 3] == 1                                             # alpha = the power of the light a bounce found (the enclosure hides the sky)
    assert ((v[:, 3] == 0) | found).all() and 0 < found.mean() < 0.5
    assert r["rays"].sum() == 2 * N_MC and not r["gap"].any() and r["occluded"].sum() == 0
    mean = v[:, :3].mean(0)
    se = v[:, :3].std(0, ddof=1) / np.sqrt(N_MC)
    print(which, "analytic", want, "mean", mean, "standard error", se, "in units of it", (mean - want) / se, "shadow rays", int(r["shadow"].sum()))
    assert (se > 0).all() and (np.abs(mean - want) <= 5 * se).all()
    # the light sample alone and the bounce alone would each be an estimator: the mean above has both parts
    assert r["shadow"].sum() > 0.3 * N_MC


# ---- the gap rays of the GPU cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", ncs.DEPTHS)
@pytest.mark.parametrize("name", sorted(ncs.CASES))
def test_gap_rays_touch_at_most_one_percent_of_the_pixels(name, depth):
    r = ncs.reference(name, depth)
    gap = r["gap"].any(-1)
    print(name, "depth", depth, "pixels", gap.size, "rays", int(r["rays"].sum()), "shadow rays", int(r["shadow"].sum()), "occluded (reference order)",
          int(r["occluded"].sum()), "pixels with a gap ray", int(gap.sum()))
    assert gap.sum() <= ncs.GAP_CAP * gap.size
    assert (r["occluded"] <= r["shadow"]).all() and (r["shadow"] <= r["rays"]).all()
    if depth == 1 or name == "dark":
        assert r["shadow"].sum() == 0
    else:
        assert r["occluded"].sum() > 0 and (r["shadow"] > r["occluded"]).any()


def test_the_many_light_case_weights_emitters_all_over_its_table():
    """The case that pins the search of an emitter's id: thirteen lights (no power of two) whose caller ids have gaps, and bounces that
    find, after a light sample, the sphere light, the last light and at least half of the table."""
    t = ncs.table_of("manylights")
    assert t.n == 13 and (np.diff(t.ids) == 2).all() and t.rec[0, 0, 3] == 0 and (t.rec[1:, 0, 3] == 1).all()
    found = ncs.reference("manylights", 4)["mis_lights"]
    print("lights weighted after a bounce found them:", found)
    assert 0 in found and t.n - 1 in found and found.size >= 7
