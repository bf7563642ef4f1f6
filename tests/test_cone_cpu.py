"""tests/cone_ref.py (the numpy restatement of MPT_LIGHT_SAMPLING_CONE, include/mpt.h) without a GPU:
  * the estimator against the closed form pi Le (r / D)^2 cos(theta) of a sphere wholly above the horizon of a Lambert point (not against
    the code under test), at D = 1.1 r, D = 100 r and one geometry in between: the mean of 16384 samples of the restated direct pass, and
    of the restated mpt_render_nee at max_depth = 2 inside a black enclosure, within 5 standard errors of those same samples — the bound
    tests/test_direct_cpu.py and tests/test_nee_cpu.py hold the area rule to;
  * a point whose horizon cuts the sphere (no closed form used): the cone mean and the area mean within 5 combined standard errors;
  * every direction drawn meets the sphere in float64, and dist is the near intersection within 2^-11 relative for points at least
    1e-3 r from the surface;
  * at each closed-form geometry the cone's sample variance is below the area's;
  * the two MIS weights of one direction and origin sum to 1 within 4 ulp of 1;
  * the gap shadow rays of the GPU cases (tests/anyhit_ref.py: rays the own-tree walk may answer either way) touch at most 1 % of each
    case's pixels."""
import numpy as np
import pytest

import anyhit_ref
import cone_cases as ccs
import cone_ref
import direct_ref
from oracle import binding as ob
from test_direct_cpu import sphere_irradiance
from test_nee_cpu import ENCLOSURE, FLOOR

F = np.float32
N_MC = 16384
LE = (0.5, 1.5, 4.0)
CAM_POS = np.array([0.0, 2.0, 12.0])      # low over the floor: a sphere 1.1 r above the point it looks at does not hide that point
# (r, D / r, the angle between the normal and the direction to the centre in degrees): all wholly above the horizon, D cos(theta) >= r
GEOMETRIES = {"D=1.1r": (1.0, 1.1, 0.0), "D=6r": (0.75, 6.0, 35.0), "D=100r": (0.2, 100.0, 60.0)}


def floor_point():
    """(X, n) in float64: the floor point the camera looks at and the floor's normal facing the camera."""
    fl = FLOOR.astype(np.float64)
    n = np.cross(fl[1] - fl[0], fl[2] - fl[0])
    n /= np.linalg.norm(n)
    target = np.array([0.3, 0.0, -0.2])
    fwd = (target - CAM_POS) / np.linalg.norm(target - CAM_POS)
    X = CAM_POS + np.dot(fl[0] - CAM_POS, n) / np.dot(fwd, n) * fwd
    return X, (-n if np.dot(n, fwd) > 0 else n), fwd


def sphere_of(geometry):
    """(centre float32, r) of a geometry over the floor point: the centre at distance D, tilted by the angle towards -x."""
    r, ratio, deg = geometry
    X, n, _ = floor_point()
    side = np.cross(n, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    a = np.radians(deg)
    c = (X + (r * ratio) * (np.cos(a) * n + np.sin(a) * side)).astype(np.float32)
    return c, r


def one_light_table(c, r):
    prims = np.array([[[*c, 0], [r, 0, 0, 0], [0, 0, 0, 0]]], np.float32)
    mats = np.array([[[0, 0, 0, 0], [*LE, 1.0]]], np.float32)
    return direct_ref.light_table(prims, mats)


def direct_samples(module, c, r, seed=(77, 1), N=N_MC):
    """The N per-sample contributions (float64, a skipped sample 0) of module.sample_lights at the floor point."""
    X, n, _ = floor_point()
    _, _, contrib, valid = module.sample_lights(X.astype(np.float32), n.astype(np.float32), np.uint32(5), one_light_table(c, r), 0, N, seed=seed)
    return np.where(valid[:, None], contrib, 0).astype(np.float64), valid


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_direct_estimator_matches_the_closed_form_with_less_variance_than_the_area_rule(name):
    c, r = sphere_of(GEOMETRIES[name])
    X, n, _ = floor_point()
    want = sphere_irradiance(X.astype(np.float32), n.astype(np.float32), c, r, LE)
    cone, valid = direct_samples(cone_ref, c, r)
    area, _ = direct_samples(direct_ref, c, r)
    mean, se = cone.mean(0), cone.std(0, ddof=1) / np.sqrt(N_MC)
    print(name, "analytic", want, "cone mean", mean, "standard error", se, "in units of it", (mean - want) / se, "skipped", int((~valid).sum()),
          "area mean", area.mean(0), "variance area / cone", area.var(0, ddof=1) / cone.var(0, ddof=1))
    assert valid.all()                                                   # the whole cone is above the horizon: nothing is skipped
    assert (se > 0).all() and (np.abs(mean - want) <= 5 * se).all()
    assert (cone.var(0, ddof=1) < area.var(0, ddof=1)).all()


def closed_form_scene(c, r):
    """(buffers, uniforms): the sphere light, the floor of albedo 1 and the black enclosure of tests/test_nee_cpu.py; a 1 x 1 image whose
    pixel is 0.02 degrees wide and looks at the floor point."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    sc.addSphere(tuple(float(x) for x in c), float(r), albedo=(0.0, 0.0, 0.0), emission=LE, emissionPower=1.0)
    sc.addTriangle(*map(tuple, FLOOR), albedo=(1.0, 1.0, 1.0))
    for a, b, d in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        sc.addTriangle(tuple(ENCLOSURE[a]), tuple(ENCLOSURE[b]), tuple(ENCLOSURE[d]), albedo=(0.0, 0.0, 0.0))
    sc.buildBVH()
    _, _, fwd = floor_point()
    cam = dict(pos=tuple(CAM_POS), fwd=tuple(fwd), up=(0.0, 1.0, 0.0), vfov=0.02)
    return sc.buffers(), host.make_uniforms(1, 1, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_nee_estimator_matches_the_closed_form(name):
    c, r = sphere_of(GEOMETRIES[name])
    buf, u = closed_form_scene(c, r)
    table = direct_ref.light_table(buf[1], buf[2])
    assert table.n == 1
    X, n, _ = floor_point()
    want = sphere_irradiance(X.astype(np.float32), n.astype(np.float32), c, r, LE) / np.pi
    res = cone_ref.render(u, buf, table, ob.first_hit, anyhit_ref.bounds, max_depth=2, count=N_MC, seed=(77, 1))
    v = res["value"][0, 0].astype(np.float64)
    found = v[:, 3] == 1                                                 # alpha = the power of the light a bounce found (the enclosure hides the sky)
    assert ((v[:, 3] == 0) | found).all()                                # (at D = 100 r a bounce finds the light once in 20000 tries)
    assert res["rays"].sum() == 2 * N_MC and not res["gap"].any() and res["occluded"].sum() == 0
    assert res["shadow"].sum() == N_MC                                   # every vertex draws a sample and none is skipped
    mean, se = v[:, :3].mean(0), v[:, :3].std(0, ddof=1) / np.sqrt(N_MC)
    print(name, "analytic", want, "mean", mean, "standard error", se, "in units of it", (mean - want) / se, "bounces that found the light", int(found.sum()))
    assert (se > 0).all() and (np.abs(mean - want) <= 5 * se).all()


def test_a_horizon_that_cuts_the_sphere_gives_the_area_rules_mean():
    """D cos(theta) = 0.3 r: part of the cone lies below the horizon and is skipped by cos_s <= 0.  No closed form: the area rule, which
    tests/test_direct_cpu.py holds to its own, is the other estimator of the same integral (independent samples: another seed)."""
    c, r = sphere_of((1.0, 3.0, np.degrees(np.arccos(0.1))))
    cone, valid = direct_samples(cone_ref, c, r, seed=(77, 1))
    area, _ = direct_samples(direct_ref, c, r, seed=(78, 1))
    assert 0.05 < (~valid).mean() < 0.95
    d = cone.mean(0) - area.mean(0)
    se = np.sqrt((cone.var(0, ddof=1) + area.var(0, ddof=1)) / N_MC)
    print("cone mean", cone.mean(0), "area mean", area.mean(0), "difference in combined standard errors", d / se, "cone samples below the horizon",
          int((~valid).sum()))
    assert (se > 0).all() and (np.abs(d) <= 5 * se).all()


def random_geometry(n, rng, gap_lo=1e-3, gap_hi=1e2):
    """n shading points o outside spheres (c, r): r over three decades, the distance to the surface from gap_lo r to gap_hi r."""
    r = np.exp(rng.uniform(np.log(0.1), np.log(100.0), n))
    gap = np.exp(rng.uniform(np.log(gap_lo), np.log(gap_hi), n)) * r
    c = rng.uniform(-50.0, 50.0, (n, 3))
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = c + (r + gap)[:, None] * v
    return o.astype(np.float32), c.astype(np.float32), r.astype(np.float32)


def test_every_direction_meets_the_sphere_and_dist_is_the_near_intersection():
    rng = np.random.default_rng(20261019)
    n = 200000
    o, c, r = random_geometry(n, rng)
    u1, u2 = rng.random(n, np.float32), rng.random(n, np.float32)
    with np.errstate(all="ignore"):
        w = c - o
        dc2, omc, J, outside = cone_ref.cone_cap(w, r, F(1))
        wi, dist = cone_ref.cone_sample(w, dc2, omc, u1, u2)
    assert wi.dtype == np.float32 and dist.dtype == np.float32
    # float64: the float32 centre, radius, origin and direction as they are; the ray o + t wi / |wi|
    o64, c64, r64, d64 = o.astype(np.float64), c.astype(np.float64), r.astype(np.float64), wi.astype(np.float64)
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    w64 = c64 - o64
    far_enough = np.linalg.norm(w64, axis=1) - r64 >= 1e-3 * r64          # (the float32 rounding of o moved a few points closer)
    assert outside.all() and far_enough.mean() > 0.99
    b = (w64 * d64).sum(1)
    disc = b * b - ((w64 * w64).sum(1) - r64 * r64)
    print("directions", n, "that miss the sphere in float64:", int((disc < 0).sum()), "smallest discriminant / r^2", (disc / (r64 * r64)).min(),
          "|wi| - 1 at most", np.abs(np.linalg.norm(wi.astype(np.float64), axis=1) - 1).max())
    assert (disc >= 0).all()
    t = b - np.sqrt(disc)
    rel = np.abs(dist.astype(np.float64) - t) / t
    print("dist against the exact near root, relative: max", rel[far_enough].max(), "bound", 2.0 ** -11, "99.9 %", np.quantile(rel[far_enough], 0.999))
    assert (t > 0).all() and (dist > 0).all()
    assert rel[far_enough].max() <= 2.0 ** -11


def test_mis_weights_of_one_direction_and_origin_sum_to_one():
    rng = np.random.default_rng(20261020)
    n = 200000
    o, c, r = random_geometry(n, rng, 1e-3, 1e3)
    inv_pdf = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n)).astype(np.float32)
    cos_s = rng.uniform(1e-3, 1.0, n).astype(np.float32)
    with np.errstate(all="ignore"):
        _, _, J, outside = cone_ref.cone_cap(c - o, r, inv_pdf)
        wl, _ = cone_ref.light_weight(cos_s, J)
        # the same direction met by the bounce from the same origin: the bounce's pdf is the cosine pdf at cos_s
        w = cone_ref.bsdf_weight(o, c, r, inv_pdf, cos_s * direct_ref.INV_PI)
    assert outside.all() and wl.dtype == np.float32 and w.dtype == np.float32
    err = np.abs((wl.astype(np.float64) + w.astype(np.float64)) - 1.0) / 2.0 ** -23
    print("largest |wl + w - 1| in ulp of 1:", err.max(), "mean:", err.mean(), "wl range", wl.min(), wl.max())
    assert wl.min() < 0.01 and wl.max() > 0.99                           # both techniques dominate somewhere
    assert err.max() <= 4.0


def test_a_point_inside_or_on_the_sphere_is_skipped_and_the_bounce_counts_in_full():
    c, r = np.array([[1.0, 2.0, 3.0]] * 3, np.float32), np.full(3, 2.0, np.float32)
    o = np.array([[1.0, 2.0, 3.0], [1.0, 2.5, 3.0], [1.0, 4.0, 3.0]], np.float32)      # the centre, inside, on the surface
    n = np.array([[0.0, 1.0, 0.0]] * 3, np.float32)
    with np.errstate(all="ignore"):
        _, _, _, _, valid = cone_ref.sphere_sample(o, n, c, r, np.full(3, 5.0, np.float32), np.full(3, 0.25, np.float32), np.full(3, 0.5, np.float32))
        w = cone_ref.bsdf_weight(o, c, r, np.full(3, 5.0, np.float32), np.full(3, 0.2, np.float32))
    assert not valid.any() and (w == 1).all()


# ---- the gap rays of the GPU cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None] + list(ccs.SMALL_SIZES))
@pytest.mark.parametrize("name", ccs.DIRECT_CASES)
def test_direct_gap_rays_touch_at_most_one_percent_of_the_pixels(name, size):
    W, H = size or (None, None)
    ref = ccs.direct_reference(name, W, H)
    surface = ref["nc"][..., 3] == 0
    skipped, lower, upper = ref["sampled"][4], ref["lower"], ref["upper"]
    gap = (upper & ~lower).any(-1)
    sphere_lights = int((ref["table"].rec[:, 0, 3] == 0).sum())
    print(name, size, "surface pixels", int(surface.sum()), "samples", int((~skipped).sum()), "skipped", int((skipped & surface[..., None]).sum()),
          "occluded (reference order)", int(lower.sum()), "pixels with a gap ray", int(gap.sum()), "sphere lights", sphere_lights)
    assert sphere_lights >= 1 and not (lower & ~upper).any() and not (lower & skipped).any()
    assert gap.sum() <= ccs.GAP_CAP * gap.size
    if size is None:                                                     # the cases are worth running: occluded and open samples both occur
        assert surface.any() and lower.any() and (~skipped & ~upper).any()


@pytest.mark.parametrize("depth", ccs.DEPTHS)
@pytest.mark.parametrize("name", sorted(ccs.CASES))
def test_nee_gap_rays_touch_at_most_one_percent_of_the_pixels(name, depth):
    ref = ccs.nee_reference(name, depth)
    gap = ref["gap"].any(-1)
    print(name, "depth", depth, "pixels", gap.size, "rays", int(ref["rays"].sum()), "shadow rays", int(ref["shadow"].sum()), "occluded (reference order)",
          int(ref["occluded"].sum()), "pixels with a gap ray", int(gap.sum()), "lights weighted after a bounce found them", ref["mis_lights"])
    assert gap.sum() <= ccs.GAP_CAP * gap.size
    assert (ref["occluded"] <= ref["shadow"]).all() and (ref["shadow"] <= ref["rays"]).all()
    if depth == 1:
        assert ref["shadow"].sum() == 0
    else:
        assert ref["occluded"].sum() > 0 and (ref["shadow"] > ref["occluded"]).any()
    if depth == 4 and name != "specular":                                # a bounce found the sphere light (table index 0) after a light sample
        assert ccs.table_of(name).rec[0, 0, 3] == 0 and 0 in ref["mis_lights"]


@pytest.mark.parametrize("size", ccs.SMALL_SIZES)
def test_nee_gap_rays_of_the_small_sizes(size):
    ref = ccs.nee_reference("scene.xml", 4, *size)
    assert ref["gap"].any(-1).sum() <= ccs.GAP_CAP * ref["gap"].any(-1).size
