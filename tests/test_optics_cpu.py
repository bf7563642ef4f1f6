"""The oracle's specular bounces against ray optics in float64 (tests/optics_ref.py, written from the laws and not from the code), on the
cases of tests/optics_cases.py, without a GPU.  tests/test_gpu_optics.py then holds the device to the oracle on the same cases, bit for bit.
Every bounce of every path is checked through the oracle's ray hook (oracle.binding.ray_log): nothing is sampled.

Direction tolerance.  Three deviations are measured, each the length of a difference of unit vectors: of a reflection from d - 2 (d . n) n;
of a transmission's tangential part from eta times the incoming ray's (Snell's law, well-conditioned at every angle); and of a transmission
from the full Snell direction divided by its condition number max(1, eta cos_i / cos_t) (the normal part is the root of 1 - eta^2 sin^2,
whose error grows without bound towards the critical angle; bounces with cos_t < 0.05 are left to the tangential check).  The largest any
of them reaches over the committed cases is MEASURED = 6.4e-7 (a reflection of "mirror back"); TOL = 4 x that = 2.6e-6, since chains of float32
normalize and sqrt differ by a few ulps between cases.

NaN directions (a refraction whose float32 discriminant rounds below zero while ri * sin > 1 is false; include/mpt.h): 36 of the 2048
paths of "critical 1.5", 54 of "critical 1.33", 104 of the 9622 rays of "critical 1.5 deep".  Each ends its path as a miss and leaves its
sample black with alpha 1: 36, 54 and 104 black samples.

The closed form of "mirror quad" (albedo * sky(reflect(d, n)) per sample, in float64, with the Philox jitter): the oracle's sum is within
4.5e-7 of it on all 2486 pixels whose footprint lies inside the quad; 29 pixels (1.2 % of the quad's) straddle its edge."""
import numpy as np
import pytest

import optics_cases as oc
import optics_ref as orf
from oracle import binding as ob

MEASURED = 6.4e-7
TOL = 4 * MEASURED
CRITICAL_BAND = 1e-5            # rad: a bounce nearer than this to the critical angle may go either way in float32

# the kinds each case exists for, with half the count the oracle gave when the case was committed (at least 20)
FLOORS = {
    "mirror": dict(mirror=1596),
    "mirror back": dict(mirror=449),
    "mirror quad": dict(mirror=4999),
    "slab+prism 1.5": dict(refl_out=165, refl_in=88, refr_in=2213, refr_out=2213, tir=1463),
    "slab+prism 2.0": dict(refl_out=337, refl_in=256, refr_in=2060, refr_out=2059, tir=1255),
    "low index": dict(refl_out=108, refl_in=136, refr_in=916, refr_out=916, tir=483),
    "index one": dict(refl_out=51, refl_in=53, refr_in=1273, refr_out=1273),
    "glass sphere": dict(refl_out=27, refr_in=348),
    "critical 1.5": dict(nan=20, refr_out=518, tir=470, refl_in=20),
    "critical 1.33": dict(nan=27, refr_out=495, tir=490, refl_in=20),
    "critical 1.5 deep": dict(nan=52, refr_out=555, tir=3162, refl_in=20),
}
_bounces = {}


def bounces_of(name):
    if name not in _bounces:
        _, _, rays = oc.logged(name)
        _, buf = oc.scene_of(name)
        _bounces[name] = orf.bounces(rays, buf[1], buf[2], oc.CASES[name].depth)
    return _bounces[name]


def test_the_cases_have_the_sizes_depths_and_modes_they_are_meant_to():
    assert set(FLOORS) == set(oc.CASES)
    assert max(c.W * c.H * c.spp for c in oc.CASES.values()) == 64 * 40 * 4
    assert any(c.bsdf == oc.BSDF_SCATTER_ALL and c.depth == 16 for c in oc.CASES.values())
    for name in oc.CRITICAL:
        c = oc.CASES[name]
        assert (c.W, c.H, c.spp) == (16, 16, 8) and c.depth == (8 if name.endswith("deep") else 2)


def test_the_ray_log_is_the_render():
    """ray_log returns the image and counters of render, one row per ray in path order, and leaves the hook cleared."""
    name = "slab+prism 1.5"
    img, ct, rays = oc.logged(name)
    ref, ct2 = oc.oracle_render(name)
    np.testing.assert_array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert ct == ct2 and rays.shape == (ct["rays"], 8)
    path, bounce = orf.split_paths(rays, oc.CASES[name].depth)
    assert path[-1] + 1 == ct["paths"] and (rays[:, 7] < 0).sum() == ct["misses"]
    first = rays[bounce == 0]
    cam = np.array(oc.uniforms_of(name).cameraPosition[:3], np.float64)
    np.testing.assert_array_equal(first[:, :3], np.broadcast_to(cam, first[:, :3].shape))
    assert np.isinf(rays[rays[:, 7] < 0, 6]).all()
    with pytest.raises(ValueError):
        ob.ray_log(ob.Uniforms.from_buffer_copy(bytes(oc.uniforms_of(name))), oc.scene_of(name)[1], threads=2, **oc.render_kwargs(name))


@pytest.mark.parametrize("name", list(oc.CASES))
def test_every_specular_bounce_obeys_the_laws(name):
    b = bounces_of(name)
    refl, thru, nan = orf.is_kind(b, *orf.REFLECTIONS), orf.is_kind(b, *orf.TRANSMISSIONS), orf.is_kind(b, "nan")
    assert (refl | thru | nan).all() and len(b["ray"]) > 0
    cond = np.maximum(1.0, b["eta"] * b["cos_i"] / np.where(thru, b["cos_t"], 1.0))
    full = thru & (np.where(thru, b["cos_t"], 0.0) >= 0.05)
    dev = dict(reflected=b["dev_reflected"][refl], snell=b["dev_snell"][thru], transmitted=(b["dev_transmitted"] / cond)[full])
    worst = {k: float(v.max()) if v.size else 0.0 for k, v in dev.items()}
    unit = float(np.abs(b["length_next"][~nan] - 1).max())
    print(name, orf.census(b), "largest deviations", worst, "| |d| - 1 |", unit, "side of reflections", b["side"][refl].min() if refl.any() else None,
          b["side"][refl].max() if refl.any() else None, "of transmissions", b["side"][thru].min() if thru.any() else None,
          b["side"][thru].max() if thru.any() else None)
    for k, v in worst.items():
        assert v <= TOL, (name, k, v)
    assert unit <= TOL
    # the next origin: 1e-4 off the surface (the hit point's own float32 error is far below that), on the incident side after a reflection
    # and on the far side after a transmission
    assert ((b["side"][refl] > 0.5e-4) & (b["side"][refl] < 1.5e-4)).all()
    assert ((b["side"][thru] < -0.5e-4) & (b["side"][thru] > -1.5e-4)).all()
    # total internal reflection: beyond the tolerance no ray is transmitted, and none becomes NaN
    beyond = b["tir_excess"] > TOL
    assert orf.is_kind(b, "tir")[beyond].all()
    # a transmission or a Schlick reflection happens only where a transmitted ray exists, give or take the tolerance
    assert (b["tir_excess"][orf.is_kind(b, "refr_in", "refr_out", "refl_in", "refl_out")] <= TOL).all()
    if name == "index one":                       # r0 = 0 and eta = 1: what is not reflected passes undeviated
        assert np.linalg.norm(b["d_next"][thru] - b["d"][thru], axis=-1).max() <= TOL
        assert not b["tir"].any() and np.abs(b["R"][thru] - (1 - b["cos_i"][thru]) ** 5).max() < 1e-15


@pytest.mark.parametrize("name", list(oc.CASES))
def test_census(name):
    b = bounces_of(name)
    got = orf.census(b)
    print(name, got)
    for kind, floor in FLOORS[name].items():
        assert floor >= 20 and got[kind] >= floor, (name, kind, got[kind], floor)
    _, ct, _ = oc.logged(name)
    if name == "mirror":                          # both sides of the quad, and the ball
        quad = np.isin(b["prim"], oc.mirror_quad_prediction()[3])
        sides = int((quad & b["entering"]).sum()), int((quad & ~b["entering"]).sum()), int((~quad).sum())
        print("quad front, quad back, ball", sides)
        assert sides[0] >= 1008 and sides[1] >= 127 and sides[2] >= 460
    if name == "slab+prism 2.0":                  # materialType == 2 takes the emission branch, with power 0
        print("emissive hits", ct["emissive_hits"])
        assert ct["emissive_hits"] >= 5969
    else:
        assert ct["emissive_hits"] == 0
    if name == "low index":                       # eta = 2 on the way in: total reflection off the outside
        outside = int((orf.is_kind(b, "tir") & b["entering"]).sum())
        print("total reflections on entry", outside)
        assert outside >= 20 and not (orf.is_kind(b, "tir") & ~b["entering"]).any()
    if name == "index one":
        assert got["tir"] == 0 and got["nan"] == 0
    if name == "glass sphere":
        assert got["refl_in"] == got["refr_out"] == got["tir"] == 0
    if name not in oc.CRITICAL:
        assert got["nan"] == 0


def test_every_kind_occurs():
    total = {k: sum(orf.census(bounces_of(n))[k] for n in oc.CASES) for k in orf.KINDS}
    print(total)
    assert all(v >= 20 for v in total.values()), total


@pytest.mark.parametrize("name", ["slab+prism 1.5", "slab+prism 2.0", "low index", "index one", "glass sphere"])
def test_schlick_reflections_are_as_many_as_the_reflectance_says(name):
    """Over the dielectric bounces at which a transmitted ray exists, each a Bernoulli trial with Schlick's R: the number of reflections is
    within 5 standard errors of sum R (variance sum R (1 - R)).  The seeds are fixed: the outcome is deterministic."""
    b = bounces_of(name)
    with np.errstate(invalid="ignore"):
        trial = ~orf.is_kind(b, "mirror") & ~b["tir"] & ~(np.abs(b["to_critical"]) < CRITICAL_BAND)
    R = b["R"][trial]
    k = int(orf.is_kind(b, "refl_out", "refl_in")[trial].sum())
    mean, sd = R.sum(), np.sqrt((R * (1 - R)).sum())
    print(name, "trials", int(trial.sum()), "reflections", k, "expected", mean, "standard error", sd, "in units of it", (k - mean) / sd)
    assert trial.sum() >= 500 and sd > 0 and abs(k - mean) <= 5 * sd
    for side in (b["entering"][trial], ~b["entering"][trial]):          # outside and inside apart, where both occur
        if side.sum() >= 500:
            ks, Rs = int(orf.is_kind(b, "refl_out", "refl_in")[trial][side].sum()), R[side]
            assert abs(ks - Rs.sum()) <= 5 * np.sqrt((Rs * (1 - Rs)).sum())


def test_a_ray_inside_a_sphere_does_not_see_it():
    """The reference's sphere test takes the near root alone (PathTracing.h:120-142): from inside, that root is behind the origin.  So a
    glass sphere refracts on entry only, and in this scene (nothing else ahead of the camera) every path that enters leaves to the sky."""
    name = "glass sphere"
    _, _, rays = oc.logged(name)
    _, (_, prims, mats, _) = oc.scene_of(name)
    ball = int(np.nonzero(prims[:, 0, 3] == 0)[0][0])
    c, r = prims[ball, 0, :3].astype(np.float64), float(prims[ball, 1, 0])
    inside = np.linalg.norm(rays[:, :3] - c, axis=1) < r
    b = bounces_of(name)
    entered = orf.is_kind(b, "refr_in") & (b["prim"] == ball)
    print("rays that start inside the sphere", int(inside.sum()), "paths that enter", int(entered.sum()))
    assert inside.sum() >= 348 and (rays[inside, 7] != ball).all()
    assert entered.sum() == inside.sum() and inside[b["ray"][entered] + 1].all()
    assert (rays[b["ray"][entered] + 1, 7] == -1).all()


@pytest.mark.parametrize("name", oc.CRITICAL)
def test_the_critical_angle_makes_nan_directions_that_end_as_black_misses(name):
    img, ct, rays = oc.logged(name)
    c = oc.CASES[name]
    b = bounces_of(name)
    nan = orf.is_kind(b, "nan")
    after = b["ray"][nan] + 1
    path, _ = orf.split_paths(rays, c.depth)
    per_pixel = np.bincount(path[after] // c.spp, minlength=c.W * c.H).reshape(c.H, c.W)
    print(name, "NaN rays", int(nan.sum()), "of", len(rays), "rays and", ct["paths"], "paths; largest distance to the critical angle",
          np.abs(b["to_critical"][nan]).max(), "rad; black samples", int(per_pixel.sum()), "in", int((per_pixel > 0).sum()), "pixels")
    assert nan.sum() >= 20
    assert np.isnan(rays[after, 3:6]).all()                               # normalize of the zero vector: all three components
    assert (np.abs(b["to_critical"][nan]) < CRITICAL_BAND).all() and not b["entering"][nan].any()
    assert (rays[after, 7] == -1).all() and np.isinf(rays[after, 6]).all()
    assert np.unique(path[after]).size == after.size                      # the miss ends the path: one black sample each
    # the image: finite; alpha counts the samples that ended as a miss, the NaN ones among them; a clamped sample adds at most 1 to a
    # colour and a NaN one adds 0
    missed = np.bincount(path[rays[:, 7] < 0] // c.spp, minlength=c.W * c.H).reshape(c.H, c.W)
    assert np.isfinite(img).all() and (img[..., 3] == missed).all() and (per_pixel <= missed).all()
    assert (img[..., :3].max(-1) <= missed - per_pixel).all()
    # no NaN direction comes from anywhere else
    assert not np.isnan(np.delete(rays[:, :6], after, axis=0)).any()


def test_mirror_quad_against_the_closed_form():
    """The oracle's sum against albedo * sky(reflect(d, n)) in float64 (tests/optics_ref.py:plane_mirror_under_sky); the device is
    allowed 4 x the deviation measured here (tests/test_gpu_optics.py)."""
    img, _, rays = oc.logged(oc.PHYSICS)
    c = oc.CASES[oc.PHYSICS]
    pred, inside, edge, quad = oc.mirror_quad_prediction()
    share = edge.sum() / (edge.sum() + inside.sum())
    dev = np.abs(img.astype(np.float64) - pred)[inside]
    print("inside", int(inside.sum()), "edge", int(edge.sum()), "share", share, "largest deviation", dev.max())
    assert inside.sum() >= 2000 and share <= 0.10
    # what the closed form assumes: every sample of an inside pixel hits the quad and its reflection sees the sky
    path, bounce = orf.split_paths(rays, c.depth)
    pix_inside = inside.reshape(-1)[path // c.spp]
    assert np.isin(rays[pix_inside & (bounce == 0), 7], quad).all() and (rays[pix_inside & (bounce == 1), 7] == -1).all()
    assert (pix_inside & (bounce == 1)).sum() == inside.sum() * c.spp
    assert dev.max() <= oc.PHYSICS_ORACLE_DEVIATION
