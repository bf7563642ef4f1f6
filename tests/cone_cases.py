"""The cases tests/test_cone_cpu.py and tests/test_gpu_cone.py share, with their references (tests/cone_ref.py: MPT_LIGHT_SAMPLING_CONE)
computed once per process and never modified:
  scene.xml 24 x 14     the headline scene: one sphere light over a ground of triangles
  conehand 16 x 12      a hand-made scene: one sphere light and one triangle light above an occluder, a dull sphere and a floor
  manylights 16 x 12    tests/nee_cases.py's thirteen lights, the first of them a sphere
  specular 16 x 12      tests/nee_cases.py's mirror and glass spheres under a triangle light (mpt_render_nee under MPT_BSDF_SCATTER only)
  lit_box               the scene of the statistical test: a sphere light inside a closed box of dull walls
The direct pass's references hold samples [0, 3) of every pixel at a given size, the render's samples [0, 3) per max_depth.  Test code."""
import numpy as np

import anyhit_ref
import cone_ref
import denoise_ref
import direct_cases
import direct_ref
import nee_cases
import nee_ref
from oracle import binding as ob

SEED = (0x0C0E, 5)
SPP_MAX = 3
DEPTHS = (1, 2, 4)
GAP_CAP = 0.01
HAND_CAM = direct_cases.HAND_CAM
# name -> (width, height, camera, bsdf_mode)
CASES = {"scene.xml": (24, 14, None, nee_ref.LAMBERT), "conehand": (16, 12, HAND_CAM, nee_ref.LAMBERT),
         "manylights": (16, 12, HAND_CAM, nee_ref.LAMBERT), "specular": (16, 12, HAND_CAM, nee_ref.SCATTER)}
DIRECT_CASES = ("scene.xml", "conehand", "manylights")
SMALL_SIZES = ((1, 1), (7, 3))
BOX_CAM = dict(pos=(0.0, 4.0, 4.2), fwd=(0.0, -0.1, -1.0), up=(0.0, 1.0, 0.0), vfov=70.0)

_scenes = {}
_direct = {}
_nee = {}


def conehand_scene():
    """Spheres first: a sphere light and a dull sphere; a triangle light; a dull triangle below both lights that hides them from the
    middle of the floor; the floor."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    sc.addSphere((-2.5, 5.5, 0.0), 1.0, emission=(1.0, 0.6, 0.3), emissionPower=6.0)
    sc.addSphere((1.0, 1.0, 1.5), 1.0, albedo=(0.7, 0.6, 0.5))
    sc.addTriangle((1.5, 5.8, -1.0), (4.0, 5.6, -1.0), (2.5, 6.2, 1.5), emission=(0.4, 0.7, 1.0), emissionPower=8.0)
    sc.addTriangle((-4.5, 3.4, -2.5), (4.5, 3.6, -2.0), (0.0, 3.2, 2.5), albedo=(0.5, 0.5, 0.5))
    sc.addTriangle((-20.0, -0.3, -20.0), (0.0, 0.2, 25.0), (20.0, 0.0, -20.0), albedo=(0.8, 0.8, 0.6))   # (not flat: a flat leaf box is never hit)
    return sc


def lit_box_scene():
    """Spheres first: a sphere light of emissionPower 1 and albedo 0 (mpt_render's per-sample clamp can never bite: thr <= 1, the light
    zeroes thr, no sky is seen) and a dull sphere, inside a closed box of twelve dull triangles.  The box's corners are moved a little off
    the axes, so that no wall is flat (a flat leaf box is never hit) and the box stays closed."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    sc.addSphere((1.0, 6.5, -1.0), 0.8, albedo=(0.0, 0.0, 0.0), emission=(1.0, 0.9, 0.8), emissionPower=1.0)
    sc.addSphere((-1.5, 1.2, -1.5), 1.2, albedo=(0.7, 0.7, 0.7))
    rng = np.random.default_rng(11)
    corner = {}
    for i in range(8):
        base = np.array([-5.0 if i & 1 == 0 else 5.0, 0.0 if i & 2 == 0 else 9.0, -5.0 if i & 4 == 0 else 5.0])
        corner[i] = tuple(float(x) for x in base + rng.uniform(-0.2, 0.2, 3))
    walls = (((0, 1, 5, 4), (0.7, 0.7, 0.6)), ((2, 3, 7, 6), (0.7, 0.7, 0.7)), ((0, 2, 6, 4), (0.7, 0.3, 0.3)), ((1, 3, 7, 5), (0.3, 0.7, 0.3)),
             ((0, 1, 3, 2), (0.6, 0.6, 0.7)), ((4, 5, 7, 6), (0.6, 0.6, 0.6)))
    for (a, b, c, d), albedo in walls:
        sc.addTriangle(corner[a], corner[b], corner[c], albedo=albedo)
        sc.addTriangle(corner[a], corner[c], corner[d], albedo=albedo)
    return sc


def scene_of(name):
    """(host Scene, (bvh, prims, mats, prim_idx)) of a case, the tree built by the reference's builder on the host."""
    if name in ("conehand", "lit_box"):
        if name not in _scenes:
            sc = conehand_scene() if name == "conehand" else lit_box_scene()
            sc.buildBVH()
            _scenes[name] = (sc, sc.buffers())
        return _scenes[name]
    return nee_cases.scene_of(name)


def uniforms_of(name, W=None, H=None):
    from metalpathtracer_amd import host
    sc, _ = scene_of(name)
    w, h, cam, _ = CASES[name]
    return host.make_uniforms(W or w, H or h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)


def table_of(name):
    _, buf = scene_of(name)
    return direct_ref.light_table(buf[1], buf[2])


def direct_reference(name, W=None, H=None):
    """A dict: buf, u, ad, nc (the oracle's first hits), table, sampled (cone_ref.samples of samples [0, 3)), lower, upper.  Computed once."""
    key = (name, W, H)
    if key not in _direct:
        _, buf = scene_of(name)
        u = uniforms_of(name, W, H)
        ad, nc, _ = denoise_ref.first_hit_guides(u, buf, ob.first_hit)
        table = table_of(name)
        sampled = cone_ref.samples(ad, nc, u, table, 0, SPP_MAX, SEED)
        lower, upper = cone_ref.occlusion_bounds(sampled, buf, anyhit_ref.bounds)
        for a in (ad, nc, lower, upper) + tuple(sampled):
            a.setflags(write=False)
        _direct[key] = dict(buf=buf, u=u, ad=ad, nc=nc, table=table, sampled=sampled, lower=lower, upper=upper)
    return _direct[key]


def direct_sliced(r, N):
    """The samples [0, N) of a direct reference: (sampled, lower, upper)."""
    o, wi, tmax, contrib, skipped = r["sampled"]
    return (o, wi[:, :, :N], tmax[:, :, :N], contrib[:, :, :N], skipped[:, :, :N]), r["lower"][:, :, :N], r["upper"][:, :, :N]


def nee_reference(name, max_depth, W=None, H=None):
    """cone_ref.render of a case for samples [0, 3) without a clamp, plus u and buf.  Computed once."""
    key = (name, max_depth, W, H)
    if key not in _nee:
        _, buf = scene_of(name)
        u = uniforms_of(name, W, H)
        out = cone_ref.render(u, buf, table_of(name), ob.first_hit, anyhit_ref.bounds, bsdf_mode=CASES[name][3], max_depth=max_depth, begin=0,
                              count=SPP_MAX, seed=SEED, clamp=np.inf)
        out.update(u=u, buf=buf)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _nee[key] = out
    return _nee[key]
