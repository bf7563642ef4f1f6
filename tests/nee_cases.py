"""The cases tests/test_nee_cpu.py and tests/test_gpu_nee.py share, with their reference computed once per process and never modified:
the cases of tests/direct_cases.py (scene.xml 24 x 14, cornell.xml 16 x 16, handmade 16 x 12, dark 8 x 6) and one hand-made scene with
a mirror sphere, a glass sphere, a triangle light and a floor for MPT_BSDF_SCATTER, and one with thirteen lights among dull primitives
(a table that is no power of two long, with gaps between its ids) for the search of an emitter's id.  Per case and max_depth the reference holds samples
[0, 3) of every pixel (tests/nee_ref.py).  Test code."""
import numpy as np

import anyhit_ref
import direct_cases
import direct_ref
import nee_ref
from oracle import binding as ob

SEED = (0x1357, 9)
SPP_MAX = 3
DEPTHS = (1, 2, 4)
GAP_CAP = 0.01
# name -> (the scene's name in direct_cases or "specular", width, height, camera, bsdf_mode)
CASES = {name: (name,) + direct_cases.CASES[name] + (nee_ref.LAMBERT,) for name in direct_cases.CASES}
CASES["specular"] = ("specular", 16, 12, direct_cases.HAND_CAM, nee_ref.SCATTER)
CASES["manylights"] = ("manylights", 16, 12, direct_cases.HAND_CAM, nee_ref.LAMBERT)

_scenes = {}
_ref = {}


def specular_scene():
    """Spheres first: a mirror and a glass sphere over a floor, under a triangle light, with a diffuse wall behind."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    sc.addSphere((-2.2, 1.5, 0.0), 1.5, albedo=(0.9, 0.9, 0.9), materialType=-1.0)
    sc.addSphere((2.2, 1.5, 1.0), 1.5, albedo=(1.0, 1.0, 1.0), materialType=1.5)
    sc.addTriangle((-2.0, 6.0, -2.0), (2.0, 6.0, -2.0), (0.0, 6.4, 2.0), emission=(1.0, 0.9, 0.8), emissionPower=12.0)
    sc.addTriangle((-20.0, -0.3, -20.0), (0.0, 0.2, 25.0), (20.0, 0.0, -20.0), albedo=(0.8, 0.8, 0.6))
    sc.addTriangle((-9.0, -1.0, -7.0), (9.0, -1.0, -7.5), (0.0, 9.0, -7.2), albedo=(0.4, 0.6, 0.8))
    return sc


def manylights_scene():
    """Spheres first: a sphere light and a dull sphere; then twelve triangle lights in a ring over the floor, each followed by a small
    dull triangle (so the lights' caller ids are 0, 2, 4, ..., 24: thirteen of them), and the floor."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    sc.addSphere((0.0, 3.0, -1.0), 1.2, emission=(1.0, 0.8, 0.6), emissionPower=3.0)
    sc.addSphere((0.0, 0.8, 2.0), 0.8, albedo=(0.7, 0.7, 0.7))
    for i in range(12):
        a = 2.0 * np.pi * i / 12.0
        x, z = 6.0 * np.cos(a), 6.0 * np.sin(a) - 1.0
        tx, tz = -np.sin(a), np.cos(a)
        sc.addTriangle((x - 1.2 * tx, 0.4, z - 1.2 * tz), (x + 1.2 * tx, 0.5, z + 1.2 * tz), (0.9 * x, 3.0 + 0.1 * i, 0.9 * z + 0.1),
                       emission=(0.3 + 0.05 * i, 1.0 - 0.05 * i, 0.5), emissionPower=2.0 + 0.5 * (i % 3))
        sc.addTriangle((0.5 * x, 0.3, 0.5 * z), (0.5 * x + 0.4, 0.35, 0.5 * z), (0.5 * x + 0.2, 0.8, 0.5 * z + 0.3), albedo=(0.5, 0.6, 0.7))
    sc.addTriangle((-20.0, -0.3, -20.0), (0.0, 0.2, 25.0), (20.0, 0.0, -20.0), albedo=(0.8, 0.8, 0.6))
    return sc


def scene_of(name):
    """(host Scene, (bvh, prims, mats, prim_idx)) of a case, the tree built by the reference's builder on the host."""
    if name in ("specular", "manylights"):
        if name not in _scenes:
            sc = specular_scene() if name == "specular" else manylights_scene()
            sc.buildBVH()
            _scenes[name] = (sc, sc.buffers())
        return _scenes[name]
    return direct_cases.scene_of(name)


def uniforms_of(name, W=None, H=None):
    from metalpathtracer_amd import host
    sc, _ = scene_of(name)
    _, w, h, cam, _ = CASES[name]
    return host.make_uniforms(W or w, H or h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)


def table_of(name):
    _, buf = scene_of(name)
    return direct_ref.light_table(buf[1], buf[2])


def render_ref(name, max_depth, W=None, H=None, begin=0, count=SPP_MAX, clamp=np.inf):
    """nee_ref.render of a case (not cached): the dict of nee_ref.render plus u and buf."""
    _, buf = scene_of(name)
    u = uniforms_of(name, W, H)
    out = nee_ref.render(u, buf, table_of(name), ob.first_hit, anyhit_ref.bounds, bsdf_mode=CASES[name][4], max_depth=max_depth, begin=begin,
                         count=count, seed=SEED, clamp=clamp)
    out.update(u=u, buf=buf)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def reference(name, max_depth):
    """render_ref of the case at its own size for samples [0, 3) without a clamp: computed once."""
    key = (name, max_depth)
    if key not in _ref:
        _ref[key] = render_ref(name, max_depth)
    return _ref[key]
