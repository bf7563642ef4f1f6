"""The cases tests/test_direct_cpu.py and tests/test_gpu_direct.py share, with their reference computed once per process and never
modified: the scene in the reference's buffer format (built on the host, no GPU), the guides from the oracle's first hit, the light
table, samples [0, 65) of every pixel and the bounds of their occlusion (tests/anyhit_ref.py).  Test code."""
import numpy as np

import anyhit_ref
import denoise_ref
import direct_ref
from conftest import CORNELL_CAM, host_scene
from oracle import binding as ob

SEED = (0x2468, 3)
N_MAX = 65
GAP_CAP = 0.01
HAND_CAM = dict(pos=(0.0, 4.0, 14.0), fwd=(0.0, -0.2425356, -0.9701425), up=(0.0, 1.0, 0.0), vfov=40.0)
CASES = {"scene.xml": (24, 14, None), "cornell.xml": (16, 16, CORNELL_CAM), "handmade": (16, 12, HAND_CAM), "dark": (8, 6, HAND_CAM)}

_scenes = {}
_ref = {}


def handmade_scene(lights=True):
    """Eight primitives, spheres first (as every builder wants them): two sphere lights of different colour, a sphere that emits
    nothing, two triangle lights, a degenerate emissive triangle, an emissive triangle with black emission and a floor.  Four lights.
    lights=False: the two non-emitters alone."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    if lights:
        sc.addSphere((-4.0, 5.0, 0.0), 0.5, emission=(1.0, 0.3, 0.1), emissionPower=20.0)
        sc.addSphere((4.0, 4.0, 1.0), 1.0, emission=(0.2, 0.4, 1.0), emissionPower=5.0)
    sc.addSphere((0.0, 1.0, 0.0), 1.0, albedo=(0.7, 0.6, 0.5))
    if lights:
        sc.addTriangle((-1.0, 6.0, -1.0), (1.0, 6.0, -1.0), (0.0, 6.3, 1.0), emission=(1.0, 1.0, 1.0), emissionPower=10.0)
        sc.addTriangle((-3.0, 1.0, -6.0), (3.0, 1.0, -6.0), (0.0, 4.0, -6.2), emission=(0.5, 1.0, 0.5), emissionPower=4.0)
        sc.addTriangle((5.0, 5.0, 5.0), (6.0, 6.0, 6.0), (7.0, 7.0, 7.0), emission=(1.0, 1.0, 1.0), emissionPower=3.0)     # no area
        sc.addTriangle((-6.0, 2.0, -3.0), (-5.0, 2.0, -3.0), (-5.5, 3.0, -3.2), emission=(0.0, 0.0, 0.0), emissionPower=1.0)  # black
    sc.addTriangle((-20.0, -0.3, -20.0), (0.0, 0.2, 25.0), (20.0, 0.0, -20.0), albedo=(0.8, 0.8, 0.6))   # (not flat: a flat leaf box is never hit)
    return sc


def scene_of(name):
    """(host Scene, (bvh, prims, mats, prim_idx)) of a case, the tree built by the reference's builder on the host."""
    if name in ("handmade", "dark"):
        if name not in _scenes:
            sc = handmade_scene(lights=name == "handmade")
            sc.buildBVH()
            _scenes[name] = (sc, sc.buffers())
        return _scenes[name]
    return host_scene(name)


def uniforms_of(name, W=None, H=None):
    from metalpathtracer_amd import host
    sc, _ = scene_of(name)
    w, h, cam = CASES[name]
    return host.make_uniforms(W or w, H or h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)


def guides_and_bounds(name, W=None, H=None, begin=0, N=N_MAX):
    """A dict: buf, u, ad, nc (the oracle's first hits), table, sampled (direct_ref.samples), lower, upper."""
    _, buf = scene_of(name)
    u = uniforms_of(name, W, H)
    ad, nc, _ = denoise_ref.first_hit_guides(u, buf, ob.first_hit)
    table = direct_ref.light_table(buf[1], buf[2])
    sampled = direct_ref.samples(ad, nc, u, table, begin, N, SEED)
    lower, upper = direct_ref.occlusion_bounds(sampled, buf, anyhit_ref.bounds)
    out = dict(buf=buf, u=u, ad=ad, nc=nc, table=table, sampled=sampled, lower=lower, upper=upper)
    for a in (ad, nc, lower, upper) + tuple(sampled):
        a.setflags(write=False)
    return out


def reference(name):
    """guides_and_bounds of the case at its own size for samples [0, 65): computed once."""
    if name not in _ref:
        _ref[name] = guides_and_bounds(name)
    return _ref[name]


def sliced(r, begin, N):
    """The samples [begin, begin + N) of a reference over [0, 65): (sampled, lower, upper)."""
    o, wi, tmax, contrib, skipped = r["sampled"]
    s = slice(begin, begin + N)
    return (o, wi[:, :, s], tmax[:, :, s], contrib[:, :, s], skipped[:, :, s]), r["lower"][:, :, s], r["upper"][:, :, s]


def gap_pixels(r, begin=0, N=N_MAX):
    """[H, W] bool: the pixels holding a ray the own-tree walk may answer either way."""
    _, lower, upper = sliced(r, begin, N)
    return (upper & ~lower).any(-1)
