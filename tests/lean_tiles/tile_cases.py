"""The cases of tests/test_gpu_lean_tiles.py, shared with its child process (render_tile_cases.py): no pytest, no GPU in here.

The eleven cases of tests/lean_tail/tail_cases.py (their first camera, and the second where it differs) and the views that put each
class of tile (mpt_lean_tiles.h) where it can go wrong.  `expect`: what the class table read back after the render must hold at both
sizes — OFF: no skip tile at all (the item is off for the launch); NONE: no table (the tree is not in LDS); a dict of minimum counts of
"sky" (skip, empty mask), "masked" (skip, a mask), "onebit" (skip, one sphere), "general", "no_sky": True where no tile may be a sky tile, "chain": the least number of nodes between the root's hit link and the tail leaf
in the device's node array, "general_at": a world point whose tile must be general.
The minima come from the geometry, not from a run: scene.xml's horizon lies 3.6 degrees below horizontal, its sphere at y = 100 ends above
the default view, its light and mesh stand in the middle of the image."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lean_tail"))
import tail_cases as tc  # noqa: E402

SIZES, SPP, DEPTH = ((70, 45), (64, 64)), 16, 8
OFF, NONE = "off", "no table"
OWN = tc.OWN
UPZ = (0.0, 0.0, -1.0)


def lone_triangle():
    """tail_cases' three spheres and 60 triangles, and one small triangle alone in the sky: a box of its own beside the mesh's"""
    prims, _ = tc._with_spheres(tc.THREE, 21, False)
    t = np.zeros(12, np.float32)
    t[0:3], t[3], t[4:7], t[8:11] = (9.0, 30.0, -20.0), 1.0, (12.0, 30.5, -20.0), (10.0, 33.0, -20.5)
    prims = np.concatenate([prims, t[None]])
    return prims, tc._mats(prims.shape[0])


LONE_CENTROID = (31.0 / 3.0, 93.5 / 3.0, -60.5 / 3.0)
SCENES = dict(tc.SCENES, **{"lone-triangle": lone_triangle})


def _case(name, cam, expect, scene="scene.xml", shards=1):
    return dict(name=name, scene=scene, cam=cam, expect=expect, shards=shards)


def _from_tail(c, which):
    cam = c["cams"][which]
    e = c["expect"][which]
    if c["scene"] == "bunny20.xml":
        expect = NONE
    elif c["scene"] == "floating":
        # on.  The large triangle roofs the view, so no tile is sky; the triangles' box ends at y >= -2.5 and z <= 25, and the rays of the bottom
        # tile row leave the camera (y = 8, z = 50) at 23.4 degrees or more below horizontal: at z = 25 they are at y <= -2.8, under the box
        expect = {"skip": 1, "no_sky": True}
    elif e == tc.ON:
        expect = {"skip": 1}
    else:   # the tail item off, the camera outside the tail box, a scene without a tail leaf
        expect = OFF
    return _case(c["name"] + ("-b" if which else ""), cam, expect, scene=c["scene"])


CASES = [_from_tail(c, 0) for c in tc.CASES] + [_from_tail(c, 1) for c in tc.CASES if c["cams"][1] is not c["cams"][0]] + [
    # the default view: at least a fifth of the tiles are sky, some see the ground alone, the mesh and the light keep theirs general
    _case("default-classes", OWN, {"sky": 11, "onebit": 1, "general": 1}),
    _case("horizon-through-a-tile-row", dict(OWN, fwd=(0.0, -0.03, -1.0)), {"sky": 8, "onebit": 8, "general": 1}),
    _case("light-silhouette", dict(OWN, pos=(0.0, 20.0, 30.0)), {"sky": 4, "masked": 4, "general": 1}),
    _case("straight-up", dict(OWN, fwd=(0.0, 1.0, 0.0), up=UPZ), {"sky": 8, "masked": 1}),
    _case("straight-down", dict(OWN, fwd=(0.0, -1.0, 0.0), up=UPZ), {"onebit": 24, "no_sky": True}),
    _case("sphere-at-100-in-view", dict(OWN, fwd=(0.0, 0.9, -1.0)), {"sky": 4, "masked": 4}),
    # The device's tree is binary with T a child of the root, so the chain is the one box of all triangles (`chain`: its length as the test
    # walks it in the node array read back) and the lone triangle stretches that box up into the sky: the tile its centroid projects to
    # (`general_at`) is general although only sky shows around it; the bottom tile row passes under the box as in "floating" (z <= 11 here):
    # skip.  A chain of two nodes cannot come out of the builder; tests/test_gpu_lean_tiles_device.py runs one through the device's functions.
    _case("lone-triangle-in-the-sky", tc.LOW, {"skip": 1, "general": 1, "chain": 1, "general_at": LONE_CENTROID}, scene="lone-triangle"),
    _case("two-shards", OWN, {"sky": 11, "onebit": 1, "general": 1}, shards=2),
]


def class_counts(words):
    w = np.asarray(words, np.uint32)
    skip = (w & 0x80000000) != 0
    mask = w & 0xFFFF
    assert ((w == 0) | skip).all(), "a word that is neither general nor skip"
    one = skip & (mask != 0) & ((mask & (mask - 1)) == 0)
    return dict(tiles=int(w.size), general=int((~skip).sum()), skip=int(skip.sum()), sky=int((skip & (mask == 0)).sum()),
                masked=int((skip & (mask != 0)).sum()), onebit=int(one.sum()))


def chain_length(words, n_nodes):
    """Nodes from the root's hit link along miss links up to, not including, the tail leaf tail_cases.find_tail finds (None: no tail leaf)."""
    t, _ = tc.find_tail(words, n_nodes)
    if not t:
        return None
    w = np.asarray(words, np.uint32).reshape(-1, 8)
    n, length = int(w[0, 3]), 0
    while n != t:
        n, length = int(w[n, 7]), length + 1
    return length


def tile_of(point, cam, W, H):
    """(tx, ty) of the tile a world point projects to, for a camera that looks along -z with +y up (tail_cases.OWN, LOW)."""
    assert tuple(cam["fwd"]) == (0.0, 0.0, -1.0) and tuple(cam["up"]) == (0.0, 1.0, 0.0)
    d = np.asarray(point, np.float64) - np.asarray(cam["pos"], np.float64)
    half_h = np.tan(np.radians(cam["vfov"]) / 2.0)
    half_w = half_h * W / H
    px, py = (0.5 + d[0] / -d[2] / (2.0 * half_w)) * W, (0.5 - d[1] / -d[2] / (2.0 * half_h)) * H
    assert 0 <= px < W and 0 <= py < H, (px, py)
    return int(px) // 8, int(py) // 8
