"""The cases tests/test_restir_temporal_cpu.py and tests/test_gpu_restir_temporal.py share, with their references
(tests/restir_temporal_ref.py: mpt_direct_restir_temporal) computed once per process and never modified.  No new scene: the four
tests/ris_cases.py DIRECT_CASES at their sizes — scene.xml 24 x 14, cornell.xml 16 x 16, handmade and manylights 16 x 12, sizes at which
a tap crosses tile and workgroup borders — along a camera path of four frames: frame f sees the case's camera moved by f steps and turned
by 2 f degrees (temporal_ref.path_camera).  A CHAIN is the frames 0..3 of one (m, C, mode), each fed the reference's reservoirs of the
frame before, and one REPEAT: frame number 3 under frame 2's camera on frame 2's reservoirs, for the same-camera rule.  Test code."""
import numpy as np

import anyhit_ref
import denoise_ref
import nee_cases
import restir_temporal_ref as rtr
import ris_cases as rcs
import temporal_ref
from oracle import binding as ob

SEED = rcs.SEED
CASES = rcs.DIRECT_CASES
STEPS = {"scene.xml": (0.6, 0.0, 0.0), "cornell.xml": (0.12, 0.0, 0.0), "handmade": (0.5, 0.0, 0.0), "manylights": (0.5, 0.0, 0.0)}
YAW_DEG = 2.0
FRAMES = 4
MS = (1, 5)
CS = (20, 2)                            # with C = 2 the cap scales the history from frame 3 on
SMALL_SIZES = ((1, 1), (7, 3))
SMALL_M, SMALL_C = 5, 20
TAINT_CAP = 0.10

scene_of = rcs.scene_of
table_of = rcs.table_of

_guides = {}
_chains = {}


def size_of(name, W=None, H=None):
    _, w, h, _, _ = nee_cases.CASES[name]
    return W or w, H or h


def camera(name, f):
    """The camera of frame f of the case's path."""
    from metalpathtracer_amd import host
    cam0 = nee_cases.CASES[name][3] or host.camera_reset()
    return temporal_ref.path_camera(cam0, f, STEPS[name], yaw_deg=YAW_DEG)


def uniforms_of(name, f, W=None, H=None):
    from metalpathtracer_amd import host
    sc, _ = scene_of(name)
    W, H = size_of(name, W, H)
    return host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=camera(name, f))


def guides(name, f, W=None, H=None):
    """A dict: buf, u, ad, nc (the oracle's first hits at frame f's camera), table.  Computed once."""
    key = (name, f, W, H)
    if key not in _guides:
        _, buf = scene_of(name)
        u = uniforms_of(name, f, W, H)
        ad, nc, _ = denoise_ref.first_hit_guides(u, buf, ob.first_hit)
        for a in (ad, nc):
            a.setflags(write=False)
        _guides[key] = dict(buf=buf, u=u, ad=ad, nc=nc, table=table_of(name))
    return _guides[key]


def _freeze(x):
    for v in x.values() if isinstance(x, dict) else ():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        else:
            _freeze(v)


def one(g, prev, frame, M, C, seed=SEED):
    """restir_temporal_ref.frame over the guides dict g with the default thresholds; prev: None or (guides dict, reservoirs)."""
    p = None if prev is None else dict(ad=prev[0]["ad"], nc=prev[0]["nc"], cam=prev[0]["u"], res=prev[1])
    return rtr.frame(g["ad"], g["nc"], g["u"], g["table"], g["buf"], anyhit_ref.bounds, prev=p, frame=frame, M=M, C=C, seed=seed)


def chain(name, M, C, mode, W=None, H=None):
    """The chain of a case: a list of dicts(frame: the frame number, g: the guides, prev: None or (guides, reservoirs [H,W,7]) of the frame
    before, ref: restir_temporal_ref.frame's result — ref[mode] is the chain's) for frames 0..3, then the repeat.  Computed once."""
    key = (name, M, C, mode, W, H)
    if key not in _chains:
        links = []
        prev = None
        for f in range(FRAMES):
            g = guides(name, f, W, H)
            ref = one(g, prev, f, M, C)
            _freeze(ref)
            links.append(dict(frame=f, g=g, prev=prev, ref=ref))
            prev = (g, ref[mode]["res"])
        again = links[2]
        prev = (again["g"], again["ref"][mode]["res"])
        ref = one(again["g"], prev, 3, M, C)
        _freeze(ref)
        links.append(dict(frame=3, g=again["g"], prev=prev, ref=ref))
        _chains[key] = links
    return _chains[key]


def grid():
    """Every (M, C, mode) of the exactness tests."""
    return [(M, C, mode) for M in MS for C in CS for mode in rtr.MODES]
