"""The cases of tests/test_gpu_lean_tail.py, shared with its child process (render_tail_cases.py): no pytest, no GPU in here.

A case: scene, two cameras and what the tail terms of a launch with each camera must be (`expect`; None: whatever the tree gives, only
cross-checked; `why`: the reason tail_cases.find_tail must give for an OFF).  Every case renders 70 x 45, 16 spp, depth 8 (ring 1 and the drain are used): `sync` with the first camera, `sync_b`
with the second in the same context, `async` two back-to-back mpt_render_async steps — samples [0, spp) with the first camera,
[spp, 2 spp) with the second — into one sum, on the context's two render lanes.  A camera whose "pos" is a string is placed by the
child from the tree it reads back: "on-thi" = y exactly on the upper plane of the tail leaf's shrunk box, "above-thi" = one ulp above."""
import numpy as np

M = np.float32(2.0 ** -10)                                                                       # MPT_LEAN_ENTRY_M
HOLD = 0x80000000                                                                                # MPT_NODE_HOLD
OWN = dict(pos=(0.0, 20.0, 50.0), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=60.0)          # Camera::reset()
ABOVE = dict(OWN, pos=(0.0, 500.0, 50.0), fwd=(0.0, -0.3, -1.0))                                    # above scene.xml's sphere leaf (hi.y = 140), looking down with the horizon in view
ON_THI = dict(OWN, pos="on-thi", fwd=(0.0, -0.8, -1.0))
ABOVE_THI = dict(OWN, pos="above-thi", fwd=(0.0, -0.8, -1.0))
LOW = dict(OWN, pos=(0.0, 8.0, 50.0))                                                              # inside the sphere leaf's box of the hand-made scenes
FAR_AT = 2.0e7
FAR_CAM = dict(OWN, pos=(FAR_AT, FAR_AT, FAR_AT + 48.0))
SIZE, SPP, DEPTH = (70, 45), 16, 8

ON, PRIMARY_OFF, OFF = "on, the camera inside", "on, the camera outside", "off"


def find_tail(words, n_nodes):
    """T as the kernels find it, written a second time: from the root's hit link along miss links.  words: the node array as uint32,
    8 per node.  Returns (T or 0, why)."""
    w = np.asarray(words, np.uint32).reshape(-1, 8)
    if n_nodes == 0:
        return 0, "no nodes"
    t = int(w[0, 3])
    if t & HOLD:
        return 0, "the root is a leaf record"
    if t == 0 or t >= n_nodes:
        return 0, "the root has no hit link"
    for _ in range(n_nodes):
        b = int(w[t, 7])
        if b >= n_nodes:
            break
        t = b
    else:
        return 0, "links never end"
    if not int(w[t, 3]) & HOLD:
        return 0, "T = %d is an internal node" % t
    lo, hi = w[t, 0:3].view(np.float32), w[t, 4:7].view(np.float32)
    tlo, thi = lo + np.float32(2) * M, hi - np.float32(2) * M
    with np.errstate(all="ignore"):
        ok = ((lo - tlo) <= -M).all() and ((hi - thi) >= M).all() and (tlo <= thi).all()
    return (t, "on") if ok else (0, "T = %d fails the staging check" % t)


def place(cam, words, n_nodes):
    """`cam` with a position derived from the tail leaf's planes filled in."""
    if not isinstance(cam["pos"], str):
        return cam
    t, why = find_tail(words, n_nodes)
    assert t, why
    hi_y = np.asarray(words, np.uint32).reshape(-1, 8)[t, 5:6].view(np.float32)[0]
    thi_y = np.float32(hi_y) - np.float32(2.0) * M
    y = thi_y if cam["pos"] == "on-thi" else np.nextafter(thi_y, np.float32(np.inf), dtype=np.float32)
    return dict(cam, pos=(0.0, float(y), 50.0))


def _triangles(v0, rng, spread):
    n = v0.shape[0]
    prims = np.zeros((n, 12), np.float32)
    prims[:, 3] = 1.0
    prims[:, 0:3], prims[:, 4:7], prims[:, 8:11] = v0, v0 + rng.uniform(-spread, spread, (n, 3)), v0 + rng.uniform(-spread, spread, (n, 3))
    return prims


def _mats(n):
    mats = np.zeros((n, 8), np.float32)
    mats[:, 0:3] = 0.25 + 0.125 * (np.arange(n) % 5)[:, None]
    mats[::3, 4:7], mats[::3, 7] = (1.0, 0.9, 0.7), 2.0            # every third one emits
    return mats


def _sphere(centre, radius):
    p = np.zeros(12, np.float32)
    p[0:3], p[4] = centre, radius
    return p


def _with_spheres(spheres, seed, floating):
    rng = np.random.default_rng(seed)
    tris = _triangles(rng.uniform((-14, 0.5, -12), (14, 11, 8), (60, 3)), rng, 3.0)
    rows = [_sphere(c, r) for c, r in spheres] + list(tris)
    if floating:   # one large triangle above every sphere's top (12): the origins of its bounce rays are outside the sphere leaf's box
        t = np.zeros(12, np.float32)
        t[0:3], t[3], t[4:7], t[8:11] = (-30.0, 30.0, -30.0), 1.0, (30.0, 31.0, -30.0), (0.0, 29.0, 25.0)
        rows.append(t)
    prims = np.array(rows, np.float32)
    return prims, _mats(prims.shape[0])


THREE = [((0.0, -1000.0, 0.0), 1000.0), ((6.0, 6.0, 0.0), 6.0), ((-5.0, 2.0, 4.0), 2.0)]
SEVEN = THREE + [((-12.0, 1.5, -3.0), 1.5), ((12.0, 1.0, 5.0), 1.0), ((0.0, 1.0, 10.0), 1.0), ((3.0, 0.75, 14.0), 0.75)]


def floating():
    """three spheres, 60 triangles and a large triangle floating above all of them"""
    return _with_spheres(THREE, 21, True)


def seven_spheres():
    """seven spheres: more than one leaf holds, so the walk's last node is a chain node"""
    return _with_spheres(SEVEN, 22, False)


def no_sphere():
    rng = np.random.default_rng(23)
    prims = _triangles(rng.uniform((-14, 0.5, -12), (14, 11, 8), (60, 3)), rng, 3.0)
    return prims, _mats(60)


def two_triangles():
    """Two triangles in front of OWN: the tree is one leaf record."""
    prims = _triangles(np.array([[-12.0, 8.0, 0.0], [2.0, 14.0, -5.0]]), np.random.default_rng(3), 10.0)
    return prims, _mats(2)


def far_scene():
    """300 triangles and three spheres around (2e7, 2e7, 2e7), where an ulp is 2: the spheres' leaf is the walk's last node, but
    tlo = lo + 2m rounds back to lo and the staging check fails."""
    rng = np.random.default_rng(5)
    tris = _triangles(FAR_AT + rng.uniform(-16, 16, (300, 3)), rng, 6.0)
    spheres = ((0.0, -48.0, 0.0, 32.0), (8.0, 4.0, -4.0, 4.0), (-10.0, 2.0, 6.0, 2.0))
    prims = np.array([_sphere((FAR_AT + x, FAR_AT + y, FAR_AT + z), r) for x, y, z, r in spheres] + list(tris), np.float32)
    return prims, _mats(prims.shape[0])


SCENES = {"floating": floating, "seven-spheres": seven_spheres, "no-sphere": no_sphere, "two-triangles": two_triangles, "far": far_scene}


def _case(name, cam, expect, scene="scene.xml", cam_b=None, expect_b=None, why=None):
    return dict(name=name, scene=scene, cams=[cam, cam_b or cam], expect=[expect, expect_b if cam_b else expect], why=why)


CASES = [_case("own", OWN, ON),
         _case("camera-above-the-tail-box", ABOVE, PRIMARY_OFF),
         _case("camera-on-thi", ON_THI, ON),
         _case("camera-one-ulp-above-thi", ABOVE_THI, PRIMARY_OFF),
         _case("two-cameras", OWN, ON, cam_b=ABOVE, expect_b=PRIMARY_OFF),
         _case("triangle-above-every-sphere", LOW, ON, scene="floating"),
         _case("seven-spheres", LOW, OFF, scene="seven-spheres", why="internal node"),
         _case("no-sphere", LOW, None, scene="no-sphere"),
         _case("root-is-a-leaf", OWN, OFF, scene="two-triangles", why="root is a leaf"),
         _case("translated-to-2e7", FAR_CAM, OFF, scene="far", why="staging check"),
         _case("bunny20", OWN, None, scene="bunny20.xml")]
