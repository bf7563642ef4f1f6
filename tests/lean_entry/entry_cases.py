"""The cases of tests/test_gpu_lean_entry.py, shared with its child process (render_entry_cases.py): no pytest, no GPU in here.

A case: scene, size, spp, depth, two cameras and what the entry terms of a launch with each camera must be (`expect`).  `sync` renders
with the first camera, `sync_b` with the second in the same context, `async` is two back-to-back mpt_render_async steps — samples
[0, spp) with the first camera, [spp, 2 spp) with the second — into one sum, on the context's two render lanes.  A camera whose "pos"
is a string is placed by the child from the tree it reads back: "on-ilo" = x exactly on the shrunk root box's lower plane, "below-ilo" =
one ulp outside it."""
import numpy as np

M = np.float32(2.0 ** -10)                                                                       # MPT_LEAN_ENTRY_M
OWN = dict(pos=(0.0, 20.0, 50.0), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=60.0)          # Camera::reset()
ABOVE = dict(OWN, pos=(0.0, 500.0, 50.0), fwd=(0.0, -0.3, -1.0))                                    # above scene.xml's root box (hi.y < 500), looking down into it with the horizon in view
ON_ILO = dict(OWN, pos="on-ilo", fwd=(1.0, 0.0, 0.0))
BELOW_ILO = dict(OWN, pos="below-ilo", fwd=(1.0, 0.0, 0.0))
FAR_AT = 2.0e7
FAR_CAM = dict(OWN, pos=(FAR_AT, FAR_AT, FAR_AT + 48.0))

ON, PRIMARY_OFF, OFF = "entry and primary entry on", "entry on, primary entry off", "off"


def place(cam, nodes01):
    """`cam` with a position derived from node 0 (8 float32 words: lo, A0, hi, B0) filled in."""
    if not isinstance(cam["pos"], str):
        return cam
    ilo_x = np.float32(nodes01[0]) + np.float32(2.0) * M
    x = ilo_x if cam["pos"] == "on-ilo" else np.nextafter(ilo_x, np.float32(-np.inf), dtype=np.float32)
    return dict(cam, pos=(float(x), 20.0, 50.0))


def _triangles(v0, rng, spread):
    n = v0.shape[0]
    prims = np.zeros((n, 12), np.float32)
    prims[:, 3] = 1.0
    prims[:, 0:3], prims[:, 4:7], prims[:, 8:11] = v0, v0 + rng.uniform(-spread, spread, (n, 3)), v0 + rng.uniform(-spread, spread, (n, 3))
    mats = np.zeros((n, 8), np.float32)
    mats[:, 0:3] = 0.25 + 0.125 * (np.arange(n) % 5)[:, None]
    mats[::3, 4:7], mats[::3, 7] = (1.0, 0.9, 0.7), 2.0            # every third one emits
    return prims, mats


def two_triangles():
    """Two triangles in front of OWN: the tree is one leaf record."""
    prims, mats = _triangles(np.array([[-12.0, 8.0, 0.0], [2.0, 14.0, -5.0]]), np.random.default_rng(3), 10.0)
    return prims, mats


def far_scene():
    """300 triangles around (2e7, 2e7, 2e7), where an ulp is 2: ilo = lo + 2m rounds back to lo and the staging check fails."""
    rng = np.random.default_rng(5)
    return _triangles(FAR_AT + rng.uniform(-16, 16, (300, 3)), rng, 6.0)


SCENES = {"two-triangles": two_triangles, "far": far_scene}


def _case(name, cam, expect, scene="scene.xml", size=(70, 45), spp=3, depth=8, cam_b=None, expect_b=None):
    return dict(name=name, scene=scene, size=size, spp=spp, depth=depth, cams=[cam, cam_b or cam], expect=[expect, expect_b or expect])


CASES = [_case("%s-d%d" % (name, depth), cam, expect, depth=depth, **kw)
         for name, cam, expect, kw in (("own", OWN, ON, {}), ("own-1023x9", OWN, ON, dict(size=(1023, 9))), ("camera-above-the-root-box", ABOVE, PRIMARY_OFF, {}),
                                       ("camera-on-ilo", ON_ILO, ON, {}), ("camera-one-ulp-below-ilo", BELOW_ILO, PRIMARY_OFF, {}),
                                       ("two-cameras", OWN, ON, dict(cam_b=ABOVE, expect_b=PRIMARY_OFF)),
                                       ("root-is-a-leaf", OWN, OFF, dict(scene="two-triangles")), ("translated-to-2e7", FAR_CAM, OFF, dict(scene="far")))
         for depth in (1, 8)] + [_case("bunny20", OWN, None, scene="bunny20.xml", spp=1)]
