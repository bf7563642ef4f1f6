"""The cases of tests/test_gpu_lean_primary.py, shared with its child process (render_cases.py): no pytest, no GPU in here.

A case: scene, size, spp, depth and two cameras.  `sync` renders with the first camera, `sync_b` with the second in the same context,
`async` is two back-to-back mpt_render_async steps — samples [0, spp) with the first camera, [spp, 2 spp) with the second — into one sum.
Where the two cameras are the same dict the case is an ordinary single-camera one."""
import numpy as np

OWN = dict(pos=(0.0, 20.0, 50.0), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=60.0)          # Camera::reset()
CENTRE = dict(OWN, pos=(0.0, 20.0, 0.0))                                                          # the centre of scene.xml's r = 10 sphere: oc = 0, b = 0
INSIDE = dict(OWN, pos=(7.0, 88.0, -11.0), fwd=(0.0, -1.0, 0.25), up=(0.0, 0.0, 1.0))             # inside the r = 40 sphere at (0, 100, 0), off its centre
FAR = dict(OWN, pos=(0.0, 20.0, 1.0e6))                                                           # 10^6 away: |oc|^2 ~ 10^12 against r^2, b^2 against a * cc
SIDE = dict(OWN, pos=(-60.0, 35.0, 20.0), fwd=(0.8, -0.2, -0.4))                                  # a second view of scene.xml
SOUP_CAM = dict(OWN, pos=(0.0, 0.0, 30.0))

SOUP_TRIANGLES, SOUP_SPHERES = 20000, 20


def soup_scene():
    """20 spheres in front of SOUP_CAM inside a soup of 20000 triangles: more than 16 spheres, so none hangs under the root, and a tree
    far larger than a workgroup's LDS, so only a prefix of the primitive records is resident.  (prims [P, 12], mats [P, 8]), spheres first."""
    rng = np.random.default_rng(17)
    n = SOUP_TRIANGLES + SOUP_SPHERES
    prims = np.zeros((n, 12), np.float32)
    prims[:, 3] = 1.0
    v0 = rng.uniform(-20, 20, (n, 3))
    prims[:, 0:3], prims[:, 4:7], prims[:, 8:11] = v0, v0 + rng.uniform(-1, 1, (n, 3)), v0 + rng.uniform(-1, 1, (n, 3))
    s = SOUP_SPHERES
    prims[:s, 3], prims[:s, 4:12] = 0.0, 0.0
    prims[:s, 0:2] = rng.uniform(-6, 6, (s, 2))
    prims[:s, 2] = rng.uniform(0, 18, s)
    prims[:s, 4] = rng.uniform(1.0, 2.5, s)
    mats = np.zeros((n, 8), np.float32)
    mats[:, 0:3] = 0.25 + 0.125 * (np.arange(n) % 5)[:, None]
    mats[:s, 4:7], mats[:s, 7] = (1.0, 0.9, 0.7), 2.0             # the spheres emit: what a primary ray finds there shows in the sum
    return prims, mats


def _case(name, cam, scene="scene.xml", size=(70, 45), spp=3, depth=8, cam_b=None):
    return dict(name=name, scene=scene, size=size, spp=spp, depth=depth, cams=[cam, cam_b or cam])


CASES = [_case("%s-d%d" % (name, depth), cam, depth=depth, **kw)
         for name, cam, kw in (("own", OWN, {}), ("centre", CENTRE, {}), ("inside", INSIDE, {}), ("far", FAR, {}),
                               ("own-1023x9", OWN, dict(size=(1023, 9))), ("two-cameras", OWN, dict(cam_b=SIDE)),
                               ("soup", SOUP_CAM, dict(scene="soup")))
         for depth in (1, 8)] + [_case("bunny20", OWN, scene="bunny20.xml", spp=1)]
