"""The cases tests/test_optics_cpu.py and tests/test_gpu_optics.py share: small procedural scenes that send paths through every branch of
the specular bounce of MPT_BSDF_SCATTER / MPT_BSDF_SCATTER_ALL (include/mpt.h) — mirror reflection off either side of a surface, refraction
into and out of glass, Schlick reflection outside and inside, total internal reflection, and the refraction at the critical angle whose
discriminant rounds below zero (a NaN direction).  Each case carries its scene, camera, image size, samples, depth and BSDF mode.

Every mesh is wound outwards (cross(v1 - v0, v2 - v0) points out of the body) and rotated off the axes: the reference's builder gives an
axis-aligned pair of coplanar triangles a flat leaf box, which its slab test never enters.  Angles come from a seeded generator.  Scenes,
the oracle's render and its ray log are computed once per process and never modified.  Nothing here touches a GPU or reads a file.  Test code."""
import collections

import numpy as np

from oracle import binding as ob

BSDF_SCATTER, BSDF_SCATTER_ALL = 1, 2
SEED = (0x0971C5, 7)
GROUND_ALBEDO = (0.6, 0.55, 0.5)
GLASS_ALBEDO = (0.95, 0.97, 0.99)
QUAD_ALBEDO = (0.8, 0.85, 0.9)
BALL_ALBEDO = (0.9, 0.8, 0.7)

Case = collections.namedtuple("Case", "scene cam W H spp depth bsdf")

_cache = {}


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def rotation(ax, ay, az):
    """R = Ry Rx Rz, angles in degrees."""
    a, b, c = np.radians([ax, ay, az])
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return ry @ rx @ rz


def wound_outwards(tris):
    """The triangles [n, 3, 3] of a convex body, each turned so that its geometric normal points away from the body's centroid."""
    tris = np.array(tris, np.float64)
    mid = tris.reshape(-1, 3).mean(0)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    flip = ((tris.mean(1) - mid) * n).sum(1) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return tris


def box(half, R, centre):
    """12 triangles, two per face; face 2 a + (0 for -, 1 for +) is triangles 2 f and 2 f + 1."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for s in (-1.0, 1.0):
            q = np.zeros((4, 3))
            q[:, a] = s * half[a]
            q[:, b] = np.array([-1, 1, 1, -1]) * half[b]
            q[:, c] = np.array([-1, -1, 1, 1]) * half[c]
            out += [q[[0, 1, 2]], q[[0, 2, 3]]]
    return wound_outwards(out) @ R.T + np.asarray(centre, np.float64)


def prism45(leg, half_depth, R, centre):
    """A right isosceles triangle (legs along x and y, the hypotenuse at 45 degrees to both) extruded along z: 8 triangles."""
    A, B, Cc = np.array([0.0, 0, 0]), np.array([leg, 0.0, 0]), np.array([0.0, leg, 0])
    lo, hi = np.array([0, 0, -half_depth]), np.array([0, 0, half_depth])
    out = [[A + lo, B + lo, Cc + lo], [A + hi, B + hi, Cc + hi]]
    for p, q in ((A, B), (B, Cc), (Cc, A)):
        out += [[p + lo, q + lo, q + hi], [p + lo, q + hi, p + hi]]
    t = wound_outwards(out)
    t -= t.reshape(-1, 3).mean(0)
    return t @ R.T + np.asarray(centre, np.float64)


def quad(half, R, centre):
    """Two triangles with the normal R e_z."""
    q = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float64)
    return np.array([q[[0, 1, 2]], q[[0, 2, 3]]]) @ R.T + np.asarray(centre, np.float64)


def _angles(rng, base, spread=2.0):
    return [b + rng.uniform(-spread, spread) for b in base]


def _scene(spheres, meshes):
    """spheres: (centre, radius, material kwargs); meshes: (triangles [n, 3, 3], material kwargs).  The host layer's Scene, its tree built by
    the reference's builder: (Scene, (bvh, prims, mats, prim_idx)), spheres first as every builder leaves them."""
    from metalpathtracer_amd import host
    sc = host.Scene()
    for c, r, kw in spheres:
        sc.addSphere([float(x) for x in c], float(r), **kw)
    for tris, kw in meshes:
        for t in np.asarray(tris, np.float32):
            sc.addTriangle(*[[float(x) for x in v] for v in t], **kw)
    sc.buildBVH()
    buf = sc.buffers()
    for a in buf:
        a.setflags(write=False)
    return sc, buf


def _ground(rng, y=-2.0):
    return quad(30.0, rotation(*_angles(rng, (-87.0, 0.0, 3.0))), (0.0, y, 0.0)), dict(albedo=GROUND_ALBEDO)


MIRROR_QUAD_HALF = 1.5
MIRROR_QUAD_CENTRE = (-1.2, 0.3, 0.0)
MIRROR_BALL = ((1.9, -0.3, -0.6), 1.0)


def mirror_quad_frame():
    """(R, centre, half) of the mirror quad: its normal R e_z looks up and towards the front camera, so that what that camera sees in it is sky."""
    rng = np.random.default_rng(41)
    return rotation(*_angles(rng, (-35.0, 20.0, 12.0))), np.array(MIRROR_QUAD_CENTRE), MIRROR_QUAD_HALF


def build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "mirror":
        R, c, h = mirror_quad_frame()
        return _scene([(MIRROR_BALL[0], MIRROR_BALL[1], dict(albedo=BALL_ALBEDO, materialType=-1.0))],
                      [(quad(h, R, c), dict(albedo=QUAD_ALBEDO, materialType=-1.0)), _ground(rng)])
    if name.startswith("slab+prism"):
        ior = float(name.split()[1])
        glass = dict(albedo=GLASS_ALBEDO, materialType=ior, emission=(1.0, 1.0, 1.0), emissionPower=0.0)
        slab = box((2.0, 1.2, 0.25), rotation(*_angles(rng, (10.0, 24.0, 5.0))), (-1.7, 0.5, 0.0))
        prism = prism45(2.4, 0.9, rotation(*_angles(rng, (8.0, -25.0, 12.0))), (1.8, 0.0, 0.4))
        return _scene([], [(slab, glass), (prism, glass), _ground(rng)])
    if name == "glass sphere":
        # what is not the sphere lies behind the camera: reflections off the sphere reach it, a ray inside the sphere cannot
        behind = quad(4.0, rotation(*_angles(rng, (-60.0, 8.0, 5.0))), (0.0, -1.5, 11.0))
        return _scene([((0.0, 0.3, 0.0), 1.3, dict(albedo=GLASS_ALBEDO, materialType=1.5))], [(behind, dict(albedo=GROUND_ALBEDO))])
    if name.startswith("critical"):
        ior = float(name.split()[1])
        R, _ = critical_frame(ior)
        return _scene([], [(box((1.0, 1.0, 1.0), R, (0.0, 0.0, 0.0)), dict(albedo=GLASS_ALBEDO, materialType=ior))])
    raise KeyError(name)


def critical_frame(ior):
    """(R of the glass box, camera): the camera sits at the box's centre and looks at the face R e_x at asin(1 / ior) to its normal, through
    a field of view of 3.4e-4 degrees: every primary ray meets the face from inside within a few 1e-6 rad of the critical angle."""
    rng = np.random.default_rng(int(ior * 100))
    R = rotation(*_angles(rng, (17.0, 31.0, -23.0)))
    th = np.arcsin(1.0 / ior)
    fwd = np.cos(th) * R[:, 0] + np.sin(th) * (0.8 * R[:, 1] + 0.6 * R[:, 2])
    return R, dict(pos=(0.0, 0.0, 0.0), fwd=tuple(fwd), up=tuple(R[:, 0]), vfov=3.4e-4)


FRONT = dict(pos=(0.0, 1.0, 7.0), fwd=(0.0, -0.1, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
BACK = dict(pos=(-3.5, 2.0, -6.5), fwd=(0.3, -0.25, 1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
# the front camera, aimed at the mirror quad so that one of its edges crosses the image and the rest of the image lies inside it
ON_QUAD = dict(pos=(0.0, 1.0, 7.0), fwd=(-0.245, -0.085, -1.0), up=(0.0, 1.0, 0.0), vfov=11.0)

CASES = {
    "mirror": Case("mirror", FRONT, 64, 40, 4, 16, BSDF_SCATTER_ALL),
    "mirror back": Case("mirror", BACK, 48, 30, 2, 8, BSDF_SCATTER),
    "mirror quad": Case("mirror", ON_QUAD, 64, 40, 4, 2, BSDF_SCATTER),
    "slab+prism 1.5": Case("slab+prism 1.5", FRONT, 64, 40, 4, 16, BSDF_SCATTER),
    "slab+prism 2.0": Case("slab+prism 2.0", FRONT, 64, 40, 4, 16, BSDF_SCATTER_ALL),
    "low index": Case("slab+prism 0.5", FRONT, 48, 30, 4, 8, BSDF_SCATTER),
    "index one": Case("slab+prism 1.0", FRONT, 48, 30, 4, 8, BSDF_SCATTER),
    "glass sphere": Case("glass sphere", FRONT, 48, 30, 4, 8, BSDF_SCATTER),
    "critical 1.5": Case("critical 1.5", None, 16, 16, 8, 2, BSDF_SCATTER),
    "critical 1.33": Case("critical 1.33", None, 16, 16, 8, 2, BSDF_SCATTER),
    "critical 1.5 deep": Case("critical 1.5", None, 16, 16, 8, 8, BSDF_SCATTER),
}
CRITICAL = tuple(n for n in CASES if n.startswith("critical"))
PHYSICS = "mirror quad"


def scene_of(name):
    """(host Scene, buffers) of a case's scene."""
    key = CASES[name].scene
    if key not in _cache:
        _cache[key] = build(key)
    return _cache[key]


def camera_of(name):
    c = CASES[name]
    return c.cam if c.cam is not None else critical_frame(float(c.scene.split()[1]))[1]


def uniforms_of(name):
    from metalpathtracer_amd import host
    c = CASES[name]
    sc, _ = scene_of(name)
    return host.make_uniforms(c.W, c.H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=camera_of(name))


def render_kwargs(name):
    c = CASES[name]
    return dict(rng_mode=ob.RNG_PHILOX, bsdf_mode=c.bsdf, max_depth=c.depth, accumulate=1, sample_count=c.spp, seed=SEED)


def oracle_render(name, buffers=None):
    """(sum image, counters) of the oracle on the case, over `buffers` (another tree of the same primitives) when given."""
    u = ob.Uniforms.from_buffer_copy(bytes(uniforms_of(name)))
    return ob.render(u, buffers if buffers is not None else scene_of(name)[1], **render_kwargs(name))


def logged(name):
    """(image, counters, rays [n, 8]) of the oracle on the case with its ray hook (oracle.binding.ray_log): computed once."""
    if ("log", name) not in _cache:
        u = ob.Uniforms.from_buffer_copy(bytes(uniforms_of(name)))
        img, ct, rays = ob.ray_log(u, scene_of(name)[1], **render_kwargs(name))
        img.setflags(write=False)
        rays.setflags(write=False)
        _cache["log", name] = (img, ct, rays)
    return _cache["log", name]


def mirror_quad_prediction():
    """optics_ref.plane_mirror_under_sky for the case PHYSICS, from the float32 vertices the scene holds: (sum, inside, edge), computed once."""
    import optics_ref
    if "prediction" not in _cache:
        c = CASES[PHYSICS]
        _, (_, prims, mats, _) = scene_of(PHYSICS)
        quad_prims = np.nonzero((prims[:, 0, 3] == 1) & (mats[:, 0, 3] < 0))[0]
        tris = prims[quad_prims][:, :, :3].astype(np.float64)
        out = optics_ref.plane_mirror_under_sky(uniforms_of(PHYSICS), c.spp, SEED, tris, mats[quad_prims[0], 0, :3])
        for a in out:
            a.setflags(write=False)
        _cache["prediction"] = out + (quad_prims,)
    return _cache["prediction"]


# the oracle's largest deviation from mirror_quad_prediction over the inside pixels, measured on the CPU (tests/test_optics_cpu.py asserts it):
# sums of four samples of up to 0.9 each, in float32
PHYSICS_ORACLE_DEVIATION = 4.5e-7
