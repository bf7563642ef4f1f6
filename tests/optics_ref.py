"""The laws of ray optics in float64, for checking the specular bounces of a ray log (oracle.binding.ray_log) one by one.  Written from
optics, not from the renderer: the law of reflection, Snell's law, total internal reflection and Schlick's approximation as include/mpt.h
states it.  A bounce is a logged ray that hits a mirror (materialType < 0) or a dielectric (materialType > 0, the index of refraction)
and is followed by another ray of the same path; the follower's origin and direction are what the renderer made of the bounce.

With d the unit direction of the incoming ray, N the geometric normal of the primitive (outward for the meshes of tests/optics_cases.py
and for a sphere) and n = -sign(d . N) N the normal on the incident side:
  hit point        P = o + t d
  entering         d . N < 0;  eta = 1 / ior entering, ior leaving  (the ratio of the index on the incident side to the other side's)
  reflection       r = d - 2 (d . n) n
  Snell            the tangential part of the transmitted direction is eta times that of d, its normal part is -sqrt(1 - eta^2 sin^2) n
  total reflection eta sin(theta) > 1: no transmitted ray exists
  Schlick          R = r0 + (1 - r0) (1 - cos(theta))^5, r0 = ((1 - eta) / (1 + eta))^2, theta the angle of incidence
  next origin      on the incident side for a reflection (+1e-4 n), on the far side for a transmission (-1e-4 n)
Test code: the product never imports it."""
import numpy as np

KINDS = ("mirror", "refl_out", "refl_in", "refr_in", "refr_out", "tir", "nan")
REFLECTIONS = ("mirror", "refl_out", "refl_in", "tir")
TRANSMISSIONS = ("refr_in", "refr_out")


def split_paths(rays, max_depth):
    """(path [n], bounce [n]) of every logged ray: a path ends with a miss or with its max_depth-th ray."""
    prim = rays[:, 7]
    path = np.empty(len(rays), np.int64)
    bounce = np.empty(len(rays), np.int64)
    p = k = 0
    for i in range(len(rays)):
        path[i], bounce[i] = p, k
        k += 1
        if prim[i] < 0 or k == max_depth:
            p, k = p + 1, 0
    return path, bounce


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return (a * b).sum(-1)


def geometric_normal(prims, prim, P):
    """N [m, 3] of primitives `prim` at the points P, from the primitive records [*, 3, 4]: cross(v1 - v0, v2 - v0), or P - centre."""
    rec = np.asarray(prims, np.float64).reshape(-1, 3, 4)[prim]
    tri = rec[:, 0, 3] == 1
    N = np.where(tri[:, None], np.cross(rec[:, 1, :3] - rec[:, 0, :3], rec[:, 2, :3] - rec[:, 0, :3]), P - rec[:, 0, :3])
    return _unit(N)


def surface_distance(prims, prim, X):
    """Signed distance of the points X from the surfaces of primitives `prim`, positive on the side N points to."""
    rec = np.asarray(prims, np.float64).reshape(-1, 3, 4)[prim]
    tri = rec[:, 0, 3] == 1
    N = _unit(np.where(tri[:, None], np.cross(rec[:, 1, :3] - rec[:, 0, :3], rec[:, 2, :3] - rec[:, 0, :3]), 1.0))
    plane = _dot(X - rec[:, 0, :3], N)
    ball = np.linalg.norm(X - rec[:, 0, :3], axis=-1) - rec[:, 1, 0]
    return np.where(tri, plane, ball)


def bounces(rays, prims, mats, max_depth):
    """Every specular bounce of the log, as a dict of arrays over the bounces:
      ray            index of the incoming ray in the log (the follower is ray + 1)
      path, bounce   of the incoming ray
      prim, ior      the primitive hit and its materialType (< 0: mirror)
      P, d, n        hit point; the incoming ray's unit direction; normal on the incident side
      entering, eta, cos_i, sin_i;  cos_t = sqrt(1 - (eta sin_i)^2) (NaN under total reflection)
      tir            eta sin_i > 1;  tir_excess = eta sin_i - 1;  to_critical = theta - asin(1 / eta) in rad (NaN where eta <= 1 or a mirror)
      R              Schlick's reflectance (1 for a mirror and under total reflection)
      reflected, transmitted   the laws' directions (transmitted: NaN under total reflection and for a mirror)
      d_next, o_next           the follower's direction (normalised in float64) and origin;  length_next = |direction| as logged
      dev_reflected            |d_next - reflected|
      dev_transmitted          |d_next - transmitted|: ill-conditioned near the critical angle, where the normal part is the root of a difference
      dev_snell                |tangential part of d_next - eta * tangential part of d|, with +inf where d_next is not on the far side: Snell's
                               law itself, well-conditioned at every angle
      side           signed distance of o_next from the surface, positive on the incident side
      kind           index into KINDS: what the renderer did, read off d_next (the nearer law)."""
    rays = np.asarray(rays, np.float64)
    mats = np.asarray(mats, np.float64).reshape(-1, 8)
    path, bounce = split_paths(rays, max_depth)
    prim = rays[:, 7].astype(np.int64)
    hit = prim >= 0
    mtype = np.where(hit, mats[np.maximum(prim, 0), 3], 0.0)
    follows = np.zeros(len(rays), bool)
    follows[:-1] = path[1:] == path[:-1]
    i = np.nonzero(hit & (mtype != 0) & follows)[0]
    o, d, t, p, ior = rays[i, 0:3], _unit(rays[i, 3:6]), rays[i, 6], prim[i], mtype[i]
    P = o + t[:, None] * d * np.linalg.norm(rays[i, 3:6], axis=-1, keepdims=True)
    N = geometric_normal(prims, p, P)
    entering = _dot(d, N) < 0
    n = np.where(entering[:, None], N, -N)
    mirror = ior < 0
    eta = np.where(mirror, 1.0, np.where(entering, 1.0 / np.where(mirror, 1.0, ior), ior))
    cos_i = -_dot(d, n)
    d_tan = d + cos_i[:, None] * n
    sin_i = np.linalg.norm(d_tan, axis=-1)
    tir = ~mirror & (eta * sin_i > 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        to_critical = np.where(~mirror & (eta > 1), np.arctan2(sin_i, cos_i) - np.arcsin(1 / eta), np.nan)
        r0 = ((1 - eta) / (1 + eta)) ** 2
        R = np.where(mirror | tir, 1.0, r0 + (1 - r0) * (1 - cos_i) ** 5)
        reflected = d + 2 * cos_i[:, None] * n
        cos_t = np.sqrt(1 - (eta * sin_i) ** 2)
        transmitted = np.where((mirror | tir)[:, None], np.nan, eta[:, None] * d_tan - cos_t[:, None] * n)
        raw_next = rays[i + 1, 3:6]
        length_next = np.linalg.norm(raw_next, axis=-1)
        d_next = raw_next / length_next[:, None]
        o_next = rays[i + 1, 0:3]
        is_nan = np.isnan(raw_next).any(-1)
        dev_r = np.linalg.norm(d_next - reflected, axis=-1)
        dev_t = np.linalg.norm(d_next - transmitted, axis=-1)
        next_cos = _dot(d_next, n)
        dev_s = np.where(next_cos < 0, np.linalg.norm(d_next - next_cos[:, None] * n - eta[:, None] * d_tan, axis=-1), np.inf)
        through = ~mirror & ~is_nan & ~(dev_r <= dev_s)
    side = surface_distance(prims, p, o_next) * np.where(entering, 1.0, -1.0)
    k = {name: j for j, name in enumerate(KINDS)}
    kind = np.where(is_nan, k["nan"], np.where(mirror, k["mirror"], np.where(
        through, np.where(entering, k["refr_in"], k["refr_out"]),
        np.where(tir, k["tir"], np.where(entering, k["refl_out"], k["refl_in"])))))
    return dict(ray=i, path=path[i], bounce=bounce[i], prim=p, ior=ior, P=P, d=d, n=n, entering=entering, eta=eta, cos_i=cos_i, sin_i=sin_i, cos_t=cos_t,
                tir=tir, tir_excess=eta * sin_i - 1, to_critical=to_critical, R=R, reflected=reflected, transmitted=transmitted,
                d_next=d_next, o_next=o_next, length_next=length_next, dev_reflected=dev_r, dev_transmitted=dev_t, dev_snell=dev_s,
                side=side, kind=kind)


def census(b):
    """{kind name: count} of a bounces() dict."""
    return {name: int((b["kind"] == j).sum()) for j, name in enumerate(KINDS)}


def is_kind(b, *names):
    return np.isin(b["kind"], [KINDS.index(x) for x in names])


def sky(d):
    """The background along the unit direction d: white at the nadir to (0.6, 0.7, 1.0) at the zenith, linear in d.y."""
    t = 0.5 * (np.asarray(d, np.float64)[..., 1] + 1.0)
    return 1.0 + (np.array([0.6, 0.7, 1.0]) - 1.0) * t[..., None]


# ---- primary rays and a closed form for a plane mirror under the sky ------------------------------------------------------------------
def primary_directions(u, spp, seed, sample_begin=0):
    """Unit directions [H, W, spp, 3] of the primary rays of a Philox render in float64: through the pixel centre moved by the jitter
    (words 0 and 1 of the block with counter word 2 = 0xFFFFFFFF, each u01 - 0.5 of a pixel), as include/mpt.h defines them."""
    import ao_ref
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    g = lambda a: np.array(list(a[:3]), np.float64)
    cam, first, vu, vv = g(u.cameraPosition), g(u.firstPixelPosition), g(u.viewportU), g(u.viewportV)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pixel = (py * W + px).astype(np.uint32)[..., None]
    s = (np.arange(spp, dtype=np.uint64) + np.uint64(sample_begin)).astype(np.uint32)[None, None, :]
    r = ao_ref.philox4x32_10(pixel, s, np.uint32(0xFFFFFFFF), np.uint32(0), seed[0], seed[1])
    x = (px[..., None] + 0.5) / W + (ao_ref.u01(r[0]).astype(np.float64) - 0.5) / W
    y = (py[..., None] + 0.5) / H + (ao_ref.u01(r[1]).astype(np.float64) - 0.5) / H
    return cam, _unit(first + x[..., None] * vu + y[..., None] * vv - cam)


def footprint_corner_directions(u):
    """Unit directions [H, W, 4, 3] through the four corners of every pixel's footprint (the jitter stays inside it)."""
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    g = lambda a: np.array(list(a[:3]), np.float64)
    cam, first, vu, vv = g(u.cameraPosition), g(u.firstPixelPosition), g(u.viewportU), g(u.viewportV)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    x = (px[..., None] + np.array([0.0, 1.0, 1.0, 0.0])) / W
    y = (py[..., None] + np.array([0.0, 0.0, 1.0, 1.0])) / H
    return cam, _unit(first + x[..., None] * vu + y[..., None] * vv - cam)


def hits_triangle(o, d, tri):
    """bool [...]: the rays o + t d, t > 0, cross the triangle [3, 3] (float64, edges included)."""
    v0, e1, e2 = tri[0], tri[1] - tri[0], tri[2] - tri[0]
    h = np.cross(d, e2)
    a = _dot(h, e1)
    s = o - v0
    bu = _dot(s, h) / a
    q = np.cross(s, e1)
    bv = _dot(d, q) / a
    t = _dot(q, e2) / a
    return (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)


def plane_mirror_under_sky(u, spp, seed, tris, albedo):
    """A flat mirror of triangles `tris` [n, 3, 3] that reflects nothing but sky, at depth 2: (predicted sum [H, W, 4] in float64, inside
    [H, W], edge [H, W]).  inside: all four corners of the pixel's footprint lie on the mirror, so every sample is albedo * sky(reflected);
    edge: some corners do.  The prediction holds for the inside pixels."""
    tris = np.asarray(tris, np.float64)
    N = _unit(np.cross(tris[0, 1] - tris[0, 0], tris[0, 2] - tris[0, 0]))
    cam, corners = footprint_corner_directions(u)
    on = np.zeros(corners.shape[:-1], bool)
    for t in tris:
        on |= hits_triangle(cam, corners, t)
    inside, edge = on.all(-1), on.any(-1) & ~on.all(-1)
    _, d = primary_directions(u, spp, seed)
    r = d - 2 * _dot(d, N)[..., None] * N
    rgb = np.clip(np.asarray(albedo, np.float64) * sky(r), 0.0, 1.0).sum(2)
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), float(spp))], -1), inside, edge
