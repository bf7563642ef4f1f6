"""The one case tests/test_light_big_cpu.py and tests/test_gpu_light_big.py share: a scene whose reference tree fits no LDS image
(n_nodes * 32 > 160 KiB, the most the context ever grants), so that MPT_WALK_REFERENCE runs the light-sampling kernels' MPT_AO_REF
instantiations — threaded nodes beyond n_lds_nodes and primitive records beyond n_lds_prims from global memory — and the own tree does
not fit either.  Generated from a fixed seed with host.Scene, nothing from outside the repository:
  spheres first       a sphere light and three dull spheres
  41 lights           40 triangle lights, each followed by a dull occluder triangle below it (caller ids 4, 6, 8, ...: gaps for the
                      search of an emitter's id), every light with a material row of its own
  floor               a jittered height field of FLOOR_N x FLOOR_N cells, its triangles dealt 40 Lambert rows at random
  duplicates patch    a second, smaller height field just above the floor, under the lights, every triangle three times (coplanar
                      copies: exact ties for the closest-first walk, which flags them and re-traces through the reference tree)
More than 80 material rows in all, so shading reads rows beyond the 32 that LDS holds.  No vertex lies on an axis plane of another:
every one is jittered, no leaf box is flat.  The image is 24 x 16: two workgroups of four 8 x 8 tiles.

Two routes put the scene on the device: mpt_upload_scene with the host's tree (`host_buffers`) and mpt_build_and_upload, whose
downloaded tree the GPU test hands to `Refs`.  The references are the existing ones unchanged, each computed once per Refs object and
never modified.  Test code."""
import numpy as np

import anyhit_ref
import cone_ref
import denoise_ref
import direct_ref
import nee_ref
import restir_ref
import ris_ref
from oracle import binding as ob

SCENE_SEED = 20261021
W, H = 24, 16
CAM = dict(pos=(0.0, 9.0, 13.0), fwd=(0.0, -0.5735764, -0.8191520), up=(0.0, 1.0, 0.0), vfov=40.0)
LDS_MOST = 160 * 1024          # the context clamps lds_budget to this
AUTO_ORDERED_PRIMS = 8192      # MPT_AUTO_ORDERED_PRIMS (include/mpt.h)
LDS_MATS = 32                  # material rows staged in LDS (MPT_LDS_MATS_N)
FLOOR_N, FLOOR_CELL, FLOOR_JITTER = 82, 0.5, 0.12
PATCH_NX, PATCH_NZ, PATCH_CELL, PATCH_COPIES = 18, 16, 0.5, 3
N_TRI_LIGHTS, N_LAMBERT_ROWS = 40, 40
AREA, CONE = 0, 1
SEED = (0x0B16, 7)
GAP_CAP = 0.01                 # the share of pixels with a gap shadow ray (as every light case file)
TAINT_CAP = 0.10               # ReSTIR's tainted pixels (restir_cases.TAINT_CAP)
# the smallest parameters of the existing case tables
DIRECT_N = 2
RIS_M = 5
NEE_SPP, NEE_DEPTH = 2, 3
RESTIR = dict(K=4, R=8, M=5, begin=0, N=1)

_scene = []
_refs = {}


def _height_field(rng, nx, nz, cell, x0, z0, y0, jitter):
    """2 * nx * nz triangles over a grid whose every vertex is moved in all three coordinates; neighbours share vertices exactly."""
    gx, gz = np.meshgrid(np.arange(nx + 1) * cell + x0, np.arange(nz + 1) * cell + z0)
    P = np.stack([gx, np.full_like(gx, y0), gz], -1) + rng.uniform(-jitter, jitter, gx.shape + (3,)) * (0.6, 1.0, 0.6)
    P = P.astype(np.float32)
    t = []
    for i in range(nz):
        for j in range(nx):
            t.append((P[i, j], P[i, j + 1], P[i + 1, j]))
            t.append((P[i, j + 1], P[i + 1, j + 1], P[i + 1, j]))
    return np.asarray(t, np.float32)


def _tri(sc, t, **kw):
    sc.addTriangle(*(tuple(float(x) for x in v) for v in t), **kw)


def big_scene():
    from metalpathtracer_amd import host
    rng = np.random.default_rng(SCENE_SEED)
    sc = host.Scene()
    sc.addSphere((-3.1, 4.6, -2.2), 0.9, emission=(1.0, 0.8, 0.6), emissionPower=5.0)
    sc.addSphere((4.2, 1.0, 4.1), 0.9, albedo=(0.7, 0.6, 0.5))
    sc.addSphere((-4.6, 0.9, 5.2), 0.8, albedo=(0.5, 0.6, 0.7))
    sc.addSphere((0.4, 0.8, -3.3), 0.7, albedo=(0.6, 0.7, 0.5))
    # 40 triangle lights over x in [-7, 7], z in [-9, 7], each with its own emission, each followed by a dull triangle below it
    for i in range(N_TRI_LIGHTS):
        gx, gz = i % 8, i // 8
        c = np.array([-7.0 + 2.0 * gx, 4.3, -9.0 + 4.0 * gz]) + rng.uniform(-0.5, 0.5, 3) * (1.0, 1.0, 1.5)
        a = rng.uniform(0.0, 2.0 * np.pi)
        r = rng.uniform(0.6, 0.9)
        v = [c + (r * np.cos(a + k * 2.1), rng.uniform(-0.3, 0.3), r * np.sin(a + k * 2.1)) for k in range(3)]
        _tri(sc, v, emission=tuple(float(x) for x in rng.uniform(0.2, 1.0, 3)), emissionPower=float(2.0 + 0.25 * (i % 9)))
        oc = c + (rng.uniform(-0.6, 0.6), -1.6 + rng.uniform(-0.3, 0.3), rng.uniform(-0.6, 0.6))
        b = rng.uniform(0.0, 2.0 * np.pi)
        w = [oc + (0.7 * np.cos(b + k * 2.1), rng.uniform(-0.15, 0.15), 0.7 * np.sin(b + k * 2.1)) for k in range(3)]
        _tri(sc, w, albedo=(0.5, 0.5 + 0.01 * (i % 3), 0.5))
    palette = rng.uniform(0.25, 0.9, (N_LAMBERT_ROWS, 3))
    floor = _height_field(rng, FLOOR_N, FLOOR_N, FLOOR_CELL, -0.5 * FLOOR_N * FLOOR_CELL, -0.5 * FLOOR_N * FLOOR_CELL - 4.0, 0.0, FLOOR_JITTER)
    for t, k in zip(floor, rng.integers(0, N_LAMBERT_ROWS, floor.shape[0])):
        _tri(sc, t, albedo=tuple(float(x) for x in palette[k]))
    patch = _height_field(rng, PATCH_NX, PATCH_NZ, PATCH_CELL, -0.5 * PATCH_NX * PATCH_CELL, -0.5, 0.45, 0.08)
    for t, k in zip(patch, rng.integers(0, N_LAMBERT_ROWS, patch.shape[0])):
        for _ in range(PATCH_COPIES):
            _tri(sc, t, albedo=tuple(float(x) for x in palette[k]))
    return sc


def scene():
    """(host Scene, (bvh, prims, mats, prim_idx)) with the tree of the reference's builder on the host: built once."""
    if not _scene:
        sc = big_scene()
        sc.buildBVH()
        buf = sc.buffers()
        for a in buf:
            a.setflags(write=False)
        # what the case exists for (tests/test_light_big_cpu.py asserts the rest: what the camera sees, what the shadow rays meet)
        bvh, prims, mats, _ = buf
        kind = prims[:, 0, 3]
        n_sph = int((kind == 0).sum())
        leaf = bvh[:, 1, 3].copy().view(np.int32) > 0
        assert bvh.shape[0] * 32 > LDS_MOST, "the reference tree would fit an LDS image"
        assert prims.shape[0] >= AUTO_ORDERED_PRIMS
        assert np.unique(mats.reshape(-1, 8).view(np.uint32), axis=0).shape[0] > LDS_MATS
        assert 0 < n_sph <= 16 and (kind[:n_sph] == 0).all() and (kind[n_sph:] == 1).all()
        assert (bvh[leaf, 1, :3] > bvh[leaf, 0, :3]).all(), "a flat leaf box is never hit"
        _scene.append((sc, buf))
    return _scene[0]


def host_buffers():
    return scene()[1]


def patch_ids():
    """The caller ids of the duplicated triangles: the last of the array."""
    n = scene()[0].getPrimitiveCount()
    return np.arange(n - 2 * PATCH_NX * PATCH_NZ * PATCH_COPIES, n)


def uniforms(w=W, h=H):
    from metalpathtracer_amd import host
    sc, _ = scene()
    return host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=CAM)


def primary_rays(u):
    """(o [H*W, 3], d [H*W, 3]): the rays through the pixel centres, as mpt_read_aovs and denoise_ref.first_hit_guides form them."""
    F = np.float32
    w, h = int(u.screenSize[0]), int(u.screenSize[1])
    cam, first, vu, vv = (np.array(x[:3], np.float32) for x in (u.cameraPosition, u.firstPixelPosition, u.viewportU, u.viewportV))
    uvx = ((np.arange(w, dtype=np.float32) + F(0.5)) / F(w))[None, :, None]
    uvy = ((np.arange(h, dtype=np.float32) + F(0.5)) / F(h))[:, None, None]
    d = ((first + uvx * vu) + uvy * vv) - cam
    d = d * (F(1) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None]
    d = d.reshape(-1, 3).astype(np.float32)
    return np.broadcast_to(cam, d.shape).copy(), d


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _freeze(v)
    return x


class Refs:
    """The references of the case over one reference-format tree (buffers = (bvh, prims, mats, prim_idx)): each computed on first use,
    frozen, and kept.  The oracle's closest hits are remembered by the ray's bits: a path's geometry does not depend on how its light
    samples are drawn."""

    def __init__(self, buffers):
        self.buf = tuple(np.ascontiguousarray(a) for a in buffers)
        self.u = uniforms()
        self.table = direct_ref.light_table(self.buf[1], self.buf[2])
        self._kept = {}
        self._hits = {}

    def first_hit(self, o, d, buffers):
        key = (np.asarray(o, np.float32).tobytes(), np.asarray(d, np.float32).tobytes())
        if key not in self._hits:
            self._hits[key] = ob.first_hit(o, d, self.buf)
        return self._hits[key]

    def _once(self, key, make):
        if key not in self._kept:
            self._kept[key] = _freeze(make())
        return self._kept[key]

    def guides(self):
        """(ad, nc, prim): the oracle's first hits through the pixel centres."""
        return self._once("guides", lambda: denoise_ref.first_hit_guides(self.u, self.buf, self.first_hit))

    def direct(self, M, sampling):
        """The direct pass's samples [0, DIRECT_N) with M candidates: a dict of sampled, lower, upper, want (rgba, traced, unoccluded).
        M = 1 is direct_ref (AREA) or cone_ref (CONE), M >= 2 ris_ref."""
        def make():
            ad, nc, _ = self.guides()
            if M == 1:
                mod = cone_ref if sampling == CONE else direct_ref
                sampled = mod.samples(ad, nc, self.u, self.table, 0, DIRECT_N, SEED)
            else:
                mod = ris_ref
                sampled = ris_ref.samples(ad, nc, self.u, self.table, 0, DIRECT_N, M, SEED, cone=sampling == CONE)
            lower, upper = mod.occlusion_bounds(sampled, self.buf, anyhit_ref.bounds)
            want = mod.direct(ad, nc, self.u, self.table, 0, DIRECT_N, SEED, lower, sampled=sampled)
            return dict(sampled=sampled, lower=lower, upper=upper, want=want, gap=(upper & ~lower).any(-1))
        return self._once(("direct", M, sampling), make)

    def nee(self, M, sampling):
        """mpt_render_nee's samples [0, NEE_SPP) at NEE_DEPTH without a clamp: the dict of nee_ref.render (cone_ref's, ris_ref's)."""
        def make():
            kw = dict(bsdf_mode=nee_ref.LAMBERT, max_depth=NEE_DEPTH, begin=0, count=NEE_SPP, seed=SEED, clamp=np.inf)
            if M == 1:
                mod = cone_ref if sampling == CONE else nee_ref
                return mod.render(self.u, self.buf, self.table, self.first_hit, anyhit_ref.bounds, **kw)
            return ris_ref.render(self.u, self.buf, self.table, self.first_hit, anyhit_ref.bounds, M, cone=sampling == CONE, **kw)
        return self._once(("nee", M, sampling), make)

    def restir(self):
        """restir_ref.restir with RESTIR's arguments: both modes."""
        def make():
            ad, nc, _ = self.guides()
            p = RESTIR
            return restir_ref.restir(ad, nc, self.u, self.table, self.buf, anyhit_ref.bounds, p["begin"], p["N"], p["M"], p["K"], p["R"], SEED)
        return self._once("restir", make)


def host_refs():
    """Refs over the host's tree: once per process."""
    if "host" not in _refs:
        _refs["host"] = Refs(host_buffers())
    return _refs["host"]


# Every estimator with its light samplings: (name, candidates M, sampling)
DIRECT_FAMILIES = [("direct", 1, AREA), ("direct_cone", 1, CONE), ("direct_ris", RIS_M, AREA), ("direct_ris_cone", RIS_M, CONE)]
NEE_FAMILIES = [("nee", 1, AREA), ("nee_cone", 1, CONE), ("nee_ris", RIS_M, AREA), ("nee_ris_cone", RIS_M, CONE)]


def material_rows_seen(prim, prim_to_row, mats):
    """(Lambert rows, emitter rows) of the device's material table that are some pixel's first hit: prim [H, W] the first-hit caller ids
    (-1: none), prim_to_row [P] the table row of every caller id, mats [P, 8] the caller's rows."""
    seen = np.unique(prim[prim >= 0])
    emit = np.asarray(mats, np.float32).reshape(-1, 8)[seen, 7] > 0
    return np.unique(prim_to_row[seen[~emit]]), np.unique(prim_to_row[seen[emit]])


def rows_of_records(prim_words):
    """prim_to_row [P] from the device's primitive records (12 words each: word 7 the material row, word 11 the caller's id)."""
    rec = np.asarray(prim_words, np.uint32).reshape(-1, 12)
    out = np.full(rec.shape[0], -1, np.int64)
    out[rec[:, 11].astype(np.int64)] = rec[:, 7]
    assert (out >= 0).all()
    return out
