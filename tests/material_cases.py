"""The scenes of tests/test_materials_cpu.py and tests/test_gpu_materials.py: material tables of 1 .. 40,000 distinct rows on one kind of
geometry, generated in numpy, and the 64-bit material hash of mpt_devbuild.h (k_mat_hash) restated in numpy, with a pair of rows that
collide in its upper half.  Nothing here touches a GPU or reads a file; everything is computed once per process and never modified.

The scene: three spheres (Lambert, mirror, glass) on a floor of two triangles, in front of a wall of K x K quads of two triangles each
that fills the image.  The caller-format arrays are prims [n, 12] and mats [n, 8]; `n_mats` distinct 32-byte rows are dealt to the
primitives in a shuffled order, so that equal rows are not neighbours in the array.  Test code."""
import numpy as np

CAM = dict(pos=(0.0, 3.0, 14.0), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
W, H = 128, 96
WALL_X, WALL_Y, WALL_Z = (-9.6, 9.6), (-2.5, 10.2), -6.0
N_EMISSIVE = 40

# name: (K, n_mats or None for "every primitive its own row", rendered)
CASES = {
    "m1": (23, 1, True), "m31": (23, 31, True), "m32": (23, 32, True), "m33": (23, 33, True), "m64": (23, 64, True),
    "m200": (23, 200, True), "collision": (23, 202, True),
    "all4k": (46, None, True), "all8k": (65, None, True), "all40k": (142, None, False),
}
TABLE_CASES = ("m1", "m31", "m32", "m33", "m64", "m200", "collision")      # every row must be somebody's first hit
ALL_DISTINCT = ("all4k", "all8k", "all40k")

_cache = {}


# ---- the hash ---------------------------------------------------------------------------------------------------------------
def mat_hash(mats):
    """k_mat_hash: FNV-1a over the eight 32-bit words of a row with an extra h ^= h >> 29 per word; [n] uint64."""
    w = np.ascontiguousarray(mats, np.float32).reshape(-1, 8).view(np.uint32).astype(np.uint64)
    h = np.full(w.shape[0], 0xcbf29ce484222325, np.uint64)
    with np.errstate(over="ignore"):
        for k in range(8):
            h = h ^ w[:, k]
            h = h * np.uint64(0x100000001b3)
            h = h ^ (h >> np.uint64(29))
    return h


def collision_candidates():
    """The 200,000 rows the collision is searched in: random albedo in [0.05, 0.95), everything else zero."""
    if "cand" not in _cache:
        rows = np.zeros((200000, 8), np.float32)
        rows[:, 0:3] = np.random.default_rng(7).uniform(0.05, 0.95, (200000, 3)).astype(np.float32)
        rows.setflags(write=False)
        _cache["cand"] = rows
    return _cache["cand"]


def colliding_pair():
    """Two different candidate rows [2, 8] whose hashes agree in the upper 32 bits and differ in the lower: what sends the device build
    from its 32-bit material keys to the 64-bit sort."""
    if "pair" not in _cache:
        rows = collision_candidates()
        h = mat_hash(rows)
        hi = (h >> np.uint64(32)).astype(np.uint32)
        order = np.argsort(hi, kind="stable")
        a, b = order[:-1], order[1:]
        hit = np.nonzero((hi[a] == hi[b]) & (h[a] != h[b]) & (rows[a].view(np.uint32) != rows[b].view(np.uint32)).any(1))[0]
        assert hit.size > 0, "no pair of the candidates collides in the upper half of the hash: k_mat_hash has changed"
        pair = np.stack([rows[a[hit[0]]], rows[b[hit[0]]]])
        pair.setflags(write=False)
        _cache["pair"] = pair
    return _cache["pair"]


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def geometry(K):
    """prims [n, 12]: three spheres, the floor's two triangles, then the wall's 2 K^2 triangles (quad q = row * K + column is primitives
    5 + 2 q and 5 + 2 q + 1).  The wall's grid points are moved a little along z: no triangle's box is flat."""
    if ("geo", K) not in _cache:
        rng = np.random.default_rng(1000 + K)
        n = 5 + 2 * K * K
        p = np.zeros((n, 12), np.float32)
        for i, x in enumerate((-4.0, 0.0, 4.0)):
            p[i, 0:3] = (x, -1.7, 2.0)
            p[i, 4] = 0.8
        p[3:, 3] = 1.0
        y0 = WALL_Y[0]
        p[3, 0:3], p[3, 4:7], p[3, 8:11] = (-12.0, y0, 8.0), (12.0, y0 - 0.1, 8.0), (12.0, y0, -8.0)       # (not flat either; the diagonal
        p[4, 0:3], p[4, 4:7], p[4, 8:11] = (-12.0, y0, 8.0), (12.0, y0, -8.0), (-12.0, y0 - 0.1, -8.0)     #  runs through the image)
        gx = np.linspace(WALL_X[0], WALL_X[1], K + 1)
        gy = np.linspace(WALL_Y[0], WALL_Y[1], K + 1)
        g = np.zeros((K + 1, K + 1, 3))
        g[..., 0], g[..., 1] = gx[None, :], gy[:, None]
        g[..., 2] = WALL_Z + rng.uniform(-0.05, 0.05, (K + 1, K + 1))
        a, b, c, d = g[:-1, :-1], g[:-1, 1:], g[1:, 1:], g[1:, :-1]            # counter-clockwise seen from the camera
        w = p[5:].reshape(K, K, 2, 12)
        w[:, :, 0, 0:3], w[:, :, 0, 4:7], w[:, :, 0, 8:11] = a, b, c
        w[:, :, 1, 0:3], w[:, :, 1, 4:7], w[:, :, 1, 8:11] = a, c, d
        p.setflags(write=False)
        _cache["geo", K] = p
    return _cache["geo", K]


def flat_tree(prims):
    """A tree of one leaf in the reference's buffer format (bvh [1, 2, 4], prim_idx [n]): enough for the oracle's first hits on the CPU."""
    p = np.asarray(prims, np.float32).reshape(-1, 12)
    tri = p[:, 3] == 1
    pts = np.concatenate([p[tri][:, [0, 1, 2]], p[tri][:, [4, 5, 6]], p[tri][:, [8, 9, 10]], p[~tri][:, 0:3] - p[~tri][:, 4:5],
                          p[~tri][:, 0:3] + p[~tri][:, 4:5]])
    bvh = np.zeros((1, 2, 4), np.float32)
    bvh[0, 0, :3], bvh[0, 1, :3] = pts.min(0) - 1, pts.max(0) + 1
    bvh[0, 0, 3:].view(np.int32)[:] = 0
    bvh[0, 1, 3:].view(np.int32)[:] = p.shape[0]
    return bvh, np.arange(p.shape[0], dtype=np.int32)


# ---- materials --------------------------------------------------------------------------------------------------------------
def table(n_mats, seed):
    """n_mats distinct rows [n_mats, 8] = (albedo, materialType, emission, emissionPower).  Rows 0..3: the Lambert, mirror and glass
    spheres' and the floor's.  Then, as far as n_mats allows: pairs that differ only in the sign of a zero albedo component, in
    materialType, or by one ulp of emissionPower; emissive rows with distinct Le up to N_EMISSIVE in all; the rest random albedo,
    one in eight of them a mirror or glass."""
    rng = np.random.default_rng(seed)
    rows = [(0.7, 0.6, 0.5, 0.0, 0, 0, 0, 0), (0.95, 0.95, 0.95, -1.0, 0, 0, 0, 0), (1.0, 1.0, 1.0, 1.5, 0, 0, 0, 0),
            (0.8, 0.8, 0.6, 0.0, 0, 0, 0, 0)]
    t = np.zeros((n_mats, 8), np.float32)
    k = min(n_mats, len(rows))
    t[:k] = rows[:k]

    def put(row):
        nonlocal k
        if k < n_mats:
            t[k] = row
            k += 1

    for c in range(3):                                            # +0 / -0 in one albedo component
        alb = rng.uniform(0.2, 0.9, 3).astype(np.float32)
        for z in (0.0, -0.0):
            alb[c] = z
            put((*alb, 0.0, 0, 0, 0, 0))
    for _ in range(2):                                            # the same albedo as Lambert, mirror and glass
        alb = rng.uniform(0.2, 0.9, 3).astype(np.float32)
        for mt in (0.0, -1.0, 1.5):
            put((*alb, mt, 0, 0, 0, 0))
    n_em = 0
    for _ in range(3):                                            # emissionPower one ulp apart
        alb, em = rng.uniform(0.2, 0.9, 3).astype(np.float32), rng.uniform(0.2, 1.0, 3).astype(np.float32)
        pw = np.float32(rng.uniform(1.0, 3.0))
        for q in (pw, np.nextafter(pw, np.float32(4))):
            if k < n_mats:
                n_em += 1
            put((*alb, 0.0, *em, q))
    rest = n_mats - k                                             # the rest at once: the emissive rows first
    if rest > 0:
        e = min(rest, max(0, min(N_EMISSIVE, n_mats // 5) - n_em))
        t[k:, 0:3] = rng.uniform(0.1, 0.9, (rest, 3))
        t[k:k + e, 4:7] = rng.uniform(0.2, 1.0, (e, 3))
        t[k:k + e, 7] = rng.uniform(0.5, 4.0, e)
        t[k + e:, 3] = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 1.5], np.float32)[rng.integers(8, size=rest - e)]
    assert np.unique(t.view(np.uint32), axis=0).shape[0] == n_mats
    return t


def scene(name):
    """(prims [n, 12], mats [n, 8], n_mats) of a case."""
    if ("scene", name) not in _cache:
        K, n_mats, _ = CASES[name]
        prims = geometry(K)
        n = prims.shape[0]
        n_wall = n - 5
        rng = np.random.default_rng(2000 + sum(map(ord, name)))
        if n_mats is None:                                        # every primitive its own row
            n_mats = n
            t = table(n, 77 + K)
            row = np.concatenate([np.arange(4), rng.permutation(np.arange(4, n))])   # (the floor's second triangle has a row of its own here)
        else:
            pair = 2 if name == "collision" else 0
            base = n_mats - pair
            t = table(base, 77)                                   # (the collision case is the 200-row scene with two rows more)
            row = np.zeros(n, np.int64)
            row[0:3] = np.arange(3) % base
            row[3:5] = 3 % base
            deal = np.resize(rng.permutation(base), n_wall)       # every row, over and over ...
            wall = rng.permutation(deal)                          # ... in a shuffled order
            if pair:
                t = np.concatenate([t, colliding_pair()])
                slots = 3 + 16 * np.arange(64)                    # 64 wall primitives, 15 others between two of them
                rest = np.ones(n_wall, bool)
                rest[slots] = False
                wall[rest] = rng.permutation(np.resize(rng.permutation(base), int(rest.sum())))
                wall[slots] = base + (np.arange(64) & 1)          # the two rows alternately
            row[5:] = wall
        mats = np.ascontiguousarray(t[row])
        assert np.unique(row).size == n_mats
        mats.setflags(write=False)
        _cache["scene", name] = (prims, mats, int(n_mats))
    return _cache["scene", name]


def uniforms(name, w=W, h=H):
    from metalpathtracer_amd import host
    n = geometry(CASES[name][0]).shape[0]
    return host.make_uniforms(w, h, n, n - 3, cam=CAM)


def pixel_rays(u):
    """(origin [3], directions [H, W, 3]) through the pixel centres, as mpt_read_aovs defines them (tests/denoise_ref.py)."""
    F = np.float32
    Wd, Hh = int(u.screenSize[0]), int(u.screenSize[1])
    cam = np.array(u.cameraPosition[:3], np.float32)
    first = np.array(u.firstPixelPosition[:3], np.float32)
    vu, vv = np.array(u.viewportU[:3], np.float32), np.array(u.viewportV[:3], np.float32)
    uvx = ((np.arange(Wd, dtype=np.float32) + F(0.5)) / F(Wd))[None, :, None]
    uvy = ((np.arange(Hh, dtype=np.float32) + F(0.5)) / F(Hh))[:, None, None]
    d = ((first + uvx * vu) + uvy * vv) - cam
    d = d * (F(1) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None]
    return cam, d.astype(np.float32)
