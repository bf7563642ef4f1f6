"""numpy restatement of the light table and the direct-lighting pass of include/mpt.h (mpt_light_info, mpt_direct_params): the table's
weights in float64 from the float32 records, every step of the pass a single IEEE float32 operation in the order of k_direct
(metalpathtracer_amd/csrc/mpt_direct.h).  Occlusion is not computed here: it comes from tests/anyhit_ref.py (bounds), whose `lower` is
what MPT_WALK_REFERENCE must answer and whose `upper & ~lower` are the gap rays the own-tree walk may answer either way.  Test code: the
product never imports it."""
import numpy as np

from ao_ref import _cam, dot, normalize, philox4x32_10, sincos_2pi, u01

F = np.float32
U32 = np.uint32
WORD2 = 0xFFFFFFFD          # Philox counter word 2 of a light sample: no bounce has it, the jitter has ...FF, AO ...FE
TMAX_SCALE = F(0.9990234375)   # 1 - 2^-10
INV_PI = F(0.31830987)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


class LightTable:
    """ids [n] int32 ascending, rec [n,4,4] float32 = (v0 | c, type) (e1 | r 0 0, 0) (e2 | 0, 0) (Le, inv_pdf), cdf [n] float32; and for
    the tests the float64 area A, luminance l and selection probability pmf of every light, and the number of emissive primitives."""

    def __init__(self, ids, rec, cdf, A, l, pmf, seen):
        self.ids, self.rec, self.cdf, self.A, self.l, self.pmf, self.seen = ids, rec, cdf, A, l, pmf, seen

    @property
    def n(self):
        return self.ids.shape[0]


def light_table(prims, mats):
    """From the caller-format arrays: prims [P,3,4] = (v0 | c, type) (v1 | r.., .) (v2, .), mats [P,2,4] = (albedo, type) (emission, power)."""
    p = np.asarray(prims, np.float32).reshape(-1, 3, 4)
    m = np.asarray(mats, np.float32).reshape(-1, 2, 4)
    emissive = np.nonzero(m[:, 1, 3] > 0)[0]
    rec = np.zeros((emissive.size, 4, 4), np.float32)
    A = np.zeros(emissive.size, np.float64)
    with np.errstate(all="ignore"):
        for j, i in enumerate(emissive):
            tri = int(p[i, 0, 3]) == 1
            rec[j, 0, :3] = p[i, 0, :3]
            rec[j, 0, 3] = F(1) if tri else F(0)
            if tri:
                rec[j, 1, :3] = p[i, 1, :3] - p[i, 0, :3]
                rec[j, 2, :3] = p[i, 2, :3] - p[i, 0, :3]
                c = cross(rec[j, 1, :3].astype(np.float64), rec[j, 2, :3].astype(np.float64))
                A[j] = 0.5 * np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
            else:
                r = p[i, 1, 0] if int(p[i, 0, 3]) == 0 else F(np.nan)      # (anything else is never hit: a sphere of radius NaN)
                rec[j, 1, 0] = r
                A[j] = ((4.0 * np.pi) * np.float64(r)) * np.float64(r)
            rec[j, 3, :3] = m[i, 1, :3] * m[i, 1, 3]
        Le = rec[:, 3, :3].astype(np.float64)
        l = (0.2126 * Le[:, 0] + 0.7152 * Le[:, 1]) + 0.0722 * Le[:, 2]
        Wk = A * l
        keep = np.isfinite(Wk) & (Wk != 0)
    ids, rec, A, l, Wk = emissive[keep].astype(np.int32), rec[keep], A[keep], l[keep], Wk[keep]
    Ck = np.zeros(ids.size, np.float64)
    C = 0.0
    for k in range(ids.size):                       # the running sum, in table order
        C = C + Wk[k]
        Ck[k] = C
    cdf = (Ck / C).astype(np.float32) if ids.size else np.zeros(0, np.float32)
    if ids.size:
        cdf[-1] = F(1)
        rec[:, 3, 3] = (C / l).astype(np.float32)
    return LightTable(ids, rec, cdf, A, l, Wk / C if ids.size else Wk, int(emissive.size))


def sample_lights(o, n, pixel, table, begin, N, seed=(0, 0)):
    """Samples [begin, begin + N) of shading points o [..., 3] with normals n [..., 3] and Philox pixel indices `pixel` [...]:
    (wi [..., N, 3], tmax [..., N], contribution [..., N, 3] = Le * ((cos_s cos_l / d2) * inv_pdf), valid [..., N]: not skipped)."""
    o = np.asarray(o, np.float32)[..., None, :]
    n = np.asarray(n, np.float32)[..., None, :]
    pixel = np.asarray(pixel, np.uint32)[..., None]
    s = (np.arange(N, dtype=np.uint64) + np.uint64(begin)).astype(np.uint32)
    old = np.seterr(all="ignore")
    try:
        r = philox4x32_10(pixel, s, U32(WORD2), U32(0), seed[0], seed[1])
        u = u01(r[0])
        k = np.searchsorted(table.cdf, u, side="right")          # the smallest k with u < cdf[k]
        assert (k < table.n).all()
        rec = table.rec[k]                                        # [..., N, 4, 4]
        tri = rec[..., 0, 3] != 0
        c, e1, e2 = rec[..., 0, :3], rec[..., 1, :3], rec[..., 2, :3]
        ua, ub = u01(r[1]), u01(r[2])
        flip = (ua + ub) > F(1)
        a = np.where(flip, F(1) - ua, ua)
        b = np.where(flip, F(1) - ub, ub)
        pt = (c + a[..., None] * e1) + b[..., None] * e2
        ng = normalize(cross(e1, e2))
        z = F(2) * ua - F(1)
        sn, cs = sincos_2pi(ub)
        rr = np.sqrt(F(1) - z * z)
        ns = np.stack([rr * cs, rr * sn, z], -1).astype(np.float32)
        ps = c + rec[..., 1, 0:1] * ns
        nl = np.where(tri[..., None], ng, ns)
        p = np.where(tri[..., None], pt, ps)
        v = p - o
        d2 = dot(v, v)
        dist = np.sqrt(d2)
        wi = (v * (F(1) / dist)[..., None]).astype(np.float32)
        cos_s = dot(np.broadcast_to(n, wi.shape), wi)
        dl = dot(nl, wi)
        cos_l = np.where(tri, np.abs(dl), -dl)
        valid = (d2 > F(0)) & (cos_s > F(0)) & (cos_l > F(0))
        tmax = (dist * TMAX_SCALE).astype(np.float32)
        g = (cos_s * cos_l) / d2
        w = g * rec[..., 3, 3]
        contrib = (rec[..., 3, :3] * w[..., None]).astype(np.float32)
    finally:
        np.seterr(**old)
    assert wi.dtype == np.float32 and tmax.dtype == np.float32 and contrib.dtype == np.float32
    return wi, tmax, contrib, valid


def samples(albedo_depth, normal_class, cam, table, begin, N, seed=(0, 0)):
    """The samples of the pass: (origins [H,W,3], directions [H,W,N,3], tmax [H,W,N], contribution [H,W,N,3], skipped [H,W,N]).  A pixel
    that is no surface has every sample skipped; the rows of skipped samples are not to be used."""
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    H, W = ad.shape[:2]
    cam_p, first, vu, vv = _cam(cam)
    surface = nc[..., 3] == 0
    with np.errstate(all="ignore"):
        px, py = np.meshgrid(np.arange(W), np.arange(H))
        uvx = ((px.astype(np.float32) + F(0.5)) / F(W))[..., None]
        uvy = ((py.astype(np.float32) + F(0.5)) / F(H))[..., None]
        dc = normalize(((first + uvx * vu) + uvy * vv) - cam_p)
        n = nc[..., :3]
        o = ((cam_p + ad[..., 3:4] * dc) + F(0.0001) * n).astype(np.float32)
    pixel = (py * W + px).astype(np.uint32)
    if table.n == 0:
        z = np.zeros((H, W, N, 3), np.float32)
        return o, z, np.zeros((H, W, N), np.float32), z, np.ones((H, W, N), bool)
    wi, tmax, contrib, valid = sample_lights(o, n, pixel, table, begin, N, seed)
    return o, wi, tmax, contrib, ~(valid & surface[..., None])


def direct(albedo_depth, normal_class, cam, table, begin, N, seed, occluded, sampled=None):
    """(rgba [H,W,4] float32, traced [H,W] uint32, unoccluded [H,W] uint32) with the occlusion array `occluded` [H,W,N] bool (read where
    a sample is not skipped).  sampled: the result of samples() for the same arguments (computed here when None)."""
    ad = np.asarray(albedo_depth, np.float32)
    o, wi, tmax, contrib, skipped = sampled if sampled is not None else samples(ad, normal_class, cam, table, begin, N, seed)
    H, W = ad.shape[:2]
    open_ = ~skipped & ~np.asarray(occluded, bool)
    S = np.zeros((H, W, 3), np.float32)
    with np.errstate(all="ignore"):
        for s in range(N):                                       # the sum runs in ascending s
            S = np.where(open_[..., s, None], S + contrib[..., s, :], S)
        rgb = (ad[..., :3] * INV_PI) * (S / F(N))
    surface = np.asarray(normal_class, np.float32)[..., 3] == 0
    rgba = np.concatenate([np.where(surface[..., None], rgb, F(0)), np.ones((H, W, 1), np.float32)], -1).astype(np.float32)
    return rgba, (~skipped).sum(-1).astype(np.uint32), open_.sum(-1).astype(np.uint32)


def occlusion_bounds(sampled, buffers, bounds):
    """(lower, upper) [H,W,N] bool of the samples that are not skipped (False elsewhere), through anyhit_ref.bounds."""
    o, wi, tmax, _, skipped = sampled
    lower = np.zeros(skipped.shape, bool)
    upper = np.zeros(skipped.shape, bool)
    live = ~skipped
    if live.any():
        oo = np.broadcast_to(o[:, :, None, :], wi.shape)[live]
        (lo, up), = bounds(oo, wi[live], [tmax[live]], buffers)
        lower[live], upper[live] = lo, up
    return lower, upper
