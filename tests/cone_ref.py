"""numpy restatement of MPT_LIGHT_SAMPLING_CONE (include/mpt.h, "light sampling"): a sphere light sampled uniformly in the cone of
directions it subtends, in the direct-lighting pass and in mpt_render_nee.  Every step is a single IEEE float32 operation in the order
written there (cone_cap / cone_sample of metalpathtracer_amd/csrc/mpt_direct.h).  Everything the mode leaves alone is imported: the light
table, the selection of a light, the triangle sample and the image arithmetic from tests/direct_ref.py, the path loop's pieces from
tests/nee_ref.py, Philox / u01 / sincos_2pi / dot / normalize from tests/ao_ref.py; occlusion comes from tests/anyhit_ref.py (bounds), as
in those references.  Test code: the product never imports it."""
import numpy as np

import direct_ref
import nee_ref
from ao_ref import dot, normalize, philox4x32_10, sincos_2pi, u01
from direct_ref import INV_PI, TMAX_SCALE, WORD2

F = np.float32
U32 = np.uint32


def cone_cap(w, r, inv_pdf):
    """(dc2, omc, J, outside) of the sphere of radius r seen along w = c - o: omc = 1 - cos(theta_max), J = the reciprocal of the
    solid-angle pdf with the light's selection included; outside = dc2 > r2 (a NaN: False)."""
    dc2 = dot(w, w)
    r2 = r * r
    s2 = r2 / dc2
    cm = np.sqrt(F(1) - s2)
    omc = s2 / (F(1) + cm)
    J = omc * (inv_pdf / ((F(2) * r) * r))
    return dc2, omc, J, dc2 > r2


def cone_sample(w, dc2, omc, u1, u2):
    """(wi, dist): the direction drawn from (u1, u2) in the frame of Duff et al. 2017 around w / |w|, and the near intersection."""
    k = u1 * omc
    ct = F(1) - k
    st = np.sqrt(k * (F(2) - k))
    sn, cs = sincos_2pi(u2)
    dc = np.sqrt(dc2)
    wc = w * (F(1) / dc)[..., None]
    x, y, z = wc[..., 0], wc[..., 1], wc[..., 2]
    sg = np.where(z >= F(0), F(1), F(-1)).astype(np.float32)
    a = F(-1) / (sg + z)
    b = (x * y) * a
    t1 = np.stack([F(1) + ((sg * x) * x) * a, sg * b, -(sg * x)], -1)
    t2 = np.stack([b, sg + (y * y) * a, -y], -1)
    wi = normalize(((st * cs)[..., None] * t1 + (st * sn)[..., None] * t2) + ct[..., None] * wc)
    dist = dc * ct - np.sqrt(dc2 * ((omc * (F(1) - u1)) * ((F(2) - omc) - k)))
    return wi.astype(np.float32), dist.astype(np.float32)


def sphere_sample(o, n, c, r, inv_pdf, u1, u2):
    """The whole sphere rule at origins o with normals n: (wi, dist, cos_s, J, valid)."""
    w = c - o
    dc2, omc, J, outside = cone_cap(w, r, inv_pdf)
    wi, dist = cone_sample(w, dc2, omc, u1, u2)
    cos_s = dot(n, wi)
    return wi, dist, cos_s, J, outside & (cos_s > F(0)) & (dist > F(0))


# ---- the direct-lighting pass ---------------------------------------------------------------------------------------------------------
def sample_lights(o, n, pixel, table, begin, N, seed=(0, 0)):
    """direct_ref.sample_lights under CONE: (wi [..., N, 3], tmax [..., N], contribution [..., N, 3], valid [..., N]).  The samples that
    drew a triangle light are direct_ref's own; those that drew a sphere light follow the cone rule, contribution = Le * (cos_s * J)."""
    wi_a, tmax_a, contrib_a, valid_a = direct_ref.sample_lights(o, n, pixel, table, begin, N, seed)
    o = np.asarray(o, np.float32)[..., None, :]
    n = np.asarray(n, np.float32)[..., None, :]
    pixel = np.asarray(pixel, np.uint32)[..., None]
    s = (np.arange(N, dtype=np.uint64) + np.uint64(begin)).astype(np.uint32)
    old = np.seterr(all="ignore")
    try:
        r = philox4x32_10(pixel, s, U32(WORD2), U32(0), seed[0], seed[1])
        k = np.searchsorted(table.cdf, u01(r[0]), side="right")
        rec = table.rec[k]
        tri = rec[..., 0, 3] != 0
        wi, dist, cos_s, J, valid = sphere_sample(np.broadcast_to(o, wi_a.shape), np.broadcast_to(n, wi_a.shape), rec[..., 0, :3], rec[..., 1, 0],
                                                  rec[..., 3, 3], u01(r[1]), u01(r[2]))
        w = cos_s * J
        contrib = (rec[..., 3, :3] * w[..., None]).astype(np.float32)
        tmax = (dist * TMAX_SCALE).astype(np.float32)
    finally:
        np.seterr(**old)
    t3 = tri[..., None]
    return (np.where(t3, wi_a, wi).astype(np.float32), np.where(tri, tmax_a, tmax).astype(np.float32),
            np.where(t3, contrib_a, contrib).astype(np.float32), np.where(tri, valid_a, valid))


def samples(albedo_depth, normal_class, cam, table, begin, N, seed=(0, 0)):
    """direct_ref.samples under CONE: (origins [H,W,3], directions [H,W,N,3], tmax [H,W,N], contribution [H,W,N,3], skipped [H,W,N])."""
    o, wi, tmax, contrib, skipped = direct_ref.samples(albedo_depth, normal_class, cam, table, begin, N, seed)
    if table.n == 0:
        return o, wi, tmax, contrib, skipped
    nc = np.asarray(normal_class, np.float32)
    H, W = nc.shape[:2]
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pixel = (py * W + px).astype(np.uint32)
    wi, tmax, contrib, valid = sample_lights(o, nc[..., :3], pixel, table, begin, N, seed)
    return o, wi, tmax, contrib, ~(valid & (nc[..., 3] == 0)[..., None])


direct = direct_ref.direct                      # (the image from the samples: unchanged; pass sampled = samples(...))
occlusion_bounds = direct_ref.occlusion_bounds


# ---- mpt_render_nee -------------------------------------------------------------------------------------------------------------------
def light_weight(cos_s, J):
    """(wl, m) of a cone sample: the power heuristic of the solid-angle pdf against the cosine pdf, and the factor (cos_s * J) * wl."""
    pbs = cos_s * INV_PI
    q = pbs * J
    wl = F(1) / (F(1) + q * q)
    return wl, (cos_s * J) * wl


def bsdf_weight(o, c, r, inv_pdf, pb):
    """w of a sphere light a bounce from o found: 1 unless o lies outside the sphere, else the power heuristic of pb against the
    solid-angle pdf."""
    _, _, J, outside = cone_cap(c - o, r, inv_pdf)
    q = F(1) / (J * pb)
    return np.where(outside, F(1) / (F(1) + q * q), F(1)).astype(np.float32)


def light_sample(on, n, pixel, sample, b, table, seed):
    """nee_ref.light_sample under CONE: (k, wi, tmax, m, valid) with m the sample's factor, the MIS weight included."""
    k, wi_a, tmax_a, cos_s, cos_l, d2, valid_a = nee_ref.light_sample(on, n, pixel, sample, b, table, seed)
    rec = table.rec[k]
    tri = rec[:, 0, 3] != 0
    _, m_a = nee_ref.light_weight(cos_s, cos_l, d2, rec[:, 3, 3])
    r = philox4x32_10(pixel, sample, U32(b), U32(1), seed[0], seed[1])
    wi, dist, cos_c, J, valid = sphere_sample(on, n, rec[:, 0, :3], rec[:, 1, 0], rec[:, 3, 3], u01(r[1]), u01(r[2]))
    _, m = light_weight(cos_c, J)
    return (k, np.where(tri[:, None], wi_a, wi).astype(np.float32), np.where(tri, tmax_a, dist * TMAX_SCALE).astype(np.float32),
            np.where(tri, m_a, m).astype(np.float32), np.where(tri, valid_a, valid))


def render(u, buffers, table, first_hit, bounds, bsdf_mode=nee_ref.LAMBERT, max_depth=4, begin=0, count=1, seed=(0, 0), clamp=np.inf):
    """nee_ref.render under CONE, with the same result dict.  The loop is nee_ref.render's; the two places the mode changes are the
    weight of a sphere light a bounce finds and the light sample."""
    bvh, prims, mats, _ = buffers
    mats = np.asarray(mats, np.float32).reshape(-1, 2, 4)
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    prim_count = int(u.primitiveCount)
    clamp = F(clamp)
    py, px, sj = np.meshgrid(np.arange(H), np.arange(W), np.arange(count), indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    pixel = (py * W + px).astype(np.uint32)
    sample = (sj.reshape(-1).astype(np.uint64) + np.uint64(begin)).astype(np.uint32)
    n_paths = pixel.size
    old = np.seterr(all="ignore")
    try:
        o, d = nee_ref.primary_rays(u, pixel, px, py, sample, seed)
        thr = np.ones((n_paths, 3), np.float32)
        L = np.zeros((n_paths, 3), np.float32)
        La = np.zeros(n_paths, np.float32)
        pb = np.zeros(n_paths, np.float32)
        sampled = np.zeros(n_paths, bool)
        alive = np.ones(n_paths, bool)
        rays = np.zeros(n_paths, np.uint32)
        n_shadow = np.zeros(n_paths, np.uint32)
        n_occ = np.zeros(n_paths, np.uint32)
        gap = np.zeros(n_paths, bool)
        mis_lights = set()
        for b in range(max_depth):
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                break
            t = np.full(n_paths, np.inf, np.float32)
            prim = np.full(n_paths, -1, np.int64)
            n = np.zeros((n_paths, 3), np.float32)
            front = np.zeros(n_paths, bool)
            for i in idx:
                ti, pi, ni, fi = first_hit(o[i], d[i], buffers)
                if pi >= 0:
                    t[i], prim[i], n[i], front[i] = ti, pi, ni, fi
            rays[idx] += 1
            miss = alive & (prim < 0)
            ud = normalize(d)
            tt = F(0.5) * (ud[:, 1] + F(1))
            sky = np.stack([F(1) + nee_ref.SKY[0] * tt, F(1) + nee_ref.SKY[1] * tt, F(1) + nee_ref.SKY[2] * tt], -1).astype(np.float32)
            L = np.where(miss[:, None], L + thr * sky, L)
            La = np.where(miss, La + F(1), La)
            hit = alive & (prim >= 0) & (prim < prim_count)
            alive = hit.copy()
            pr = np.maximum(prim, 0)
            albedo, mtype, emission, power = mats[pr, 0, :3], mats[pr, 0, 3], mats[pr, 1, :3], mats[pr, 1, 3]
            point = o + t[:, None] * d
            # emission: a triangle light is weighted as under AREA, a sphere light by the cone seen from the ray's origin
            emit = hit & ((power > F(0)) | (mtype == F(2)))
            if table.n:
                k = np.minimum(np.searchsorted(table.ids, pr), table.n - 1)
                found = table.ids[k] == pr
                tri = table.rec[k, 0, 3] != 0
                inv_pdf = table.rec[k, 3, 3]
                w_tri = nee_ref.bsdf_weight(t, -dot(n, d), inv_pdf, pb)
                w_sph = bsdf_weight(o, table.rec[k, 0, :3], table.rec[k, 1, 0], inv_pdf, pb)
                weighted = sampled & found & (tri | front)
                w = np.where(weighted, np.where(tri, w_tri, w_sph), F(1)).astype(np.float32)
                mis_lights.update(k[emit & weighted].tolist())
            else:
                w = np.ones(n_paths, np.float32)
            L = np.where(emit[:, None], L + ((thr * emission) * power[:, None]) * w[:, None], L)
            La = np.where(emit, La + power, La)
            # the bounce
            rb = philox4x32_10(pixel, sample, U32(b), U32(0), seed[0], seed[1])
            z = F(2) * u01(rb[0]) - F(1)
            sn, cs = sincos_2pi(u01(rb[1]))
            rr = np.sqrt(F(1) - z * z)
            ruv = np.stack([rr * cs, rr * sn, z], -1).astype(np.float32)
            lambert = hit & ((mtype == F(0)) if bsdf_mode != nee_ref.LAMBERT else True)
            nd_l = normalize(n + ruv)
            on = point + nee_ref.EPS * n
            attempt = lambert & (table.n > 0) & (b + 1 < max_depth)
            ia = np.nonzero(attempt)[0]
            if ia.size:
                k, wi, tmax, m, valid = light_sample(on[ia], n[ia], pixel[ia], sample[ia], b, table, seed)
                iv, kv = ia[valid], k[valid]
                if iv.size:
                    (lo, up), = bounds(on[iv], wi[valid], [tmax[valid]], buffers)
                    n_shadow[iv] += 1
                    n_occ[iv[lo]] += 1
                    gap[iv[up & ~lo]] = True
                    contrib = ((thr[iv] * albedo[iv]) * INV_PI) * (table.rec[kv, 3, :3] * m[valid][:, None])
                    vis = iv[~lo]
                    L[vis] = L[vis] + contrib[~lo]
            pb = np.where(lambert, dot(n, nd_l) * INV_PI, pb).astype(np.float32)
            sampled = attempt
            # mirror / dielectric (MPT_BSDF_SCATTER, materialType != 0)
            ri = np.where(front, F(1) / mtype, mtype).astype(np.float32)
            refl = nee_ref._reflect(d, n)
            nd_d = normalize(np.where(nee_ref._mirror_angle(ri, n, d, u01(rb[2]))[:, None], refl, nee_ref._refract(d, n, ri)))
            through = hit & ~lambert & (mtype > F(0)) & (dot(nd_d, n) < F(0))
            nd = np.where(lambert[:, None], nd_l, np.where((mtype < F(0))[:, None], normalize(refl), nd_d)).astype(np.float32)
            o = np.where(hit[:, None], np.where(through[:, None], point - nee_ref.EPS * n, on), o).astype(np.float32)
            d = np.where(hit[:, None], nd, d).astype(np.float32)
            thr = np.where(hit[:, None], thr * albedo, thr).astype(np.float32)
        value = np.concatenate([np.where(L > F(0), np.minimum(L, clamp), F(0)), np.fmin(np.fmax(La, F(0)), F(1))[:, None]], -1)
    finally:
        np.seterr(**old)
    assert value.dtype == np.float32 and L.dtype == np.float32 and thr.dtype == np.float32
    shape = (H, W, count)
    return dict(value=value.reshape(shape + (4,)), rays=rays.reshape(shape), shadow=n_shadow.reshape(shape), occluded=n_occ.reshape(shape),
                gap=gap.reshape(shape), mis_lights=np.array(sorted(mis_lights), np.int64))


accumulate = nee_ref.accumulate
