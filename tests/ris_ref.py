"""numpy restatement of the "light candidates" section of include/mpt.h (mpt_set_light_candidates: resampled light sampling in the
direct pass and in mpt_render_nee; ris_pick of metalpathtracer_amd/csrc/mpt_ris.h).  Every step is a single IEEE float32 operation in
the order written there.  What the setting leaves alone is imported: the light table, the image arithmetic and the occlusion bounds from
tests/direct_ref.py, the cone of a sphere light from tests/cone_ref.py, the MIS weights and the pieces of the path loop from
tests/nee_ref.py and tests/cone_ref.py, Philox / u01 / sincos_2pi / dot / normalize from tests/ao_ref.py.  A candidate's geometry is
written out here once for any Philox block (the references above fix the block's last word); with M = 1 it is held to theirs bit for bit
by tests/test_ris_cpu.py.  Occlusion comes from tests/anyhit_ref.py (bounds) and gap rays are marked as in tests/nee_ref.py.  Test code:
the product never imports it."""
import numpy as np

import cone_ref
import direct_ref
import nee_ref
from ao_ref import dot, normalize, philox4x32_10, sincos_2pi, u01
from direct_ref import INV_PI, TMAX_SCALE, WORD2, cross

F = np.float32
U32 = np.uint32
M_MAX = 32
LUM = (F(0.2126), F(0.7152), F(0.0722))


def luminance(Le):
    """l = (0.2126f * Le.r + 0.7152f * Le.g) + 0.0722f * Le.b in float32."""
    return ((LUM[0] * Le[..., 0] + LUM[1] * Le[..., 1]) + LUM[2] * Le[..., 2]).astype(np.float32)


def candidate(r, o, n, table, cone):
    """The sample the Philox block r = (x, y, z, w) [n each] forms at the points o [n,3] with normals n [n,3]: a dict of k, tri, Le,
    inv_pdf, wi, dist, cos_s, cos_l, d2, J (0 unless a sphere under cone) and ok (not skipped)."""
    k = np.searchsorted(table.cdf, u01(r[0]), side="right")          # the smallest k with u < cdf[k]
    assert (k < table.n).all()
    rec = table.rec[k]
    tri = rec[:, 0, 3] != 0
    c, e1, e2 = rec[:, 0, :3], rec[:, 1, :3], rec[:, 2, :3]
    ua, ub = u01(r[1]), u01(r[2])
    flip = (ua + ub) > F(1)
    a = np.where(flip, F(1) - ua, ua)
    b = np.where(flip, F(1) - ub, ub)
    pt = (c + a[:, None] * e1) + b[:, None] * e2
    ng = normalize(cross(e1, e2))
    z = F(2) * ua - F(1)
    sn, cs = sincos_2pi(ub)
    rr = np.sqrt(F(1) - z * z)
    ns = np.stack([rr * cs, rr * sn, z], -1).astype(np.float32)
    ps = c + rec[:, 1, 0:1] * ns
    area_sphere = ~tri & (not cone)
    nl = np.where(area_sphere[:, None], ns, ng)
    p = np.where(area_sphere[:, None], ps, pt)
    v = p - o
    d2 = dot(v, v)
    dist = np.sqrt(d2)
    wi = (v * (F(1) / dist)[:, None]).astype(np.float32)
    cos_s = dot(n, wi)
    dl = dot(nl, wi)
    cos_l = np.where(area_sphere, -dl, np.abs(dl))
    ok = (d2 > F(0)) & (cos_s > F(0)) & (cos_l > F(0))
    J = np.zeros(k.shape, np.float32)
    if cone:
        wi_c, dist_c, cos_c, J_c, ok_c = cone_ref.sphere_sample(o, n, c, rec[:, 1, 0], rec[:, 3, 3], ua, ub)
        wi = np.where(tri[:, None], wi, wi_c).astype(np.float32)
        dist = np.where(tri, dist, dist_c)
        cos_s = np.where(tri, cos_s, cos_c)
        ok = np.where(tri, ok, ok_c)
        J = np.where(tri, F(0), J_c)
    return dict(k=k, tri=tri, Le=rec[:, 3, :3], inv_pdf=rec[:, 3, 3], wi=wi, dist=dist.astype(np.float32), cos_s=cos_s.astype(np.float32),
                cos_l=cos_l.astype(np.float32), d2=d2.astype(np.float32), J=J.astype(np.float32), ok=ok)


def factor(cd, cone, nee):
    """fac_j of the direct pass, or (nee) m_j of the render: the factor times its power-heuristic weight against the bounce's pdf."""
    if nee:
        _, m = nee_ref.light_weight(cd["cos_s"], cd["cos_l"], cd["d2"], cd["inv_pdf"])
        if cone:
            _, m_c = cone_ref.light_weight(cd["cos_s"], cd["J"])
            m = np.where(cd["tri"], m, m_c)
        return m.astype(np.float32)
    fac = ((cd["cos_s"] * cd["cos_l"]) / cd["d2"]) * cd["inv_pdf"]
    if cone:
        fac = np.where(cd["tri"], fac, cd["cos_s"] * cd["J"])
    return fac.astype(np.float32)


def pick(o, n, c0, c1, c2, c3, M, table, seed, cone, nee, active=None):
    """The reservoir over candidates j = 0 .. M-1 from the blocks philox(c0, c1, c2, c3 + j) at the points o [n,3] with normals n:
    a dict of taken [n] bool, wi [n,3], tmax [n], C [n,3] = Le_y * Fy, k [n] (the light kept), Fy, wsum, and counted [n] (how many
    candidates counted)."""
    o = np.asarray(o, np.float32)
    n = np.asarray(n, np.float32)
    cnt = o.shape[0]
    active = np.ones(cnt, bool) if active is None else np.asarray(active, bool)
    wsum = np.zeros(cnt, np.float32)
    taken = np.zeros(cnt, bool)
    counted = np.zeros(cnt, np.uint32)
    y = dict(wi=np.ones((cnt, 3), np.float32), dist=np.zeros(cnt, np.float32), Le=np.zeros((cnt, 3), np.float32), l=np.ones(cnt, np.float32),
             k=np.zeros(cnt, np.int64))
    old = np.seterr(all="ignore")
    try:
        for j in range(M):
            r = philox4x32_10(c0, c1, c2, U32(c3 + j), seed[0], seed[1])
            cd = candidate(r, o, n, table, cone)
            l = luminance(cd["Le"])
            w = (l * factor(cd, cone, nee)).astype(np.float32)
            counts = active & cd["ok"] & (w > F(0)) & (w < F(np.inf))
            wsum = np.where(counts, wsum + w, wsum).astype(np.float32)
            take = counts & (~taken | (u01(r[3]) * wsum < w))
            y["wi"] = np.where(take[:, None], cd["wi"], y["wi"])
            y["dist"] = np.where(take, cd["dist"], y["dist"])
            y["Le"] = np.where(take[:, None], cd["Le"], y["Le"])
            y["l"] = np.where(take, l, y["l"])
            y["k"] = np.where(take, cd["k"], y["k"])
            taken = taken | counts
            counted += counts
        Fy = ((wsum / F(M)) / y["l"]).astype(np.float32)
        C = (y["Le"] * Fy[:, None]).astype(np.float32)
        tmax = (y["dist"] * TMAX_SCALE).astype(np.float32)
    finally:
        np.seterr(**old)
    assert C.dtype == np.float32 and wsum.dtype == np.float32 and y["wi"].dtype == np.float32
    return dict(taken=taken, wi=y["wi"], tmax=tmax, C=C, k=y["k"], Fy=Fy, wsum=wsum, counted=counted)


# ---- the direct-lighting pass ---------------------------------------------------------------------------------------------------------
def samples(albedo_depth, normal_class, cam, table, begin, N, M, seed=(0, 0), cone=False):
    """direct_ref.samples with every sample resampled from M candidates: (origins [H,W,3], directions [H,W,N,3], tmax [H,W,N],
    contribution [H,W,N,3] = Le_y * Fy, skipped [H,W,N]).  direct_ref.direct and direct_ref.occlusion_bounds take it as it is."""
    o, wi0, tmax0, contrib0, skipped0 = direct_ref.samples(albedo_depth, normal_class, cam, table, begin, 1, seed)
    nc = np.asarray(normal_class, np.float32)
    H, W = nc.shape[:2]
    if table.n == 0:
        z = np.zeros((H, W, N, 3), np.float32)
        return o, z, np.zeros((H, W, N), np.float32), z, np.ones((H, W, N), bool)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    pixel = np.broadcast_to((py * W + px).astype(np.uint32)[..., None], (H, W, N)).reshape(-1)
    s = np.broadcast_to((np.arange(N, dtype=np.uint64) + np.uint64(begin)).astype(np.uint32), (H, W, N)).reshape(-1)
    oo = np.broadcast_to(o[:, :, None, :], (H, W, N, 3)).reshape(-1, 3)
    nn = np.broadcast_to(nc[:, :, None, :3], (H, W, N, 3)).reshape(-1, 3)
    surface = np.broadcast_to((nc[..., 3] == 0)[..., None], (H, W, N)).reshape(-1)
    p = pick(oo, nn, pixel, s, U32(WORD2), 0, M, table, seed, cone, False, active=surface)
    return (o, p["wi"].reshape(H, W, N, 3), p["tmax"].reshape(H, W, N), p["C"].reshape(H, W, N, 3), ~p["taken"].reshape(H, W, N))


direct = direct_ref.direct                      # (the image from the samples: unchanged; pass sampled = samples(...))
occlusion_bounds = direct_ref.occlusion_bounds


# ---- mpt_render_nee -------------------------------------------------------------------------------------------------------------------
def render(u, buffers, table, first_hit, bounds, M, cone=False, bsdf_mode=nee_ref.LAMBERT, max_depth=4, begin=0, count=1, seed=(0, 0),
           clamp=np.inf):
    """nee_ref.render (cone: cone_ref.render) with the light sample of a vertex resampled from M candidates, with the same result dict.
    The loop is theirs; the one place the setting changes is the light sample."""
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
            # emission: the M = 1 branch under the sampling mode in effect
            emit = hit & ((power > F(0)) | (mtype == F(2)))
            if table.n:
                k = np.minimum(np.searchsorted(table.ids, pr), table.n - 1)
                found = table.ids[k] == pr
                tri = table.rec[k, 0, 3] != 0
                inv_pdf = table.rec[k, 3, 3]
                w = nee_ref.bsdf_weight(t, -dot(n, d), inv_pdf, pb)
                if cone:
                    w = np.where(tri, w, cone_ref.bsdf_weight(o, table.rec[k, 0, :3], table.rec[k, 1, 0], inv_pdf, pb))
                weighted = sampled & found & (tri | front)
                w = np.where(weighted, w, F(1)).astype(np.float32)
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
                # the light sample: resampled from the blocks (pixel, sample, b, 1 + j)
                p = pick(on[ia], n[ia], pixel[ia], sample[ia], U32(b), 1, M, table, seed, cone, True)
                valid = p["taken"]
                iv = ia[valid]
                if iv.size:
                    (lo, up), = bounds(on[iv], p["wi"][valid], [p["tmax"][valid]], buffers)
                    n_shadow[iv] += 1
                    n_occ[iv[lo]] += 1
                    gap[iv[up & ~lo]] = True
                    contrib = ((thr[iv] * albedo[iv]) * INV_PI) * p["C"][valid]
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
