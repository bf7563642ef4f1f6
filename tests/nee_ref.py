"""numpy restatement of the next-event-estimation render of include/mpt.h (mpt_nee_params): every step a single IEEE float32 operation in
the order written there (and in k_nee, metalpathtracer_amd/csrc/mpt_nee.h).  All paths advance together, one bounce per step — a path's
geometry does not depend on what its shadow rays find.  Closest hits come from the oracle (oracle.binding.first_hit on the host-built
tree), occlusion from tests/anyhit_ref.py (bounds): `lower` is what MPT_WALK_REFERENCE must answer and gives the values here; a sample
with a ray in `upper & ~lower` (a gap ray: the own-tree walk may answer either way) is marked.  Philox, u01, sincos_2pi and the light
table are the existing reference modules'.  Test code: the product never imports it."""
import numpy as np

from ao_ref import _cam, dot, normalize, philox4x32_10, sincos_2pi, u01
from direct_ref import INV_PI, TMAX_SCALE, cross

F = np.float32
U32 = np.uint32
LAMBERT, SCATTER = 0, 1
EPS = F(0.0001)
SKY = (F(0.6) - F(1.0), F(0.7) - F(1.0), F(1.0) - F(1.0))     # the constants of shade_bounce, folded in float32


def primary_rays(u, pixel, px, py, sample, seed):
    """(o [n,3], d [n,3]) of mpt_render's philox primary rays: jitter block (pixel, sample, 0xFFFFFFFF, 0)."""
    cam, first, vu, vv = _cam(u)
    Wf, Hf = F(u.screenSize[0]), F(u.screenSize[1])
    r = philox4x32_10(pixel, sample, U32(0xFFFFFFFF), U32(0), seed[0], seed[1])
    uvx = (px.astype(np.float32) + F(0.5)) / Wf
    uvy = (py.astype(np.float32) + F(0.5)) / Hf
    x_off = (u01(r[0]) - F(0.5)) / Wf
    y_off = (u01(r[1]) - F(0.5)) / Hf
    dv = ((first + (uvx + x_off)[:, None] * vu) + (uvy + y_off)[:, None] * vv) - cam
    return np.broadcast_to(cam, dv.shape).astype(np.float32), normalize(dv).astype(np.float32)


def light_sample(on, n, pixel, sample, b, table, seed):
    """The direct-lighting pass's sample from block (pixel, sample, b, 1) at the points `on` with normals n:
    (k, wi, tmax, cos_s, cos_l, d2, valid)."""
    r = philox4x32_10(pixel, sample, U32(b), U32(1), seed[0], seed[1])
    k = np.searchsorted(table.cdf, u01(r[0]), side="right")          # the smallest k with u < cdf[k]
    assert (k < table.n).all()
    rec = table.rec[k]
    tri = rec[:, 0, 3] != 0
    c, e1, e2 = rec[:, 0, :3], rec[:, 1, :3], rec[:, 2, :3]
    ua, ub = u01(r[1]), u01(r[2])
    flip = (ua + ub) > F(1)
    a = np.where(flip, F(1) - ua, ua)
    bb = np.where(flip, F(1) - ub, ub)
    pt = (c + a[:, None] * e1) + bb[:, None] * e2
    ng = normalize(cross(e1, e2))
    z = F(2) * ua - F(1)
    sn, cs = sincos_2pi(ub)
    rr = np.sqrt(F(1) - z * z)
    ns = np.stack([rr * cs, rr * sn, z], -1).astype(np.float32)
    ps = c + rec[:, 1, 0:1] * ns
    nl = np.where(tri[:, None], ng, ns)
    p = np.where(tri[:, None], pt, ps)
    v = p - on
    d2 = dot(v, v)
    dist = np.sqrt(d2)
    wi = (v * (F(1) / dist)[:, None]).astype(np.float32)
    cos_s = dot(n, wi)
    dl = dot(nl, wi)
    cos_l = np.where(tri, np.abs(dl), -dl)
    valid = (d2 > F(0)) & (cos_s > F(0)) & (cos_l > F(0))
    return k, wi, (dist * TMAX_SCALE).astype(np.float32), cos_s, cos_l, d2, valid


def light_weight(cos_s, cos_l, d2, inv_pdf):
    """(wl, m) of a light sample: the power heuristic against the cosine pdf, and the sample's factor (g * inv_pdf) * wl."""
    g = (cos_s * cos_l) / d2
    pl = d2 / (cos_l * inv_pdf)
    pbs = cos_s * INV_PI
    q = pbs / pl
    wl = F(1) / (F(1) + q * q)
    return wl, (g * inv_pdf) * wl


def bsdf_weight(t, cos_l, inv_pdf, pb):
    """w of an emitter a bounce found: the power heuristic of the bounce's pdf pb against the light sample's."""
    pl = (t * t) / (cos_l * inv_pdf)
    q = pl / pb
    return F(1) / (F(1) + q * q)


def _reflect(i, n):
    return i - (F(2) * dot(n, i))[:, None] * n


def _refract(i, n, eta):
    dd = dot(n, i)
    k = F(1) - (eta * eta) * (F(1) - dd * dd)
    out = eta[:, None] * i - (eta * dd + np.sqrt(k))[:, None] * n
    return np.where((k < F(0))[:, None], F(0), out).astype(np.float32)


def _mirror_angle(ri, n, d, uu):
    cos_t = dot(F(-1) * d, n)
    sin_t = np.sqrt(F(1) - cos_t * cos_t)
    r0 = (F(1) - ri) / (F(1) + ri)
    r0 = r0 * r0
    m = F(1) - cos_t
    m2 = m * m
    refl = r0 + (F(1) - r0) * ((m2 * m2) * m)
    return (ri * sin_t > F(1)) | (refl > uu)


def render(u, buffers, table, first_hit, bounds, bsdf_mode=LAMBERT, max_depth=4, begin=0, count=1, seed=(0, 0), clamp=np.inf):
    """Samples [begin, begin + count) of every pixel.  A dict of arrays over [H, W, count]: value [.., 4] (the per-sample value with the
    reference-order occlusion), rays, shadow, occluded (counts per sample) and gap (bool: the sample holds a gap shadow ray); and
    mis_lights, the table indices of the lights whose emission, found by a bounce, was weighted against a light sample."""
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
        o, d = primary_rays(u, pixel, px, py, sample, seed)
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
            sky = np.stack([F(1) + SKY[0] * tt, F(1) + SKY[1] * tt, F(1) + SKY[2] * tt], -1).astype(np.float32)
            L = np.where(miss[:, None], L + thr * sky, L)
            La = np.where(miss, La + F(1), La)
            hit = alive & (prim >= 0) & (prim < prim_count)            # (beyond primitiveCount: the material guard ends the path)
            alive = hit.copy()
            pr = np.maximum(prim, 0)
            albedo, mtype, emission, power = mats[pr, 0, :3], mats[pr, 0, 3], mats[pr, 1, :3], mats[pr, 1, 3]
            point = o + t[:, None] * d
            # emission
            emit = hit & ((power > F(0)) | (mtype == F(2)))
            if table.n:
                k = np.minimum(np.searchsorted(table.ids, pr), table.n - 1)
                found = table.ids[k] == pr
                tri = table.rec[k, 0, 3] != 0
                inv_pdf = table.rec[k, 3, 3]
                w = bsdf_weight(t, -dot(n, d), inv_pdf, pb)
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
            lambert = hit & ((mtype == F(0)) if bsdf_mode != LAMBERT else True)
            nd_l = normalize(n + ruv)
            on = point + EPS * n
            attempt = lambert & (table.n > 0) & (b + 1 < max_depth)
            ia = np.nonzero(attempt)[0]
            if ia.size:
                k, wi, tmax, cos_s, cos_l, d2, valid = light_sample(on[ia], n[ia], pixel[ia], sample[ia], b, table, seed)
                iv, kv = ia[valid], k[valid]
                if iv.size:
                    (lo, up), = bounds(on[iv], wi[valid], [tmax[valid]], buffers)
                    n_shadow[iv] += 1
                    n_occ[iv[lo]] += 1
                    gap[iv[up & ~lo]] = True
                    _, m = light_weight(cos_s[valid], cos_l[valid], d2[valid], table.rec[kv, 3, 3])
                    contrib = ((thr[iv] * albedo[iv]) * INV_PI) * (table.rec[kv, 3, :3] * m[:, None])
                    vis = iv[~lo]
                    L[vis] = L[vis] + contrib[~lo]
            pb = np.where(lambert, dot(n, nd_l) * INV_PI, pb).astype(np.float32)
            sampled = attempt
            # mirror / dielectric (MPT_BSDF_SCATTER, materialType != 0)
            ri = np.where(front, F(1) / mtype, mtype).astype(np.float32)
            refl = _reflect(d, n)
            nd_d = normalize(np.where(_mirror_angle(ri, n, d, u01(rb[2]))[:, None], refl, _refract(d, n, ri)))
            through = hit & ~lambert & (mtype > F(0)) & (dot(nd_d, n) < F(0))
            nd = np.where(lambert[:, None], nd_l, np.where((mtype < F(0))[:, None], normalize(refl), nd_d)).astype(np.float32)
            o = np.where(hit[:, None], np.where(through[:, None], point - EPS * n, on), o).astype(np.float32)
            d = np.where(hit[:, None], nd, d).astype(np.float32)
            thr = np.where(hit[:, None], thr * albedo, thr).astype(np.float32)
        value = np.concatenate([np.where(L > F(0), np.minimum(L, clamp), F(0)), np.fmin(np.fmax(La, F(0)), F(1))[:, None]], -1)
    finally:
        np.seterr(**old)
    assert value.dtype == np.float32 and L.dtype == np.float32 and thr.dtype == np.float32
    shape = (H, W, count)
    return dict(value=value.reshape(shape + (4,)), rays=rays.reshape(shape), shadow=n_shadow.reshape(shape), occluded=n_occ.reshape(shape),
                gap=gap.reshape(shape), mis_lights=np.array(sorted(mis_lights), np.int64))


def accumulate(value, start=None):
    """sum = ((start + v_0) + v_1) + ... over the sample axis of value [H, W, n, 4], in float32."""
    acc = np.zeros(value.shape[:2] + (4,), np.float32) if start is None else np.array(start, np.float32)
    for s in range(value.shape[2]):
        acc = acc + value[:, :, s]
    return acc
