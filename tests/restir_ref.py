"""numpy restatement of the "spatial reservoir reuse" section of include/mpt.h (mpt_direct_restir; k_restir_initial and k_restir_merge of
metalpathtracer_amd/csrc/mpt_restir.h).  Every step is a single IEEE float32 operation in the order written there.  What the call leaves
alone is imported: the origins and the image arithmetic from tests/direct_ref.py, the luminance and the factor of a candidate from
tests/ris_ref.py, Philox / u01 / sincos_2pi / dot / normalize from tests/ao_ref.py.  A sample's geometry is written here once for any
(k, ua, ub) and any (o, n) — the same code forms a candidate, a neighbour's sample seen from this pixel and this pixel's sample seen from
a neighbour — and tests/test_restir_cpu.py holds it to ris_ref's candidate loop bit for bit through K = 0.  Occlusion comes from
tests/anyhit_ref.py (bounds), following `lower`; a ray with upper & ~lower is a GAP ray, and a pixel-round is TAINTED if any ray it depends
on is one: its own initial ray, an accepted neighbour's initial ray, its final ray, its correction rays.  Both modes come out of one run:
they share steps A to C.  Test code: the product never imports it."""
import numpy as np

import direct_ref
import ris_ref
from ao_ref import dot, normalize, philox4x32_10, sincos_2pi, u01
from direct_ref import INV_PI, TMAX_SCALE, WORD2, cross

F = np.float32
U32 = np.uint32
WORD2_NEIGHBOUR = 0xFFFFFFFC
UNBIASED, BIASED = 0, 1
MODES = (UNBIASED, BIASED)
K_MAX, R_MAX = 16, 64
DEFAULTS = dict(radius=4, normal_threshold=0.5, depth_tolerance=0.05)


def offsets(ux, R):
    """dx = min((int)(u * (float)(2R+1)), 2R) - R for uniforms ux (float32)."""
    return np.minimum((ux * F(2 * R + 1)).astype(np.int32), 2 * R) - R


def form(k, ua, ub, o, n, table):
    """The light sample (k, ua, ub) formed from the points o [n,3] with normals n [n,3], area geometry: a dict of wi, dist, fac, ok, Le —
    the candidate of ris_ref.candidate (cone = False) with the light and the two uniforms given instead of drawn."""
    rec = table.rec[k]
    tri = rec[:, 0, 3] != 0
    c, e1, e2 = rec[:, 0, :3], rec[:, 1, :3], rec[:, 2, :3]
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
    nl = np.where(tri[:, None], ng, ns)
    p = np.where(tri[:, None], pt, ps)
    v = p - o
    d2 = dot(v, v)
    dist = np.sqrt(d2)
    wi = (v * (F(1) / dist)[:, None]).astype(np.float32)
    cos_s = dot(n, wi)
    dl = dot(nl, wi)
    cos_l = np.where(tri, np.abs(dl), -dl)
    ok = (d2 > F(0)) & (cos_s > F(0)) & (cos_l > F(0))
    cd = dict(tri=tri, cos_s=cos_s.astype(np.float32), cos_l=cos_l.astype(np.float32), d2=d2.astype(np.float32), inv_pdf=rec[:, 3, 3])
    return dict(wi=wi, dist=dist.astype(np.float32), fac=ris_ref.factor(cd, False, False), ok=ok, Le=rec[:, 3, :3])


def _trace(o, wi, tmax, live, buffers, bounds):
    """(occluded, gap) [n] bool of the rays of the lanes `live` (False elsewhere): lower, and upper & ~lower."""
    occ = np.zeros(live.shape, bool)
    gap = np.zeros(live.shape, bool)
    if live.any():
        (lo, up), = bounds(o[live], wi[live], [tmax[live]], buffers)
        occ[live] = lo
        gap[live] = up & ~lo
    return occ, gap


def _words(holds, k, ua, ub, wsum, fac, flags):
    """A reservoir as mpt_read_restir_reservoirs gives it: [n, 6] uint32, six zero words where it does not hold."""
    w = np.stack([k.astype(np.uint32), ua.astype(np.float32).view(np.uint32), ub.astype(np.float32).view(np.uint32),
                  wsum.astype(np.float32).view(np.uint32), fac.astype(np.float32).view(np.uint32), flags.astype(np.uint32)], -1)
    return np.where(holds[:, None], w, U32(0)).astype(np.uint32)


def initial(o, n, pixel, surface, s, M, table, seed):
    """Step A before its ray: the candidate loop of ris_ref.pick (cone = False, nee = False) remembering k, ua, ub, fac."""
    cnt = o.shape[0]
    y = dict(k=np.zeros(cnt, np.int64), ua=np.zeros(cnt, np.float32), ub=np.zeros(cnt, np.float32), fac=np.zeros(cnt, np.float32),
             wi=np.ones((cnt, 3), np.float32), dist=np.zeros(cnt, np.float32))
    wsum = np.zeros(cnt, np.float32)
    taken = np.zeros(cnt, bool)
    for j in range(M):
        r = philox4x32_10(pixel, U32(s), U32(WORD2), U32(j), seed[0], seed[1])
        k = np.searchsorted(table.cdf, u01(r[0]), side="right")
        assert (k < table.n).all()
        ua, ub = u01(r[1]), u01(r[2])
        cd = form(k, ua, ub, o, n, table)
        l = ris_ref.luminance(cd["Le"])
        w = (l * cd["fac"]).astype(np.float32)
        counts = surface & cd["ok"] & (w > F(0)) & (w < F(np.inf))
        wsum = np.where(counts, wsum + w, wsum).astype(np.float32)
        take = counts & (~taken | (u01(r[3]) * wsum < w))
        for key, val in (("k", k), ("ua", ua), ("ub", ub), ("fac", cd["fac"]), ("dist", cd["dist"])):
            y[key] = np.where(take, val, y[key])
        y["wi"] = np.where(take[:, None], cd["wi"], y["wi"])
        taken = taken | counts
    y.update(wsum=wsum, taken=taken)
    return y


def restir(albedo_depth, normal_class, cam, table, buffers, bounds, begin, N, M, K, R=0, seed=(0, 0), normal_threshold=0.0, depth_tolerance=0.0):
    """Rounds [begin, begin + N) of mpt_direct_restir with m = M candidates, in both modes.  A dict: for mode in MODES, out[mode] =
    dict(rgba [H,W,4], traced [H,W], unoccluded [H,W], pick [H,W,6] (the last round's), tainted [H,W] bool, info: the totals of
    mpt_restir_info) and out["initial"] [H,W,6] (the last round's reservoirs after step A, the same in both modes)."""
    assert 0 <= K <= K_MAX and 0 <= R <= R_MAX and M >= 1
    R = R or DEFAULTS["radius"]
    thr = F(normal_threshold if normal_threshold > 0 else DEFAULTS["normal_threshold"])
    tol = F(depth_tolerance if depth_tolerance > 0 else DEFAULTS["depth_tolerance"])
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    H, W = ad.shape[:2]
    P = H * W
    o = direct_ref.samples(ad, nc, cam, table, begin, 1, seed)[0].reshape(P, 3)
    n = nc[..., :3].reshape(P, 3)
    t = ad[..., 3].reshape(P)
    surface = (nc[..., 3] == 0).reshape(P)
    py, px = np.divmod(np.arange(P), W)
    pixel = np.arange(P, dtype=np.uint32)
    S = {m: np.zeros((P, 3), np.float32) for m in MODES}
    traced = {m: np.zeros(P, np.uint32) for m in MODES}
    unocc = {m: np.zeros(P, np.uint32) for m in MODES}
    tainted = {m: np.zeros(P, bool) for m in MODES}
    info = {m: dict(pixels_surface=int(surface.sum()), rays_initial=0, rays_final=0, rays_correction=0, rays_occluded=0, neighbours_accepted=0,
                    samples_from_neighbours=0, lights=table.n) for m in MODES}
    zeros6 = np.zeros((P, 6), np.uint32)
    words_initial, words_pick = zeros6, zeros6
    old = np.seterr(all="ignore")
    try:
        for s in range(begin, begin + N if table.n else begin):
            # step A
            y0 = initial(o, n, pixel, surface, s, M, table, seed)
            taken = y0["taken"]
            occ_a, gap_a = _trace(o, y0["wi"], (y0["dist"] * TMAX_SCALE).astype(np.float32), taken, buffers, bounds)
            holds = taken & ~occ_a
            words_initial = _words(holds, y0["k"], y0["ua"], y0["ub"], y0["wsum"], y0["fac"], np.ones(P, np.uint32))
            # step B
            held = holds.copy()
            own = holds.copy()
            y = {key: y0[key].copy() for key in ("k", "ua", "ub", "fac")}
            Wp = np.where(holds, y0["wsum"], F(0)).astype(np.float32)
            taint = gap_a.copy()
            taps = []
            for i in range(K):
                r = philox4x32_10(pixel, U32(s), U32(WORD2_NEIGHBOUR), U32(i), seed[0], seed[1])
                dx, dy = offsets(u01(r[0]), R), offsets(u01(r[1]), R)
                qx, qy = px + dx, py + dy
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                q = np.where(inside, qy * W + qx, 0)
                accepted = (surface & ((dx != 0) | (dy != 0)) & inside & surface[q] & (dot(n, n[q]) >= thr)
                            & (np.abs(t[q] - t) <= tol * t))
                taps.append((accepted, q))
                taint |= accepted & gap_a[q]
                cd = form(y0["k"][q], y0["ua"][q], y0["ub"][q], o, n, table)
                w = (y0["wsum"][q] * (cd["fac"] / y0["fac"][q])).astype(np.float32)
                counts = accepted & holds[q] & cd["ok"] & (w > F(0)) & (w < F(np.inf))
                Wp = np.where(counts, Wp + w, Wp).astype(np.float32)
                take = counts & (~held | (u01(r[2]) * Wp < w))
                for key, val in (("k", y0["k"][q]), ("ua", y0["ua"][q]), ("ub", y0["ub"][q]), ("fac", cd["fac"])):
                    y[key] = np.where(take, val, y[key])
                own = own & ~take
                held = held | counts
            words_pick = _words(held, y["k"], y["ua"], y["ub"], Wp, y["fac"], 1 + 2 * own.astype(np.uint32))
            n_accepted = int(sum(a.sum() for a, _ in taps))
            # step C
            fy = form(y["k"], y["ua"], y["ub"], o, n, table)
            fin = held & ~own
            occ_c, gap_c = _trace(o, fy["wi"], (fy["dist"] * TMAX_SCALE).astype(np.float32), fin, buffers, bounds)
            taint |= gap_c
            go = held & ~(fin & occ_c)
            # step D
            c = {m: np.ones(P, np.int64) for m in MODES}
            n_corr = np.zeros(P, np.uint32)
            n_corr_open = np.zeros(P, np.uint32)
            taint_d = np.zeros(P, bool)
            for accepted, q in taps:
                fq = form(y["k"], y["ua"], y["ub"], o[q], n[q], table)
                live = go & accepted & fq["ok"] & (fq["fac"] > F(0)) & (fq["fac"] < F(np.inf))
                occ_d, gap_d = _trace(o[q], fq["wi"], (fq["dist"] * TMAX_SCALE).astype(np.float32), live, buffers, bounds)
                taint_d |= gap_d
                n_corr += live
                n_corr_open += live & ~occ_d
                c[UNBIASED] += live & ~occ_d
                c[BIASED] += live
            # step E and the counts
            l = ris_ref.luminance(fy["Le"])
            for m in MODES:
                Fy = ((Wp / (M * c[m]).astype(np.float32)) / l).astype(np.float32)
                S[m] = np.where(go[:, None], S[m] + fy["Le"] * Fy[:, None], S[m]).astype(np.float32)
                corr = n_corr if m == UNBIASED else np.zeros(P, np.uint32)
                corr_open = n_corr_open if m == UNBIASED else np.zeros(P, np.uint32)
                traced[m] += taken + fin.astype(np.uint32) + corr
                unocc[m] += holds + (fin & ~occ_c).astype(np.uint32) + corr_open
                tainted[m] |= taint | (taint_d if m == UNBIASED else False)
                d = info[m]
                d["rays_initial"] += int(taken.sum())
                d["rays_final"] += int(fin.sum())
                d["rays_correction"] += int(corr.sum())
                d["neighbours_accepted"] += n_accepted
                d["samples_from_neighbours"] += int(fin.sum())
        out = dict(initial=words_initial.reshape(H, W, 6))
        for m in MODES:
            rgb = (ad[..., :3] * INV_PI) * (S[m].reshape(H, W, 3) / F(N))
            rgba = np.concatenate([np.where(surface.reshape(H, W, 1), rgb, F(0)), np.ones((H, W, 1), np.float32)], -1).astype(np.float32)
            info[m]["rays_occluded"] = int(traced[m].sum()) - int(unocc[m].sum())
            out[m] = dict(rgba=rgba, traced=traced[m].reshape(H, W), unoccluded=unocc[m].reshape(H, W), pick=words_pick.reshape(H, W, 6),
                          tainted=tainted[m].reshape(H, W), info=info[m])
    finally:
        np.seterr(**old)
    return out
