"""numpy restatement of the "temporal reservoir reuse" section of include/mpt.h (mpt_direct_restir_temporal; k_restir_initial of
metalpathtracer_amd/csrc/mpt_restir.h and k_restir_temporal of mpt_restir_temporal.h).  Every step is a single IEEE float32 operation in
the order written there.  What the call leaves alone is imported: a sample's geometry (form), step A (initial) and the rays (_trace) from
tests/restir_ref.py, the camera key, the history guide and dot from tests/temporal_ref.py — steps 1-3 of the reprojection are written
here in temporal_ref.accumulate's order, for a hit — the luminance from tests/ris_ref.py.  Occlusion comes from tests/anyhit_ref.py
(bounds), following `lower`; a ray with upper & ~lower is a GAP ray and a pixel is TAINTED if one of its OWN rays (initial, final,
correction) is one.  The previous frame's reservoirs are an argument, so taint does not compound over frames when the caller feeds the
reference's.  Both modes come out of one run: they share steps A to C.  Test code: the product never imports it."""
import numpy as np

import restir_ref
import ris_ref
from ao_ref import philox4x32_10, u01
from direct_ref import INV_PI, TMAX_SCALE
from restir_ref import BIASED, MODES, UNBIASED, _trace, form, initial
from temporal_ref import camera_key, dot, pack_guide

F = np.float32
U32 = np.uint32
WORD2_TEMPORAL = 0xFFFFFFFB
C_DEFAULT, C_MAX = 20, 1024
DEFAULTS = dict(max_history=C_DEFAULT, normal_threshold=restir_ref.DEFAULTS["normal_threshold"],
                depth_tolerance=restir_ref.DEFAULTS["depth_tolerance"])
INFO_KEYS = ("pixels_surface", "rays_initial", "rays_final", "rays_correction", "rays_occluded", "history_accepted", "samples_from_history",
             "pixels_reset", "lights")


def origin(key, W, H, px, py, t, n):
    """The origin o of the direct-lighting section at the integer pixels (px, py) of the camera `key` (fourteen floats), with the guide's
    t [n] and normal n [n,3]."""
    cam_p, vu, vv, first = key[0:3], key[3:6], key[6:9], key[9:12]
    uvx = ((px.astype(np.float32) + F(0.5)) / F(W))[..., None]
    uvy = ((py.astype(np.float32) + F(0.5)) / F(H))[..., None]
    dv = ((first + uvx * vu) + uvy * vv) - cam_p
    dc = dv * (F(1) / np.sqrt(dot(dv, dv)))[..., None]
    return ((cam_p + t[..., None] * dc) + F(0.0001) * n).astype(np.float32)


def reproject(key, key_h, W, H, px, py, t):
    """Steps 1-3 of mpt_temporal_accumulate with the hit rule: (r [n,3], |r|, fx, fy, ok) — ok: s > 0, s finite, -1 <= fx < W, -1 <= fy < H."""
    cam_p, vu, vv, first = key[0:3], key[3:6], key[6:9], key[9:12]
    cam_h, vu_h, vv_h, first_h = key_h[0:3], key_h[3:6], key_h[6:9], key_h[9:12]
    fW, fH = F(W), F(H)
    uvx = ((px.astype(np.float32) + F(0.5)) / fW)[..., None]
    uvy = ((py.astype(np.float32) + F(0.5)) / fH)[..., None]
    dv = ((first + uvx * vu) + uvy * vv) - cam_p
    d = dv * (F(1) / np.sqrt(dot(dv, dv)))[..., None]
    r = ((cam_p + t[..., None] * d) - cam_h).astype(np.float32)
    nn = np.array([vu_h[1] * vv_h[2] - vu_h[2] * vv_h[1], vu_h[2] * vv_h[0] - vu_h[0] * vv_h[2], vu_h[0] * vv_h[1] - vu_h[1] * vv_h[0]], np.float32)
    fc = first_h - cam_h
    s = dot(fc, nn) / dot(r, nn)
    q = s[..., None] * r - fc
    u = dot(q, vu_h) / dot(vu_h, vu_h)
    v = dot(q, vv_h) / dot(vv_h, vv_h)
    fx = u * fW - F(0.5)
    fy = v * fH - F(0.5)
    ok = (s > 0) & (s < F(np.inf)) & (fx >= -1) & (fx < fW) & (fy >= -1) & (fy < fH)
    return r, np.sqrt(dot(r, r)).astype(np.float32), fx.astype(np.float32), fy.astype(np.float32), ok


def words(holds, k, ua, ub, wsum, fac, flags, Mh):
    """Reservoirs as mpt_read_restir_temporal_reservoirs gives them: [n, 7] uint32; one that does not hold is zeros but for Mh."""
    w = np.stack([k.astype(np.uint32), ua.astype(np.float32).view(np.uint32), ub.astype(np.float32).view(np.uint32),
                  wsum.astype(np.float32).view(np.uint32), fac.astype(np.float32).view(np.uint32), flags.astype(np.uint32)], -1)
    w = np.where(holds[:, None], w, U32(0)).astype(np.uint32)
    return np.concatenate([w, Mh.astype(np.uint32)[:, None]], -1)


def frame(albedo_depth, normal_class, cam, table, buffers, bounds, prev=None, frame=0, M=1, C=0, seed=(0, 0), normal_threshold=0.0,
          depth_tolerance=0.0):
    """One mpt_direct_restir_temporal frame in both modes.  prev: None (no history) or a dict(ad, nc, cam, res [H,W,7]) — the previous
    frame's guides, camera and reservoirs.  A dict: for mode in MODES, out[mode] = dict(rgba [H,W,4], traced [H,W], unoccluded [H,W],
    res [H,W,7], tainted [H,W] bool, info: the totals of mpt_restir_temporal_info); out["initial"] [H,W,6] (the reservoirs after step A),
    out["o"] [H,W,3] (the origins), out["tap"]: dict(q [H,W] int (-1: none), accepted [H,W] bool, o_prev [H,W,3], and the count of surface
    pixels whose tap was rejected as outside, miss, depth, normal, empty — the first reason that applies, in that order)."""
    assert M >= 1 and 0 <= C <= C_MAX
    C = C or C_DEFAULT
    thr = F(normal_threshold if normal_threshold > 0 else DEFAULTS["normal_threshold"])
    tol = F(depth_tolerance if depth_tolerance > 0 else DEFAULTS["depth_tolerance"])
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    H, W = ad.shape[:2]
    P = H * W
    key = camera_key(cam)
    py, px = np.divmod(np.arange(P), W)
    n = nc[..., :3].reshape(P, 3)
    t = ad[..., 3].reshape(P)
    surface = (nc[..., 3] == 0).reshape(P)
    pixel = np.arange(P, dtype=np.uint32)
    old = np.seterr(all="ignore")
    try:
        o = origin(key, W, H, px, py, t, n)
        # step A
        if table.n:
            y0 = initial(o, n, pixel, surface, frame, M, table, seed)
        else:
            y0 = dict(k=np.zeros(P, np.int64), ua=np.zeros(P, np.float32), ub=np.zeros(P, np.float32), fac=np.zeros(P, np.float32),
                      wi=np.ones((P, 3), np.float32), dist=np.zeros(P, np.float32), wsum=np.zeros(P, np.float32), taken=np.zeros(P, bool))
        taken = y0["taken"]
        occ_a, gap_a = _trace(o, y0["wi"], (y0["dist"] * TMAX_SCALE).astype(np.float32), taken, buffers, bounds)
        holds = taken & ~occ_a
        words_initial = restir_ref._words(holds, y0["k"], y0["ua"], y0["ub"], y0["wsum"], y0["fac"], np.ones(P, np.uint32))
        # step T
        q = np.zeros(P, np.int64)
        counts_tap = np.zeros(P, bool)
        reject = dict(outside=0, miss=0, depth=0, normal=0, empty=0)
        if prev is not None:
            key_h = camera_key(prev["cam"])
            gh = pack_guide(prev["ad"], prev["nc"]).reshape(P, 4)
            res_h = np.asarray(prev["res"], np.uint32).reshape(P, 7)
            if key.tobytes() == key_h.tobytes():
                q = np.arange(P)
                counts_tap = surface.copy()
            else:
                _, rl, fx, fy, ok0 = reproject(key, key_h, W, H, px, py, t)
                fx = np.where(ok0, fx, F(0))
                fy = np.where(ok0, fy, F(0))
                qx = np.floor(fx + F(0.5)).astype(np.int64)
                qy = np.floor(fy + F(0.5)).astype(np.int64)
                inside = ok0 & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                q = np.where(inside, qy * W + qx, 0)
                gq = gh[q]
                hit_q = gq[:, 3] < F(np.inf)
                depth_ok = np.abs(gq[:, 3] - rl) <= tol * rl
                normal_ok = dot(n, gq) >= thr
                counts_tap = surface & inside & hit_q & depth_ok & normal_ok
                reject["outside"] = int((surface & ~inside).sum())
                reject["miss"] = int((surface & inside & ~hit_q).sum())
                reject["depth"] = int((surface & inside & hit_q & ~depth_ok).sum())
                reject["normal"] = int((surface & inside & hit_q & depth_ok & ~normal_ok).sum())
            Mh = res_h[q, 6].astype(np.int64)
            accepted = counts_tap & (Mh > 0)
            reject["empty"] = int((counts_tap & ~accepted).sum())
        else:
            key_h = key
            gh = np.zeros((P, 4), np.float32)
            res_h = np.zeros((P, 7), np.uint32)
            Mh = np.zeros(P, np.int64)
            accepted = np.zeros(P, bool)
        # step B
        Mc = np.minimum(Mh, C * M)
        held = holds.copy()
        own = holds.copy()
        y = {k_: y0[k_].copy() for k_ in ("k", "ua", "ub", "fac")}
        Wp = np.where(holds, y0["wsum"], F(0)).astype(np.float32)
        rq = res_h[q]
        q_holds = accepted & ((rq[:, 5] & 1) != 0)
        kq = np.where(q_holds, rq[:, 0], 0).astype(np.int64)
        uaq, ubq, wsq, facq = (rq[:, i].copy().view(np.float32) for i in (1, 2, 3, 4))
        if table.n:
            cd = form(kq, uaq, ubq, o, n, table)
            w = ((wsq * (cd["fac"] / facq)) * (Mc.astype(np.float32) / Mh.astype(np.float32))).astype(np.float32)
            counts = q_holds & cd["ok"] & (w > F(0)) & (w < F(np.inf))
            Wp = np.where(counts, Wp + w, Wp).astype(np.float32)
            r = philox4x32_10(pixel, U32(frame), U32(WORD2_TEMPORAL), U32(0), seed[0], seed[1])
            take = counts & (~held | (u01(r[2]) * Wp < w))
            for k_, val in (("k", kq), ("ua", uaq), ("ub", ubq), ("fac", cd["fac"])):
                y[k_] = np.where(take, val, y[k_])
            own = own & ~take
            held = held | counts
            # step C
            fy_ = form(y["k"], y["ua"], y["ub"], o, n, table)
        else:
            fy_ = dict(wi=np.ones((P, 3), np.float32), dist=np.zeros(P, np.float32), Le=np.zeros((P, 3), np.float32))
        fin = held & ~own
        occ_c, gap_c = _trace(o, fy_["wi"], (fy_["dist"] * TMAX_SCALE).astype(np.float32), fin, buffers, bounds)
        go = held & ~(fin & occ_c)
        # step D
        qy_i, qx_i = np.divmod(q, W)
        o_prev = origin(key_h, W, H, qx_i, qy_i, gh[q, 3], gh[q, :3])
        if table.n:
            fq = form(y["k"], y["ua"], y["ub"], o_prev, gh[q, :3], table)
            live = go & accepted & fq["ok"] & (fq["fac"] > F(0)) & (fq["fac"] < F(np.inf))
            occ_d, gap_d = _trace(o_prev, fq["wi"], (fq["dist"] * TMAX_SCALE).astype(np.float32), live, buffers, bounds)
        else:
            live = occ_d = gap_d = np.zeros(P, bool)
        Z = {UNBIASED: M + np.where(live & ~occ_d, Mc, 0), BIASED: M + np.where(live, Mc, 0)}
        # step E and the counts
        l = ris_ref.luminance(fy_["Le"])
        Mnew = M + np.where(accepted, Mc, 0)
        out = dict(initial=words_initial.reshape(H, W, 6), o=o.reshape(H, W, 3),
                   tap=dict(q=np.where(accepted | counts_tap, q, -1).reshape(H, W), accepted=accepted.reshape(H, W), o_prev=o_prev.reshape(H, W, 3), **reject))
        for m in MODES:
            Zf = Z[m].astype(np.float32)
            Fy = ((Wp / Zf) / l).astype(np.float32)
            S = np.where(go[:, None], fy_["Le"] * Fy[:, None], F(0)).astype(np.float32)
            rgb = ((ad[..., :3].reshape(P, 3) * INV_PI) * (S / F(1))).astype(np.float32)
            rgba = np.concatenate([np.where(surface[:, None], rgb, F(0)), np.ones((P, 1), np.float32)], -1).astype(np.float32)
            corr = live if m == UNBIASED else np.zeros(P, bool)
            traced = taken.astype(np.uint32) + fin + corr
            unocc = holds.astype(np.uint32) + (fin & ~occ_c) + (corr & ~occ_d)
            wnew = (Wp * (Mnew.astype(np.float32) / Zf)).astype(np.float32)
            res = words(go, y["k"], y["ua"], y["ub"], wnew, y["fac"], 1 + 2 * own.astype(np.uint32), np.where(surface, Mnew, 0))
            tainted = gap_a | gap_c | (gap_d if m == UNBIASED else False)
            info = dict(pixels_surface=int(surface.sum()), rays_initial=int(taken.sum()), rays_final=int(fin.sum()), rays_correction=int(corr.sum()),
                        rays_occluded=int(traced.sum()) - int(unocc.sum()), history_accepted=int(accepted.sum()), samples_from_history=int(fin.sum()),
                        pixels_reset=int(surface.sum()) - int(accepted.sum()), lights=table.n)
            out[m] = dict(rgba=rgba.reshape(H, W, 4), traced=traced.reshape(H, W), unoccluded=unocc.reshape(H, W), res=res.reshape(H, W, 7),
                          tainted=tainted.reshape(H, W), info=info)
    finally:
        np.seterr(**old)
    return out
