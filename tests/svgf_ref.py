"""numpy float32 restatement of the SVGF stage of include/mpt.h (mpt_svgf_params), in the tap order and operation order of
k_sv_reproject, k_sv_variance and k_sv_level (metalpathtracer_amd/csrc/mpt_svgf.h).  Step A uses only + - * / sqrt floor and
comparisons, each a single IEEE float32 operation: the device must agree bit for bit.  Steps B and C call exp and pow, which may
differ from the device's by an ulp or so.  Test code: the product never imports it."""
import numpy as np

import temporal_ref as tr
from denoise_ref import H5, lum

F = np.float32
# include/mpt.h MPT_SVGF_DEFAULT_* (step A's four parameters are the MPT_TEMPORAL_DEFAULT_* of temporal_ref.DEFAULTS)
DEFAULTS = dict(iterations=2, sigma_luminance=2.0, sigma_normal=32.0, sigma_depth=0.25, feedback=0)
EPSILON = F(1e-4)            # MPT_SVGF_EPSILON
SPATIAL_BELOW = F(4)         # a history shorter than this takes its variance from the 7 x 7 window
K3 = np.array([0.25, 0.5, 0.25], np.float32)


def pack_guide(albedo_depth, normal_class):
    """(normal, t) with the class in t: t for a surface, -t for an emitter, +inf for a miss: the history guide."""
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    g = nc.copy()
    g[..., 3] = np.where(nc[..., 3] == 2, F(np.inf), np.where(nc[..., 3] == 1, -ad[..., 3], ad[..., 3]))
    return g


def resolve(iterations=-1, sigma_luminance=0.0, sigma_normal=0.0, sigma_depth=0.0, feedback=-1):
    return (DEFAULTS["iterations"] if iterations is None or iterations < 0 else int(iterations),
            F(sigma_luminance if sigma_luminance and sigma_luminance > 0 else DEFAULTS["sigma_luminance"]),
            F(sigma_normal if sigma_normal and sigma_normal > 0 else DEFAULTS["sigma_normal"]),
            F(sigma_depth if sigma_depth and sigma_depth > 0 else DEFAULTS["sigma_depth"]),
            DEFAULTS["feedback"] if feedback is None or feedback < 0 else int(feedback != 0))


def albedo(albedo_depth, normal_class):
    """a: max(albedo, 1e-3) for a surface pixel, 1 for an emitter or a miss."""
    ad = np.asarray(albedo_depth, np.float32)
    surf = np.asarray(normal_class)[..., 3] == 0
    return np.where(surf[..., None], np.maximum(ad[..., :3], F(1e-3)), F(1)).astype(np.float32)


def accumulate(color, albedo_depth, normal_class, cam, history=None, moments=None, albedo_depth_prev=None, normal_class_prev=None,
               cam_prev=None, max_history=0, depth_tolerance=0.0, normal_threshold=0.0, min_weight=0.0):
    """Step A.  Returns (illumination history (X, n) [H, W, 4], moments (M1, M2) [H, W, 2], number of pixels reset)."""
    maxh, ztol, nth, minw = tr.resolve(max_history, depth_tolerance, normal_threshold, min_weight)
    c = np.asarray(color, np.float32)
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    H, W = c.shape[:2]
    x = c[..., :3] / albedo(ad, nc)
    l = lum(x)
    ll = l * l
    hist_out = np.empty((H, W, 4), np.float32)
    mom_out = np.empty((H, W, 2), np.float32)
    if history is None:
        hist_out[..., :3] = x
        hist_out[..., 3] = 1
        mom_out[..., 0] = l
        mom_out[..., 1] = ll
        return hist_out, mom_out, H * W
    hm = np.concatenate([np.asarray(history, np.float32), np.asarray(moments, np.float32)], -1)   # (X rgb, n, M1, M2)
    k, kh = tr.camera_key(cam), tr.camera_key(cam_prev)
    acc = np.zeros((H, W, 6), np.float32)
    sw = np.zeros((H, W), np.float32)
    old = np.seterr(all="ignore")
    try:
        if k.tobytes() == kh.tobytes():
            acc = hm.copy()
            sw[...] = 1
        else:
            gh = pack_guide(albedo_depth_prev, normal_class_prev)
            cam_p, vu, vv, first = k[0:3], k[3:6], k[6:9], k[9:12]
            cam_h, vu_h, vv_h, first_h = kh[0:3], kh[3:6], kh[6:9], kh[9:12]
            fW, fH = F(W), F(H)
            px, py = np.meshgrid(np.arange(W), np.arange(H))
            uvx = ((px.astype(np.float32) + F(0.5)) / fW)[..., None]
            uvy = ((py.astype(np.float32) + F(0.5)) / fH)[..., None]
            dv = ((first + uvx * vu) + uvy * vv) - cam_p
            d = dv * (F(1) / np.sqrt(tr.dot(dv, dv)))[..., None]
            cls = nc[..., 3]
            hit = cls != 2
            emit = cls == 1
            t = ad[..., 3]
            r = np.where(hit[..., None], (cam_p + t[..., None] * d) - cam_h, d).astype(np.float32)
            nn = np.array([vu_h[1] * vv_h[2] - vu_h[2] * vv_h[1], vu_h[2] * vv_h[0] - vu_h[0] * vv_h[2],
                           vu_h[0] * vv_h[1] - vu_h[1] * vv_h[0]], np.float32)
            fc = first_h - cam_h
            s = tr.dot(fc, nn) / tr.dot(r, nn)
            q = s[..., None] * r - fc
            u = tr.dot(q, vu_h) / tr.dot(vu_h, vu_h)
            v = tr.dot(q, vv_h) / tr.dot(vv_h, vv_h)
            fx = u * fW - F(0.5)
            fy = v * fH - F(0.5)
            ok0 = (s > 0) & (s < F(np.inf)) & (fx >= -1) & (fx < fW) & (fy >= -1) & (fy < fH)
            fx = np.where(ok0, fx, F(0))
            fy = np.where(ok0, fy, F(0))
            flx, fly = np.floor(fx), np.floor(fy)
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            ax, ay = fx - flx, fy - fly
            rl = np.sqrt(tr.dot(r, r))
            tol = ztol * rl
            n = nc[..., :3]
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inb = ok0 & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    gq = gh[qyc, qxc]
                    qhit = gq[..., 3] < F(np.inf)
                    okh = (qhit & ((gq[..., 3] < 0) == emit) & (np.abs(np.abs(gq[..., 3]) - rl) <= tol) & (tr.dot(n, gq) >= nth))
                    valid = inb & np.where(hit, okh, ~qhit)
                    w = ((ax if i else F(1) - ax) * (ay if j else F(1) - ay)).astype(np.float32)
                    acc = np.where(valid[..., None], acc + w[..., None] * hm[qyc, qxc], acc)
                    sw = np.where(valid, sw + w, sw)
        assert acc.dtype == np.float32 and sw.dtype == np.float32
        good = sw >= minw
        h = acc / sw[..., None]
        nlen = np.minimum(h[..., 3] + F(1), maxh)
        res = h[..., :3] + (x - h[..., :3]) / nlen[..., None]
        m1 = h[..., 4] + (l - h[..., 4]) / nlen
        m2 = h[..., 5] + (ll - h[..., 5]) / nlen
        hist_out[..., :3] = np.where(good[..., None], res, x)
        hist_out[..., 3] = np.where(good, nlen, F(1))
        mom_out[..., 0] = np.where(good, m1, l)
        mom_out[..., 1] = np.where(good, m2, ll)
    finally:
        np.seterr(**old)
    return hist_out, mom_out, int((~good).sum())


def _shift(Hh, W, dx, dy):
    """Slices (ys, xs) of the pixels p whose tap q = p + (dx, dy) is inside the image, and (yq, xq) of those taps; None if empty."""
    ys = slice(max(0, -dy), min(Hh, Hh - dy))
    xs = slice(max(0, -dx), min(W, W - dx))
    if ys.start >= ys.stop or xs.start >= xs.stop:
        return None
    return ys, xs, slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)


def variance(history, moments, albedo_depth, normal_class, sigma_normal, sigma_depth):
    """Step B: V_0 [H, W] (0 for classes 1 / 2)."""
    hist = np.asarray(history, np.float32)
    mom = np.asarray(moments, np.float32)
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    sn, sz = F(sigma_normal), F(sigma_depth)
    Hh, W = hist.shape[:2]
    surf = nc[..., 3] == 0
    n = nc[..., :3]
    t = ad[..., 3]
    cnt = hist[..., 3]
    m1, m2 = mom[..., 0], mom[..., 1]
    old = np.seterr(all="ignore")
    try:
        vt = np.fmax(F(0), m2 - m1 * m1) / cnt
        den_z = sz * t
        s1 = np.zeros((Hh, W), np.float32)
        s2 = np.zeros((Hh, W), np.float32)
        sw = np.zeros((Hh, W), np.float32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                sh = _shift(Hh, W, dx, dy)
                if sh is None:
                    continue
                ys, xs, yq, xq = sh
                ok = surf[yq, xq]
                if dx == 0 and dy == 0:
                    w = np.ones(ok.shape, np.float32)
                else:
                    npp, nq = n[ys, xs], n[yq, xq]
                    nd = (npp[..., 0] * nq[..., 0] + npp[..., 1] * nq[..., 1]) + npp[..., 2] * nq[..., 2]
                    wn = np.power(np.fmax(F(0), nd), sn)
                    wz = np.exp(-np.abs(t[ys, xs] - t[yq, xq]) / den_z[ys, xs])
                    w = (wn * wz).astype(np.float32)
                s1[ys, xs] = np.where(ok, s1[ys, xs] + w * m1[yq, xq], s1[ys, xs])
                s2[ys, xs] = np.where(ok, s2[ys, xs] + w * m2[yq, xq], s2[ys, xs])
                sw[ys, xs] = np.where(ok, sw[ys, xs] + w, sw[ys, xs])
        e1 = s1 / sw
        vs = np.fmax(F(0), s2 / sw - e1 * e1) / cnt
        v = np.where(cnt >= SPATIAL_BELOW, vt, vs)
    finally:
        np.seterr(**old)
    assert v.dtype == np.float32
    return np.where(surf, v, F(0)).astype(np.float32)


def level(xv, albedo_depth, normal_class, i, sigma_luminance, sigma_normal, sigma_depth):
    """Step C, level i: (x_i rgb, V_i) [H, W, 4] -> (x_{i+1} rgb, V_{i+1}); pixels of class 1 / 2 come back as they went in."""
    xv = np.asarray(xv, np.float32)
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    sl, sn, sz = F(sigma_luminance), F(sigma_normal), F(sigma_depth)
    Hh, W = xv.shape[:2]
    surf = nc[..., 3] == 0
    n = nc[..., :3]
    t = ad[..., 3]
    x, V = xv[..., :3], xv[..., 3]
    l = lum(x)
    s = 1 << i
    old = np.seterr(all="ignore")
    try:
        gs = np.zeros((Hh, W), np.float32)
        gw = np.zeros((Hh, W), np.float32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                sh = _shift(Hh, W, dx, dy)
                if sh is None:
                    continue
                ys, xs, yq, xq = sh
                ok = surf[yq, xq]
                k = K3[dx + 1] * K3[dy + 1]
                gs[ys, xs] = np.where(ok, gs[ys, xs] + k * V[yq, xq], gs[ys, xs])
                gw[ys, xs] = np.where(ok, gw[ys, xs] + k, gw[ys, xs])
        den_l = sl * np.sqrt(gs / gw) + EPSILON
        den_z = (sz * t) * F(s)
        acc = np.zeros((Hh, W, 4), np.float32)   # sum w x (rgb), sum w^2 V
        sw = np.zeros((Hh, W), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sh = _shift(Hh, W, s * dx, s * dy)
                if sh is None:
                    continue
                ys, xs, yq, xq = sh
                ok = surf[yq, xq]
                k = H5[dx + 2] * H5[dy + 2]
                if dx == 0 and dy == 0:
                    w = np.full(ok.shape, k, np.float32)
                else:
                    npp, nq = n[ys, xs], n[yq, xq]
                    nd = (npp[..., 0] * nq[..., 0] + npp[..., 1] * nq[..., 1]) + npp[..., 2] * nq[..., 2]
                    wn = np.power(np.fmax(F(0), nd), sn)
                    wz = np.exp(-np.abs(t[ys, xs] - t[yq, xq]) / den_z[ys, xs])
                    wl = np.exp(-np.abs(l[ys, xs] - l[yq, xq]) / den_l[ys, xs])
                    w = (k * ((wn * wz) * wl)).astype(np.float32)
                term = np.concatenate([w[..., None] * x[yq, xq], ((w * w) * V[yq, xq])[..., None]], -1)
                acc[ys, xs] = np.where(ok[..., None], acc[ys, xs] + term, acc[ys, xs])
                sw[ys, xs] = np.where(ok, sw[ys, xs] + w, sw[ys, xs])
        out = np.concatenate([acc[..., :3] / sw[..., None], (acc[..., 3] / (sw * sw))[..., None]], -1)
    finally:
        np.seterr(**old)
    assert out.dtype == np.float32
    return np.where(surf[..., None], out, xv).astype(np.float32)


def filter_history(history, moments, albedo_depth, normal_class, iterations=-1, sigma_luminance=0.0, sigma_normal=0.0,
                   sigma_depth=0.0, feedback=-1):
    """Steps B and C on the state step A left.  Returns (history kept for the next frame, V_0 [H, W], filtered frame [H, W, 4])."""
    it, sl, sn, sz, fb = resolve(iterations, sigma_luminance, sigma_normal, sigma_depth, feedback)
    hist = np.asarray(history, np.float32)
    surf = np.asarray(normal_class)[..., 3] == 0
    v0 = variance(hist, moments, albedo_depth, normal_class, sn, sz)
    xv = np.concatenate([hist[..., :3], v0[..., None]], -1)
    kept = hist.copy()
    for i in range(it):
        xv = level(xv, albedo_depth, normal_class, i, sl, sn, sz)
        if i == 0 and fb:
            kept[..., :3] = np.where(surf[..., None], xv[..., :3], hist[..., :3])
    out = hist.copy()
    out[..., :3] = np.where(surf[..., None], xv[..., :3] * albedo(albedo_depth, normal_class), hist[..., :3])
    return kept, v0, out


def svgf_image(color, albedo_depth, normal_class, cam, history=None, moments=None, albedo_depth_prev=None, normal_class_prev=None,
               cam_prev=None, max_history=0, depth_tolerance=0.0, normal_threshold=0.0, min_weight=0.0, **filt):
    """One mpt_svgf_accumulate / mpt_svgf_image.  Returns (history_out [H, W, 4], moments_variance_out [H, W, 4] = (M1, M2, V_0, 0),
    filtered_out [H, W, 4], number of pixels reset)."""
    hist, mom, n_reset = accumulate(color, albedo_depth, normal_class, cam, history, moments, albedo_depth_prev, normal_class_prev,
                                    cam_prev, max_history, depth_tolerance, normal_threshold, min_weight)
    kept, v0, out = filter_history(hist, mom, albedo_depth, normal_class, **filt)
    mv = np.zeros(hist.shape, np.float32)
    mv[..., :2] = mom
    mv[..., 2] = v0
    return kept, mv, out, n_reset


def run_path(frames, hi, **params):
    """The restatement along a path of temporal_ref.oracle_path: (F = MSE(last raw frame) / MSE(last filtered frame), share of the
    last frame reset, last filtered frame).  Without feedback only the last frame needs steps B and C."""
    fb = resolve(**{k: v for k, v in params.items() if k in ("iterations", "feedback")})
    need_all = fb[4] and fb[0] >= 1
    a_keys = ("max_history", "depth_tolerance", "normal_threshold", "min_weight")
    pa = {k: v for k, v in params.items() if k in a_keys}
    pf = {k: v for k, v in params.items() if k not in a_keys}
    hist = mom = prev = out = None
    n_reset = 0
    for f, (u, c, ad, nc) in enumerate(frames):
        if prev is None:
            hist, mom, n_reset = accumulate(c, ad, nc, u, **pa)
        else:
            hist, mom, n_reset = accumulate(c, ad, nc, u, hist, mom, prev[2], prev[3], prev[0], **pa)
        if need_all or f == len(frames) - 1:
            hist, _, out = filter_history(hist, mom, ad, nc, **pf)
        prev = (u, c, ad, nc)
    c = frames[-1][1]
    return tr.mse(c, hi) / tr.mse(out, hi), n_reset / float(c.shape[0] * c.shape[1]), out
