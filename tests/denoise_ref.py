"""numpy float32 restatement of the denoise filter of include/mpt.h (mpt_denoise_params), in the tap order and operation order of
k_dn_level (metalpathtracer_amd/csrc/mpt_denoise.h).  The arithmetic is IEEE float32 throughout; only exp and pow may differ
from the device's by an ulp or so.  Test code: the product never imports it."""
import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
DEFAULTS = dict(iterations=3, sigma_luminance=8.0, sigma_normal=32.0, sigma_depth=0.25)   # include/mpt.h MPT_DENOISE_DEFAULT_*


def lum(x):
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def denoise(color, albedo_depth, normal_class, iterations=None, sigma_luminance=None, sigma_normal=None, sigma_depth=None):
    """color, albedo_depth = (albedo, t), normal_class = (normal, class): [H, W, 4] float32.  Returns the [H, W, 4] output."""
    it = DEFAULTS["iterations"] if iterations is None or iterations < 0 else int(iterations)
    sl = F(sigma_luminance if sigma_luminance and sigma_luminance > 0 else DEFAULTS["sigma_luminance"])
    sn = F(sigma_normal if sigma_normal and sigma_normal > 0 else DEFAULTS["sigma_normal"])
    sz = F(sigma_depth if sigma_depth and sigma_depth > 0 else DEFAULTS["sigma_depth"])
    c = np.asarray(color, np.float32)
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    if it == 0:
        return c.copy()
    Hh, W = c.shape[:2]
    surf = nc[..., 3] == 0
    n = nc[..., :3]
    t = ad[..., 3]
    amax = np.maximum(ad[..., :3], F(1e-3))
    x = c[..., :3] / amax
    l = lum(x)
    old = np.seterr(all="ignore")
    try:
        for i in range(it):
            s = 1 << i
            sli = sl * F(2.0 ** -i)
            den_z = (sz * t) * F(s)
            sr = np.zeros((Hh, W), np.float32)
            sg = np.zeros((Hh, W), np.float32)
            sb = np.zeros((Hh, W), np.float32)
            sw = np.zeros((Hh, W), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = H5[dx + 2] * H5[dy + 2]
                    # tap q = p + s (dx, dy) for every p: shifted views, invalid where q leaves the image or is not a surface
                    ys = slice(max(0, -s * dy), min(Hh, Hh - s * dy))
                    xs = slice(max(0, -s * dx), min(W, W - s * dx))
                    yq = slice(ys.start + s * dy, ys.stop + s * dy)
                    xq = slice(xs.start + s * dx, xs.stop + s * dx)
                    if ys.start >= ys.stop or xs.start >= xs.stop:
                        continue
                    ok = surf[yq, xq]
                    if dx == 0 and dy == 0:
                        w = np.full(ok.shape, k, np.float32)
                    else:
                        npp, nq = n[ys, xs], n[yq, xq]
                        nd = (npp[..., 0] * nq[..., 0] + npp[..., 1] * nq[..., 1]) + npp[..., 2] * nq[..., 2]
                        wn = np.power(np.maximum(F(0), nd), sn)
                        wz = np.exp(-np.abs(t[ys, xs] - t[yq, xq]) / den_z[ys, xs])
                        wl = np.exp(-np.abs(l[ys, xs] - l[yq, xq]) / sli)
                        w = k * ((wn * wz) * wl)
                    w = np.where(ok, w, F(0)).astype(np.float32)
                    xqv = x[yq, xq]
                    m = ok
                    sr[ys, xs] = np.where(m, sr[ys, xs] + w * xqv[..., 0], sr[ys, xs])
                    sg[ys, xs] = np.where(m, sg[ys, xs] + w * xqv[..., 1], sg[ys, xs])
                    sb[ys, xs] = np.where(m, sb[ys, xs] + w * xqv[..., 2], sb[ys, xs])
                    sw[ys, xs] = np.where(m, sw[ys, xs] + w, sw[ys, xs])
            x = np.stack([sr / sw, sg / sw, sb / sw], -1)
            l = lum(x)
    finally:
        np.seterr(**old)
    out = c.copy()
    rgb = x * amax
    out[..., :3] = np.where(surf[..., None], rgb, c[..., :3])
    return out


def first_hit_guides(u, buffers, first_hit):
    """Guide buffers from the oracle's first_hit through every pixel centre (mpt_read_aovs' definition): (albedo_depth,
    normal_class, prim).  u: uniforms (screenSize, camera); buffers: (bvh, prims, mats, prim_idx) of the reference format."""
    W, Hh = int(u.screenSize[0]), int(u.screenSize[1])
    mats = np.asarray(buffers[2], np.float32).reshape(-1, 8)
    cam = np.array(u.cameraPosition[:3], np.float32)
    first = np.array(u.firstPixelPosition[:3], np.float32)
    vu = np.array(u.viewportU[:3], np.float32)
    vv = np.array(u.viewportV[:3], np.float32)
    ad = np.zeros((Hh, W, 4), np.float32)
    nc = np.zeros((Hh, W, 4), np.float32)
    prim = np.full((Hh, W), -1, np.int32)
    fW, fH = F(u.screenSize[0]), F(u.screenSize[1])
    for py in range(Hh):
        uvy = (F(py) + F(0.5)) / fH
        for px in range(W):
            uvx = (F(px) + F(0.5)) / fW
            d = (first + uvx * vu + uvy * vv) - cam
            d = d * (F(1) / np.sqrt(F((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))   # normalize3: v * (1 / sqrt(dot(v, v)))
            t, p, nrm, _ = first_hit(cam, d, buffers)
            if p < 0:
                ad[py, px] = (0, 0, 0, np.inf)
                nc[py, px] = (0, 0, 0, 2)
                continue
            m = mats[p]
            ad[py, px] = (m[0], m[1], m[2], t)
            nc[py, px] = (nrm[0], nrm[1], nrm[2], 1.0 if m[7] > 0 else 0.0)
            prim[py, px] = p
    return ad, nc, prim
