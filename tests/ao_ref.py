"""numpy float32 restatement of the ambient-occlusion pass of include/mpt.h (mpt_ao_params): Philox4x32-10, u01, sincos_2pi and the
origin and direction arithmetic of k_ao (metalpathtracer_amd/csrc/mpt_ao.h) in the order written there, each a single IEEE float32
operation.  Occlusion itself comes from the oracle's closest hit: a ray is occluded iff first_hit's t is below the limit (the way
tests/denoise_ref.py:first_hit_guides uses the oracle).  Test code: the product never imports it."""
import numpy as np

F = np.float32
U32 = np.uint32
WORD2 = 0xFFFFFFFE          # Philox counter word 2 of an AO sample: no bounce has it, the pixel jitter has 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words and key words: uint32 arrays (or scalars) that broadcast.  Returns the four output words."""
    c = [np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0 = np.uint64(int(k0) & 0xFFFFFFFF)
    k1 = np.uint64(int(k1) & 0xFFFFFFFF)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return [x.astype(np.uint32) for x in c]


def u01(x):
    return (np.asarray(x, np.uint32) >> U32(8)).astype(np.float32) * F(5.9604644775390625e-08)


def sincos_2pi(u):
    """sin / cos(2 pi u), u in [0, 1): the quadrant reduction and the two Taylor polynomials of mpt_device.h."""
    u = np.asarray(u, np.float32)
    x = u * F(4.0)
    q = (x + F(0.5)).astype(np.int32)
    r = x - q.astype(np.float32)
    th = r * F(1.57079637050628662109375)
    t2 = th * th
    ps = F(-1.98412701138295233249664306640625e-4) + t2 * F(2.755731884462875314056873321533203125e-6)
    ps = F(8.3333337679505348205566406250e-3) + t2 * ps
    ps = F(-0.16666667163372039794921875) + t2 * ps
    s = th + (th * t2) * ps
    pc = F(-1.38888892251998186111450195312500e-3) + t2 * F(2.48015876422869041562080383300781250e-5)
    pc = F(4.1666667908430099487304687500e-2) + t2 * pc
    pc = F(-0.5) + t2 * pc
    c = F(1.0) + t2 * pc
    k = q & 3
    s_out = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c)))
    c_out = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s)))
    return s_out.astype(np.float32), c_out.astype(np.float32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    return v * (F(1) / np.sqrt(dot(v, v)))[..., None]


def _cam(u):
    g = lambda a: np.array(list(a[:3]), np.float32)
    return g(u.cameraPosition), g(u.firstPixelPosition), g(u.viewportU), g(u.viewportV)


def sample_rays(albedo_depth, normal_class, cam, sample_begin, sample_count, seed=(0, 0)):
    """The rays of the pass: (surface [H,W] bool, origins [H,W,3], directions [H,W,N,3]); rows of non-surface pixels are not to be used."""
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    H, W = ad.shape[:2]
    cam_p, first, vu, vv = _cam(cam)
    old = np.seterr(all="ignore")
    try:
        px, py = np.meshgrid(np.arange(W), np.arange(H))
        uvx = ((px.astype(np.float32) + F(0.5)) / F(W))[..., None]
        uvy = ((py.astype(np.float32) + F(0.5)) / F(H))[..., None]
        dc = normalize(((first + uvx * vu) + uvy * vv) - cam_p)
        n = nc[..., :3]
        t = ad[..., 3]
        P = cam_p + t[..., None] * dc
        o = (P + F(0.0001) * n).astype(np.float32)
        pixel = (py * W + px).astype(np.uint32)[..., None]
        s = (np.arange(sample_count, dtype=np.uint64) + np.uint64(sample_begin)).astype(np.uint32)[None, None, :]
        r = philox4x32_10(pixel, s, U32(WORD2), U32(0), seed[0], seed[1])
        uz, uphi = u01(r[0]), u01(r[1])
        z = F(2.0) * uz - F(1.0)
        sn, cs = sincos_2pi(uphi)
        rr = np.sqrt(F(1.0) - z * z)
        ruv = np.stack([rr * cs, rr * sn, z], -1).astype(np.float32)
        d = normalize(n[:, :, None, :] + ruv).astype(np.float32)
    finally:
        np.seterr(**old)
    return nc[..., 3] == 0, o, d


def occluded(tstar, directions, tmax):
    """The any-hit answer from the closest hit's t (include/mpt.h): nothing for !(tmax > 1e-4) or a NaN direction, else t* < tmax."""
    d = np.asarray(directions, np.float32)
    tmax = np.asarray(tmax, np.float32)
    with np.errstate(invalid="ignore"):
        wanted = (tmax > F(1e-4)) & ~np.isnan(d).any(-1)
        return wanted & (np.asarray(tstar, np.float32) < tmax)


def closest_t(origins, directions, buffers, first_hit):
    """The oracle's closest t per ray (+inf for a miss); origins broadcast against directions [..., 3]."""
    d = np.asarray(directions, np.float32)
    o = np.broadcast_to(np.asarray(origins, np.float32), d.shape)
    out = np.empty(d.shape[:-1], np.float32)
    flat_o, flat_d, flat_t = o.reshape(-1, 3), d.reshape(-1, 3), out.reshape(-1)
    for i in range(flat_t.shape[0]):
        t, p = first_hit(flat_o[i], flat_d[i], buffers)[:2]
        flat_t[i] = t if p >= 0 else np.inf
    return out


def closest_t_of_pass(albedo_depth, normal_class, cam, buffers, first_hit, sample_begin, sample_count, seed=(0, 0)):
    """t* of every ray of the pass, [H,W,N] (+inf where the pixel is no surface: never read): share it among the tests of one scene."""
    surface, o, d = sample_rays(albedo_depth, normal_class, cam, sample_begin, sample_count, seed)
    t = np.full(d.shape[:-1], np.inf, np.float32)
    if surface.any():
        t[surface] = closest_t(o[surface][:, None, :], d[surface], buffers, first_hit)
    return t


def ambient_occlusion(albedo_depth, normal_class, cam, sample_begin, sample_count, radius, seed=(0, 0), tstar=None, buffers=None,
                      first_hit=None):
    """(ao [H,W] float32, occluded [H,W] uint32).  tstar: closest_t_of_pass for the same samples (computed here when None)."""
    surface, _, d = sample_rays(albedo_depth, normal_class, cam, sample_begin, sample_count, seed)
    if tstar is None:
        tstar = closest_t_of_pass(albedo_depth, normal_class, cam, buffers, first_hit, sample_begin, sample_count, seed)
    tmax = F(radius) if radius > 0 else F(np.inf)
    count = np.where(surface, occluded(tstar, d, tmax).sum(-1), 0).astype(np.uint32)
    N = F(sample_count)
    ao = np.where(surface, (F(sample_count) - count.astype(np.float32)) / N, F(1)).astype(np.float32)
    return ao, count
