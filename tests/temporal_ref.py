"""numpy float32 restatement of the temporal accumulation of include/mpt.h (mpt_temporal_params), in the tap order and operation
order of k_tp_reproject (metalpathtracer_amd/csrc/mpt_temporal.h).  Only + - * / sqrt floor and comparisons, each a single IEEE
float32 operation: the device must agree bit for bit.  Test code: the product never imports it."""
import numpy as np

F = np.float32
DEFAULTS = dict(max_history=32, depth_tolerance=0.05, normal_threshold=0.5, min_weight=0.05)   # include/mpt.h MPT_TEMPORAL_DEFAULT_*


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def camera_key(u):
    """The fourteen floats that identify a camera: position, viewportU, viewportV, firstPixelPosition, screenSize."""
    return np.array(list(u.cameraPosition[:3]) + list(u.viewportU[:3]) + list(u.viewportV[:3]) + list(u.firstPixelPosition[:3])
                    + list(u.screenSize[:2]), np.float32)


def pack_guide(albedo_depth, normal_class):
    """(normal, t) with t = +inf for a miss (class 2): the history guide."""
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    g = nc.copy()
    g[..., 3] = np.where(nc[..., 3] == 2, F(np.inf), ad[..., 3])
    return g


def resolve(max_history=0, depth_tolerance=0.0, normal_threshold=0.0, min_weight=0.0):
    return (F(max_history if max_history else DEFAULTS["max_history"]),
            F(depth_tolerance if depth_tolerance > 0 else DEFAULTS["depth_tolerance"]),
            F(normal_threshold if normal_threshold > 0 else DEFAULTS["normal_threshold"]),
            F(min_weight if min_weight > 0 else DEFAULTS["min_weight"]))


def accumulate(color, albedo_depth, normal_class, cam, history=None, albedo_depth_prev=None, normal_class_prev=None, cam_prev=None,
               **params):
    """One mpt_temporal_accumulate: color = c, guides as mpt_read_aovs returns them ([H, W, 4] float32), cam / cam_prev: uniforms.
    Returns (new history [H, W, 4], number of pixels reset)."""
    maxh, ztol, nth, minw = resolve(**params)
    c = np.asarray(color, np.float32)
    ad = np.asarray(albedo_depth, np.float32)
    nc = np.asarray(normal_class, np.float32)
    H, W = c.shape[:2]
    out = np.empty((H, W, 4), np.float32)
    if history is None:                                           # step 7
        out[..., :3] = c[..., :3]
        out[..., 3] = 1
        return out, H * W
    hist = np.asarray(history, np.float32)
    k, kh = camera_key(cam), camera_key(cam_prev)
    acc = np.zeros((H, W, 4), np.float32)
    sw = np.zeros((H, W), np.float32)
    old = np.seterr(all="ignore")
    try:
        if k.tobytes() == kh.tobytes():                           # step 6
            acc = hist.copy()
            sw[...] = 1
        else:
            gh = pack_guide(albedo_depth_prev, normal_class_prev)
            cam_p, vu, vv, first = k[0:3], k[3:6], k[6:9], k[9:12]
            cam_h, vu_h, vv_h, first_h = kh[0:3], kh[3:6], kh[6:9], kh[9:12]
            fW, fH = F(W), F(H)
            px, py = np.meshgrid(np.arange(W), np.arange(H))
            uvx = ((px.astype(np.float32) + F(0.5)) / fW)[..., None]
            uvy = ((py.astype(np.float32) + F(0.5)) / fH)[..., None]
            dv = ((first + uvx * vu) + uvy * vv) - cam_p          # step 1
            d = dv * (F(1) / np.sqrt(dot(dv, dv)))[..., None]
            hit = nc[..., 3] != 2
            t = ad[..., 3]
            r = np.where(hit[..., None], (cam_p + t[..., None] * d) - cam_h, d).astype(np.float32)
            nn = np.array([vu_h[1] * vv_h[2] - vu_h[2] * vv_h[1], vu_h[2] * vv_h[0] - vu_h[0] * vv_h[2],
                           vu_h[0] * vv_h[1] - vu_h[1] * vv_h[0]], np.float32)   # step 2
            fc = first_h - cam_h
            s = dot(fc, nn) / dot(r, nn)
            q = s[..., None] * r - fc                              # step 3
            u = dot(q, vu_h) / dot(vu_h, vu_h)
            v = dot(q, vv_h) / dot(vv_h, vv_h)
            fx = u * fW - F(0.5)
            fy = v * fH - F(0.5)
            ok0 = (s > 0) & (s < F(np.inf)) & (fx >= -1) & (fx < fW) & (fy >= -1) & (fy < fH)
            fx = np.where(ok0, fx, F(0))
            fy = np.where(ok0, fy, F(0))
            flx, fly = np.floor(fx), np.floor(fy)
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            ax, ay = fx - flx, fy - fly
            rl = np.sqrt(dot(r, r))
            tol = ztol * rl
            n = nc[..., :3]
            for j in (0, 1):                                       # step 4
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inb = ok0 & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    gq = gh[qyc, qxc]
                    qhit = gq[..., 3] < F(np.inf)
                    okh = qhit & (np.abs(gq[..., 3] - rl) <= tol) & (dot(n, gq) >= nth)
                    valid = inb & np.where(hit, okh, ~qhit)
                    w = ((ax if i else F(1) - ax) * (ay if j else F(1) - ay)).astype(np.float32)
                    hq = hist[qyc, qxc]
                    acc = np.where(valid[..., None], acc + w[..., None] * hq, acc)
                    sw = np.where(valid, sw + w, sw)
        assert acc.dtype == np.float32 and sw.dtype == np.float32
        good = sw >= minw                                          # step 5
        h = acc / sw[..., None]
        nlen = np.minimum(h[..., 3] + F(1), maxh)
        res = h[..., :3] + (c[..., :3] - h[..., :3]) / nlen[..., None]
        out[..., :3] = np.where(good[..., None], res, c[..., :3])
        out[..., 3] = np.where(good, nlen, F(1))
    finally:
        np.seterr(**old)
    return out, int((~good).sum())


# ---- the calibration paths (tests/test_temporal_cpu.py, tests/test_gpu_temporal.py, tools/temporal_sweep.py) ----------------------
# 24 frames of 1 philox spp (sample index = frame, depth 8, seed (1, 0)); the camera of frame f is the start camera moved by f steps
# and turned by f x 0.1 degrees about the y axis.  The error of the last frame is taken against 1024 spp of seed (7, 0).
CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)   # (tests/conftest.py)
PATHS = {"cornell.xml": dict(cam=CORNELL_CAM, W=64, H=64, step=(0.01, 0.0, 0.0)),
         "scene.xml": dict(cam=None, W=96, H=54, step=(0.2, 0.0, 0.0)),
         "bunny20.xml": dict(cam=None, W=96, H=54, step=(0.2, 0.0, 0.0))}
PATH_FRAMES = 24
PATH_YAW_DEG = 0.1


def path_camera(cam0, f, step, yaw_deg=PATH_YAW_DEG):
    a = np.deg2rad(yaw_deg * f)
    x, y, z = [float(v) for v in cam0["fwd"]]
    fwd = (x * np.cos(a) + z * np.sin(a), y, -x * np.sin(a) + z * np.cos(a))
    pos = tuple(float(p) + float(s) * f for p, s in zip(cam0["pos"], step))
    return dict(pos=pos, fwd=fwd, up=cam0["up"], vfov=cam0["vfov"])


def path_uniforms(name, sc, frames=PATH_FRAMES):
    """The oracle uniforms of every frame of a calibration path."""
    from oracle import binding as ob
    P = PATHS[name]
    cam0 = P["cam"] or ob.camera_reset()
    return [ob.make_uniforms(P["W"], P["H"], sc.prim_count, sc.triangle_count, cam=path_camera(cam0, f, P["step"])) for f in range(frames)]


def oracle_path(name, sc, buf, frames=PATH_FRAMES, threads=16):
    """Everything of a path that does not depend on the temporal parameters: per frame (uniforms, colour, albedo_depth, normal_class)
    from the oracle, and the 1024-spp image at the last camera."""
    from oracle import binding as ob
    import denoise_ref as dr
    out = []
    for f, u in enumerate(path_uniforms(name, sc, frames)):
        c, _ = ob.render(u, buf, rng_mode=ob.RNG_PHILOX, max_depth=8, sample_begin=f, sample_count=1, seed=(1, 0), threads=threads)
        ad, nc, _ = dr.first_hit_guides(u, buf, ob.first_hit)
        out.append((u, c, ad, nc))
    hi, _ = ob.render(out[-1][0], buf, rng_mode=ob.RNG_PHILOX, max_depth=8, sample_count=1024, seed=(7, 0), threads=threads)
    return out, hi / F(1024)


def mse(a, b):
    return float(((a[..., :3] - b[..., :3]).astype(np.float64) ** 2).mean())


def run_path(frames, hi, **params):
    """The restatement along a path: (F = MSE(last raw frame) / MSE(last history), share of the last frame reset, last history)."""
    hist = prev = None
    n_reset = 0
    for u, c, ad, nc in frames:
        if prev is None:
            hist, n_reset = accumulate(c, ad, nc, u, **params)
        else:
            hist, n_reset = accumulate(c, ad, nc, u, hist, prev[2], prev[3], prev[0], **params)
        prev = (u, c, ad, nc)
    c = frames[-1][1]
    return mse(c, hi) / mse(hist, hi), n_reset / float(c.shape[0] * c.shape[1]), hist
