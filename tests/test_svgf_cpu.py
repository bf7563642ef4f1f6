"""SVGF without a GPU: the new C-ABI symbols, their structs and argument checks, properties of the numpy restatement
(tests/svgf_ref.py) that follow from the contract of include/mpt.h, and the calibration of the defaults along the three camera
paths of tests/temporal_ref.py against the oracle and against the two filters the tree already had (profiles/r08_svgf_sweep.txt)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as dr
import svgf_ref as sr
import temporal_ref as tr
from conftest import ROOT, oracle_scene
from metalpathtracer_amd import capi, host

F = np.float32
NEW_MPT = ("mpt_svgf_accumulate", "mpt_read_svgf", "mpt_svgf_buffer", "mpt_read_svgf_state", "mpt_svgf_reset", "mpt_svgf_image")
NEW_HOST = ("mpt_renderer_draw_svgf", "mpt_renderer_read_svgf")
# F = MSE(last 1-spp frame) / MSE(last filtered frame) of the restatement with the defaults, 24 frames against 1024 spp
# (profiles/r08_svgf_sweep.txt, the row of the defaults).  tests/test_gpu_svgf.py asks the device for 0.9 x these.
HELD_F = {"cornell.xml": 61.90, "scene.xml": 44.74, "bunny20.xml": 16.45}
MAX_RESET = 0.05
PARAM_FIELDS = [("int32_t", "source"), ("uint32_t", "samples"), ("uint32_t", "max_history"), ("float", "depth_tolerance"),
                ("float", "normal_threshold"), ("float", "min_weight"), ("int32_t", "iterations"), ("float", "sigma_luminance"),
                ("float", "sigma_normal"), ("float", "sigma_depth"), ("int32_t", "feedback")]


def test_svgf_symbols_exported_declared_and_listed():
    L = C.CDLL(capi.LIB_PATH)
    hl = host.load()
    mpt_h = open(os.path.join(ROOT, "include", "mpt.h")).read()
    host_h = open(os.path.join(ROOT, "include", "mpt_host.h")).read()
    for n in NEW_MPT:
        assert n in capi.SYMBOLS and hasattr(L, n) and re.search(r"\bint %s\(" % n, mpt_h), n
    for n in NEW_HOST:
        assert n in host.SYMBOLS and hasattr(hl, n) and re.search(r"\bint %s\(" % n, host_h), n


def test_svgf_struct_layout():
    P, I = capi.SvgfParams, capi.SvgfInfo
    assert C.sizeof(P) == 44 and C.sizeof(I) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [(n, 4 * i) for i, (_, n) in enumerate(PARAM_FIELDS)]
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [("pixels_reprojected", 0), ("pixels_reset", 8)]
    text = open(os.path.join(ROOT, "include", "mpt.h")).read()
    body = re.search(r"typedef struct mpt_svgf_params \{(.*?)\} mpt_svgf_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == PARAM_FIELDS


def test_svgf_defaults_agree_with_header():
    text = open(os.path.join(ROOT, "include", "mpt.h")).read()
    for key in ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth", "feedback"):
        line = [l for l in text.splitlines() if l.startswith("#define MPT_SVGF_DEFAULT_" + key.upper() + " ")][0]
        v = float(line.split()[2].rstrip("fu"))
        assert v == capi.SVGF_DEFAULTS[key] == sr.DEFAULTS[key], key
    line = [l for l in text.splitlines() if l.startswith("#define MPT_SVGF_EPSILON ")][0]
    assert F(line.split()[2].rstrip("f")) == sr.EPSILON == F(capi.SVGF_EPSILON)


def test_svgf_null_arguments():
    L = capi.load()
    hl = host.load()
    INVALID = 1
    buf = np.zeros(16, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    p = capi.svgf_params(samples=1)
    u = capi.Uniforms()
    info = capi.SvgfInfo()
    assert L.mpt_svgf_accumulate(None, C.byref(p), C.byref(info)) == INVALID
    assert L.mpt_svgf_accumulate(None, None, None) == INVALID
    assert L.mpt_read_svgf(None, fp) == INVALID
    out, n = C.c_void_p(), C.c_uint64()
    assert L.mpt_svgf_buffer(None, C.byref(out), C.byref(n)) == INVALID
    assert L.mpt_read_svgf_state(None, fp, fp) == INVALID
    assert L.mpt_svgf_reset(None) == INVALID
    assert L.mpt_svgf_image(None, 2, 2, fp, fp, fp, C.byref(u), fp, fp, fp, fp, C.byref(u), C.byref(p), fp, fp, fp, C.byref(info)) == INVALID
    assert hl.mpt_renderer_draw_svgf(None, 1, C.byref(p), C.byref(info)) == INVALID
    assert hl.mpt_renderer_read_svgf(None, fp) == INVALID


# ---- properties of the restatement ----------------------------------------------------------------------------------------------
def _cam(pos=(0.0, 0.0, 0.0), fwd=(0.0, 0.0, -1.0), W=64, H=48, vfov=40.0):
    from oracle import binding as ob
    return ob.make_uniforms(W, H, 1, 0, cam=dict(pos=pos, fwd=fwd, up=(0.0, 1.0, 0.0), vfov=vfov))


def _plane_guides(u, W, H, depth=5.0, albedo=0.5, cls=0):
    """Guides of the plane z = -depth seen from camera u (which looks down -z from z = 0)."""
    k = tr.camera_key(u).astype(np.float64)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    dv = k[9:12] + ((px + 0.5) / W)[..., None] * k[3:6] + ((py + 0.5) / H)[..., None] * k[6:9] - k[0:3]
    d = dv / np.linalg.norm(dv, axis=-1, keepdims=True)
    t = depth / -d[..., 2]
    ad = np.concatenate([np.full((H, W, 3), albedo), t[..., None]], -1).astype(np.float32)
    nc = np.zeros((H, W, 4), np.float32)
    nc[..., :3] = (0.0, 0.0, 1.0)
    nc[..., 3] = cls
    return ad, nc


def _flat_guides(W, H, albedo=1.0, t=5.0):
    """ONE hit distance and one normal for every pixel (the unit hook allows it): wn = wz = 1 for every tap."""
    ad = np.empty((H, W, 4), np.float32)
    ad[..., :3] = albedo
    ad[..., 3] = t
    nc = np.zeros((H, W, 4), np.float32)
    nc[..., 2] = 1
    return ad, nc


def test_same_camera_is_the_running_mean_of_x_l_and_l_squared():
    W, H = 16, 12
    u = _cam(W=W, H=H)
    ad, nc = _plane_guides(u, W, H)
    nc[:3, :, 3] = 2   # some sky, some light
    nc[3:5, :, 3] = 1
    a = sr.albedo(ad, nc).astype(np.float64)
    rng = np.random.default_rng(0)
    for maxh in (4, 32):
        hist = mom = None
        xs = []
        for k in range(1, 9):
            c = rng.random((H, W, 4), np.float32)
            xs.append(c[..., :3].astype(np.float64) / a)
            if hist is None:
                hist, mom, n_reset = sr.accumulate(c, ad, nc, u, max_history=maxh)
                assert n_reset == W * H
            else:
                hist, mom, n_reset = sr.accumulate(c, ad, nc, u, hist, mom, ad, nc, u, max_history=maxh)
                assert n_reset == 0
            assert (hist[..., 3] == min(k, maxh)).all()
            if k <= maxh:
                ls = [0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2] for x in xs]
                # 1e-6 in the convention of tests/test_gpu_denoise.py: relative to max(1, the largest value) — x reaches 2 here (albedo
                # 0.5) and l^2 reaches 4, where one float32 ulp is already 4.8e-7 — so M2, a mean of squares, is held relative to scale^2
                scale = max(1.0, float(np.max(xs)))
                assert np.abs(hist[..., :3] - np.mean(xs, axis=0)).max() <= 1e-6 * scale
                assert np.abs(mom[..., 0] - np.mean(ls, axis=0)).max() <= 1e-6 * scale
                assert np.abs(mom[..., 1] - np.mean(np.square(ls), axis=0)).max() <= 1e-6 * scale * scale


def test_camera_turned_round_resets_every_pixel():
    W, H = 32, 24
    u0, u1 = _cam(W=W, H=H), _cam(fwd=(0.0, 0.0, 1.0), W=W, H=H)
    ad, nc = _plane_guides(u0, W, H, albedo=1.0)
    rng = np.random.default_rng(1)
    c, hist = rng.random((H, W, 4), np.float32), rng.random((H, W, 4), np.float32) + F(1)
    mom = rng.random((H, W, 2), np.float32)
    out, m, n_reset = sr.accumulate(c, ad, nc, u1, hist, mom, ad, nc, u0)
    assert n_reset == W * H and (out[..., 3] == 1).all()
    assert np.array_equal(out[..., :3].view(np.uint32), c[..., :3].view(np.uint32))
    l = dr.lum(c)
    assert np.array_equal(m[..., 0], l) and np.array_equal(m[..., 1], l * l)


def test_emitters_and_sky_come_back_unfiltered_and_are_never_taps():
    W, H = 24, 20
    u = _cam(W=W, H=H)
    ad, nc = _plane_guides(u, W, H)
    nc[8:12, 8:14, 3] = 1      # a light in the middle of the surface
    nc[:2, :, 3] = 2           # a strip of sky
    ad[:2, :, 3] = np.inf
    rng = np.random.default_rng(2)
    c = rng.random((H, W, 4), np.float32)
    c2 = c.copy()
    c2[8:12, 8:14, :3] = 1000.0
    c2[:2, :, :3] *= 50.0
    other = nc[..., 3] != 0
    for n in range(0, 4):
        h1, mv1, f1, _ = sr.svgf_image(c, ad, nc, u, iterations=n)
        h2, mv2, f2, _ = sr.svgf_image(c2, ad, nc, u, iterations=n)
        assert np.array_equal(f1[other][:, :3], c[other][:, :3]) and (f1[other][:, 3] == 1).all()      # (X, n) of step A: a = 1
        assert np.array_equal(f2[other][:, :3], c2[other][:, :3])
        assert (mv1[other][:, 2] == 0).all()
        assert np.array_equal(f1[~other].view(np.uint32), f2[~other].view(np.uint32)), n               # the surface does not see them
        assert np.array_equal(mv1[~other][:, 2], mv2[~other][:, 2])
    assert np.array_equal(sr.svgf_image(c, ad, nc, u, iterations=0)[2][~other][:, :3],
                          ((c[..., :3] / sr.albedo(ad, nc)) * sr.albedo(ad, nc))[~other])


@pytest.mark.parametrize("cls", [0, 1])
def test_step_a_with_albedo_one_and_one_hit_class_is_the_temporal_stage(cls):
    """Then the two stages differ in nothing: this ties the new reprojection to the tested one."""
    W, H, depth = 48, 32, 5.0
    u0 = _cam(W=W, H=H)
    k0 = tr.camera_key(u0).astype(np.float64)
    u1 = _cam(pos=(3.3 * np.linalg.norm(k0[3:6]) * depth / W, 0.01, 0.0), fwd=(0.01, 0.0, -1.0), W=W, H=H)
    ad0, nc0 = _plane_guides(u0, W, H, depth, albedo=1.0, cls=cls)
    ad1, nc1 = _plane_guides(u1, W, H, depth, albedo=1.0, cls=cls)
    nc1[:4, :, 3] = 2                                          # some sky in both frames
    nc0[:5, :, 3] = 2
    ad0[10:14, 10:20, 3] *= F(1.5)                             # a depth step the taps must not cross
    rng = np.random.default_rng(3)
    c = rng.random((H, W, 4), np.float32)
    hist = rng.random((H, W, 4), np.float32)
    hist[..., 3] = rng.integers(1, 40, (H, W))
    mom = rng.random((H, W, 2), np.float32)
    ref, ref_reset = tr.accumulate(c, ad1, nc1, u1, hist, ad0, nc0, u0)
    got, _, n_reset = sr.accumulate(c, ad1, nc1, u1, hist, mom, ad0, nc0, u0)
    assert n_reset == ref_reset and 0 < n_reset < W * H
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_no_tap_crosses_from_one_hit_class_to_the_other():
    W, H, depth = 32, 16, 5.0
    u0 = _cam(W=W, H=H)
    k0 = tr.camera_key(u0).astype(np.float64)
    u1 = _cam(pos=(0.3 * np.linalg.norm(k0[3:6]) * depth / W, 0.0, 0.0), W=W, H=H)
    right = np.zeros((H, W), bool)
    right[:, W // 2:] = True
    for cls_frame, cls_foreign in ((0, 1), (1, 0)):
        ad0, nc0 = _plane_guides(u0, W, H, depth, albedo=1.0, cls=cls_frame)
        ad1, nc1 = _plane_guides(u1, W, H, depth, albedo=1.0, cls=cls_frame)
        nc0[right, 3] = cls_foreign                            # same geometry, the other class: only the class test can stop the tap
        hist = np.ones((H, W, 4), np.float32)
        hist[right, :3] = 100
        mom = np.ones((H, W, 2), np.float32)
        mom[right] = 100
        c = np.ones((H, W, 4), np.float32)
        out, m, _ = sr.accumulate(c, ad1, nc1, u1, hist, mom, ad0, nc0, u0)
        assert out[..., :3].max() <= 1.0 + 1e-6 and m.max() <= 1.0 + 1e-6
        assert (out[:, : W // 2 - 1, 3] == 2).all() and (out[:, W // 2:, 3] == 1).all()
        # the temporal stage, which has no such test, does take those taps
        ref, _ = tr.accumulate(c, ad1, nc1, u1, hist, ad0, nc0, u0)
        assert ref[..., :3].max() > 50


def test_zero_variance_closes_the_filter():
    """A converged luminance step of 0.5 (a shadow edge) on a flat plane: with V = 0 the stop is MPT_SVGF_EPSILON wide and the frame
    comes back as it went in, where the fixed stop of mpt_denoise (sigma_luminance 8: exp(-0.5 / 8) = 0.94) smears it."""
    W, H = 40, 24
    u = _cam(W=W, H=H)
    ad, nc = _plane_guides(u, W, H, albedo=1.0)
    hist = np.empty((H, W, 4), np.float32)
    hist[..., :3] = 0.25
    hist[:, W // 2:, :3] = 0.75
    hist[..., 3] = 8
    m1 = dr.lum(hist[..., :3])
    mom = np.stack([m1, m1 * m1], -1)
    for n in (1, 2, 3, 5):
        kept, v0, out = sr.filter_history(hist, mom, ad, nc, iterations=n)
        assert (v0 == 0).all()
        assert np.abs(out[..., :3] - hist[..., :3]).max() <= 1e-3, n
        assert np.array_equal(out[..., 3], hist[..., 3])
    dn = dr.denoise(hist, ad, nc)
    change = np.abs(dn[..., :3] - hist[..., :3]).max(-1)
    print("denoise_ref with the mpt_denoise defaults changes the pixels next to the step by %.3f .. %.3f"
          % (change[:, W // 2 - 1: W // 2 + 1].min(), change[:, W // 2 - 1: W // 2 + 1].max()))
    assert (change[:, W // 2 - 1: W // 2 + 1] > 0.05).all()


def test_the_spatial_estimate_is_calibrated():
    """First frame (n = 1), 49 equal weights, iid Gaussian luminance noise: E[V_0] = sigma^2 (1 - 1/49), the biased sample variance
    of 49 values.  The 5 % covers the sampling error of ~2800 overlapping windows."""
    W, H, sigma = 64, 54, 0.1
    ad, nc = _flat_guides(W, H)
    rng = np.random.default_rng(4)
    c = np.ones((H, W, 4), np.float32)
    c[..., :3] = (1.0 + sigma * rng.standard_normal((H, W)))[..., None]
    u = _cam(W=W, H=H)
    hist, mom, _ = sr.accumulate(c, ad, nc, u)
    v0 = sr.variance(hist, mom, ad, nc, sr.DEFAULTS["sigma_normal"], sr.DEFAULTS["sigma_depth"])
    got = float(v0[3:-3, 3:-3].astype(np.float64).mean())
    want = sigma * sigma * (1.0 - 1.0 / 49.0)
    print("mean V_0 %.6f, expected %.6f (%.2f %% off)" % (got, want, 100 * (got / want - 1)))
    assert abs(got / want - 1.0) <= 0.05


def test_one_level_propagates_a_constant_variance_by_the_squared_kernel():
    """All edge-stopping weights 1: sum w = 1 and sum w^2 = (sum h^2)^2 = (70 / 256)^2."""
    W, H = 40, 30
    ad, nc = _flat_guides(W, H)
    xv = np.empty((H, W, 4), np.float32)
    xv[..., :3] = 0.5
    xv[..., 3] = 0.02
    for i in (0, 1, 2):
        out = sr.level(xv, ad, nc, i, 2.0, 32.0, 0.25)
        m = 2 << i
        inner = out[m:-m, m:-m]
        assert np.abs(inner[..., 3] / (0.02 * (70.0 / 256.0) ** 2) - 1.0).max() <= 1e-5, i
        assert np.abs(inner[..., :3] - 0.5).max() <= 1e-6


def test_feedback_replaces_the_history_of_surfaces_only_and_keeps_n():
    W, H = 24, 20
    u = _cam(W=W, H=H)
    ad, nc = _plane_guides(u, W, H)
    nc[8:12, 8:14, 3] = 1
    rng = np.random.default_rng(5)
    c = rng.random((H, W, 4), np.float32)
    h0, mv0, f0, _ = sr.svgf_image(c, ad, nc, u, iterations=2, feedback=0)
    h1, mv1, f1, _ = sr.svgf_image(c, ad, nc, u, iterations=2, feedback=1)
    x1 = sr.level(np.concatenate([h0[..., :3], mv0[..., 2:3]], -1), ad, nc, 0, *sr.resolve()[1:4])
    surf = nc[..., 3] == 0
    assert np.array_equal(h1[surf][:, :3], x1[surf][:, :3]) and np.array_equal(h1[~surf], h0[~surf])
    assert np.array_equal(h1[..., 3], h0[..., 3]) and np.array_equal(mv0, mv1) and np.array_equal(f0, f1)
    assert np.array_equal(sr.svgf_image(c, ad, nc, u, iterations=0, feedback=1)[0], sr.svgf_image(c, ad, nc, u, iterations=0, feedback=0)[0])


@pytest.mark.parametrize("W,H", [(1, 1), (2, 1), (1, 5), (3, 3)])
def test_images_smaller_than_the_filter_kernels(W, H):
    """Every tap but the centre may be outside: a single surface pixel comes back as X * a with V_0 = 0 (one sample: M2 = M1^2)."""
    u = _cam(W=W, H=H)
    ad, nc = _flat_guides(W, H, albedo=0.5)
    c = np.random.default_rng(6).random((H, W, 4), np.float32)
    hist, mv, out, n_reset = sr.svgf_image(c, ad, nc, u, iterations=3)
    assert n_reset == W * H and np.isfinite(out).all() and np.isfinite(mv).all()
    if W * H == 1:
        assert mv[0, 0, 2] == 0 and np.abs(out[..., :3] - c[..., :3]).max() <= 1e-6


# ---- calibration ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tr.PATHS))
def test_defaults_beat_the_history_and_the_fixed_stop_filter_along_a_camera_path(name):
    sc, buf = oracle_scene(name)
    frames, hi = tr.oracle_path(name, sc, buf)
    f_hist, _, hist = tr.run_path(frames, hi)
    _, c, ad, nc = frames[-1]
    f_dt = tr.mse(c, hi) / tr.mse(dr.denoise(hist, ad, nc), hi)
    f, reset_share, out = sr.run_path(frames, hi)
    print("%s: F_svgf %.3f, F_hist %.3f, F_dt %.3f, %.2f %% of the last frame reset" % (name, f, f_hist, f_dt, 100 * reset_share))
    assert f >= f_hist and f >= f_dt, (name, f, f_hist, f_dt)
    assert reset_share <= MAX_RESET, (name, reset_share)
    assert f == pytest.approx(HELD_F[name], rel=0.01), (name, f)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


@pytest.mark.parametrize("extra,why", [([], "a run without --camera-path"), (["--camera-path", "p.txt", "--temporal"], "--temporal"),
                                       (["--camera-path", "p.txt", "--denoise"], "--denoise"),
                                       (["--camera-path", "p.txt", "--rng", "literal"], "--rng literal"),
                                       (["--camera-path", "p.txt", "--gpus", "2"], "--gpus > 1"),
                                       (["--camera-path", "p.txt", "--checkpoint", "x.sum"], "--checkpoint"),
                                       (["--camera-path", "p.txt", "--resume", "x.sum"], "--resume"),
                                       (["--camera-path", "p.txt", "--temporal-spp", "0"], "--temporal-spp 0")])
def test_cli_refuses_svgf_combinations(extra, why):
    import subprocess
    from conftest import scene_path
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--svgf"] + extra, capture_output=True, text=True)
    assert r.returncode == 2
    assert "--svgf cannot be combined with %s" % why in r.stderr


def test_cli_refuses_svgf_with_adaptive():
    import subprocess
    from conftest import scene_path
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--svgf", "--adaptive", "0.05", "--camera-path", "p.txt"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "cannot be combined with" in r.stderr     # (--adaptive refuses --camera-path first)
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--svgf", "--adaptive", "0.05"], capture_output=True, text=True)
    assert r.returncode == 2 and "--svgf cannot be combined with --adaptive" in r.stderr


@pytest.mark.parametrize("n", ["9", "-1", "100"])
def test_cli_refuses_svgf_iterations_out_of_range(n):
    import subprocess
    from conftest import scene_path
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--svgf", "--camera-path", "p.txt", "--svgf-iterations", n],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--svgf-iterations must be between 0 and 8" in r.stderr


def test_cli_help_describes_svgf():
    import subprocess
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--svgf ", "--svgf-iterations", "--temporal-spp", "--temporal-history"):
        assert flag in r.stdout, flag
