"""Temporal accumulation without a GPU: the new C-ABI symbols, their structs and argument checks, properties of the numpy
restatement (tests/temporal_ref.py), and the calibration of the defaults of include/mpt.h along three camera paths against the oracle
(profiles/r07_temporal_sweep.txt)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_ref as tr
from conftest import ROOT, oracle_scene
from metalpathtracer_amd import capi, host

F = np.float32
NEW_MPT = ("mpt_temporal_accumulate", "mpt_read_temporal", "mpt_temporal_buffer", "mpt_temporal_reset", "mpt_denoise_temporal",
           "mpt_temporal_image")
NEW_HOST = ("mpt_renderer_draw_temporal", "mpt_renderer_read_temporal", "mpt_renderer_denoise_temporal")
# F = MSE(last 1-spp frame) / MSE(last history) of the restatement with the defaults, 24 frames against 1024 spp
# (profiles/r07_temporal_sweep.txt, the row of the defaults).  The conditions of the calibration: F >= 5, at most 5 % of the last
# frame reset.  tests/test_gpu_temporal.py asks the device for 0.9 x these.
HELD_F = {"cornell.xml": 29.77, "scene.xml": 26.22, "bunny20.xml": 14.78}
MIN_F = 5.0
MAX_RESET = 0.05


def test_temporal_symbols_exported_declared_and_listed():
    L = C.CDLL(capi.LIB_PATH)
    hl = host.load()
    mpt_h = open(os.path.join(ROOT, "include", "mpt.h")).read()
    host_h = open(os.path.join(ROOT, "include", "mpt_host.h")).read()
    for n in NEW_MPT:
        assert n in capi.SYMBOLS and hasattr(L, n) and re.search(r"\bint %s\(" % n, mpt_h), n
    for n in NEW_HOST:
        assert n in host.SYMBOLS and hasattr(hl, n) and re.search(r"\bint %s\(" % n, host_h), n


def test_temporal_struct_layout():
    P, I = capi.TemporalParams, capi.TemporalInfo
    assert C.sizeof(P) == 24 and C.sizeof(I) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("source", 0), ("samples", 4), ("max_history", 8), ("depth_tolerance", 12),
                                                                  ("normal_threshold", 16), ("min_weight", 20)]
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [("pixels_reprojected", 0), ("pixels_reset", 8)]
    text = open(os.path.join(ROOT, "include", "mpt.h")).read()
    body = re.search(r"typedef struct mpt_temporal_params \{(.*?)\} mpt_temporal_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", "source"), ("uint32_t", "samples"), ("uint32_t", "max_history"),
                                                   ("float", "depth_tolerance"), ("float", "normal_threshold"), ("float", "min_weight")]


def test_temporal_defaults_agree_with_header():
    text = open(os.path.join(ROOT, "include", "mpt.h")).read()
    for key in ("max_history", "depth_tolerance", "normal_threshold", "min_weight"):
        line = [l for l in text.splitlines() if l.startswith("#define MPT_TEMPORAL_DEFAULT_" + key.upper() + " ")][0]
        v = float(line.split()[2].rstrip("fu"))
        assert v == capi.TEMPORAL_DEFAULTS[key] == tr.DEFAULTS[key], key


def test_temporal_null_arguments():
    L = capi.load()
    hl = host.load()
    INVALID = 1
    buf = np.zeros(16, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    p = capi.temporal_params(samples=1)
    dp = capi.denoise_params(samples=1)
    u = capi.Uniforms()
    info = capi.TemporalInfo()
    assert L.mpt_temporal_accumulate(None, C.byref(p), C.byref(info)) == INVALID
    assert L.mpt_temporal_accumulate(None, None, None) == INVALID
    assert L.mpt_read_temporal(None, fp) == INVALID
    out, n = C.c_void_p(), C.c_uint64()
    assert L.mpt_temporal_buffer(None, C.byref(out), C.byref(n)) == INVALID
    assert L.mpt_temporal_reset(None) == INVALID
    assert L.mpt_denoise_temporal(None, C.byref(dp)) == INVALID
    assert L.mpt_denoise_temporal(None, None) == INVALID
    assert L.mpt_temporal_image(None, 2, 2, fp, fp, fp, C.byref(u), fp, fp, fp, C.byref(u), C.byref(p), fp, C.byref(info)) == INVALID
    assert hl.mpt_renderer_draw_temporal(None, 1, C.byref(p), C.byref(info)) == INVALID
    assert hl.mpt_renderer_read_temporal(None, fp) == INVALID
    assert hl.mpt_renderer_denoise_temporal(None, C.byref(dp), fp) == INVALID


# ---- properties of the restatement ----------------------------------------------------------------------------------------------
def _cam(pos=(0.0, 0.0, 0.0), fwd=(0.0, 0.0, -1.0), W=64, H=48, vfov=40.0):
    from oracle import binding as ob
    return ob.make_uniforms(W, H, 1, 0, cam=dict(pos=pos, fwd=fwd, up=(0.0, 1.0, 0.0), vfov=vfov))


def _directions(u, W, H):
    """Pixel-centre directions (float64 is enough for building test geometry)."""
    k = tr.camera_key(u).astype(np.float64)
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    dv = k[9:12] + ((px + 0.5) / W)[..., None] * k[3:6] + ((py + 0.5) / H)[..., None] * k[6:9] - k[0:3]
    return dv / np.linalg.norm(dv, axis=-1, keepdims=True)


def _plane_guides(u, W, H, depth=5.0, normal=(0.0, 0.0, 1.0)):
    """Guides of the plane z = -depth seen from camera u (which looks down -z from z = 0)."""
    d = _directions(u, W, H)
    t = depth / -d[..., 2]
    ad = np.concatenate([np.full((H, W, 3), 0.5), t[..., None]], -1).astype(np.float32)
    nc = np.zeros((H, W, 4), np.float32)
    nc[..., :3] = normal
    return ad, nc


def _miss_guides(W, H):
    ad = np.zeros((H, W, 4), np.float32)
    ad[..., 3] = np.inf
    nc = np.zeros((H, W, 4), np.float32)
    nc[..., 3] = 2
    return ad, nc


def test_same_camera_is_the_running_mean():
    W, H = 16, 12
    u = _cam(W=W, H=H)
    ad, nc = _plane_guides(u, W, H)
    nc[:3, :, 3] = 2   # some sky, some light: the same-camera rule makes no test
    nc[3:5, :, 3] = 1
    rng = np.random.default_rng(0)
    for maxh in (4, 32):
        hist, cs = None, []
        for k in range(1, 9):
            c = rng.random((H, W, 4), np.float32)
            cs.append(c)
            if hist is None:
                hist, n_reset = tr.accumulate(c, ad, nc, u, max_history=maxh)
                assert n_reset == W * H
            else:
                hist, n_reset = tr.accumulate(c, ad, nc, u, hist, ad, nc, u, max_history=maxh)
                assert n_reset == 0
            assert (hist[..., 3] == min(k, maxh)).all()
            if k <= maxh:
                assert np.abs(hist[..., :3] - np.mean(cs, axis=0, dtype=np.float64)[..., :3]).max() <= 1e-6


def test_camera_turned_round_resets_every_pixel():
    W, H = 32, 24
    u0, u1 = _cam(W=W, H=H), _cam(fwd=(0.0, 0.0, 1.0), W=W, H=H)
    ad, nc = _plane_guides(u0, W, H)
    rng = np.random.default_rng(1)
    c, hist = rng.random((H, W, 4), np.float32), rng.random((H, W, 4), np.float32) + F(1)
    out, n_reset = tr.accumulate(c, ad, nc, u1, hist, ad, nc, u0)
    assert n_reset == W * H and (out[..., 3] == 1).all()
    assert np.array_equal(out[..., :3].view(np.uint32), c[..., :3].view(np.uint32))


def test_sideways_translation_reproduces_a_linear_history():
    """A fronto-parallel plane, a history linear in the pixel coordinates, the camera moved sideways: bilinear taps return the
    linear function at the reprojected place; the strip that was outside the old image is reset."""
    W, H, depth = 64, 48, 5.0
    u0 = _cam(W=W, H=H)
    k0 = tr.camera_key(u0).astype(np.float64)
    shift = 5.3 * np.linalg.norm(k0[3:6]) * depth / W           # 5.3 pixels at the plane's depth (|first - cam| along z is 1)
    u1 = _cam(pos=(shift, 0.0, 0.0), W=W, H=H)
    ad0, nc0 = _plane_guides(u0, W, H, depth)
    ad1, nc1 = _plane_guides(u1, W, H, depth)
    px, py = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    lin = lambda x, y: 0.25 + 0.01 * x + 0.005 * y              # range over the image: 0.25 .. 1.12
    hist = np.zeros((H, W, 4), np.float32)
    hist[..., :3] = lin(px, py)[..., None]
    hist[..., 3] = 1
    c = np.zeros((H, W, 4), np.float32)
    out, n_reset = tr.accumulate(c, ad1, nc1, u1, hist, ad0, nc0, u0)
    fx = px + 5.3                                               # where pixel p of the new frame was in the old one
    full = fx <= W - 1
    gone = fx >= W
    assert gone.any() and full.any()
    assert (out[gone][:, 3] == 1).all() and n_reset == int(gone.sum())
    assert (out[full][:, 3] == 2).all()
    rng_ = lin(W - 1, H - 1) - lin(0, 0)
    # c = 0 and n = 2: out = h + (0 - h) / 2 = h / 2
    assert np.abs(2.0 * out[full][:, 0] - lin(fx, py)[full]).max() <= 1e-3 * rng_


def _half_and_half(mutate):
    """The still plane seen by a camera moved by a third of a pixel; the history's right half is made foreign by `mutate(ad0, nc0,
    right)` and holds 100 where the left half holds 1.  Returns the new history."""
    W, H, depth = 32, 16, 5.0
    u0 = _cam(W=W, H=H)
    k0 = tr.camera_key(u0).astype(np.float64)
    u1 = _cam(pos=(0.3 * np.linalg.norm(k0[3:6]) * depth / W, 0.0, 0.0), W=W, H=H)
    ad0, nc0 = _plane_guides(u0, W, H, depth)
    ad1, nc1 = _plane_guides(u1, W, H, depth)
    right = np.zeros((H, W), bool)
    right[:, W // 2:] = True
    ad0, nc0, ad1, nc1 = mutate(ad0, nc0, ad1, nc1, right)
    hist = np.ones((H, W, 4), np.float32)
    hist[right, :3] = 100
    c = np.ones((H, W, 4), np.float32)
    out, _ = tr.accumulate(c, ad1, nc1, u1, hist, ad0, nc0, u0)
    return out, right


def test_a_tap_across_a_depth_step_never_contributes():
    def mutate(ad0, nc0, ad1, nc1, right):
        ad0[right, 3] *= F(1.0 + 2 * tr.DEFAULTS["depth_tolerance"])
        return ad0, nc0, ad1, nc1
    out, right = _half_and_half(mutate)
    assert out[..., :3].max() <= 1.0 + 1e-6
    assert (out[:, : out.shape[1] // 2 - 1, 3] == 2).all() and (out[:, out.shape[1] // 2:, 3] == 1).all()


def test_a_tap_across_a_right_angle_crease_never_contributes():
    def mutate(ad0, nc0, ad1, nc1, right):
        nc0[right, :3] = (1.0, 0.0, 0.0)
        return ad0, nc0, ad1, nc1
    out, right = _half_and_half(mutate)
    assert out[..., :3].max() <= 1.0 + 1e-6
    assert (out[:, out.shape[1] // 2:, 3] == 1).all()


def test_a_miss_takes_history_only_from_misses_and_a_hit_only_from_hits():
    def to_sky(ad0, nc0, ad1, nc1, right):     # the frame is all sky; the history's right half was a surface
        H, W = right.shape
        ad1, nc1 = _miss_guides(W, H)
        m_ad, m_nc = _miss_guides(W, H)
        ad0[~right], nc0[~right] = m_ad[~right], m_nc[~right]
        return ad0, nc0, ad1, nc1
    out, right = _half_and_half(to_sky)
    assert out[..., :3].max() <= 1.0 + 1e-6
    assert (out[:, : out.shape[1] // 2 - 1, 3] == 2).all() and (out[:, out.shape[1] // 2:, 3] == 1).all()

    def from_sky(ad0, nc0, ad1, nc1, right):   # the frame is all surface; the history's right half was sky
        H, W = right.shape
        m_ad, m_nc = _miss_guides(W, H)
        ad0[right], nc0[right] = m_ad[right], m_nc[right]
        return ad0, nc0, ad1, nc1
    out, right = _half_and_half(from_sky)
    assert out[..., :3].max() <= 1.0 + 1e-6
    assert (out[:, out.shape[1] // 2:, 3] == 1).all()


# ---- calibration ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tr.PATHS))
def test_defaults_cut_the_error_along_a_camera_path(name):
    sc, buf = oracle_scene(name)
    frames, hi = tr.oracle_path(name, sc, buf)
    f, reset_share, hist = tr.run_path(frames, hi)
    print("%s: F %.3f, %.2f %% of the last frame reset, mean history length %.1f" % (name, f, 100 * reset_share, hist[..., 3].mean()))
    assert f >= MIN_F and reset_share <= MAX_RESET, (name, f, reset_share)
    assert f == pytest.approx(HELD_F[name], rel=0.01), (name, f)


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


@pytest.mark.parametrize("extra,why", [([], "a run without --camera-path"), (["--camera-path", "p.txt", "--rng", "literal"], "--rng literal"),
                                       (["--camera-path", "p.txt", "--gpus", "2"], "--gpus > 1"),
                                       (["--camera-path", "p.txt", "--checkpoint", "x.sum"], "--checkpoint"),
                                       (["--camera-path", "p.txt", "--resume", "x.sum"], "--resume"),
                                       (["--camera-path", "p.txt", "--temporal-spp", "0"], "--temporal-spp 0")])
def test_cli_refuses_temporal_combinations(extra, why):
    import subprocess
    from conftest import scene_path
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--temporal"] + extra, capture_output=True, text=True)
    assert r.returncode == 2
    assert "--temporal cannot be combined with %s" % why in r.stderr


def test_cli_refuses_temporal_with_adaptive():
    import subprocess
    from conftest import scene_path
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--temporal", "--adaptive", "0.05", "--camera-path", "p.txt"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "cannot be combined with" in r.stderr     # (--adaptive refuses --camera-path first)


def test_cli_help_describes_temporal():
    import subprocess
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--temporal ", "--temporal-history", "--temporal-spp"):
        assert flag in r.stdout, flag
