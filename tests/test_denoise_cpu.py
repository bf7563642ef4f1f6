"""The denoiser without a GPU: the new C-ABI symbols and their argument checks, properties of the numpy restatement of the filter
(tests/denoise_ref.py), and the calibration of the defaults of include/mpt.h against the oracle (profiles/r06_denoise_sweep.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref as dr
from conftest import CORNELL_CAM, ROOT, oracle_scene
from metalpathtracer_amd import capi, host

NEW_MPT = ("mpt_read_aovs", "mpt_denoise", "mpt_read_denoised", "mpt_denoised_buffer", "mpt_denoise_image")
# calibrated on 128 x 128 oracle renders (4 spp against 1024 spp of another seed, depth 8) with the defaults: Cornell 23.7x,
# scene.xml 9.0x (profiles/r06_denoise_sweep.txt); the bounds keep a third of margin
MIN_FACTOR = {"cornell.xml": 16.0, "scene.xml": 6.0}


def test_denoise_symbols_exported_and_listed():
    L = C.CDLL(capi.LIB_PATH)
    for n in NEW_MPT:
        assert n in capi.SYMBOLS and hasattr(L, n), n
    assert "mpt_renderer_denoise" in host.SYMBOLS and hasattr(host.load(), "mpt_renderer_denoise")


def test_denoise_defaults_agree_with_header():
    text = open(os.path.join(ROOT, "include", "mpt.h")).read()
    for key, macro in (("iterations", "ITERATIONS"), ("sigma_luminance", "SIGMA_LUMINANCE"), ("sigma_normal", "SIGMA_NORMAL"),
                       ("sigma_depth", "SIGMA_DEPTH")):
        line = [l for l in text.splitlines() if l.startswith("#define MPT_DENOISE_DEFAULT_" + macro + " ")][0]
        v = float(line.split()[2].rstrip("f"))
        assert v == capi.DENOISE_DEFAULTS[key] == dr.DEFAULTS[key], key


def test_denoise_null_arguments():
    L = capi.load()
    hl = host.load()
    INVALID = 1
    buf = np.zeros(16, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    p = capi.denoise_params(samples=1)
    assert L.mpt_read_aovs(None, fp, fp, None) == INVALID
    assert L.mpt_denoise(None, C.byref(p)) == INVALID
    assert L.mpt_denoise(None, None) == INVALID
    assert L.mpt_read_denoised(None, fp) == INVALID
    out, n = C.c_void_p(), C.c_uint64()
    assert L.mpt_denoised_buffer(None, C.byref(out), C.byref(n)) == INVALID
    assert L.mpt_denoise_image(None, 2, 2, fp, fp, fp, C.byref(p), fp) == INVALID
    assert hl.mpt_renderer_denoise(None, C.byref(p), fp) == INVALID


def _case(H=24, W=32, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.random((H, W, 4), np.float32)
    ad = np.concatenate([rng.random((H, W, 3), np.float32), rng.random((H, W, 1), np.float32) + np.float32(1)], -1)
    n = rng.normal(size=(H, W, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True).astype(np.float32)
    cls = rng.choice(np.array([0, 0, 0, 1, 2], np.float32), size=(H, W, 1))
    return c, ad, np.concatenate([n, cls], -1).astype(np.float32)


def test_restatement_zero_iterations_is_identity():
    c, ad, nc = _case()
    assert np.array_equal(dr.denoise(c, ad, nc, iterations=0).view(np.uint32), c.view(np.uint32))


def test_restatement_passes_emissive_and_sky_through():
    c, ad, nc = _case(seed=1)
    out = dr.denoise(c, ad, nc, iterations=4)
    keep = nc[..., 3] != 0
    assert keep.any()
    assert np.array_equal(out[keep].view(np.uint32), c[keep].view(np.uint32))
    assert np.array_equal(out[..., 3].view(np.uint32), c[..., 3].view(np.uint32))


def test_restatement_orthogonal_normals_do_not_mix():
    H, W = 16, 20
    c = np.ones((H, W, 4), np.float32)
    c[:, : W // 2, :3] = 0
    ad = np.ones((H, W, 4), np.float32)
    nc = np.zeros((H, W, 4), np.float32)
    nc[:, : W // 2, :3] = (1, 0, 0)
    nc[:, W // 2:, :3] = (0, 1, 0)
    out = dr.denoise(c, ad, nc, iterations=5)
    assert (out[:, : W // 2, :3] == 0).all()
    assert np.allclose(out[:, W // 2:, :3], 1, rtol=0, atol=1e-6)


def test_restatement_constant_irradiance_stays_constant():
    c, ad, nc = _case(seed=2)
    nc[..., 3] = 0
    ad[..., :3] = ad[..., :3] * np.float32(0.9) + np.float32(0.05)   # (above the 1e-3 floor of the demodulation)
    c[..., :3] = np.float32(0.25) * ad[..., :3]           # irradiance 0.25 everywhere
    out = dr.denoise(c, ad, nc, iterations=5)
    irr = out[..., :3] / ad[..., :3]
    assert np.abs(irr - np.float32(0.25)).max() <= 4 * np.spacing(np.float32(0.25))


@pytest.mark.parametrize("name,cam", [("cornell.xml", CORNELL_CAM), ("scene.xml", None)])
def test_defaults_cut_the_error_by_the_calibrated_factor(name, cam):
    from oracle import binding as ob
    sc, buf = oracle_scene(name)
    S = 128
    u = ob.make_uniforms(S, S, sc.prim_count, sc.triangle_count, cam=cam)
    lo, _ = ob.render(u, buf, rng_mode=ob.RNG_PHILOX, max_depth=8, sample_count=4, seed=(1, 0), threads=16)
    hi, _ = ob.render(u, buf, rng_mode=ob.RNG_PHILOX, max_depth=8, sample_count=1024, seed=(7, 0), threads=16)
    lo, hi = lo / np.float32(4), hi / np.float32(1024)
    ad, nc, _ = dr.first_hit_guides(u, buf, ob.first_hit)
    out = dr.denoise(lo, ad, nc)
    m0 = float(((lo[..., :3] - hi[..., :3]).astype(np.float64) ** 2).mean())
    m1 = float(((out[..., :3] - hi[..., :3]).astype(np.float64) ** 2).mean())
    assert m0 / m1 >= MIN_FACTOR[name], (name, m0 / m1)
