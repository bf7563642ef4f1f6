"""Adaptive sampling without a GPU: properties of the numpy restatement (tests/adaptive_ref.py), the argument checks of the new entry
points (NULL arguments are refused before a context or a device is touched), the ctypes layouts against include/mpt.h, and the
CLI's refusals (they come before any device call)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
from conftest import ROOT, scene_path
from metalpathtracer_amd import capi, host

INVALID = 1
CLI = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def test_zero_variance_gives_zero_error():
    n = 16
    v = np.array([0.5, 0.25, 0.125])
    l = ar.lum64(v)
    s = np.zeros((3, 5, 4))
    s[..., :3] = n * v
    m2 = np.zeros((3, 5, 4))
    m2[..., 3] = n * (l * l)
    assert (ar.pixel_errors(s, m2, n) == 0.0).all()
    assert (ar.tile_errors(s, m2, n) == 0.0).all()


def test_floor_applies_below_it():
    n = 8
    vals = np.array([0.01, 0.03, 0.01, 0.03, 0.01, 0.03, 0.01, 0.03])   # a dim pixel: mean luminance 0.02 < the default floor
    rgb = np.repeat(vals[:, None], 3, axis=1)
    l = ar.lum64(rgb)
    s = np.zeros((1, 1, 4))
    s[0, 0, :3] = rgb.sum(0)
    m2 = np.zeros((1, 1, 4))
    m2[0, 0, 3] = (l * l).sum()
    mean = ar.lum64(s)[0, 0] / n
    var = max(0.0, (m2[0, 0, 3] - ar.lum64(s)[0, 0] * mean) / (n - 1))
    assert mean < ar.DEFAULT_LUMINANCE_FLOOR
    assert np.isclose(ar.pixel_errors(s, m2, n)[0, 0], np.sqrt(var / n) / np.float64(np.float32(0.05)), rtol=1e-12)
    assert np.isclose(ar.pixel_errors(s, m2, n, luminance_floor=0.001)[0, 0], np.sqrt(var / n) / mean, rtol=1e-12)
    # above the floor the mean divides
    s2, m22 = s * 100.0, m2 * 1e4
    assert np.isclose(ar.pixel_errors(s2, m22, n)[0, 0], np.sqrt(var * 1e4 / n) / (mean * 100.0), rtol=1e-9)


@pytest.mark.parametrize("N,m,b,want", [(256, 16, 16, list(range(16, 257, 16))), (100, 16, 32, [16, 48, 80, 100]),
                                        (8, 16, 16, [8]), (20, 0, 0, [16, 20]), (2, 2, 1, [2]), (5, 2, 1, [2, 3, 4, 5])])
def test_schedule(N, m, b, want):
    got = ar.schedule(N, m, b)
    assert got == want
    assert got[-1] == N and all(x < y for x, y in zip(got, got[1:]))


def test_stop_counts_and_tile_max():
    e = np.arange(10 * 12, dtype=np.float64).reshape(10, 12)
    t = ar.tile_max(e)
    assert t.shape == (2, 2) and t[0, 0] == e[7, 7] and t[1, 1] == e[9, 11]
    errs = [np.array([[0.5, 0.05]]), np.array([[0.2, 0.01]]), np.array([[0.09, 0.0]])]
    assert ar.stop_counts(errs, [4, 8, 12], 0.1, 12).tolist() == [[12, 4]]
    assert ar.stop_counts(errs, [4, 8, 12], 0.3, 12).tolist() == [[8, 4]]


def test_null_arguments_refused_without_a_device():
    L = capi.load()
    fake_ctx = C.create_string_buffer(64)          # never dereferenced by the checks below
    p = capi.Context.params(sample_count=8)
    a = capi.AdaptiveParams(4, 4, 0.1, 0.0)
    info = capi.AdaptiveInfo()
    assert L.mpt_render_adaptive(None, C.byref(p), C.byref(a), C.byref(info)) == INVALID
    assert L.mpt_render_adaptive(fake_ctx, None, C.byref(a), C.byref(info)) == INVALID
    assert L.mpt_render_adaptive(fake_ctx, C.byref(p), None, C.byref(info)) == INVALID
    assert L.mpt_render_adaptive(fake_ctx, C.byref(p), C.byref(a), None) == INVALID
    buf = np.zeros(64, np.float32)
    cnt = np.zeros(16, np.uint32)
    assert L.mpt_read_moments(None, buf.ctypes.data_as(C.POINTER(C.c_float))) == INVALID
    assert L.mpt_read_moments(fake_ctx, None) == INVALID
    assert L.mpt_read_tile_samples(None, cnt.ctypes.data_as(C.POINTER(C.c_uint32))) == INVALID
    assert L.mpt_read_tile_samples(fake_ctx, None) == INVALID
    assert not buf.any() and not cnt.any()
    H = host.load()
    assert H.mpt_renderer_render_adaptive(None, 0, 8, C.byref(a), C.byref(info)) == INVALID
    assert H.mpt_renderer_render_adaptive(fake_ctx, 0, 8, None, C.byref(info)) == INVALID
    assert H.mpt_renderer_render_adaptive(fake_ctx, 0, 8, C.byref(a), None) == INVALID
    assert info.samples == 0 and info.passes == 0


_LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "mpt.h"
#define F(T, f) std::printf("%s.%s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
int main() {
    std::printf("mpt_adaptive_params %zu\nmpt_adaptive_info %zu\n", sizeof(mpt_adaptive_params), sizeof(mpt_adaptive_info));
    F(mpt_adaptive_params, min_samples); F(mpt_adaptive_params, batch_samples); F(mpt_adaptive_params, threshold);
    F(mpt_adaptive_params, luminance_floor);
    F(mpt_adaptive_info, samples); F(mpt_adaptive_info, passes); F(mpt_adaptive_info, tiles_converged);
    F(mpt_adaptive_info, tiles_at_max); F(mpt_adaptive_info, _pad);
    std::printf("MPT_FLAG_MOMENTS %u\nMIN %u\nBATCH %u\nFLOOR %.9g\n", (unsigned)MPT_FLAG_MOMENTS, MPT_ADAPTIVE_DEFAULT_MIN_SAMPLES,
                MPT_ADAPTIVE_DEFAULT_BATCH, (double)MPT_ADAPTIVE_DEFAULT_LUMINANCE_FLOOR);
}
"""


def test_ctypes_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(_LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lines = dict(l.split(" ", 1) for l in out.splitlines())
    assert int(lines["mpt_adaptive_params"]) == C.sizeof(capi.AdaptiveParams)
    assert int(lines["mpt_adaptive_info"]) == C.sizeof(capi.AdaptiveInfo)
    for T, name in ((capi.AdaptiveParams, "mpt_adaptive_params"), (capi.AdaptiveInfo, "mpt_adaptive_info")):
        for f, _ in T._fields_:
            off, size = (int(x) for x in lines["%s.%s" % (name, f)].split())
            assert getattr(T, f).offset == off and getattr(T, f).size == size, (name, f)
    assert int(lines["MPT_FLAG_MOMENTS"]) == capi.FLAG_MOMENTS
    assert int(lines["MIN"]) == capi.ADAPTIVE_DEFAULTS["min_samples"] == ar.DEFAULT_MIN_SAMPLES
    assert int(lines["BATCH"]) == capi.ADAPTIVE_DEFAULTS["batch_samples"] == ar.DEFAULT_BATCH
    assert np.float32(float(lines["FLOOR"])) == np.float32(capi.ADAPTIVE_DEFAULTS["luminance_floor"])


def test_expand_tile_counts():
    c = np.array([[1, 2, 3], [4, 5, 6]], np.uint32)
    e = capi.expand_tile_counts(c, 13, 20)
    assert e.shape == (13, 20)
    assert e[0, 0] == 1 and e[7, 15] == 2 and e[8, 16] == 6 and e[12, 19] == 6


@pytest.mark.parametrize("extra,why", [(["--frames", "2"], "--frames"), (["--gpus", "2"], "--gpus > 1"),
                                       (["--rng", "literal"], "--rng literal"), (["--checkpoint", "x.sum"], "--checkpoint"),
                                       (["--resume", "x.sum"], "--resume"), (["--camera-path", "p.txt"], "--camera-path")])
def test_cli_refuses_adaptive_combinations(extra, why):
    r = subprocess.run([CLI, "--scene", scene_path("scene.xml"), "--adaptive", "0.05"] + extra, capture_output=True, text=True)
    assert r.returncode == 2
    assert "--adaptive cannot be combined with %s" % why in r.stderr


def test_cli_help_describes_adaptive():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--adaptive T", "--adaptive-min", "--adaptive-batch", "--adaptive-floor"):
        assert flag in r.stdout, flag
