"""The display stage's contract without a GPU (include/mpt.h, "display"): the committed threshold tables, the histogram's bin edges, the
exposure's behaviour under scaling, the tone curves, and continuity with the bytes mpt_write_ppm writes today.  The numpy restatement
(tests/display_ref.py) is what test_gpu_display.py holds the device to, bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import display_ref as dr
from conftest import ROOT

F = np.float32
TRANSFERS = (dr.SRGB, dr.GAMMA22, dr.LINEAR)


def _tool():
    spec = importlib.util.spec_from_file_location("make_display_table", os.path.join(ROOT, "tools", "make_display_table.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ulps(a, b):
    """Distance in float32 steps between positive floats."""
    return np.abs(np.ascontiguousarray(a, F).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, F).view(np.int32).astype(np.int64))


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_tables_increase_and_stay_below_one(transfer):
    T = dr.table(transfer)
    assert T.dtype == np.float32 and T.shape == (255,)
    assert T[0] > 0 and np.all(np.diff(T) > 0) and T[254] < 1


@pytest.mark.parametrize("transfer", TRANSFERS)
def test_tables_are_the_tools_float64_values_rounded(transfer):
    tool = _tool()
    want = tool.table64(transfer).astype(np.float32)
    assert _ulps(dr.table(transfer), want).max() <= 1
    # what the thresholds mean: T[k] is where round(255 f(y)) steps from k - 1 to k, so f^-1(k / 255) lies between T[k] and T[k + 1]
    mid = tool.inverse(transfer, np.arange(1, 255) / 255.0)
    T = dr.table(transfer).astype(np.float64)
    assert np.all(T[:-1] < mid) and np.all(mid < T[1:])


def test_table_arguments():
    import ctypes as C
    from metalpathtracer_amd import capi
    L = capi.load()
    out = (C.c_float * 255)()
    assert L.mpt_display_table(3, out) == 1 and L.mpt_display_table(-1, out) == 1 and L.mpt_display_table(0, None) == 1


def test_bin_edges():
    b = np.arange(256)
    E = dr.bin_edge(b)
    assert E[0] == F(2.0) ** -32 and E[128] == 1 and E[4] == F(2.0) ** -31
    assert np.array_equal(dr.bin_of(E), b)
    below = np.nextafter(E, F(0))
    assert np.array_equal(dr.bin_of(below)[1:], b[:-1])
    assert dr.bin_of(below[:1])[0] == 0                                       # smaller values fall in bin 0 ...
    assert dr.bin_of(np.array([2.0 ** 32, 3e38], F)).tolist() == [255, 255]   # ... larger ones in bin 255
    # zero, negative, NaN and inf are not counted; a denormal is
    c = np.zeros((1, 6, 3), F)
    c[0, :, 1] = [0.0, -1.0, np.nan, np.inf, 1e-42, 0.5]
    h = dr.histogram(c)
    assert h.sum() == 2 and h[0] == 1 and h[dr.bin_of(dr.lum(c[0, 5:6]))[0]] == 1


@pytest.mark.parametrize("j", [-5, 3, 7])
@pytest.mark.parametrize("percentile", [1, 50, 100])
def test_scaling_the_image_shifts_the_key_bin(j, percentile):
    rng = np.random.default_rng(5)
    c = np.exp2(rng.uniform(-10, 10, (32, 48, 3))).astype(F)
    _, h0, i0, _ = dr.display(c, auto_exposure=True, percentile=percentile)
    _, h1, i1, _ = dr.display(c * F(2.0 ** j), auto_exposure=True, percentile=percentile)
    assert i0["pixels_counted"] == i1["pixels_counted"] == 32 * 48
    assert i1["key_bin"] == i0["key_bin"] + 4 * j
    assert np.array_equal(np.roll(h0, 4 * j), h1)
    assert i1["auto_scale"] == i0["auto_scale"] / F(2.0 ** j) and i1["auto_scale"] * F(2.0 ** j) == i0["auto_scale"]   # exactly


def test_exposure_corners():
    h = np.zeros(256, np.uint32)
    assert dr.exposure(h) == (F(1), dr.NO_BIN)
    h[[10, 200]] = [99, 1]
    assert dr.exposure(h, percentile=99)[1] == 10 and dr.exposure(h, percentile=100)[1] == 200 and dr.exposure(h, percentile=1)[1] == 10
    a, kb = dr.exposure(h, percentile=100, key=0.5)
    assert a == F(0.5) / dr.bin_edge(200)
    s, _ = dr.exposure(h, percentile=100, key=0.5, adaptation=0.25, prev=F(8))
    assert s == F(F(8) + F(F(a - F(8)) * F(0.25)))
    for adaptation in (0.0, 1.0, -1.0, 2.0):                                   # outside (0, 1): no smoothing
        assert dr.exposure(h, percentile=100, key=0.5, adaptation=adaptation, prev=F(8))[0] == a


@pytest.mark.parametrize("tone", [dr.CLAMP, dr.REINHARD, dr.ACES])
def test_curves_are_monotone_and_clipping_is_y_at_least_one(tone):
    x = np.exp2(np.linspace(-30, 20, 4001)).astype(F)
    for white in (0.0, 1.5, 16.0):
        y = dr.curve(x, F(1), tone, white)
        assert y.dtype == np.float32 and y[0] >= 0
        # Monotone as displayed, that is after step C's y = min(y, 1), and strictly speaking everywhere below 1.  Above 1 the ACES fit
        # flattens towards 2.51 / 2.43 = 1.033 and the float32 roundings of its numerator and denominator move y by an ulp or three
        # either way (x > 180, y > 1.03 on this grid): all of that is clipped and encodes as 255.
        shown = np.minimum(y, F(1)).astype(np.float64)
        assert np.all(np.diff(shown) >= 0)
        falls = np.flatnonzero(np.diff(y.astype(np.float64)) < 0)
        assert np.all(y[falls + 1] >= 1) and (tone == dr.ACES or falls.size == 0)
        for transfer in TRANSFERS:
            assert np.all(np.diff(dr.encode(np.minimum(y, F(1)), transfer).astype(int)) >= 0)
        c = np.stack([x, np.zeros_like(x), np.zeros_like(x)], -1)[None]
        out, _, info, _ = dr.display(c, tone=tone, white=white)
        assert info["pixels_clipped"] == int((y >= 1).sum())
        assert np.all(out[0, y >= 1, 0] == 255) and np.all(out[..., 3] == 255)
    special = np.array([0.0, -1.0, np.nan, -np.inf, np.inf, 1e-42, 65504.0, 1e30], F)
    y = dr.curve(special, F(1), tone)
    assert np.all(y[:4] == 0) and np.all(np.isfinite(y)) and y[4] == y[6] == y[7]
    # CLAMP clips from exactly 1
    c = np.zeros((1, 2, 3), F)
    c[0, :, 2] = [np.nextafter(F(1), F(0)), 1.0]
    assert dr.display(c)[2]["pixels_clipped"] == 1


def _near_thresholds():
    """Every threshold of GAMMA22 and its neighbours up to four float steps away: 255 * 9 values as a 51 x 45 image."""
    T = dr.table(dr.GAMMA22).view(np.int32)
    v = (T[:, None] + np.arange(-4, 5, dtype=np.int32)[None, :]).astype(np.int32).view(F)
    return np.repeat(v.reshape(45, 51, 1), 4, axis=2)


@pytest.mark.parametrize("which", ["random", "near-thresholds"])
def test_continuity_with_mpt_write_ppm(tmp_path, which):
    """CLAMP + GAMMA22 + exposure 1 is today's mpt_write_ppm (clamp, pow(v, 1 / 2.2) * 255 + 0.5, truncated) made exact: a byte differs
    by at most 1, and only where the value sits within 4 float steps of a threshold — where the float pow falls on the other side.
    The random image is the case to pass; the second one puts values where the two can differ at all."""
    from metalpathtracer_amd import host
    rng = np.random.default_rng(11)
    img = np.exp2(rng.uniform(-14, 1, (128, 128, 4))).astype(F) if which == "random" else _near_thresholds()
    H, W = img.shape[:2]
    path = str(tmp_path / "today.ppm")
    assert host.write_ppm(path, img, scale=1.0, gamma=2.2) == 0
    raw = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 3
    today = np.frombuffer(raw[len(head):], np.uint8).reshape(H, W, 3).astype(int)
    ours = dr.display(img, tone=dr.CLAMP, transfer=dr.GAMMA22, exposure_=1.0)[0][..., :3].astype(int)
    differ = today != ours
    print("bytes that differ: %d of %d" % (differ.sum(), differ.size))
    assert np.abs(today - ours).max() <= 1
    T = dr.table(dr.GAMMA22)
    v = img[..., :3][differ]
    k = np.maximum(today, ours)[differ]                    # the threshold between the two codes is T[k]
    dist = _ulps(v, T[k - 1])
    print("largest distance from the threshold, in float steps: %d" % (dist.max() if dist.size else 0))
    assert np.all(dist <= 4)
    # the finished bytes go to a file unchanged
    out8 = dr.display(img, tone=dr.CLAMP, transfer=dr.GAMMA22)[0]
    p8 = str(tmp_path / "ours.ppm")
    assert host.write_ppm8(p8, out8) == 0
    assert open(p8, "rb").read() == head + out8[..., :3].tobytes()
