"""The short arithmetic forms of the lean wave-local kernels (metalpathtracer_amd/csrc/mpt_device.h) against the compiler's correctly
rounded operations, bit for bit, on the device — through tests/lean_math/lean_math_harness.hip, which includes the product's header.

  sqrt_core(x) == sqrtf(x)                       for every bit pattern x with 2^-96 <= x < inf   (all 2^32 patterns are run)
  rcp_chain(sqrt_core(l2)) == 1.0f / sqrtf(l2)   for every bit pattern l2 in [2^-96, 2^126]      (the lean normalize3's inverse length)
  cdiv_chain(x, W, cdiv_recip(W)) == x / W       for all 2^24 numerators x = k 2^-24 - 0.5 of gen_primary, for every integer W in
                                                 1..1024, the common image sizes up to 2^24 - 1, and 40 fixed pseudo-random integers
  normalize3<true> == normalize3<false>          on 64-lane waves that mix in-range lanes with one lane outside the guard (zero,
                                                 denormal, overflowing l2, NaN, -0), in lane 0 and in lane 63: the wave-uniform branch
                                                 and the slow path behind it

(The guarded form of the two bare square roots, mpt_sqrt, was priced and left out of the product — profiles/r16_lean_math.txt — so there
is nothing of it to test.)

Two NaNs count as the same answer (the harness compares that way, as k_kat_rcp does); the mixed-wave tests compare NaNs by position."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_lib = None


def harness():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "tests", "lean_math", "_build", "libleanmath.so"))
        fp, u64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        L.lean_math_sqrt_all.argtypes = [u64p]
        L.lean_math_inv_len_all.argtypes = [u64p]
        L.lean_math_cdiv.argtypes = [fp, C.c_uint32, u32p]
        L.lean_math_normalize.argtypes = [fp, C.c_uint32, fp, fp]
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _patterns(lo, hi):
    """Number of float bit patterns x with lo <= x <= hi, 0 < lo <= hi (positive floats order as their bits)."""
    b = np.array([lo, hi], np.float32).view(np.uint32)
    return int(b[1]) - int(b[0]) + 1


def test_sqrt_core_is_sqrtf_on_every_operand_of_its_range():
    out = (C.c_uint64 * 4)()
    assert harness().lean_math_sqrt_all(out) == 0
    bad_in, n_in, bad_out, n_out = list(out)
    print("sqrt_core: %d operands in [2^-96, inf), %d differ; outside: %d operands, %d differ (informational)" % (n_in, bad_in, n_out, bad_out))
    assert n_in == _patterns(2.0 ** -96, np.finfo(np.float32).max) and n_in + n_out == 1 << 32
    assert bad_in == 0


def test_lean_inverse_length_is_the_division_by_the_root():
    out = (C.c_uint64 * 4)()
    assert harness().lean_math_inv_len_all(out) == 0
    bad_in, n_in, bad_out, n_out = list(out)
    print("inverse length: %d operands in [2^-96, 2^126], %d differ; outside: %d operands, %d differ (informational)" % (n_in, bad_in, n_out, bad_out))
    assert n_in == _patterns(2.0 ** -96, 2.0 ** 126) and n_in + n_out == 1 << 32
    assert bad_in == 0


def test_constant_division_chain_is_the_division():
    rnd = np.random.RandomState(20241).randint(1, 1 << 24, size=40)
    W = np.concatenate([np.arange(1, 1025), [1080, 1920, 2160, 3840, 4096, 7680, 16384, (1 << 24) - 1], rnd]).astype(np.float32)
    assert W.size == 1024 + 8 + 40
    bad = np.full(W.size, 0xFFFFFFFF, np.uint32)
    assert harness().lean_math_cdiv(_fp(W), W.size, bad.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    wrong = {int(w): int(b) for w, b in zip(W, bad) if b}
    assert not wrong, "W -> numerators of 2^24 whose quotient differs: %s" % wrong


# the lanes that leave the guard's range
ODD_VECTORS = {"zero": (0.0, 0.0, 0.0), "denormal": (1e-40, -3e-41, 2e-45), "below 2^-96": (1e-20, 0.0, 1e-21), "overflow": (1e30, -1e30, 1e30),
               "nan": (np.nan, 1.0, 2.0), "minus zero": (-0.0, -0.0, -0.0), "inf": (np.inf, 1.0, 0.0)}


def _same(a, b):
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def test_mixed_waves_normalize():
    rs = np.random.RandomState(7)
    base = (rs.uniform(-1, 1, (64, 3)) * 10.0 ** rs.uniform(-6, 6, (64, 1))).astype(np.float32)
    waves, names = [base.copy()], ["all in range"]
    for name, v in ODD_VECTORS.items():
        for lane in (0, 63):
            w = base.copy()
            w[lane] = v
            waves.append(w)
            names.append("%s in lane %d" % (name, lane))
    waves.append(np.tile(np.array(list(ODD_VECTORS.values()), np.float32), (10, 1))[:64])   # every lane outside
    names.append("all odd")
    xyz = np.ascontiguousarray(np.stack(waves), np.float32)
    lean, ref = np.full_like(xyz, 7.0), np.full_like(xyz, 9.0)
    with np.errstate(all="ignore"):
        assert harness().lean_math_normalize(_fp(xyz), len(waves), _fp(lean), _fp(ref)) == 0
    for k, name in enumerate(names):
        assert _same(lean[k], ref[k]), "%s: lanes %s differ" % (name, np.nonzero((lean[k].view(np.uint32) != ref[k].view(np.uint32)).any(-1))[0].tolist())
    assert np.isfinite(ref[0]).all() and abs(np.linalg.norm(ref[0].astype(np.float64), axis=1) - 1).max() < 1e-6   # (the harness did normalize)
