"""GPU tests of the builders' radix sort (metalpathtracer_amd/csrc/mpt_radix.h) on its own, through tests/radix/radix_harness.hip: the
product's radix_reserve / radix_sort_pairs on device copies of the pairs, against numpy's stable argsort of the sorted bits.  The keys
come back whole (the bits above the sorted range ride along), the values are the permutation itself when they are arange(n) — so a sort
that is not stable fails — and the harness reports a word written behind any of the four pair buffers as an error of its own.

Sizes: both sides of a 64-item step, of a wave's tile of 1024 and of a workgroup of four tiles; the key families are the regimes of the
eight-ballot peer mask (one digit, two, 64 distinct digits in a step, digits 0 and 255) and what the builders sort (depths below 48 in
one pass, the upper halves of material hashes in four)."""
import ctypes as C
import os

import numpy as np
import pytest

import material_cases as mc
from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
LARGE = ((100003, (1, 2, 3, 4)), (1000003, (4,)))
ERR_ARG, ERR_GUARD = -1, -4
_lib = None
_hash_hi = {}


def harness():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "tests", "radix", "_build", "libradixharness.so"))
        up = C.POINTER(C.c_uint32)
        L.radix_harness_sort.argtypes = [up, up, C.c_uint32, C.c_int, up, up, C.POINTER(C.c_int)]
        L.radix_harness_mat_hash.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def sort_pairs(keys, vals, passes):
    keys, vals = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(vals, np.uint32)
    ko, vo = np.full_like(keys, 0x55555555), np.full_like(vals, 0x55555555)
    second = C.c_int(-1)
    rc = harness().radix_harness_sort(_up(keys), _up(vals), keys.size, passes, _up(ko), _up(vo), C.byref(second))
    return rc, ko, vo, second.value


def check(keys, vals, passes, what):
    keys = np.ascontiguousarray(keys, np.uint32)
    mask = np.uint32((1 << (8 * passes)) - 1)
    order = np.argsort(keys & mask, kind="stable")
    rc, ko, vo, second = sort_pairs(keys, vals, passes)
    assert rc != ERR_GUARD, "%s: a word behind a pair buffer was written" % what
    assert rc == 0, "%s: radix_harness_sort returned %d" % (what, rc)
    bad_k, bad_v = int((ko != keys[order]).sum()), int((vo != vals[order]).sum())
    assert bad_k == 0 and bad_v == 0, "%s: %d keys and %d values of %d are not where the stable sort puts them" % (what, bad_k, bad_v, keys.size)
    assert second == passes % 2, what


def hash_hi(m):
    """The upper halves of the hashes of m distinct material rows (what the device build sorts its materials by)."""
    if m not in _hash_hi:
        h = (mc.mat_hash(mc.table(m, 500 + m)) >> np.uint64(32)).astype(np.uint32)
        h.setflags(write=False)
        _hash_hi[m] = h
    return _hash_hi[m]


def _bytes4(d):
    return (d.astype(np.uint32) & np.uint32(255)) * np.uint32(0x01010101)


# name: (keys(n, rng), passes)
FAMILIES = {
    "uniform": (lambda n, rng: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), (1, 2, 3, 4)),
    "all_equal": (lambda n, rng: np.full(n, 0x9E3779B9, np.uint32), (1, 2, 3, 4)),
    "descending": (lambda n, rng: (n - 1 - np.arange(n)).astype(np.uint32), (1, 2, 3, 4)),
    "ascending": (lambda n, rng: np.arange(n, dtype=np.uint32), (1, 2, 3, 4)),
    "two_by_lane": (lambda n, rng: np.where(np.arange(n) & 1, 0x3C5AA5C3, 0xC3A55A3C).astype(np.uint32), (1, 2, 3, 4)),
    "64_digits_a_step": (lambda n, rng: _bytes4(np.arange(n) * 4 + np.arange(n) // 64), (1, 2, 3, 4)),
    "zero_and_ones": (lambda n, rng: np.where(rng.integers(0, 2, n) == 1, 0xFFFFFFFF, 0).astype(np.uint32), (1, 2, 3, 4)),
    "depths": (lambda n, rng: np.minimum(rng.geometric(0.15, n) - 1, 47).astype(np.uint32), (1,)),
    "hashes_of_5": (lambda n, rng: hash_hi(5)[rng.integers(0, 5, n)], (1, 2, 3, 4)),
    "hashes_of_22": (lambda n, rng: hash_hi(22)[rng.integers(0, 22, n)], (1, 2, 3, 4)),
    "hashes_of_5000": (lambda n, rng: hash_hi(5000)[rng.integers(0, 5000, n)], (1, 2, 3, 4)),
}
LARGE_FAMILIES = ("uniform", "64_digits_a_step", "hashes_of_5000")


def test_the_families_are_what_they_claim():
    """(no sort: the inputs themselves)"""
    rng = np.random.default_rng(1)
    k = FAMILIES["64_digits_a_step"][0](8193, rng)
    for b in range(4):
        d = (k >> np.uint32(8 * b)) & np.uint32(255)
        assert all(np.unique(d[s:s + 64]).size == 64 for s in range(0, 8192, 64))
    assert FAMILIES["depths"][0](4097, rng).max() < 48
    for m in (5, 22, 5000):
        assert np.unique(hash_hi(m)).size == m
    a, b = 0x3C5AA5C3, 0xC3A55A3C
    assert all(((a >> s) & 255) != ((b >> s) & 255) for s in (0, 8, 16, 24))


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_sort_is_numpys_stable_sort(family, n):
    make, passes = FAMILIES[family]
    rng = np.random.default_rng(n * 31 + len(family))
    keys = make(n, rng)
    for p in passes:
        check(keys, np.arange(n, dtype=np.uint32), p, "%s n=%d passes=%d" % (family, n, p))


@pytest.mark.parametrize("n", SMALL + (100003,))
def test_values_travel_with_their_keys(n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for p in (1, 4):
        check(keys, vals, p, "random values n=%d passes=%d" % (n, p))


@pytest.mark.parametrize("n,passes", LARGE)
@pytest.mark.parametrize("family", LARGE_FAMILIES)
def test_sort_of_many_tiles(family, n, passes):
    rng = np.random.default_rng(n + len(family))
    keys = FAMILIES[family][0](n, rng)
    for p in passes:
        check(keys, np.arange(n, dtype=np.uint32), p, "%s n=%d passes=%d" % (family, n, p))


def test_what_the_harness_refuses():
    """Nothing is launched for no items or a pass count outside 1..4: the builders never ask for either."""
    one = np.zeros(4, np.uint32)
    out = np.zeros(4, np.uint32)
    second = C.c_int(-1)
    L = harness()
    assert L.radix_harness_sort(_up(one), _up(one), 0, 4, _up(out), _up(out), C.byref(second)) == ERR_ARG
    for p in (0, 5, -1):
        assert L.radix_harness_sort(_up(one), _up(one), 4, p, _up(out), _up(out), C.byref(second)) == ERR_ARG
    assert second.value == -1 and not out.any()
    assert L.radix_harness_mat_hash(None, 0, None) == ERR_ARG


def test_material_hash_is_the_restatement():
    """k_mat_hash against tests/material_cases.py mat_hash over rows of every kind the scenes use."""
    rows = np.concatenate([mc.table(5000, 9), mc.colliding_pair()])
    got = np.zeros(rows.shape[0], np.uint64)
    rc = harness().radix_harness_mat_hash(rows.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], got.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0
    np.testing.assert_array_equal(got, mc.mat_hash(rows))
