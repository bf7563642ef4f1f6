"""The entry guard of the lean wave-local kernels implies the box trip it elides, on the device (tests/lean_entry/lean_entry_harness.hip,
built like tests/lean_math/).

One kernel evaluates, for every (origin, direction, best_t) sample, the guard as wavelocal_body evaluates it — lean_entry_terms of node
0, origin inside [ilo, ihi], |d| <= 2 on every axis, no NaN in d — and the product's own box-trip expression on node 0 (slab_hit,
mpt_device.h) with the reciprocals of mpt_rcp3.  A wave whose 64 directions are all inside the range of
the reciprocal chain takes the chain, any other the IEEE division: waves of ordinary directions and waves with zeros, -0, denormals and
tiny components are both among the samples, so both paths occur.

Asserted for every box: the guard implies hit, and the minimum of the far terms of a skipped sample exceeds 0.0001f; at least 40 % of the
samples have the guard true.  Boxes: scene.xml's [-1e4, 1e4] x
[-2e4, 60] x [-1e4, 1e4], the unit cube around the origin, and a box 2^-4 thick away from the origin.  2^18 samples per box."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

M = np.float32(2.0 ** -10)
BOXES = {"scene.xml": ((-1e4, -2e4, -1e4), (1e4, 60.0, 1e4)), "unit": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "thin": ((5.0, -3.0, 100.0), (5.0625, 7.0, 1000.0))}
N = 1 << 18


def _samples(lo, hi, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ilo, ihi = lo + np.float32(2) * M, hi - np.float32(2) * M
    o = rng.uniform(ilo, ihi, (N, 3)).astype(np.float32).clip(ilo, ihi)                       # inside the shrunk box ...
    where = rng.integers(0, 10, N)
    face = rng.integers(0, 3, (N, 3))
    on_face = np.where(face == 0, ilo, np.where(face == 1, ihi, o)).astype(np.float32)
    o[where == 6] = on_face[where == 6]                                                       # ... on its faces ...
    between = np.where(face == 0, rng.uniform(lo, ilo, (N, 3)), rng.uniform(ihi, hi, (N, 3))).astype(np.float32)
    o[where == 7] = between[where == 7]                                                       # ... between the two boxes ...
    o[where == 8] = np.where(face == 0, lo, hi).astype(np.float32)[where == 8]                # ... on the root's faces ...
    around = rng.uniform(lo - 1, hi + 1, (N, 3)).astype(np.float32)
    o[where == 9] = around[where == 9]                                                        # ... and around it
    d = rng.normal(size=(N, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)                           # unit vectors: whole waves take the reciprocal chain
    odd = np.array([0.0, -0.0, 1e-40, -3e-41, 1e-30, -1e-30, 2.0, -2.0, np.nextafter(np.float32(2), np.float32(3)), np.inf, 1.0, -0.5], np.float32)
    pick = rng.integers(0, odd.size, (N, 3))
    special = (np.arange(N) // 64) % 2 == 1                                                   # every other wave: special components in a third of its slots
    use = special[:, None] & (rng.integers(0, 3, (N, 3)) == 0)
    d = np.where(use, odd[pick], d).astype(np.float32)
    best_t = np.where(rng.integers(0, 2, N) == 0, np.float32(np.inf), np.nextafter(np.float32(0.0001), np.float32(1)) * (1 + 3 * rng.random(N))).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(best_t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BOXES))
def test_entry_guard_implies_the_root_box_trip(name):
    L = C.CDLL(os.path.join(ROOT, "tests", "lean_entry", "_build", "libleanentry.so"))
    fp = C.POINTER(C.c_float)
    L.lean_entry_implication.argtypes = [fp, C.c_uint32, fp, fp, fp, C.c_uint32, C.POINTER(C.c_uint32)]
    lo, hi = BOXES[name]
    node0 = np.zeros(8, np.float32)
    node0[0:3], node0[4:7] = lo, hi
    node0.view(np.uint32)[3], node0.view(np.uint32)[7] = 1, 3          # A0 = 1, B0 = n_nodes = 3
    o, d, best_t = _samples(lo, hi, 11)
    flags = np.full(N, 0xFFFFFFFF, np.uint32)
    p = lambda a: a.ctypes.data_as(fp)
    assert L.lean_entry_implication(p(node0), 3, p(o), p(d), p(best_t), N, flags.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert (flags < 8).all()
    skip, hit, far_ok = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0
    print("%s: %d samples, guard true for %d (%.1f %%), box hit for %d; guard and miss: %d, guard and far term <= 0.0001: %d"
          % (name, N, skip.sum(), 100.0 * skip.mean(), hit.sum(), (skip & ~hit).sum(), (skip & ~far_ok).sum()))
    assert skip.mean() >= 0.4
    assert not (skip & ~hit).any() and not (skip & ~far_ok).any()
    assert (~skip).sum() > N // 10 and (~hit).any()                    # (and the samples do include rays that miss the root)
