"""The tail guard of the lean wave-local kernels implies the box test it elides, on the device (tests/lean_tail/lean_tail_harness.hip,
built like tests/lean_entry/).

One kernel evaluates, for every (origin, direction, best_t) sample, the guard as closest_hit_resume evaluates it behind its
loop — lean_tail_terms of the tree, origin inside [tlo, thi], |d| <= 2 on every axis, no NaN in d — and the product's own box-trip
expression on T's planes (slab_hit, mpt_device.h) with the reciprocals of mpt_rcp3.  A wave whose 64 directions are all inside the
range of the reciprocal chain takes the chain, any other the IEEE division: waves of ordinary directions and waves with zeros, -0,
denormals and tiny components are both among the samples, so both paths occur.  The tree is the three-node tree of a scene with hoisted
spheres: the root, one leaf record for the rest, T.  Asserted for every box: 0 samples with the guard true and the box test answering
miss, 0 with a far minimum <= 0.0001f; at least 40 % of the samples have the guard true.  Boxes: scene.xml's sphere leaf [-1e4, 1e4] x
[-2e4, 140] x [-1e4, 1e4], the unit cube around the origin, and a box 2^-4 thick away from the origin.  2^18 samples per box."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

M = np.float32(2.0 ** -10)
BOXES = {"scene.xml": ((-1e4, -2e4, -1e4), (1e4, 140.0, 1e4)), "unit": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "thin": ((5.0, -3.0, 100.0), (5.0625, 7.0, 1000.0))}
N = 1 << 18
HOLD = 0x80000000


def _lib():
    return C.CDLL(os.path.join(ROOT, "tests", "lean_tail", "_build", "libleantail.so"))


def _tree(lo, hi):
    """root (hit -> 1, miss -> end), node 1 a leaf record (miss -> 2), node 2 = T: three primitives from 0, miss -> end."""
    nodes = np.zeros((3, 8), np.float32)
    w = nodes.view(np.uint32)
    nodes[0, 0:3], nodes[0, 4:7] = (-3e4, -3e4, -3e4), (3e4, 3e4, 3e4)
    w[0, 3], w[0, 7] = 1, 3
    nodes[1, 0:3], nodes[1, 4:7] = (-8.0, 0.0, -9.0), (9.0, 17.0, 6.0)
    w[1, 3], w[1, 7] = HOLD | (3 << 4) | 1, 2
    nodes[2, 0:3], nodes[2, 4:7] = lo, hi
    w[2, 3], w[2, 7] = HOLD | 2, 3
    return nodes


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
    o[where == 8] = np.where(face == 0, lo, hi).astype(np.float32)[where == 8]                # ... on T's faces ...
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
def test_tail_guard_implies_the_box_test_of_the_tail_leaf(name):
    L = _lib()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.lean_tail_implication.argtypes = [fp, C.c_uint32, fp, fp, fp, C.c_uint32, up]
    lo, hi = BOXES[name]
    nodes = _tree(lo, hi)
    o, d, best_t = _samples(lo, hi, 13)
    flags = np.full(N + 1, 0xFFFFFFFF, np.uint32)
    p = lambda a: a.ctypes.data_as(fp)
    assert L.lean_tail_implication(p(nodes), 3, p(o), p(d), p(best_t), N, flags.ctypes.data_as(up)) == 0
    assert flags[N] == 2, "lean_tail_terms did not find T"
    flags = flags[:N]
    assert (flags < 8).all()
    certain, hit, far_ok = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0
    print("%s: %d samples, guard true for %d (%.1f %%), box hit for %d; guard and miss: %d, guard and far term <= 0.0001: %d"
          % (name, N, certain.sum(), 100.0 * certain.mean(), hit.sum(), (certain & ~hit).sum(), (certain & ~far_ok).sum()))
    assert certain.mean() >= 0.4
    assert (certain & ~hit).sum() == 0 and (certain & ~far_ok).sum() == 0
    assert (~certain).sum() > N // 10 and (~hit).any()                 # (and the samples do include rays that miss T's box)

