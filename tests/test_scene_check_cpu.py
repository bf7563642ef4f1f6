"""Proof on the CPU that tests/scene_check.py notices: it passes on layout_scene's arrays (the dump mode of
tests/scene_layout/scene_layout_check.cpp; refbox, which the device makes, derived from its rule) for the four asset scenes and three
hand-made trees, and every single mutation of a passing layout trips the invariant it names.  What a passing
tests/test_gpu_scene_arrays.py means rests on this."""
import numpy as np
import pytest

import scene_cases as sc
from conftest import host_scene
from scene_check import INVARIANTS, SceneCheckError, check_scene
from test_scene_layout_cpu import checker  # noqa: F401  (the fixture: the stand-alone program, built with the sanitizers)

_layouts = {}


def layout(checker, tmp_path_factory, name):  # noqa: F811
    """(arrays, counts, acc_ok, the caller's four arrays) of a scene, laid out once"""
    if name not in _layouts:
        bvh, prims, mats, idx = sc.hand_made(name) if name in sc.HAND_MADE else host_scene(name)[1]
        arrays, counts, ok = sc.layout_dump(checker, tmp_path_factory.mktemp("dump"), bvh, prims, mats, idx)
        caller = (np.asarray(bvh, np.float32).reshape(-1, 8), np.asarray(prims, np.float32).reshape(-1, 12), np.asarray(mats, np.float32).reshape(-1, 8),
                  np.asarray(idx, np.int32).ravel())
        _layouts[name] = (arrays, counts, ok, caller)
    return _layouts[name]


def run(arrays, counts, caller):
    bvh, prims, mats, idx = caller
    return check_scene(arrays, counts, prims, mats, bvh, idx)


@pytest.mark.parametrize("name", sc.ASSET_SCENES + sc.HAND_MADE)
def test_checker_passes_on_the_host_layout(checker, tmp_path_factory, name):  # noqa: F811
    arrays, counts, ok, caller = layout(checker, tmp_path_factory, name)
    rep = run(arrays, counts, caller)
    print(name, counts, rep)
    assert ok == 1 and rep["exempt_leaves"] == 0 and rep["exempt_slots"] == 0
    assert rep["leaf_boxes_bit_equal"]                              # the host pads the reference box in one float32 operation per face
    if name == "40-primitive leaf":
        assert counts["n_leaves"] == 3 and counts["n_nodes"] == 7   # 16 + 16 + 8 under one reference leaf
    if name == "sphere with triangles":
        assert rep["tight_leaves"] == 1 and counts["n_always"] == 1
    if name == "single leaf":
        assert counts["n_own"] == 1 and counts["depth"] == 1


# ---- mutations: each is applied alone to a passing layout and names the invariant it must trip ----------------------------------------
class View:
    """the arrays of a layout, decoded for choosing where to mutate (copies: the cached layout stays as it is)"""

    def __init__(self, arrays, counts):
        self.a = {k: v.copy() for k, v in arrays.items()}
        self.c = dict(counts)
        self.T = self.a["nodes"].reshape(-1, 8)
        self.P = self.a["prims"].reshape(-1, 12)
        self.O = self.a["own"].reshape(-1, 28)
        self.RL = self.a["refleaf"].reshape(-1, 8)
        self.RB = self.a["refbox"].reshape(-1, 8)
        self.AL = self.a["always"].reshape(-1, 20)
        self.ref = self.O[:, 24:28]
        self.empty = self.ref == 0xFFFFFFFF
        self.leaf = ~self.empty & ((self.ref & 0x80000000) != 0)
        self.inner = ~self.empty & ~self.leaf

    def slots(self, mask):
        return [tuple(s) for s in np.argwhere(mask)]

    def plain_leaf_slots(self):
        """leaf slots whose reference leaf holds no sphere (their box is the padded reference box)"""
        tag = self.P[:, 3]
        sphere_leaves = set((tag[(tag & 1) == 0] >> 1).tolist())
        return [(n, s) for n, s in self.slots(self.leaf) if int(tag[self.ref[n, s] & 0x7FFFFFF] >> 1) not in sphere_leaves]


def ulp_up(words, i):
    f = words.view(np.float32)
    f[i] = np.nextafter(f[i], np.float32(np.inf))


def m_lo_one_ulp_up(v):
    n, s = v.slots(v.inner)[-1]
    ulp_up(v.O[n], 0 + s)                                           # lo.x of that slot


def m_hi_unpadded(v):
    n, s = v.plain_leaf_slots()[0]
    leaf = v.P[v.ref[n, s] & 0x7FFFFFF, 3] >> 1
    v.O[n, 12 + s] = v.RL[leaf, 4]                                  # hi.x := the reference leaf's, without the pad


def m_leaf_refs_swapped(v):
    (n0, s0), (n1, s1) = v.plain_leaf_slots()[0], v.plain_leaf_slots()[-1]
    v.ref[n0, s0], v.ref[n1, s1] = v.ref[n1, s1], v.ref[n0, s0]


def m_leaf_count_off(v):
    n, s = v.slots(v.leaf)[0]
    v.ref[n, s] ^= 1 << 27


def m_numbering_swapped(v):
    (n0, s0), (n1, s1) = v.slots(v.inner)[0], v.slots(v.inner)[-1]
    v.ref[n0, s0], v.ref[n1, s1] = v.ref[n1, s1], v.ref[n0, s0]


def m_empty_slot_finite(v):
    n, s = v.slots(v.empty)[0]
    v.O[n, 0 + s] = v.O[n, 12 + s] = 0                              # lo.x = hi.x = 0.0


def inner_threaded(v):
    return [i for i in range(1, v.T.shape[0]) if not v.T[i, 3] & 0x80000000]


def m_miss_to_next(v):
    i = next(i for i in inner_threaded(v) if v.T[i, 7] < v.T.shape[0])
    v.T[i, 7] += 1


def m_hit_to_left(v):
    i = inner_threaded(v)[0]
    v.T[i, 3] = v.T[v.T[i, 3], 7]                                    # the node after the right child's subtree is the left child


def m_tag_off(v):
    i = next(i for i in range(1, v.P.shape[0]) if (v.P[i, 3] >> 1) + 1 < v.RL.shape[0] and v.P[i, 3] >> 1 == v.P[i - 1, 3] >> 1)   # not its leaf's first
    v.P[i, 3] += 2


def m_refbox_neighbour(v):
    i = v.P.shape[0] // 2
    leaf = v.P[i, 3] >> 1
    v.RB[i] = v.RL[leaf + 1 if leaf + 1 < v.RL.shape[0] else leaf - 1]


def m_back_pointer_off(v):
    v.P[v.AL[0, 5], 6] += 1


def m_material_duplicated(v):
    v.a["mats"] = np.concatenate([v.a["mats"], v.a["mats"][:8]])
    v.c["n_mats"] += 1


def m_e1_one_ulp(v):
    i = next(i for i in range(v.P.shape[0]) if v.P[i, 3] & 1)
    ulp_up(v.P[i], 5)


def m_inner_box_in(v):
    ulp_up(v.T[inner_threaded(v)[0]], 0)


def m_chain_box(v):
    chain = [i for i in range(v.T.shape[0]) if v.T[i, 3] & 0x80000000 and v.T[i, 3] & 15 == 15]
    ulp_up(v.T[chain[0] + 1], 0)                                    # the node after the chain's first full one


def m_tight_lo_unpadded(v):
    plain = set(v.plain_leaf_slots())
    n, s = next(ns for ns in v.slots(v.leaf) if ns not in plain)   # the leaf that shares its reference leaf with the sphere
    first, count = int(v.ref[n, s] & 0x7FFFFFF), int((v.ref[n, s] >> 27) & 15) + 1
    rec = v.P[first:first + count]
    f = rec[(rec[:, 3] & 1) == 1].view(np.float32)
    v.O[n].view(np.float32)[0 + s] = min(f[:, 0].min(), (f[:, 0] + f[:, 4]).min(), (f[:, 0] + f[:, 8]).min())   # lo.x := the smallest corner, no pad


def m_always_names_another(v):
    v.AL[0, 5] = v.AL[1, 5]


MUTATIONS = [
    ("one own slot's lo one ulp up", m_lo_one_ulp_up, "own inner containment", "scene.xml"),
    ("one own leaf slot's hi set to the unpadded reference value", m_hi_unpadded, "own leaf containment", "scene.xml"),
    ("two leaf refs swapped between slots, boxes left in place", m_leaf_refs_swapped, "own leaf containment", "scene.xml"),
    ("a leaf ref's count off by one", m_leaf_count_off, "own leaf ref", "scene.xml"),
    ("two node indices swapped in the breadth-first numbering", m_numbering_swapped, "own numbering", "scene.xml"),
    ("an empty slot given a finite box", m_empty_slot_finite, "own empty slot", "sphere with triangles"),
    ("a miss link moved to the next node", m_miss_to_next, "miss link", "scene.xml"),
    ("a hit link pointing at the left child", m_hit_to_left, "visit order", "scene.xml"),
    ("one record's leaf tag off by one", m_tag_off, "record leaf id", "scene.xml"),
    ("one refbox row taken from the neighbouring leaf", m_refbox_neighbour, "refbox", "scene.xml"),
    ("an always entry's back-pointer off by one", m_back_pointer_off, "always back-pointer", "scene.xml"),
    ("a duplicated material row", m_material_duplicated, "materials distinct", "scene.xml"),
    ("one e1 component one ulp off", m_e1_one_ulp, "triangle record", "scene.xml"),
    # ... and four more: an inner box of the threaded tree, a chain node's box, a sphere missing from the always list, a tight box without its pad
    ("one inner box of the threaded tree one ulp in", m_inner_box_in, "reference nodes", "scene.xml"),
    ("a chain node with a box of its own", m_chain_box, "chain", "40-primitive leaf"),
    ("an always entry naming another sphere", m_always_names_another, "always entry", "scene.xml"),
    ("a tight box's lo set to the unpadded corner", m_tight_lo_unpadded, "own leaf containment", "sphere with triangles"),
]


@pytest.mark.parametrize("what,mutate,invariant,base", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_checker_raises_for_a_single_mutation(checker, tmp_path_factory, what, mutate, invariant, base):  # noqa: F811
    assert invariant in INVARIANTS
    arrays, counts, _, caller = layout(checker, tmp_path_factory, base)
    run(arrays, counts, caller)                                     # the layout passes as it is
    v = View(arrays, counts)
    mutate(v)
    changed = sum(int((v.a[k].size != arrays[k].size) or (v.a[k] != arrays[k]).any()) for k in arrays)
    assert changed == 1, "the mutation must change exactly one array"
    with pytest.raises(SceneCheckError) as e:
        run(v.a, v.c, caller)
    print(e.value)
    assert e.value.invariant == invariant, str(e.value)
