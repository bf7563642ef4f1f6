"""An independent checker of the device scene arrays (mpt_read_scene_array), in numpy: every invariant the arrays carry, with exact
comparisons on the float32 values or on their bits.

Written from the format comments of mpt_accel.h (own 4-wide tree), mpt_device.h (threaded tree), mpt_scene_layout.h and mpt_devbuild.h
(records, leaf boxes, always list) — it calls nothing of the product.  check_scene raises SceneCheckError at the first violated
invariant; `.invariant` names it (the names are the INVARIANTS below) and the message names the node, slot or position.  There is no
Python loop over nodes or primitives: list ranking by pointer doubling for the threaded tree's visit order, one pass per level for the
reference-format tree and the own tree.

The tight box of a leaf that shares its reference leaf with a sphere is checked in float32 as well.  "Contains the float64 corners
v0 + e with the pad to spare" cannot hold to the last bit on either route: both clip the tight box to the reference leaf box, which ends
at a vertex p, while v0 + fl(p - v0) may lie half an ulp of the edge beside p, and the pad is then subtracted in one rounded float32
operation.  What both routes do give, exactly, is: every face lies at or beyond fl(c -/+ pad), c the smallest / largest FLOAT32 corner
fl(v0 + e) of the leaf's triangles — the sum the intersection code itself forms — or it is the clipped one, bit-equal to the padded
reference face fl(refleaf -/+ pad), which is what every other leaf gets.  That is asserted, without a tolerance.
"""
import numpy as np

INVARIANTS = (
    "sizes", "ids are a permutation", "record type", "triangle record", "sphere record", "material index", "material row", "materials distinct",
    "leaf tag", "root", "links in range", "leaf range", "visit order", "tree shape", "miss link", "leaf partition", "record leaf id", "chain",
    "leaf box", "breadth-first depth", "reference tree", "reference nodes", "reference leaves", "refbox", "always count", "always entry", "always back-pointer",
    "own size", "own empty slot", "own numbering", "own lds", "own depth", "own leaf ref", "own leaf set", "own leaf containment",
    "own inner containment", "own tightness")

HOLD = 0x80000000
OWN_LEAF = 0x80000000
OWN_EMPTY = 0xFFFFFFFF
OWN_WORDS = 28          # MPT_OT_NODE_STRIDE (7) float4
MAX_ALWAYS = 16


class SceneCheckError(AssertionError):
    def __init__(self, invariant, message):
        assert invariant in INVARIANTS, invariant
        super().__init__("%s: %s" % (invariant, message))
        self.invariant = invariant


def _need(ok, invariant, what, **where):
    """ok: a bool or a bool array; `where`: arrays of ok's shape (or its leading shape) that name the offender"""
    ok = np.asarray(ok)
    if ok.all():
        return
    at = tuple(np.argwhere(~ok)[0]) if ok.ndim else ()
    names = ", ".join("%s %s" % (k, np.asarray(v)[at[:np.asarray(v).ndim]]) for k, v in where.items())
    raise SceneCheckError(invariant, "%s (%s%s%d of %d fail)" % (what, names, "; " if names else "", int((~ok).sum()), ok.size))


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint32 else a


def _f(a):
    return np.ascontiguousarray(a).view(np.float32)


def _same(a, b):
    """bit equality of float32 arrays, a computed NaN standing for any NaN (inf - inf has no agreed payload)"""
    return (_u(a) == _u(b)) | (np.isnan(_f(a)) & np.isnan(_f(b)))


def _steps_to_end(nxt, n):
    """nxt[i] <= n for i < n: the number of links from every node to the end n, by pointer doubling (a cycle gives a number > n)"""
    j = np.append(nxt.astype(np.int64), n)
    d = np.ones(n + 1, np.int64)
    d[n] = 0
    for _ in range(int(n).bit_length() + 1):
        d = d + d[j]
        j = j[j]
    return d[:n]


def _ragged(first, count):
    """indices first[0] .. first[0] + count[0] - 1, first[1] .. : the concatenation of the ranges"""
    count = count.astype(np.int64)
    start = np.cumsum(count) - count
    return np.repeat(first.astype(np.int64) - start, count) + np.arange(int(count.sum()), dtype=np.int64)


def tri_pad(prims_in):
    """(tri_extent, pad) as own_tree_items / k_leaves compute them: the largest finite |coordinate| of a triangle vertex, in float32"""
    p = np.asarray(prims_in, np.float32).reshape(-1, 12)
    with np.errstate(invalid="ignore"):
        tri = np.nan_to_num(p[:, 3], nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64) == 1
    v = np.abs(p[tri][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])
    v = v[np.isfinite(v)]
    ext = np.float32(v.max()) if v.size else np.float32(0.0)
    return ext, np.float32(max(ext, np.float32(1e-6))) * np.float32(6.103515625e-05)


def reference_leaves(ref_bvh, ref_idx, n_prims):
    """The leaves of a reference-format tree (node = (bmin, leftFirst) (bmax, count): count > 0 a leaf of prim_idx[leftFirst ..], else
    left child leftFirst, right child -count) in the reference's visit order — root, right subtree, left subtree: (node index, first,
    count, boxes [L, 2, 3] as float32) per leaf, and every reachable node in that order.  One pass per level down (reachability), one up (subtree sizes), one down (positions)."""
    rb = _u(ref_bvh).reshape(-1, 8)
    N = rb.shape[0]
    lf, cnt = rb[:, 3].view(np.int32).astype(np.int64), rb[:, 7].view(np.int32).astype(np.int64)
    _need(N >= 1, "reference tree", "no nodes")
    levels, frontier, seen = [], np.zeros(1, np.int64), 1
    while frontier.size:
        levels.append(frontier)
        inner = frontier[cnt[frontier] <= 0]
        kids = np.concatenate([-cnt[inner], lf[inner]])
        _need((kids > 0) & (kids < N), "reference tree", "child index out of range")
        seen += kids.size
        _need(seen <= N, "reference tree", "more visits than nodes: not a tree")
        frontier = kids
    size = np.ones(N, np.int64)
    for lv in levels[::-1]:
        inner = lv[cnt[lv] <= 0]
        size[inner] = 1 + size[lf[inner]] + size[-cnt[inner]]
    pos = np.zeros(N, np.int64)
    for lv in levels:
        inner = lv[cnt[lv] <= 0]
        pos[-cnt[inner]] = pos[inner] + 1
        pos[lf[inner]] = pos[inner] + 1 + size[-cnt[inner]]
    reached = np.concatenate(levels)
    _need(np.unique(reached).size == reached.size, "reference tree", "a node has two parents")
    leaves = reached[cnt[reached] > 0]
    leaves = leaves[np.argsort(pos[leaves], kind="stable")]
    _need((lf[leaves] >= 0) & (lf[leaves] + cnt[leaves] <= n_prims), "reference tree", "leaf range out of bounds", node=leaves)
    boxes = np.stack([rb[leaves, 0:3], rb[leaves, 4:7]], axis=1).view(np.float32)
    return leaves, lf[leaves], cnt[leaves], boxes, reached[np.argsort(pos[reached], kind="stable")]


def check_scene(arrays, counts, prims_in, mats_in, ref_bvh=None, ref_idx=None, accel_info=None):
    """arrays: name -> words of nodes, prims, mats, own, refleaf, refbox, always (mpt_read_scene_array 0..6); counts: n_nodes, n_prims,
    n_mats, n_own, n_leaves, n_always, depth (mpt_scene_digest 9..15); prims_in / mats_in: the caller's rows; ref_bvh / ref_idx: the
    reference-format tree the arrays were derived from (the caller's on the upload route, mpt_download_bvh's on the device route);
    accel_info: mpt_accel_info's dictionary, for the LDS counts.  Returns what it measured: whether the plain leaf boxes are bit-equal to the padded
    reference boxes, the tight leaves and how many of their faces are the clipped ones, the exempt and void leaves and the exempt slots."""
    nodes, prims, mats, own = (_u(arrays[k]) for k in ("nodes", "prims", "mats", "own"))
    refleaf, refbox, always = (_u(arrays[k]) for k in ("refleaf", "refbox", "always"))
    n_nodes, n_prims, n_mats, n_own = (int(counts[k]) for k in ("n_nodes", "n_prims", "n_mats", "n_own"))
    n_leaves, n_always, depth = (int(counts[k]) for k in ("n_leaves", "n_always", "depth"))
    pin = np.ascontiguousarray(np.asarray(prims_in, np.float32).reshape(-1, 12))
    min_ = np.ascontiguousarray(np.asarray(mats_in, np.float32).reshape(-1, 8))
    report = {}

    sizes = dict(nodes=(nodes.size, 8 * n_nodes), prims=(prims.size, 12 * n_prims), mats=(mats.size, 8 * n_mats), own=(own.size, OWN_WORDS * n_own),
                 refleaf=(refleaf.size, 8 * n_leaves), refbox=(refbox.size, 8 * n_prims), always=(always.size, 20 * n_always),
                 prims_in=(pin.shape[0], n_prims), mats_in=(min_.shape[0], n_prims))
    for k, (got, want) in sizes.items():
        _need(got == want, "sizes", "%s has %d words or rows, the counts say %d" % (k, got, want))
    _need(n_nodes >= 1 and n_prims >= 1 and n_leaves >= 1, "sizes", "an empty scene")

    # ---- primitive records: v0 | tag, e1 | material, e2 | original id ---------------------------------------------------------------
    P = prims.reshape(n_prims, 12)
    PF = P.view(np.float32)
    tag, mat, pid = P[:, 3], P[:, 7], P[:, 11].astype(np.int64)
    is_tri, rec_leaf = (tag & 1) == 1, (tag >> 1).astype(np.int64)
    at = np.arange(n_prims)
    _need(np.sort(pid) == at, "ids are a permutation", "the original ids, sorted, are not 0 .. n-1", rank=at)
    src = pin[pid]
    with np.errstate(invalid="ignore"):
        type_in = np.nan_to_num(src[:, 3], nan=-1.0, posinf=-1.0, neginf=-1.0).astype(np.int64)   # (int)p[3]
    _need(is_tri == (type_in == 1), "record type", "the tag's triangle bit is not the caller's type", position=at, id=pid)
    same_v0 = _u(src[:, 0:3]) == P[:, 0:3]
    _need(~is_tri[:, None] | same_v0, "triangle record", "v0 is not the caller's p0", position=at, id=pid)
    _need(is_tri[:, None] | same_v0, "sphere record", "the centre is not the caller's", position=at, id=pid)
    with np.errstate(invalid="ignore"):
        e1, e2 = src[:, 4:7] - src[:, 0:3], src[:, 8:11] - src[:, 0:3]
    t = is_tri[:, None]
    _need(~t | _same(e1, PF[:, 4:7]), "triangle record", "e1 is not p1 - p0 in float32", position=at, id=pid)
    _need(~t | _same(e2, PF[:, 8:11]), "triangle record", "e2 is not p2 - p0 in float32", position=at, id=pid)
    sph = ~is_tri
    _need(~sph | np.where(type_in == 0, P[:, 4] == _u(src[:, 4]), np.isnan(PF[:, 4])), "sphere record", "radius is not the caller's (NaN for another type)",
          position=at, id=pid)
    _need(~sph[:, None] | (P[:, [5, 8, 9, 10]] == 0), "sphere record", "words 5, 8, 9, 10 of a sphere record are not zero", position=at)
    _need(mat < n_mats, "material index", "material index out of range", position=at)
    M = mats.reshape(n_mats, 8)
    _need(M[np.minimum(mat, n_mats - 1)] == _u(min_)[pid], "material row", "mats[index] is not the caller's material row", position=at, id=pid)
    _need(np.unique(M, axis=0).shape[0] == n_mats, "materials distinct", "two rows of mats are bit-equal")
    _need(rec_leaf < n_leaves, "leaf tag", "tag >> 1 is not a reference leaf", position=at)

    # ---- threaded tree -------------------------------------------------------------------------------------------------------------
    T = nodes.reshape(n_nodes, 8)
    A, B = T[:, 3].astype(np.int64), T[:, 7].astype(np.int64)
    ni = np.arange(n_nodes)
    leafm = (A & HOLD) != 0
    _need(B <= n_nodes, "links in range", "miss link past the end", node=ni)
    _need(leafm | (A < n_nodes), "links in range", "hit link of an inner node is not a node", node=ni)
    first, count = np.where(leafm, (A & 0x7FFFFFFF) >> 4, 0), np.where(leafm, (A & 15) + 1, 0)
    _need(first + count <= n_prims, "leaf range", "first + count past the records", node=ni)
    nxt = np.where(leafm, B, A)
    steps = _steps_to_end(nxt, n_nodes)
    _need(steps[0] == n_nodes, "visit order", "the walk from the root (hit at every inner node) makes %d steps, there are %d nodes" % (steps[0], n_nodes))
    order = np.argsort(steps, kind="stable")[::-1]              # visit position -> node
    _need(steps[order] == np.arange(n_nodes, 0, -1), "visit order", "a node is not on the walk from the root", node=order)
    _need(order[0] == 0, "root", "the walk does not start at index 0")
    vpos = n_nodes - steps                                      # node -> visit position
    lf = leafm[order]
    lid_v = np.where(lf, rec_leaf[np.minimum(first[order], n_prims - 1)], -1)
    cont = np.zeros(n_nodes, bool)                              # continues the chain of the node before (same reference leaf)
    cont[1:] = lf[1:] & lf[:-1] & (lid_v[1:] == lid_v[:-1])
    last = lf & ~np.append(cont[1:], False)
    w = np.where(~lf, 1, np.where(last, -1, 0))
    S = np.cumsum(w)
    vp = np.arange(n_nodes)
    _need(S[:-1] >= 0, "tree shape", "a subtree of the walk ends before its parent's", position=vp[:-1])
    _need(S[-1] == -1, "tree shape", "the walk ends with %d subtrees open" % (S[-1] + 1))
    smin = int(S.min())
    keys = (S - smin) * (n_nodes + 1) + vp                      # the first position q >= p with S[q] == S[p] - w[p] - 1 ends p's subtree
    ks = np.argsort(keys)
    q = ks[np.minimum(np.searchsorted(keys[ks], (S - w - 1 - smin) * (n_nodes + 1) + vp), n_nodes - 1)]
    _need((S[q] == S - w - 1) & (q >= vp), "tree shape", "no end of the subtree", position=vp)
    sub_end = q + 1
    after = np.append(order, n_nodes)[sub_end]
    _need(lf | (B[order] == after), "miss link", "the miss link is not the node after the subtree", node=order, miss=B[order], after=after)
    # parents by position: the right child follows its parent, the left one follows the right one's subtree; a chain node hangs on the one before
    inner_p = vp[~lf]
    parent = np.zeros(n_nodes, np.int64)
    parent[inner_p + 1] = inner_p
    left = sub_end[inner_p + 1]
    _need(left < n_nodes, "tree shape", "an inner node without a left child", position=inner_p)
    parent[left] = inner_p
    parent[cont] = vp[cont] - 1
    dep = (~cont).astype(np.int64)
    dep[0] = 0
    j = parent.copy()
    for _ in range(int(n_nodes).bit_length() + 1):
        dep = dep + dep[j]
        j = j[j]
    dep_by_index = dep[vpos]
    _need(np.diff(dep_by_index) >= 0, "breadth-first depth", "depth decreases along the index", node=ni[1:])
    # leaves: ranges, ids, chains, boxes
    lnode = order[lf]                                           # the leaves in visit order
    lfirst, lcount, lid = first[lnode], count[lnode], lid_v[lf]
    lcont = cont[lf]
    unit = np.cumsum(~lcont) - 1                                # leaf -> number of its reference leaf in visit order
    unit_lid = lid[~lcont]                                      # ... -> the id its records carry (the host numbers in visit order, the device in the builder's)
    _need(unit_lid.size == n_leaves, "record leaf id", "%d leaves on the walk, n_leaves is %d" % (unit_lid.size, n_leaves))
    _need(np.sort(unit_lid) == np.arange(n_leaves), "record leaf id", "the ids the leaves' first records carry are not a permutation of 0 .. n_leaves-1",
          rank=np.arange(n_leaves))
    by_first = np.argsort(lfirst, kind="stable")
    sf, sc_ = lfirst[by_first], lcount[by_first]
    _need(sf[0] == 0 and sf[-1] + sc_[-1] == n_prims, "leaf partition", "the leaf ranges do not span [0, n_prims)")
    _need(sf[1:] == sf[:-1] + sc_[:-1], "leaf partition", "two leaf ranges overlap or leave a gap", node=lnode[by_first][1:])
    owner = np.repeat(by_first, sc_)                            # record position -> its leaf (index into lnode)
    _need(rec_leaf == lid[owner], "record leaf id", "a record's tag >> 1 is not its leaf's id", position=at, tag_leaf=rec_leaf, leaf=lid[owner])
    prev = np.maximum(np.arange(lnode.size) - 1, 0)
    _need(~lcont | ((lcount[prev] == 16) & (lnode == lnode[prev] + 1) & (T[lnode][:, [0, 1, 2, 4, 5, 6]] == T[lnode[prev]][:, [0, 1, 2, 4, 5, 6]]).all(1)),
          "chain", "a chain node does not follow a full node of the same box at the next index", node=lnode)
    RL = refleaf.reshape(n_leaves, 8)
    _need(RL[:, [3, 7]] == 0, "leaf box", "words 3 and 7 of a refleaf row are not zero", leaf=np.arange(n_leaves))
    _need(T[lnode][:, [0, 1, 2, 4, 5, 6]] == RL[lid][:, [0, 1, 2, 4, 5, 6]], "leaf box", "a leaf's box is not refleaf[leaf]", node=lnode, leaf=lid)

    # ---- against the reference-format tree --------------------------------------------------------------------------------------------
    exempt_leaf, void_leaf = np.zeros(n_leaves, bool), np.zeros(n_leaves, bool)
    if ref_bvh is not None:
        ridx = np.asarray(ref_idx).astype(np.int64).ravel()
        _need(ridx.size == n_prims, "reference tree", "prim_idx has %d entries" % ridx.size)
        rnode, rfirst, rcount, rbox, rvisit = reference_leaves(ref_bvh, ridx, n_prims)
        # node for node: the walk of the threaded tree (a chain standing for its one leaf) is the reference's walk, with the reference's boxes
        rb = _u(ref_bvh).reshape(-1, 8)
        heads = order[~cont]
        _need(heads.size == rvisit.size, "reference nodes", "the walk visits %d nodes (chains as one), the reference tree has %d" % (heads.size, rvisit.size))
        _need(leafm[heads] == (rb[rvisit, 7].view(np.int32) > 0), "reference nodes", "a leaf stands where the reference's walk has an inner node, or the reverse",
              node=heads, reference_node=rvisit)
        _need(T[heads][:, [0, 1, 2, 4, 5, 6]] == rb[rvisit][:, [0, 1, 2, 4, 5, 6]], "reference nodes", "a node's box is not the reference node's", node=heads,
              reference_node=rvisit)
        _need(rnode.size == n_leaves, "reference leaves", "the reference tree has %d leaves, n_leaves is %d" % (rnode.size, n_leaves))
        ucount = np.bincount(unit, weights=lcount, minlength=n_leaves).astype(np.int64)
        _need(ucount == rcount, "reference leaves", "a leaf holds another number of primitives than the reference leaf", leaf=np.arange(n_leaves), reference_node=rnode)
        _need(pid[_ragged(lfirst, lcount)] == ridx[_ragged(rfirst, rcount)], "reference leaves", "the ids of the leaves in visit order are not the reference tree's",
              rank=np.arange(n_prims))
        _need(_u(rbox).reshape(-1, 6) == RL[unit_lid][:, [0, 1, 2, 4, 5, 6]], "reference leaves", "refleaf is not the reference leaf's box", leaf=np.arange(n_leaves), reference_node=rnode)
        exempt_leaf = ~np.isfinite(rbox).all(axis=(1, 2))
        void_leaf = ~(rbox[:, 1] >= rbox[:, 0]).all(axis=1)
    report["exempt_leaves"] = int(exempt_leaf.sum())

    # ---- refbox, always ---------------------------------------------------------------------------------------------------------------
    _need(refbox.reshape(n_prims, 8) == RL[rec_leaf], "refbox", "refbox[i] is not refleaf[tag_i >> 1]", position=at, leaf=rec_leaf)
    n_sph = int(sph.sum())
    use_always = n_sph <= MAX_ALWAYS
    _need(n_always == (n_sph if use_always else 0), "always count", "n_always is %d with %d sphere records" % (n_always, n_sph))
    if n_always:
        AL = always.reshape(n_always, 20)
        k = np.arange(n_always)
        where = AL[:, 5].astype(np.int64)
        _need((where < n_prims) & sph[np.minimum(where, n_prims - 1)], "always entry", "word 5 is not the position of a sphere record", entry=k)
        _need(np.unique(where).size == n_always, "always entry", "two entries name the same sphere")
        _need(AL[:, 6] == k, "always entry", "word 6 is not the entry's number", entry=k)
        keep = [0, 1, 2, 3, 4, 7, 8, 9, 10, 11]
        _need(AL[:, keep] == P[where][:, keep], "always entry", "the entry does not repeat its sphere's record", entry=k, position=where)
        _need(AL[:, 12:20] == RL[rec_leaf[where]], "always entry", "the entry's box is not its sphere's reference leaf box", entry=k, position=where)
        _need(P[where, 6] == k, "always back-pointer", "word 6 of the sphere's record is not its entry", entry=k, position=where)

    # ---- own tree -------------------------------------------------------------------------------------------------------------------------
    _need(n_own >= 1, "own size", "no root")
    O = own.reshape(n_own, OWN_WORDS)
    lo = O[:, 0:12].view(np.float32).reshape(n_own, 3, 4)       # [node, axis, slot]
    hi = O[:, 12:24].view(np.float32).reshape(n_own, 3, 4)
    ref = O[:, 24:28].astype(np.int64)
    node_of = np.repeat(np.arange(n_own), 4).reshape(n_own, 4)
    slot_of = np.tile(np.arange(4), n_own).reshape(n_own, 4)
    empty = ref == OWN_EMPTY
    _need(~empty | ((lo[:, 0, :] == np.inf) & (hi[:, 0, :] == np.inf)), "own empty slot", "an empty slot's x planes are not both +inf", node=node_of, slot=slot_of)
    inner_s = ~empty & ((ref & OWN_LEAF) == 0)
    leaf_s = ~empty & ~inner_s
    refs = ref[inner_s]                                         # (node order, then slot order)
    _need(refs.size == n_own - 1, "own numbering", "%d inner children, %d nodes" % (refs.size, n_own))
    _need(refs == np.arange(1, n_own), "own numbering", "the inner children are not 1, 2, ... in node and slot order", node=node_of[inner_s], slot=slot_of[inner_s])
    if accel_info is not None:
        _need(accel_info["lds_nodes"] <= n_own and accel_info["lds_prims"] <= n_prims and accel_info["nodes"] == n_own, "own lds", "mpt_accel_info's counts exceed the arrays")
    level_of = np.zeros(n_own, np.int64)
    bounds, a, b = [], 0, 1                                     # levels are ranges of the breadth-first numbering
    while a < b:
        bounds.append((a, b))
        level_of[a:b] = len(bounds) - 1
        kids = ref[a:b][inner_s[a:b]]
        a, b = b, b + kids.size
    _need(b == n_own, "own numbering", "the levels below node 0 cover %d of %d nodes" % (b, n_own))
    # (a tree without a leaf is one node of four empty slots: layout_scene counts no level for it, the device's collapse the one it wrote)
    _need(len(bounds) == depth or (empty.all() and depth == 0), "own depth", "the walk finds %d levels, the count says %d" % (len(bounds), depth))
    # leaf refs
    ofirst, ocount = ref[leaf_s] & 0x7FFFFFF, ((ref[leaf_s] >> 27) & 15) + 1
    onode, oslot = node_of[leaf_s], slot_of[leaf_s]
    hit = np.minimum(np.searchsorted(sf, ofirst), sf.size - 1)
    _need((sf[hit] == ofirst) & (sc_[hit] == ocount), "own leaf ref", "(first, count) is not the range of a leaf of the threaded tree", node=onode, slot=oslot,
          first=ofirst, count=ocount)
    oleaf = by_first[hit]                                       # index into lnode
    ntri = np.add.reduceat(is_tri.astype(np.int64), sf)         # per leaf in by_first order
    has_tri = np.zeros(lnode.size, bool)
    has_tri[by_first] = ntri > 0
    wanted = has_tri if use_always else np.ones(lnode.size, bool)
    times = np.bincount(oleaf, minlength=lnode.size)
    _need(times <= 1, "own leaf set", "a leaf appears twice in the own tree", node=lnode)
    # A leaf whose reference-format box is no box at all (not hi >= lo: every corner of its triangles NaN, which min and max skip) is entered
    # by no ray; layout_scene keeps it as an item, the device route (k_item_flags, mpt_devbuild.h) leaves it out.  Either is right, so such a
    # leaf may be absent — the rule reads the reference-format tree, not the arrays under test.  Every other wanted leaf must be there.
    void = void_leaf[unit]
    _need(((times == 1) == wanted) | (void & (times <= wanted)), "own leaf set",
          "the own leaves are not the leaves with a triangle" if use_always else "the own leaves are not all leaves", node=lnode, in_own_tree=times, wanted=wanted)
    report["void_leaves"], report["void_leaves_in_own_tree"] = int(void_leaf.sum()), int((void & (times == 1)).sum())
    # exempt slots: a leaf slot of an exempt reference leaf, an inner slot above one (the rule reads the reference-format tree alone)
    slot_ex = np.zeros((n_own, 4), bool)
    slot_ex[leaf_s] = exempt_leaf[unit[oleaf]]
    for a, b in bounds[::-1]:
        m = inner_s[a:b]
        slot_ex[a:b][m] = slot_ex[ref[a:b][m]].any(axis=1)
    report["slots"], report["exempt_slots"] = int((~empty).sum()), int(slot_ex.sum())
    # containment of the leaves
    ext, pad = tri_pad(pin)
    report["pad"] = float(pad)
    sph_leaf = np.bincount(rec_leaf, weights=sph, minlength=n_leaves) > 0   # by reference leaf
    shared = use_always & sph_leaf[lid[oleaf]]
    slo, shi = lo[onode, :, oslot], hi[onode, :, oslot]         # [leaf slot, axis]
    rl = RL[lid[oleaf]].view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        want_lo, want_hi = rl[:, 0:3] - pad, rl[:, 4:7] + pad
        plain = ~shared & ~slot_ex[leaf_s]
        _need(~plain[:, None] | ((slo <= want_lo) & (shi >= want_hi)), "own leaf containment", "a leaf slot does not contain refleaf grown by the pad", node=onode, slot=oslot,
              leaf=lid[oleaf])
        report["leaf_boxes_bit_equal"] = bool((~plain[:, None] | ((slo == want_lo) & (shi == want_hi))).all())
        # ... and of the leaves that share their reference leaf with a sphere (the module's docstring): every face lies at or beyond the
        # float32 corners of the leaf's triangles moved out by the pad, or is the reference leaf's face moved out by the pad
        v0 = PF[:, 0:3]
        corners = np.stack([v0, v0 + PF[:, 4:7], v0 + PF[:, 8:11]])                    # float32 sums, as the shader's and the builders'
        cmin = np.where(t, np.fmin.reduce(corners, axis=0), np.float32(np.inf))        # (min and max skip a NaN, as std::min and fminf do)
        cmax = np.where(t, np.fmax.reduce(corners, axis=0), np.float32(-np.inf))
        lmin, lmax = np.empty((lnode.size, 3), np.float32), np.empty((lnode.size, 3), np.float32)
        lmin[by_first], lmax[by_first] = np.fmin.reduceat(cmin, sf, axis=0), np.fmax.reduceat(cmax, sf, axis=0)
        tight = shared & ~slot_ex[leaf_s]
        ok_lo = (slo <= lmin[oleaf] - pad) | (slo == want_lo)
        ok_hi = (shi >= lmax[oleaf] + pad) | (shi == want_hi)
        _need(~tight[:, None] | (ok_lo & ok_hi), "own leaf containment",
              "the tight box of a sphere's leaf-mates neither contains their float32 corners grown by the pad nor ends at the padded leaf box", node=onode, slot=oslot,
              leaf=lid[oleaf])
        report["tight_leaves"] = int(tight.sum())
        report["tight_faces_clipped"] = int((tight[:, None] & ((slo == want_lo) | (shi == want_hi))).sum())
        # inner children: containment of the child's four slot boxes, and the bit-equal union
        pn, ps = node_of[inner_s], slot_of[inner_s]
        plo, phi = lo[pn, :, ps], hi[pn, :, ps]                 # [inner slot, axis]
        ce = empty[refs][:, None, :]
        clo, chi = np.where(ce, np.inf, lo[refs]), np.where(ce, -np.inf, hi[refs])
        live = ~slot_ex[inner_s]
        _need(~live[:, None, None] | ce | ((plo[:, :, None] <= clo) & (chi <= phi[:, :, None])), "own inner containment",
              "the slot box of an inner child does not contain a slot box of the child's node", node=pn, slot=ps, child=refs)
        # Tightness: on both routes the box of an inner child is min / max over boxes below it and nothing else (mpt_accel.h Builder::build
        # grows the node box from the items; the device routes copy or refit with fminf / fmaxf), so the union is exact: values compared
        # with ==, which tells a zero from a zero of the other sign no more than min and max do.
        _need(~live[:, None] | ((plo == clo.min(2)) & (phi == chi.max(2))), "own tightness", "the slot box of an inner child is not the union of the child's slot boxes",
              node=pn, slot=ps, child=refs)
    return report
