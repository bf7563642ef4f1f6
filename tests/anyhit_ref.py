"""numpy float32 restatement of the any-hit walk of include/mpt.h (shadow rays), by brute force over the reference-format tree.

The walk's limit is the constant tmax and it stops at the first acceptance, so the order of the visits does not matter: a ray is
occluded in reference order iff SOME primitive passes its test with 1e-4 < t < tmax AND every box from the root down to that primitive's
leaf passes the slab test with tMin = 1e-4, tMax = tmax.  Every value below is float32 and every line one IEEE operation, in the order
of ah_test_prim and of any_hit_ref's slab test (metalpathtracer_amd/csrc/mpt_anyhit.h; the library is built with -ffp-contract=off and
its mpt_rcp is IEEE 1 / x).  Two answers come out of it:
  occluded_reference      what MPT_WALK_REFERENCE must say, exactly                                   (the lower bound of the own walk)
  occluded_any_primitive  what a walk that tested primitives without looking at any box could say     (the upper bound of the own walk)
There is no closest hit here on purpose: the min of the accepted t is NOT the closest walk's answer (its boxes shrink with best t);
t* comes from the oracle (ao_ref.closest_t).  Test code: the product never imports it."""
import numpy as np

F = np.float32
T_MIN = F(0.0001)
CHUNK_ELEMS = 1 << 22      # rays x max(primitives, nodes) per chunk: 16 MB a temporary, a few hundred MB alive at most


def _dot(ax, ay, az, bx, by, bz):
    return ax * bx + ay * by + az * bz          # dot3: left to right


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx


def prim_t(o, d, prims):
    """[R, P] float32: the computed t of every primitive test that is accepted for t > 1e-4 (no upper limit), +inf otherwise."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    p = np.asarray(prims, np.float32).reshape(-1, 3, 4)
    ox, oy, oz = (o[:, i:i + 1] for i in range(3))
    dx, dy, dz = (d[:, i:i + 1] for i in range(3))
    is_tri = (p[:, 0, 3] == 1)[None, :]
    with np.errstate(all="ignore"):
        # triangle (PathTracing.h:143-176): e1 = v1 - v0, e2 = v2 - v0 as the upload stores them
        v0x, v0y, v0z = (p[None, :, 0, i] for i in range(3))
        e1x, e1y, e1z = (p[None, :, 1, i] - p[None, :, 0, i] for i in range(3))
        e2x, e2y, e2z = (p[None, :, 2, i] - p[None, :, 0, i] for i in range(3))
        hx, hy, hz = _cross(dx, dy, dz, e2x, e2y, e2z)
        a = _dot(e1x, e1y, e1z, hx, hy, hz)
        f = F(1.0) / a
        sx, sy, sz = ox - v0x, oy - v0y, oz - v0z
        u = f * _dot(sx, sy, sz, hx, hy, hz)
        qx, qy, qz = _cross(sx, sy, sz, e1x, e1y, e1z)
        v = f * _dot(dx, dy, dz, qx, qy, qz)
        tt = f * _dot(e2x, e2y, e2z, qx, qy, qz)
        hit_t = (np.abs(a) > F(1e-5)) & (u >= F(0)) & (u <= F(1)) & (v >= F(0)) & (u + v <= F(1)) & (tt > T_MIN)
        del hx, hy, hz, qx, qy, qz, u, v, f, a
        # sphere (PathTracing.h:120-142): centre = the first row, radius = the first word of the second
        radius = p[None, :, 1, 0]
        a = np.broadcast_to(_dot(dx, dy, dz, dx, dy, dz), sx.shape)
        b = _dot(sx, sy, sz, dx, dy, dz)
        cc = _dot(sx, sy, sz, sx, sy, sz) - radius * radius
        disc = b * b - a * cc
        ts = (-b - np.sqrt(disc)) / a
        hit_s = (disc > F(0)) & (ts > T_MIN)
        out = np.where(is_tri, np.where(hit_t, tt, F(np.inf)), np.where(hit_s, ts, F(np.inf)))
    return out.astype(np.float32)


def node_pass(o, d, bvh, tmax):
    """[R, N] bool: the slab test (PathTracing.h:52-72) of every node's box with tMin = 1e-4, tMax = tmax ([R] or a scalar)."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    box = np.asarray(bvh, np.float32).reshape(-1, 2, 4)
    tmax = np.broadcast_to(np.asarray(tmax, np.float32), (o.shape[0],))
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        lo = np.full((o.shape[0], box.shape[0]), T_MIN, np.float32)
        hi = np.broadcast_to(tmax[:, None], lo.shape)
        for i in range(3):
            t0 = (box[None, :, 0, i] - o[:, i:i + 1]) * inv[:, i:i + 1]
            t1 = (box[None, :, 1, i] - o[:, i:i + 1]) * inv[:, i:i + 1]
            neg = inv[:, i:i + 1] < F(0)
            lo = np.fmax(lo, np.where(neg, t1, t0))      # fmaxf / fminf drop the NaN of 0 * inf; np.maximum would keep it
            hi = np.fmin(hi, np.where(neg, t0, t1))
        return hi > lo


def tree_tables(bvh, prim_idx):
    """(levels, parent [N], leaf_of [P]) of a reference-format tree: the node indices of every depth below the root, every node's parent,
    and the leaf that holds each primitive (-1: none).  count > 0: a leaf over prim_idx[leftFirst : leftFirst + count]; otherwise the
    children are leftFirst and -count.  The root is node 0; the builders number the others as they like (the host builders put
    children behind their parent, the device builder of big scenes does not), so the levels come from a walk down from the root."""
    w = np.ascontiguousarray(np.asarray(bvh, np.float32).reshape(-1, 2, 4)).view(np.int32)
    left_first, count = w[:, 0, 3].astype(np.int64), w[:, 1, 3].astype(np.int64)
    idx = np.asarray(prim_idx, np.int64)
    N = w.shape[0]
    parent = np.full(N, -1, np.int64)
    leaf_of = np.full(idx.shape[0], -1, np.int64)
    levels = []
    level = np.zeros(min(N, 1), np.int64)
    seen = level.size
    while level.size:
        leaves = level[count[level] > 0]
        for i in leaves:
            leaf_of[idx[left_first[i]: left_first[i] + count[i]]] = i
        inner = level[count[level] <= 0]
        below = np.concatenate([left_first[inner], -count[inner]])
        assert ((below > 0) & (below < N)).all() and (parent[below] == -1).all() and np.unique(below).size == below.size, "not a reference-format tree"
        parent[below] = np.concatenate([inner, inner])
        seen += below.size
        assert seen <= N
        if below.size:
            levels.append(below)
        level = below
    assert seen == N, "a node that the root does not reach"
    return levels, parent, leaf_of


def reach(bvh, prim_idx, passed, tables=None):
    """[R, P] bool: the conjunction of `passed` [R, N] from the root down to each primitive's leaf."""
    levels, parent, leaf_of = tables or tree_tables(bvh, prim_idx)
    ok = np.array(passed, bool)
    for nodes in levels:
        ok[:, nodes] &= ok[:, parent[nodes]]
    out = ok[:, np.maximum(leaf_of, 0)]
    out[:, leaf_of < 0] = False
    return out


def wanted(d, tmax):
    """ah_wanted: a limit that asks for something and a direction without a NaN (as ao_ref.occluded)."""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    tmax = np.broadcast_to(np.asarray(tmax, np.float32), (d.shape[0],))
    with np.errstate(invalid="ignore"):
        return (tmax > T_MIN) & ~np.isnan(d).any(-1)


def bounds(o, d, tmaxes, buffers, want_t=False):
    """For every limit array of `tmaxes` (each [R] or a scalar): (lower [R] bool, upper [R] bool) = (occluded_reference,
    occluded_any_primitive), with the primitive tests computed once.  want_t: also the accepted t of every ray, as a third entry
    [R, P] (for small inputs only).  Chunked over the rays."""
    bvh, prims, _mats, prim_idx = buffers
    o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    R, P, N = o.shape[0], np.asarray(prims).reshape(-1, 12).shape[0], np.asarray(bvh).reshape(-1, 8).shape[0]
    tm = [np.broadcast_to(np.asarray(t, np.float32), (R,)) for t in tmaxes]
    tables = tree_tables(bvh, prim_idx)
    lower = [np.zeros(R, bool) for _ in tm]
    upper = [np.zeros(R, bool) for _ in tm]
    T_all = np.empty((R, P), np.float32) if want_t else None
    step = max(1, CHUNK_ELEMS // max(P, N, 1))
    for s in range(0, R, step):
        e = min(R, s + step)
        T = prim_t(o[s:e], d[s:e], prims)
        if want_t:
            T_all[s:e] = T
        for k, t in enumerate(tm):
            w = wanted(d[s:e], t[s:e])
            below = T < t[s:e, None]
            upper[k][s:e] = w & below.any(1)
            below &= reach(bvh, prim_idx, node_pass(o[s:e], d[s:e], bvh, t[s:e]), tables)
            lower[k][s:e] = w & below.any(1)
    out = [(lo, up) for lo, up in zip(lower, upper)]
    return (out, T_all) if want_t else out


def occluded_reference(o, d, tmax, buffers):
    """The lower bound: wanted & any(reach & (T < tmax)).  What the reference-order any-hit walk answers."""
    return bounds(o, d, [tmax], buffers)[0][0]


def occluded_any_primitive(o, d, tmax, buffers):
    """The upper bound: wanted & any(T < tmax).  The most a walk that tests a primitive without any box could say."""
    return bounds(o, d, [tmax], buffers)[0][1]


def degenerate(o, d, o_limit):
    """ot_degenerate (mpt_ordered.h): true unless every |d_i| is in [2^-20, 2] and every |o_i| <= o_limit."""
    o = np.abs(np.asarray(o, np.float32).reshape(-1, 3))
    d = np.abs(np.asarray(d, np.float32).reshape(-1, 3))
    with np.errstate(invalid="ignore"):
        return ~((d >= F(2.0 ** -20)).all(-1) & (d <= F(2.0)).all(-1) & (o <= F(o_limit)).all(-1))


def o_limit_of(prims):
    """AccelDev::o_limit: 64 x the largest finite |coordinate| of a triangle vertex (+inf for a scene without triangles)."""
    p = np.asarray(prims, np.float32).reshape(-1, 3, 4)
    c = np.abs(p[p[:, 0, 3] == 1][:, :, :3])
    c = c[np.isfinite(c)]
    return F(64.0) * c.max() if c.size and c.max() > 0 else F(np.inf)
