// mpt_lean_entry.h — where a fresh closest-hit query of the lean wave-local kernels (mpt_kernels.h) enters the tree: at the root's hit
// link instead of the root, for rays whose box test of the root is known to answer "hit" before it is made.  Pure arithmetic on plain
// floats (host and device, no HIP needed): the kernels evaluate it once per workgroup when they stage their LDS image, tests/lean_entry/
// compiles it alone.
//
// Node 0 has planes lo, hi and the links A0 (box hit) / B0 (box missed).  A fresh query has best_t = +inf, or a best_t that passed
// `tt > 0.0001f`.  The trip of the box loop (closest_hit_resume, mpt_device.h) computes, per axis a,
//     t0 = fl(fl(lo_a - o_a) * id_a),  t1 = fl(fl(hi_a - o_a) * id_a),  near = id_a < 0 ? t1 : t0,  far = id_a < 0 ? t0 : t1
// and answers hit when min(best_t, far_x, far_y, far_z) > max(0.0001f, near_x, near_y, near_z), min and max dropping NaN operands.
// With m = 2^-10 suppose on every axis
//     fl(lo_a - o_a) <= -m,   fl(hi_a - o_a) >= m,   |d_a| <= 2   and d has no NaN.
// id_a is the correctly rounded 1 / d_a (mpt_rcp3, either of its forms); rounding is monotone, so |id_a| >= 0.5 or id_a = +-inf
// (d_a = +-0, or a denormal whose reciprocal overflows).  fl(lo_a - o_a) is negative and fl(hi_a - o_a) positive, both of magnitude
// >= m, so no 0 * inf arises and no term is NaN; `near` is the product of two factors of opposite sign, negative (or -inf), `far` the
// product of two of the same sign, at least fl(m * 0.5) = 2^-11 = 4.9e-4 > 0.0001f (or +inf).  So max(..) = 0.0001f, min(..) >
// 0.0001f, the test answers hit and the trip's only effect is i = A0: `skip = B0` is overwritten by the lane's next trip, which it
// makes before any leaf phase reads `skip` (i = A0 < n_nodes is "searching").  A lane that starts at i = A0 sees the same sequence of
// tests from its second trip on.  (In a budgeted step the elided trip is not counted, so such a ray gets one real trip more before it
// is parked; a path's result does not depend on where its walk is cut.)
//
// The condition on the origin is made a box of its own, ilo = lo + 2m, ihi = hi - 2m, that the staging check below accepts only when
// fl(lo_a - ilo_a) <= -m and fl(hi_a - ihi_a) >= m: for ilo_a <= o_a <= ihi_a the exact differences obey lo_a - o_a <= lo_a - ilo_a
// and hi_a - o_a >= hi_a - ihi_a, and rounding keeps the order.  Boxes thinner than 4m (ilo_a <= ihi_a is required too), or at coordinates where an ulp exceeds 2m (the
// sums round back to lo, hi), fail that check: the item is then off for the launch (entry = 0, ilo = +inf, ihi = -inf).  It is also off
// when the root is a leaf record (A0 carries MPT_NODE_HOLD, so A0 >= n_nodes), when A0 == 0, and when a plane is NaN.
//
// |d_a| <= 2 is tested per ray by the kernel (one v_max3_f32 of magnitudes, one compare): normalize3 returns components of magnitude
// <= 1.23 when the squared length is representable — but (+-inf, +-inf, +-inf) when three non-zero components are so small that it
// rounds to zero, and then id = 0, every term is +-0 and the root's test answers MISS.
// (priced: profiles/r18_lean_entry.txt)
#pragma once
#include <stdint.h>

#define MPT_LEAN_ENTRY_M 0x1p-10f
#define MPT_LEAN_ENTRY_DMAX 2.0f
#if defined(__HIPCC__)
#define MPT_LEAN_ENTRY_HD __host__ __device__
#else
#define MPT_LEAN_ENTRY_HD
#endif

struct LeanEntry {
    float ilo[3], ihi[3];      // origins with ilo <= o <= ihi on every axis may skip the root (none when the item is off)
    uint32_t entry;            // A0, or 0: where such a query starts
    uint32_t entry_primary;    // A0 when the camera is such an origin, else 0: where a primary ray starts
};

// n0 = (lo, A0 as bits), n1 = (hi, B0 as bits): node 0 as the tree stores it.  V4 is any type with float members x, y, z, w.
template <class V4>
MPT_LEAN_ENTRY_HD inline LeanEntry lean_entry_terms(const V4& n0, const V4& n1, uint32_t n_nodes, float cam_x, float cam_y, float cam_z) {
    const float m = MPT_LEAN_ENTRY_M, inf = __builtin_huge_valf();
    const float lo[3] = {n0.x, n0.y, n0.z}, hi[3] = {n1.x, n1.y, n1.z}, cam[3] = {cam_x, cam_y, cam_z};
    uint32_t A0;
    const float a0 = n0.w;
    __builtin_memcpy(&A0, &a0, sizeof A0);
    LeanEntry e;
    bool on = A0 != 0u && A0 < n_nodes, cam_in = true;
    for (int a = 0; a < 3; ++a) {
        e.ilo[a] = lo[a] + 2.0f * m;
        e.ihi[a] = hi[a] - 2.0f * m;
        // (written so that a NaN anywhere switches the item off)
        on = on && (lo[a] - e.ilo[a] <= -m) && (hi[a] - e.ihi[a] >= m) && e.ilo[a] <= e.ihi[a];
        cam_in = cam_in && e.ilo[a] <= cam[a] && cam[a] <= e.ihi[a];
    }
    if (!on)
        for (int a = 0; a < 3; ++a) {
            e.ilo[a] = inf;
            e.ihi[a] = -inf;
        }
    e.entry = on ? A0 : 0u;
    e.entry_primary = on && cam_in ? A0 : 0u;
    return e;
}

// ---- the tail leaf --------------------------------------------------------------------------------------------------------------------
// The last node of every complete walk, T: start at the root's hit link A0 and follow miss links while they name a node.  When the
// device builder has hoisted the spheres (k_sah_to_radix_hoisted) T is their leaf record, the left child of the root, and the walk pops
// the right child first: every walk that is not cut ends with T's box test, T's primitives, "done".  The lean kernels whose whole tree
// is in LDS (ALL_LDS) replace every link to T in their staged image by the marker MPT_NODE_TAIL — a value >= n_nodes and below the
// leaf bit, so "done" for the box loop and never parked — and closest_hit_resume tests T once, after its loop, for the lanes that hold
// the marker: the same tests in the same order with the same best_t, at the width of those lanes and without the loop's rounds.
// T's box test is made there only by lanes for which it is not known to answer "hit": by the argument at the top of this file, with T's
// planes in the place of the root's, origins inside [tlo, thi] = [lo + 2m, hi - 2m] with |d_a| <= 2 hit (best_t at T is +inf or passed
// `tt > 0.0001f`, as for a fresh query; a NaN direction never reaches the marker).
// The item is on for a launch when the root is internal, T != 0, T is a leaf record whose miss link ends the walk (it does, by the
// way T is found), n_nodes is below the marker (the link that ends a walk in the device's tree is n_nodes itself, mpt_scene_layout.h,
// so no link of the tree is the marker by accident) and T's planes pass the staging check of lean_entry_terms.  Off: node = 0,
// nothing is patched and the kernels run as without the item.
// (priced: profiles/r20_lean_tail.txt)
#define MPT_NODE_TAIL 0x40000000u      // a link to T in the staged image
#define MPT_LEAN_LEAF_BIT 0x80000000u  // MPT_NODE_HOLD (mpt_device.h): the hit link of a leaf record

struct LeanTail {
    float tlo[3], thi[3];      // origins with tlo <= o <= thi on every axis need no box test of T (none when the item is off)
    uint32_t node;             // T, or 0 when the item is off
    uint32_t leaf;             // T's hit link: MPT_NODE_HOLD | first << 4 | (count - 1); 0 when off
    uint32_t tail_primary;     // 1 when the camera is such an origin, else 0
};

// nodes: the threaded tree as the device stores it, two V4 per node — (lo, hit link as bits) (hi, miss link as bits).
template <class V4>
MPT_LEAN_ENTRY_HD inline LeanTail lean_tail_terms(const V4* nodes, uint32_t n_nodes, float cam_x, float cam_y, float cam_z) {
    const float m = MPT_LEAN_ENTRY_M, inf = __builtin_huge_valf();
    const float cam[3] = {cam_x, cam_y, cam_z};
    LeanTail t;
    for (int a = 0; a < 3; ++a) {
        t.tlo[a] = inf;
        t.thi[a] = -inf;
    }
    t.node = t.leaf = t.tail_primary = 0u;
    if (n_nodes == 0u || n_nodes >= MPT_NODE_TAIL) return t;
    uint32_t T, B, steps = 0u;
    const float a0 = nodes[0].w;
    __builtin_memcpy(&T, &a0, sizeof T);
    if (T == 0u || T >= n_nodes) return t;   // the root is a leaf record (or a tree of one box)
    for (;; ++steps) {
        const float b = nodes[2u * T + 1u].w;
        __builtin_memcpy(&B, &b, sizeof B);
        if (B >= n_nodes) break;
        if (B == 0u || steps == n_nodes) return t;   // (links that never end: not a tree this code knows)
        T = B;
    }
    uint32_t leaf;
    const float l = nodes[2u * T].w;
    __builtin_memcpy(&leaf, &l, sizeof leaf);
    if ((leaf & MPT_LEAN_LEAF_BIT) == 0u) return t;   // T is internal (a chain node)
    const float lo[3] = {nodes[2u * T].x, nodes[2u * T].y, nodes[2u * T].z}, hi[3] = {nodes[2u * T + 1u].x, nodes[2u * T + 1u].y, nodes[2u * T + 1u].z};
    float tlo[3], thi[3];
    bool on = true, cam_in = true;
    for (int a = 0; a < 3; ++a) {
        tlo[a] = lo[a] + 2.0f * m;
        thi[a] = hi[a] - 2.0f * m;
        // (written so that a NaN anywhere switches the item off)
        on = on && (lo[a] - tlo[a] <= -m) && (hi[a] - thi[a] >= m) && tlo[a] <= thi[a];
        cam_in = cam_in && tlo[a] <= cam[a] && cam[a] <= thi[a];
    }
    if (!on) return t;
    for (int a = 0; a < 3; ++a) {
        t.tlo[a] = tlo[a];
        t.thi[a] = thi[a];
    }
    t.node = T;
    t.leaf = leaf;
    t.tail_primary = cam_in ? 1u : 0u;
    return t;
}
