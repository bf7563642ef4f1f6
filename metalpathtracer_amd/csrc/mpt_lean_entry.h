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
// (MPT_LEAN_ENTRY=0: pricing build of the lean kernels without it — profiles/r18_lean_entry.txt)
#pragma once
#include <stdint.h>

#ifndef MPT_LEAN_ENTRY
#define MPT_LEAN_ENTRY 1
#endif
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
