// mpt_lean_tiles.h — what the camera knows per 8x8 pixel tile: a class word for the primary steps of the lean wave-local kernels whose whole
// tree is in LDS (mpt_kernels.h).  Pure arithmetic, host and device, no HIP needed: k_lean_tile_classes evaluates it once per tile when
// the scene, the camera or the image changes, tests/lean_tiles/ compiles it alone.
//
// A primary ray of a launch with the r18 entry and the tail item on (mpt_lean_entry.h, entry_primary and tail_primary set) starts at the
// root's hit link A0, follows the CHAIN — A0 and the nodes its miss links name, up to but not including the tail leaf T — and ends with
// T's primitives.  For one tile the word says
//     skip (bit 31)   every chain node's box test answers "miss" for every primary ray the tile can have, and every such ray has
//                     |d_a| <= MPT_LEAN_ENTRY_DMAX and no NaN: the walk is "T's primitives with best_t = +inf", nothing else
//     mask (bit k)    clear when primitive k of T (a sphere) is rejected for every such ray — b >= 0 or disc <= 0 in leaf_test, which
//                     leaves best_t and best_prim as they are; set otherwise
// so a step of a skip tile runs leaf_test on the primitives of `mask` in index order and gets the bits the walk would have got.
// 0 ("general"): the step walks as before.
//
// The proof obligation: every float32 value the kernel can compute for any ray of the tile lies inside the interval this file
// computes for it.  The primary path is restated operator for operator — pixel_uv, gen_primary (its constant division is the correctly
// rounded one: lean_cdiv_ok has measured that for the launch's W and H), normalize3, the reciprocals of mpt_rcp3 (correctly rounded in
// both of their forms), slab_hit, the sphere branch of leaf_test — on intervals with double-precision bounds over the domain
//     pixel column, row: the tile's 8 x 8, those past the image's edge included;  both jitter words: u01 in [0, 1 - 2^-24],
// one pixel at a time: a tile is `skip`, and a sphere is out of its mask, when that holds for each of its 64 pixels under every jitter.
// (Whole-tile intervals treat the components of d as independent and lose the sphere at y = 100 in scene.xml's top tile row.)
// Each operation takes the exact range of its operands' intervals (monotone per operand, so the four corner products etc.), in double
// (relative error 2^-53), and is then widened outward by |bound| * MPT_LEAN_TILES_REL + MPT_LEAN_TILES_ABS:
//     REL = 2^-21   eight times the 2^-24 a correctly rounded float32 operation moves its exact result by — the float32 rounding,
//                   the double rounding of the bound and the few operations this file merges (a point operand taken exactly)
//     ABS = 2^-120  a float32 result below 2^-126 is rounded to a multiple of 2^-149, or flushed to zero: either moves it by less
// and a bound beyond +-2^126 (where float32 may have overflowed to infinity) or a NaN makes its value UNUSABLE: the tile is general when
// that is the direction, a slab axis is dropped, a sphere keeps its bit.
// A select on a sign (`id < 0 ? t1 : t0`) is followed only when the sign is definite over the interval and |d| >= 2^-100; otherwise the
// axis is dropped from lo's max and hi's min.  That keeps both bounds valid — lo can only be larger with the axis, hi only smaller —
// and it is what fmaxf and fminf do with a NaN.  A chain node misses when the upper bound of hi is <= the lower bound of lo.
//
// General for every tile of the launch: the r18 entry or the tail item is off, or the camera is not inside both shrunk boxes; T holds
// a primitive that is no sphere; the chain is longer than MPT_LEAN_TILES_CHAIN_MAX; W or H is not the whole number of pixels that the
// tile counts cover (tiles_x = ceil(W / 8), tiles_y = ceil(H / 8)); a NaN anywhere.
// (Priced, `skip` alone and with the masks: profiles/r23_lean_tiles.txt.  MPT_LEAN_TILES_CONTROL: a build whose intervals shrink to the
//  tile-centre ray — wrong on purpose, the tests must fail with it.)
#pragma once
#include <stdint.h>
#if defined(MPT_LEAN_TILES_CONTROL) && !defined(MPT_LEAN_TILES_TESTING)
#error "MPT_LEAN_TILES_CONTROL makes the class table wrong on purpose: test builds only (-DMPT_LEAN_TILES_TESTING)"
#endif

#include "mpt_lean_entry.h"

#define MPT_LEAN_TILES_SKIP 0x80000000u
#define MPT_LEAN_TILES_MASK_BITS 0xFFFFu   // a leaf record holds at most 16 primitives
#define MPT_LEAN_TILES_CHAIN_MAX 8u
#define MPT_LEAN_TILES_REL 0x1p-21
#define MPT_LEAN_TILES_ABS 0x1p-120
#define MPT_LEAN_TILES_BIG 0x1p126
#define MPT_LEAN_TILES_DMIN 0x1p-100

struct LeanTileView {          // the camera as gen_primary reads it, and the tile grid
    float cam[3], first[3], vu[3], vv[3];
    float W, H;                // uniforms.screenSize
    uint32_t tiles_x, tiles_y;
};

struct LtIv {
    double lo, hi;
};
MPT_LEAN_ENTRY_HD inline LtIv lt_widen(double lo, double hi) {
    return LtIv{lo - (__builtin_fabs(lo) * MPT_LEAN_TILES_REL + MPT_LEAN_TILES_ABS), hi + (__builtin_fabs(hi) * MPT_LEAN_TILES_REL + MPT_LEAN_TILES_ABS)};
}
// usable: ordered bounds (no NaN) inside the range where float32 has not overflowed
MPT_LEAN_ENTRY_HD inline bool lt_ok(LtIv a) { return a.lo <= a.hi && a.lo >= -MPT_LEAN_TILES_BIG && a.hi <= MPT_LEAN_TILES_BIG; }
MPT_LEAN_ENTRY_HD inline LtIv lt_pt(float x) { return LtIv{(double)x, (double)x}; }
MPT_LEAN_ENTRY_HD inline LtIv lt_add(LtIv a, LtIv b) { return lt_widen(a.lo + b.lo, a.hi + b.hi); }
MPT_LEAN_ENTRY_HD inline LtIv lt_sub(LtIv a, LtIv b) { return lt_widen(a.lo - b.hi, a.hi - b.lo); }
MPT_LEAN_ENTRY_HD inline LtIv lt_mul(LtIv a, LtIv b) {
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    double lo = p0, hi = p0;
    lo = p1 < lo ? p1 : lo;
    lo = p2 < lo ? p2 : lo;
    lo = p3 < lo ? p3 : lo;
    hi = p1 > hi ? p1 : hi;
    hi = p2 > hi ? p2 : hi;
    hi = p3 > hi ? p3 : hi;
    if (!(p0 == p0 && p1 == p1 && p2 == p2 && p3 == p3)) lo = hi = __builtin_nan("");
    return lt_widen(lo, hi);
}
MPT_LEAN_ENTRY_HD inline LtIv lt_sq(LtIv a) {
    const double l = a.lo * a.lo, h = a.hi * a.hi;
    if (a.lo >= 0.0) return lt_widen(l, h);
    if (a.hi <= 0.0) return lt_widen(h, l);
    return lt_widen(0.0, l > h ? l : h);   // (a NaN bound: neither branch above, and the result carries it or lt_ok refuses the operand before)
}
// 1 / a and sqrt(a) for 0 < a.lo; a / w for a point w > 0
MPT_LEAN_ENTRY_HD inline LtIv lt_rcp_pos(LtIv a) { return lt_widen(1.0 / a.hi, 1.0 / a.lo); }
MPT_LEAN_ENTRY_HD inline LtIv lt_sqrt_pos(LtIv a) { return lt_widen(__builtin_sqrt(a.lo), __builtin_sqrt(a.hi)); }
MPT_LEAN_ENTRY_HD inline LtIv lt_div_pt(LtIv a, float w) { return lt_widen(a.lo / (double)w, a.hi / (double)w); }
MPT_LEAN_ENTRY_HD inline LtIv lt_neg(LtIv a) { return LtIv{-a.hi, -a.lo}; }

// The directions of the primary rays of one pixel (px, py) under every jitter, d[3], and a = dot3(d, d).  False: unusable (the tile is general).
MPT_LEAN_ENTRY_HD inline bool lean_tile_dirs(const LeanTileView& v, uint32_t ipx, uint32_t ipy, LtIv d[3], LtIv& a) {
    const LtIv px = {(double)ipx, (double)ipx}, py = {(double)ipy, (double)ipy};
#if defined(MPT_LEAN_TILES_CONTROL)
    const LtIv j = {0.0, 0.0};
#else
    const LtIv j = {-0.5, 0.5 - 0x1p-24};   // u01(r) - 0.5f
#endif
    const LtIv half = {0.5, 0.5};
    const LtIv sx = lt_add(lt_div_pt(lt_add(px, half), v.W), lt_div_pt(j, v.W));   // uvx + xOff
    const LtIv sy = lt_add(lt_div_pt(lt_add(py, half), v.H), lt_div_pt(j, v.H));
    LtIv dir[3];
    for (int c = 0; c < 3; ++c) {   // ((first + sx * vu) + sy * vv) - cam
        dir[c] = lt_sub(lt_add(lt_add(lt_pt(v.first[c]), lt_mul(sx, lt_pt(v.vu[c]))), lt_mul(sy, lt_pt(v.vv[c]))), lt_pt(v.cam[c]));
        if (!lt_ok(dir[c])) return false;
    }
    const LtIv l2 = lt_add(lt_add(lt_sq(dir[0]), lt_sq(dir[1])), lt_sq(dir[2]));
    if (!(lt_ok(l2) && l2.lo >= 0x1p-90 && l2.hi <= 0x1p120)) return false;   // (inside norm_core_exact's range with room: no zero, no infinity)
    const LtIv inv = lt_rcp_pos(lt_sqrt_pos(l2));
    for (int c = 0; c < 3; ++c) {
        d[c] = lt_mul(dir[c], inv);
        if (!(lt_ok(d[c]) && d[c].lo >= -(double)MPT_LEAN_ENTRY_DMAX && d[c].hi <= (double)MPT_LEAN_ENTRY_DMAX)) return false;
    }
    a = lt_add(lt_add(lt_sq(d[0]), lt_sq(d[1])), lt_sq(d[2]));
    return lt_ok(a);
}

// slab_hit of the box (n0, n1) from the origin o with best_t = +inf answers "miss" for every direction of d
template <class V4>
MPT_LEAN_ENTRY_HD inline bool lean_tile_box_misses(const V4& n0, const V4& n1, const float o[3], const LtIv d[3]) {
    const float lo3[3] = {n0.x, n0.y, n0.z}, hi3[3] = {n1.x, n1.y, n1.z};
    double lo = (double)0.0001f, hi = __builtin_huge_val();
    for (int c = 0; c < 3; ++c) {
        const bool pos = d[c].lo >= MPT_LEAN_TILES_DMIN, neg = d[c].hi <= -MPT_LEAN_TILES_DMIN;
        if (!pos && !neg) continue;   // the sign of id is not definite (or id may overflow): the axis is dropped
        const LtIv id = pos ? lt_rcp_pos(d[c]) : lt_neg(lt_rcp_pos(lt_neg(d[c])));
        const LtIv t0 = lt_mul(lt_sub(lt_pt(lo3[c]), lt_pt(o[c])), id), t1 = lt_mul(lt_sub(lt_pt(hi3[c]), lt_pt(o[c])), id);
        if (!(lt_ok(id) && lt_ok(t0) && lt_ok(t1))) continue;
        const LtIv near = neg ? t1 : t0, far = neg ? t0 : t1;
        lo = near.lo > lo ? near.lo : lo;
        hi = far.hi < hi ? far.hi : hi;
    }
    return hi <= lo;
}

// the sphere (p0 = centre, p1.x = radius) is rejected by leaf_test for every direction of d: b >= 0, or disc <= 0
template <class V4>
MPT_LEAN_ENTRY_HD inline bool lean_tile_sphere_rejected(const V4& p0, const V4& p1, const float o[3], const LtIv d[3], LtIv a) {
    const float c3[3] = {p0.x, p0.y, p0.z};
    LtIv oc[3];
    for (int c = 0; c < 3; ++c) oc[c] = lt_sub(lt_pt(o[c]), lt_pt(c3[c]));
    const LtIv cc = lt_sub(lt_add(lt_add(lt_sq(oc[0]), lt_sq(oc[1])), lt_sq(oc[2])), lt_mul(lt_pt(p1.x), lt_pt(p1.x)));
    const LtIv b = lt_add(lt_add(lt_mul(oc[0], d[0]), lt_mul(oc[1], d[1])), lt_mul(oc[2], d[2]));
    if (!(lt_ok(cc) && lt_ok(b))) return false;
    if (b.lo >= 0.0) return true;
    const LtIv disc = lt_sub(lt_sq(b), lt_mul(a, cc));
    return lt_ok(disc) && disc.hi <= 0.0;
}

// nodes: the threaded tree as the device stores it (two V4 per node), prims: its primitive records (three V4 each).
template <class V4>
MPT_LEAN_ENTRY_HD inline uint32_t lean_tile_class(const V4* nodes, uint32_t n_nodes, const V4* prims, uint32_t n_prims, const LeanTileView& v,
                                                  uint32_t tx, uint32_t ty) {
    if (n_nodes == 0u || tx >= v.tiles_x || ty >= v.tiles_y) return 0u;
    // the image: W x H whole pixels, covered by the tile grid (written so that a NaN is refused)
    if (!(v.W >= 1.0f && v.W <= 8.0f * (float)v.tiles_x && v.W > 8.0f * (float)v.tiles_x - 8.0f && v.W == (float)(uint32_t)v.W)) return 0u;
    if (!(v.H >= 1.0f && v.H <= 8.0f * (float)v.tiles_y && v.H > 8.0f * (float)v.tiles_y - 8.0f && v.H == (float)(uint32_t)v.H)) return 0u;
    if (v.tiles_x > (1u << 20) || v.tiles_y > (1u << 20)) return 0u;
    const LeanEntry e = lean_entry_terms(nodes[0], nodes[1], n_nodes, v.cam[0], v.cam[1], v.cam[2]);
    const LeanTail t = lean_tail_terms(nodes, n_nodes, v.cam[0], v.cam[1], v.cam[2]);
    if (e.entry_primary == 0u || t.node == 0u || t.tail_primary == 0u) return 0u;
    const uint32_t enc = t.leaf & ~MPT_LEAN_LEAF_BIT, first = enc >> 4, count = (enc & 15u) + 1u;
    if ((uint64_t)first + count > n_prims) return 0u;
    for (uint32_t k = 0; k < count; ++k) {   // spheres only
        const float w = prims[3u * (first + k)].w;
        uint32_t bits;
        __builtin_memcpy(&bits, &w, sizeof bits);
        if ((bits & 1u) != 0u) return 0u;
    }
    // pixel by pixel: the intervals of one pixel's rays are narrow enough that treating the components of d as independent loses little;
    // the tile's answer is the conjunction over its 64 pixels (the control build: the centre pixel without jitter)
    uint32_t mask = 0u;
#if defined(MPT_LEAN_TILES_CONTROL)
    for (uint32_t p = 36u; p < 37u; ++p) {
#else
    for (uint32_t p = 0u; p < 64u; ++p) {
#endif
        LtIv d[3], a;
        if (!lean_tile_dirs(v, tx * 8u + (p & 7u), ty * 8u + (p >> 3), d, a)) return 0u;
        uint32_t n = e.entry_primary, len = 0u;
        for (; n != t.node; ++len) {
            if (len == MPT_LEAN_TILES_CHAIN_MAX || n >= n_nodes) return 0u;
            if (!lean_tile_box_misses(nodes[2u * n], nodes[2u * n + 1u], v.cam, d)) return 0u;
            const float b = nodes[2u * n + 1u].w;
            __builtin_memcpy(&n, &b, sizeof n);
        }
        for (uint32_t k = 0; k < count; ++k)
            if ((mask >> k & 1u) == 0u && !lean_tile_sphere_rejected(prims[3u * (first + k)], prims[3u * (first + k) + 1u], v.cam, d, a)) mask |= 1u << k;
    }
    return MPT_LEAN_TILES_SKIP | mask;
}
