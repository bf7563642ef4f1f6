// mpt_anyhit.h — shadow rays: "is anything in the way before tmax?" (included by mpt_hip.hip after mpt_ordered.h).  gfx950 only.
//   any_hit_ref<ALL_LDS>   any-hit walk of the threaded reference-order tree (the sibling of closest_hit_resume, mpt_device.h)
//   any_hit_own            any-hit walk of the product's own 4-wide tree (the sibling of closest_hit_ordered, mpt_ordered.h)
//   k_occluded_ref/_own    one ray per lane through either walk (mpt_trace_occluded)
// The closest-hit walks, their leaf tests and their kernels are not touched: everything here is a sibling.
//
// Semantics.  A ray (o, d) with the limit tmax is OCCLUDED iff the reference's walk (R/Renderer/Shaders/PathTracing.h:75-204, as
// closest_hit_resume restates it) started with best t = tmax instead of +inf accepts any primitive.  The arithmetic is that walk's:
// the slab test with tMin = 1e-4 and tMax = best t, the sphere and triangle tests, acceptance `t > 1e-4 && t < best t`.  A lane that has
// accepted a primitive is done.  !(tmax > 1e-4) (a NaN tmax included) and a direction with a NaN component (the rule at the top of
// closest_hit_resume) are "not occluded" without a walk; tmax = +inf asks for any hit at all.
//
// Relation to the closest hit, with the same tree and arithmetic:
//   occluded  =>  mpt_trace_rays returns t < tmax.  EXACT.  Best t is the constant tmax here and never below tmax in the closest-hit
//       walk until that walk has itself accepted something below tmax; box tests only shrink with best t, so every node this walk visits
//       the closest-hit walk visits too (or has a hit below tmax already), and the primitive accepted here with t < tmax is accepted or
//       beaten there.
//   t < tmax  =>  occluded, EXCEPT the reference's known artefact: a hit whose computed t lies in front of its own leaf's slab entry
//       (mpt_ordered.h:13-25: the r = 10^4 ground sphere, slivers seen along their plane) with tmax between the two.  The closest-hit
//       walk enters that leaf with best t = +inf and accepts; this walk, with best t = tmax, is turned away at the leaf's box.
//       The same happens by one rounding when tmax is within an ulp or so of t: the slab entry of the hit's leaf (or of a box above
//       it) rounds to >= tmax, `hi > lo` fails and the hit below tmax is not seen (1-2 rays in 2048 on sliver scenes at
//       tmax = nextafter(t); tests/anyhit_ref.py restates the walk by brute force and tests/test_gpu_anyhit_exact.py holds both walks to it).
// The own tree reaches the same leaves another way (padded boxes, reciprocal arithmetic, spheres on the always list), culls with the
// closest-first walk's margin around tmax and tests primitives with the reference's exact tests, so it accepts what the reference
// accepts; it has no final check, so for the artefact above it answers by the primitive test alone ("occluded").
#pragma once
#include "mpt_ordered.h"

// One primitive against the ray: the reference's tests (PathTracing.h:120-176) with the operations and the order of leaf_test /
// ot_test_prim, and the acceptance against a constant limit.
__device__ __forceinline__ bool ah_test_prim(const Prim3& pr, F3 o, F3 d, float tmax) {
    const float4 p0 = pr.p0, p1 = pr.p1, p2 = pr.p2;
    float tt = 0.0f;
    bool hit = false;
    if (prim_type(p0) == 1) {   // (without early-outs, as ot_test_prim: the same operations give the same values, the rest is discarded)
        const F3 v0 = f3(p0.x, p0.y, p0.z), e1 = f3(p1.x, p1.y, p1.z), e2 = f3(p2.x, p2.y, p2.z);
        const F3 h = cross3(d, e2);
        const float a = dot3(e1, h);
        const float f = mpt_rcp(a);
        const F3 s = o - v0;
        const float u = f * dot3(s, h);
        const F3 q = cross3(s, e1);
        const float v = f * dot3(d, q);
        tt = f * dot3(e2, q);
        hit = fabsf(a) > 1e-5f && u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f && tt > 0.0001f;
    } else {
        const F3 c = f3(p0.x, p0.y, p0.z);
        const float radius = p1.x;
        const F3 oc = o - c;
        const float a = dot3(d, d);
        const float b = dot3(oc, d);
        if (!(b >= 0.0f)) {   // (b >= 0: the root is <= 0 whatever disc is — leaf_test)
            const float cc = dot3(oc, oc) - radius * radius;
            const float disc = b * b - a * cc;
            if (disc > 0.0f) {
                const float sq = sqrtf(disc);
                tt = (-b - sq) / a;
                hit = tt > 0.0001f;
            }
        }
    }
    return hit && tt < tmax;
}

// `live`: this lane has a ray (the others run along with state "done": the loops are wave-uniform, as in closest_hit_resume).
__device__ __forceinline__ bool ah_wanted(F3 d, float tmax, bool live) {
    return live && tmax > 0.0001f && !(d.x != d.x || d.y != d.y || d.z != d.z);
}

// Any hit in the reference's order.  The shape of closest_hit_resume: a wave-uniform box loop with the idle lanes masked, a leaf phase
// for all holders at once, top nodes and primitives from LDS; no budget and no resume state — the wave leaves when no lane searches or
// holds a leaf — and the limit of the slab test is a per-lane constant.  A lane's state is the one integer of that walk:
//   i < n_nodes searching, HOLD | enc holds a leaf, n_nodes <= i < HOLD done (an accepting lane goes there at once).
template <bool ALL_LDS>
__device__ __forceinline__ bool any_hit_ref(const SceneDev& sc, LdsNodes lds_nodes, F3 o, F3 d, float tmax, bool live) {
    float idx, idy, idz;
    mpt_rcp3(d.x, d.y, d.z, idx, idy, idz);
    const uint32_t n_nodes = sc.n_nodes, n_lds = sc.n_lds_nodes;
    uint32_t i = ah_wanted(d, tmax, live) ? 0u : n_nodes;
    bool hit = false;
    for (;;) {
        uint32_t skip = 0;
        const uint32_t n_entered0 = (uint32_t)__popcll(__ballot(i < n_nodes)), n_entered = max(n_entered0, 1u);
        uint32_t n_searching = n_entered0;
        while (n_searching * MPT_LEAF_EARLY >= n_entered) {
            const bool searching = i < n_nodes;
            const uint32_t j = i < n_nodes - 1u ? i : n_nodes - 1u;
            float4 n0 = make_float4(0, 0, 0, 0), n1 = n0;
            bool box = false;
            if (searching) {
                if (ALL_LDS || j < n_lds) {
                    const v4f a = lds_nodes[2 * j], b = lds_nodes[2 * j + 1];
                    n0 = make_float4(a.x, a.y, a.z, a.w);
                    n1 = make_float4(b.x, b.y, b.z, b.w);
                } else {
                    n0 = sc.nodes[2 * j];
                    n1 = sc.nodes[2 * j + 1];
                }
                // PathTracing.h:52-72 with tMin = 1e-4, tMax = tmax
                float t0 = (n0.x - o.x) * idx, t1 = (n1.x - o.x) * idx;
                float lo = fmaxf(0.0001f, idx < 0.0f ? t1 : t0);
                float hi = fminf(tmax, idx < 0.0f ? t0 : t1);
                t0 = (n0.y - o.y) * idy;
                t1 = (n1.y - o.y) * idy;
                lo = fmaxf(lo, idy < 0.0f ? t1 : t0);
                hi = fminf(hi, idy < 0.0f ? t0 : t1);
                t0 = (n0.z - o.z) * idz;
                t1 = (n1.z - o.z) * idz;
                lo = fmaxf(lo, idz < 0.0f ? t1 : t0);
                hi = fminf(hi, idz < 0.0f ? t0 : t1);
                box = hi > lo;
            }
            const uint32_t A = __float_as_uint(n0.w), B = __float_as_uint(n1.w);
            const uint32_t next = box ? A : B;
            i = searching ? next : i;
            skip = searching ? B : skip;
            n_searching = (uint32_t)__popcll(__ballot(i < n_nodes));
        }
        if ((i & MPT_NODE_HOLD) != 0u) {
            const uint32_t enc = i & ~MPT_NODE_HOLD, first = enc >> 4, count = (enc & 15u) + 1u;
            for (uint32_t k = 0; k < count && !hit; ++k) hit = ah_test_prim(load_prim(sc, lds_nodes, first + k), o, d, tmax);
            i = hit ? n_nodes : skip;
        }
        if (__ballot(i < n_nodes) == 0ull) break;
    }
    return hit;
}

// Any hit through the own 4-wide tree.  No child ordering: every child whose box test passes against the closest-first walk's culling
// limit around tmax (ot_cull_limit: tmax * (1 + 2^-10) + eps_abs) is entered — the first at once, the others by way of the lane's LDS
// stack — every primitive of an entered leaf is tested (the spheres come first, from the always list) and the first acceptance ends the
// lane's walk: no final check, no tie rule.  Rays closest_hit_ordered hands to the reference-order walk for their direction or origin
// (flag 1) go to any_hit_ref here too, and so does a ray whose stack overflowed (flag 8: it is traced again from the start).
// `sc` = the reference-order scene as k_trace_rays_ordered sees it (threaded nodes in global memory).
__device__ __forceinline__ bool any_hit_own(const AccelDev& ac, const SceneDev& sc, LdsNodes lds, const OtStack& st, F3 o, F3 d,
                                            float tmax, bool live, uint32_t& flags) {
    flags = 0u;
    const bool wanted = ah_wanted(d, tmax, live);
    if (live && ot_degenerate(o, d, ac.o_limit)) flags = 1u;
    const bool walk = wanted && flags == 0u;
    const OtRay r = ot_ray(o, d);
    const float lim = ot_cull_limit(tmax, ac);
    bool hit = false;
    if (walk) {
        for (uint32_t k = 0; k < ac.n_always && !hit; ++k) {
            const LdsNodes q = lds + ac.lds_always_off + 5u * k;
            const v4f a = q[0], b = q[1], c = q[2];
            Prim3 pr;
            pr.p0 = make_float4(a.x, a.y, a.z, a.w);
            pr.p1 = make_float4(b.x, b.y, b.z, b.w);
            pr.p2 = make_float4(c.x, c.y, c.z, c.w);
            hit = ah_test_prim(pr, o, d, tmax);
        }
    }
    uint32_t cur = walk && !hit ? 0u : MPT_OT_DONE, sp = 0u;
    for (;;) {
        const uint32_t n_entered = (uint32_t)__popcll(__ballot(cur < MPT_OT_LEAF)) * MPT_OT_EARLY_NUM;
        for (;;) {
            const uint32_t n_search = (uint32_t)__popcll(__ballot(cur < MPT_OT_LEAF));
            if (n_search == 0u || n_search * MPT_OT_EARLY < n_entered) break;
            if (!(cur < MPT_OT_LEAF)) continue;
            const OtNode nd = ot_load_node<false>(ac, lds, cur, r);
            const uint32_t k0 = ot_box_key(r, nd.lx.x, nd.ly.x, nd.lz.x, nd.hx.x, nd.hy.x, nd.hz.x, nd.ref.x, lim, 0u);
            const uint32_t k1 = ot_box_key(r, nd.lx.y, nd.ly.y, nd.lz.y, nd.hx.y, nd.hy.y, nd.hz.y, nd.ref.y, lim, 1u);
            const uint32_t k2 = ot_box_key(r, nd.lx.z, nd.ly.z, nd.lz.z, nd.hx.z, nd.hy.z, nd.hz.z, nd.ref.z, lim, 2u);
            const uint32_t k3 = ot_box_key(r, nd.lx.w, nd.ly.w, nd.lz.w, nd.hx.w, nd.hy.w, nd.hz.w, nd.ref.w, lim, 3u);
            const bool h0 = k0 < MPT_OT_KEY_MISS, h1 = k1 < MPT_OT_KEY_MISS, h2 = k2 < MPT_OT_KEY_MISS, h3 = k3 < MPT_OT_KEY_MISS;
            // the first child that is hit is entered now, the others wait on the stack: at most three entries, written one after the
            // other at sp, sp + [1 waits], sp + [1 waits] + [2 waits] (an entry that does not wait is overwritten or stays above the top)
            const bool w1 = h1 && h0, w2 = h2 && (h0 || h1), w3 = h3 && (h0 || h1 || h2);
            const uint32_t n_wait = (uint32_t)w1 + (uint32_t)w2 + (uint32_t)w3;
            uint32_t next = h0 ? nd.ref.x : h1 ? nd.ref.y : h2 ? nd.ref.z : h3 ? nd.ref.w : MPT_OT_DONE;
            if (sp + n_wait > st.depth) {   // no room: this ray is traced again in reference order
                flags |= 8u;
                next = MPT_OT_DONE;
                sp = 0u;
            } else if (n_wait != 0u) {
                if (w1) st.lds[sp++ * 64u] = v2u{k1, nd.ref.y};
                if (w2) st.lds[sp++ * 64u] = v2u{k2, nd.ref.z};
                if (w3) st.lds[sp++ * 64u] = v2u{k3, nd.ref.w};
            } else if (!(h0 || h1 || h2 || h3)) {
                if (sp > 0u) next = st.lds[--sp * 64u].y;
            }
            cur = next;
        }
        if (cur != MPT_OT_DONE && cur >= MPT_OT_LEAF) {   // a leaf: primitives [first, first + count)
            const uint32_t first = cur & 0x07FFFFFFu, count = ((cur >> 27) & 15u) + 1u;
            for (uint32_t k = 0; k < count && !hit; ++k) {
                const Prim3 pr = load_prim(sc, lds, first + k);
                if (ac.n_always != 0u && prim_type(pr.p0) == 0) continue;   // spheres are on the always list
                hit = ah_test_prim(pr, o, d, tmax);
            }
            cur = MPT_OT_DONE;
            if (!hit && sp > 0u) cur = st.lds[--sp * 64u].y;
        }
        if (__ballot(cur != MPT_OT_DONE) == 0ull) break;
    }
    if (__ballot(flags != 0u) != 0ull) {
        const bool again = any_hit_ref<false>(sc, lds, o, d, tmax, wanted && flags != 0u);
        if (flags != 0u) hit = again;
    }
    return hit;
}

// ---- mpt_trace_occluded: one ray per lane ------------------------------------------------------------------------------------------
// tmax = nullptr: +inf for every ray.  The LDS images are those of k_trace_rays / k_trace_rays_ordered.
template <bool ALL_LDS>
__global__ __launch_bounds__(256) void k_occluded_ref(SceneDev sc, const float* o, const float* d, const float* tmax, uint32_t n,
                                                      uint8_t* occluded_out) {
    extern __shared__ float4 lds_raw[];
    stage_nodes(sc, lds_raw);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    F3 ro = f3(1, 1, 1), rd = f3(1, 1, 1);
    float tm = 0.0f;
    if (live) {
        ro = f3(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
        rd = f3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        tm = tmax ? tmax[i] : INFINITY;
    }
    const bool hit = any_hit_ref<ALL_LDS>(sc, (LdsNodes)lds_raw, ro, rd, tm, live);
    if (live) occluded_out[i] = hit ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_occluded_own(SceneDev sc, AccelDev ac, const float* o, const float* d, const float* tmax, uint32_t n,
                                                      uint8_t* occluded_out, uint32_t* flags_out) {
    extern __shared__ float4 lds_raw[];
    ot_stage(sc, ac, lds_raw);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const OtStack st = ot_stack(ac, lds_raw, 0u);
    const bool live = i < n;
    F3 ro = f3(1, 1, 1), rd = f3(1, 1, 1);
    float tm = 0.0f;
    if (live) {
        ro = f3(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
        rd = f3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        tm = tmax ? tmax[i] : INFINITY;
    }
    uint32_t flags;
    const bool hit = any_hit_own(ac, sc, (LdsNodes)lds_raw, st, ro, rd, tm, live, flags);
    if (live) {
        occluded_out[i] = hit ? 1 : 0;
        if (flags_out) flags_out[i] = flags;
    }
}
