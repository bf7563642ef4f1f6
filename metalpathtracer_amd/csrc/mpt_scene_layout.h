// mpt_scene_layout.h — mpt_upload_scene's conversion of the reference's flat scene arrays into the device layout: threaded breadth-first
// BVH, leaf-ordered primitives, de-duplicated materials, the product's own 4-wide tree (mpt_accel.h), the leaf boxes and the always
// list.  Pure host C++, no HIP: mpt_hip.hip calls layout_scene and uploads what it returns; tests/scene_layout/scene_layout_check.cpp
// compiles this header alone with the host compiler's sanitizers and feeds it good, hand-made and malformed trees.
// The arrays come from the caller: every index read from them (child links, first, count, prim_idx) is checked before it is used.
// Compile with -ffp-contract=off (the box padding of own_tree_items is a sequence of single IEEE operations).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "mpt.h"
#include "mpt_accel.h"

namespace mpt_layout {

static inline int bits_to_int(float f) {
    int i;
    memcpy(&i, &f, 4);
    return i;
}
static inline float int_to_bits(int i) {
    float f;
    memcpy(&f, &i, 4);
    return f;
}

// The six host arrays of an uploaded scene (floats; the integer fields are bit patterns) and what the closest-first pipeline asks of it.
struct SceneLayout {
    std::vector<float> nodes;      // 8 per threaded node, breadth-first
    std::vector<float> prims;      // 12 per primitive record
    std::vector<float> mats;       // 8 per distinct material
    std::vector<float> acc_nodes;  // MPT_ACCEL_NODE_FLOATS per node of the own tree
    std::vector<float> refleaf;    // 8 per reference leaf: (bmin, 0) (bmax, 0)
    std::vector<float> always;     // 20 per sphere of the always list
    uint32_t acc_depth = 0;
    float tri_extent = 0.0f;       // largest |coordinate| of a triangle vertex
    bool nested = true;            // every child box lies inside its parent's
    bool use_always = true;        // at most MPT_ACCEL_MAX_ALWAYS spheres
    bool acc_ok() const { return nested && use_always; }   // the closest-first pipeline may be used for this scene
    const char* acc_why() const { return !nested ? "a child box is not inside its parent's box" : !use_always ? "more than 16 spheres" : ""; }
};

// A node of the threaded tree in VISIT order (permuted breadth-first at the end)
struct DNode {
    float bmin[3], bmax[3];
    bool leaf;
    uint32_t first, count;   // leaf
    uint32_t hit, miss;      // links as indices into dn (visit order); N_total = end
    uint32_t ref_leaf;       // leaf: number of the reference leaf it came from (visit order)
};

// 1. walk the reference tree in ITS visit order (root; right subtree; left subtree —
//    PathTracing.h:188-193 pushes left then right, so right pops first) and record the order.
//    order: visit position -> reference node; sub_end: visit position -> visit position just past its subtree.
static inline bool visit_order(const float* bvh, uint32_t N, uint64_t n_prims, std::vector<uint32_t>& order, std::vector<uint32_t>& sub_end,
                               std::string& err) {
    order.clear();
    order.reserve(N);
    std::vector<uint8_t> seen(N, 0);
    // iterative DFS with explicit post-processing for subtree ends
    struct Fr {
        uint32_t node, pos;
        int stage;
    };
    std::vector<Fr> st;
    st.push_back({0u, 0u, 0});
    sub_end.assign(N, 0);
    auto bad = [&](const char* msg) {
        err = msg;
        return false;
    };
    while (!st.empty()) {
        Fr& f = st.back();
        if (f.stage == 0) {
            if (f.node >= N || seen[f.node]) return bad("BVH is not a tree (cycle or index out of range)");
            seen[f.node] = 1;
            f.pos = (uint32_t)order.size();
            order.push_back(f.node);
            int count = bits_to_int(bvh[8 * (size_t)f.node + 7]);
            if (count > 0) {
                int first = bits_to_int(bvh[8 * (size_t)f.node + 3]);
                if (first < 0 || (uint64_t)first + (uint64_t)count > n_prims) return bad("leaf primitive range out of bounds");
                sub_end[f.pos] = f.pos + 1;
                st.pop_back();
            } else {
                f.stage = 1;
                uint32_t right = (uint32_t)(-(long long)count);
                if (count == 0) return bad("internal node with right child 0");
                st.push_back({right, 0u, 0});
            }
        } else if (f.stage == 1) {
            f.stage = 2;
            int left = bits_to_int(bvh[8 * (size_t)f.node + 3]);
            if (left < 0) return bad("negative left child");
            st.push_back({(uint32_t)left, 0u, 0});
        } else {
            sub_end[f.pos] = (uint32_t)order.size();
            st.pop_back();
        }
    }
    return true;
}

// 1b. every child box must lie inside its parent's box: then the reference's walk equals a scan over the leaves in
//     visit order (mpt_ordered.h) and the closest-first pipeline may be used; otherwise only the reference-order ones.
static inline bool boxes_nested(const float* bvh, const std::vector<uint32_t>& order, const std::vector<uint32_t>& sub_end) {
    const uint32_t NV = (uint32_t)order.size();
    bool nested = true;
    for (uint32_t pos = 0; pos < NV && nested; ++pos) {
        const float* n = bvh + 8 * (size_t)order[pos];
        if (bits_to_int(n[7]) > 0) continue;
        const uint32_t kids[2] = {pos + 1, pos + 1 < NV ? sub_end[pos + 1] : NV};
        for (uint32_t k : kids) {
            if (k >= NV) continue;
            const float* c = bvh + 8 * (size_t)order[k];
            for (int a = 0; a < 3; ++a)
                if (!(c[a] >= n[a] && c[4 + a] <= n[4 + a])) nested = false;
        }
    }
    return nested;
}

// 2. leaves: gather primitives into leaf order; split leaves of more than 16 primitives into a chain.
//    Device node list in VISIT order (dn; pos_to_dn: visit position -> dn index of its (first) node, NV + 1 entries), the primitive
//    records, the materials de-duplicated by their bits (first occurrence in leaf order), the reference leaf boxes.
struct Leaves {
    std::vector<DNode> dn;
    std::vector<uint32_t> pos_to_dn;
    std::vector<float> prims, mats, refleaf;
    uint32_t n_spheres = 0;
    float tri_extent = 0.0f;
};
static inline bool split_leaves(const float* bvh, const float* prims, const float* mats, const int32_t* prim_idx, uint64_t n_prims,
                                const std::vector<uint32_t>& order, const std::vector<uint32_t>& sub_end, Leaves& out, std::string& err) {
    const uint32_t NV = (uint32_t)order.size();
    std::vector<DNode>& dn = out.dn;
    dn.reserve(NV + 16);
    out.pos_to_dn.assign(NV + 1, 0);
    out.prims.reserve((size_t)n_prims * 12);
    std::map<std::vector<uint32_t>, uint32_t> mat_lookup;
    auto mat_index = [&](uint32_t pid) -> uint32_t {
        std::vector<uint32_t> key(8);
        memcpy(key.data(), mats + 8 * (size_t)pid, 32);
        auto it = mat_lookup.find(key);
        if (it != mat_lookup.end()) return it->second;
        uint32_t id = (uint32_t)(out.mats.size() / 8);
        out.mats.insert(out.mats.end(), mats + 8 * (size_t)pid, mats + 8 * (size_t)pid + 8);
        mat_lookup.emplace(std::move(key), id);
        return id;
    };
    // first pass: create dn entries; a long leaf becomes ceil(count/16) chained nodes
    for (uint32_t pos = 0; pos < NV; ++pos) {
        const float* n = bvh + 8 * (size_t)order[pos];
        int count = bits_to_int(n[7]);
        out.pos_to_dn[pos] = (uint32_t)dn.size();
        DNode d;
        memcpy(d.bmin, n, 12);
        memcpy(d.bmax, n + 4, 12);
        d.hit = d.miss = 0;
        d.ref_leaf = 0;
        if (count > 0) {
            int first = bits_to_int(n[3]);
            d.leaf = true;
            d.ref_leaf = (uint32_t)(out.refleaf.size() / 8);
            const float rl[8] = {n[0], n[1], n[2], 0.0f, n[4], n[5], n[6], 0.0f};
            out.refleaf.insert(out.refleaf.end(), rl, rl + 8);
            for (int k0 = 0; k0 < count; k0 += 16) {
                d.first = (uint32_t)(out.prims.size() / 12);
                d.count = (uint32_t)std::min(16, count - k0);
                for (uint32_t k = 0; k < d.count; ++k) {
                    int32_t pid = prim_idx[first + k0 + (int)k];
                    if (pid < 0 || (uint64_t)pid >= n_prims) {
                        err = "primitive index out of range";
                        return false;
                    }
                    const float* p = prims + 12 * (size_t)pid;
                    float rec[12];
                    int type = (int)p[3];
                    uint32_t m = mat_index((uint32_t)pid);
                    if (type == 1) {  // triangle: v0, e1 = v1 - v0, e2 = v2 - v0 (PathTracing.h:149-150)
                        rec[0] = p[0]; rec[1] = p[1]; rec[2] = p[2];
                        rec[4] = p[4] - p[0]; rec[5] = p[5] - p[1]; rec[6] = p[6] - p[2];
                        rec[8] = p[8] - p[0]; rec[9] = p[9] - p[1]; rec[10] = p[10] - p[2];
                        for (int q = 0; q < 11; ++q)
                            if ((q & 3) != 3 && std::isfinite(p[q])) out.tri_extent = std::max(out.tri_extent, fabsf(p[q]));
                    } else {  // sphere; anything that is neither is never hit (PathTracing.h:120,143) — kept as a sphere of radius NaN
                        rec[0] = p[0]; rec[1] = p[1]; rec[2] = p[2];
                        rec[4] = type == 0 ? p[4] : NAN; rec[5] = 0; rec[6] = 0;
                        rec[8] = 0; rec[9] = 0; rec[10] = 0;
                        out.n_spheres++;
                    }
                    rec[3] = int_to_bits((int)((d.ref_leaf << 1) | (type == 1 ? 1u : 0u)));
                    rec[7] = int_to_bits((int)m);
                    rec[11] = int_to_bits(pid);
                    out.prims.insert(out.prims.end(), rec, rec + 12);
                }
                dn.push_back(d);
            }
        } else {
            d.leaf = false;
            d.first = d.count = 0;
            dn.push_back(d);
        }
    }
    out.pos_to_dn[NV] = (uint32_t)dn.size();
    // second pass: links.  In visit order the node after position pos is pos+1; a missed internal node
    // skips to sub_end[pos].
    for (uint32_t pos = 0; pos < NV; ++pos) {
        uint32_t a = out.pos_to_dn[pos], b = out.pos_to_dn[pos + 1];
        if (dn[a].leaf) {
            for (uint32_t k = a; k < b; ++k) dn[k].hit = dn[k].miss = k + 1;  // chain, then the next position
        } else {
            dn[a].hit = a + 1;
            dn[a].miss = out.pos_to_dn[sub_end[pos]];
        }
    }
    return true;
}

// 3. the product's own tree over the leaves (mpt_accel.h): spheres go to the always list (their t has no usable
//    error bound: the r = 10^4 ground sphere), every leaf that holds triangles becomes an item whose box contains
//    the reference leaf box — or, for the triangles that share a leaf with a sphere, a tight box of their own.
//    items / item_dn: the items and the dn index of each; sphere_only_dn: the leaves without an item.
static inline void own_tree_items(const std::vector<DNode>& dn, const std::vector<float>& dprims, bool use_always, float tri_extent,
                                  std::vector<mpt_accel::Item>& items, std::vector<uint32_t>& item_dn, std::vector<uint32_t>& sphere_only_dn) {
    const float pad = std::max(tri_extent, 1e-6f) * 6.103515625e-05f;  // 2^-14: covers the rcp / fma slab arithmetic
    for (uint32_t i = 0; i < (uint32_t)dn.size(); ++i) {
        const DNode& d = dn[i];
        if (!d.leaf) continue;
        mpt_accel::Box tb = mpt_accel::empty_box();
        uint32_t ntri = 0, nsph = 0;
        for (uint32_t k = 0; k < d.count; ++k) {
            const float* r = dprims.data() + (size_t)(d.first + k) * 12;
            if (bits_to_int(r[3]) & 1) {
                ntri++;
                const float v[3][3] = {{r[0], r[1], r[2]}, {r[0] + r[4], r[1] + r[5], r[2] + r[6]}, {r[0] + r[8], r[1] + r[9], r[2] + r[10]}};
                for (auto& q : v) {
                    mpt_accel::Box c;
                    memcpy(c.lo, q, 12);
                    memcpy(c.hi, q, 12);
                    mpt_accel::grow(tb, c);
                }
            } else {
                nsph++;
            }
        }
        if (ntri == 0 && use_always) {
            sphere_only_dn.push_back(i);
            continue;
        }
        mpt_accel::Item it;
        memcpy(it.box.lo, d.bmin, 12);
        memcpy(it.box.hi, d.bmax, 12);
        if (nsph != 0 && use_always) {  // a sphere's leaf-mates: v0 + e is not exactly the vertex, hence the generous margin
            float ext = 0.0f;
            for (int a = 0; a < 3; ++a) ext = std::max(ext, tb.hi[a] - tb.lo[a]);
            for (int a = 0; a < 3; ++a) {
                it.box.lo[a] = std::max(d.bmin[a], tb.lo[a] - 0.05f * ext - pad);
                it.box.hi[a] = std::min(d.bmax[a], tb.hi[a] + 0.05f * ext + pad);
            }
        }
        for (int a = 0; a < 3; ++a) {
            it.box.lo[a] -= pad;
            it.box.hi[a] += pad;
        }
        it.count = d.count;
        it.key = i;
        items.push_back(it);
        item_dn.push_back(i);
    }
}

// 4. ONE primitive array for both structures: leaves without an item (spheres only) first — the reference-order
//    kernels test them for almost every ray, so they belong to the LDS-staged prefix — then the items in the
//    breadth-first order of the own tree (shallow leaves first).  Returns item -> first primitive of its leaf.
static inline std::vector<uint32_t> reorder_prims(std::vector<DNode>& dn, std::vector<float>& dprims, const std::vector<uint32_t>& sphere_only_dn,
                                                  const std::vector<uint32_t>& item_dn, const std::vector<uint32_t>& item_order) {
    std::vector<uint32_t> first_of(item_dn.size(), 0);
    std::vector<float> ordered(dprims.size());
    uint32_t at = 0;
    auto place = [&](DNode& d) {
        memcpy(ordered.data() + (size_t)at * 12, dprims.data() + (size_t)d.first * 12, (size_t)d.count * 48);
        d.first = at;
        at += d.count;
    };
    for (uint32_t i : sphere_only_dn) place(dn[i]);
    for (uint32_t it : item_order) {
        place(dn[item_dn[it]]);
        first_of[it] = dn[item_dn[it]].first;
    }
    dprims.swap(ordered);
    return first_of;
}
// ... and the always list: every sphere of the reordered array with the box of its reference leaf; its record points back at its entry.
static inline std::vector<float> always_list(std::vector<float>& dprims, const std::vector<float>& refleaf) {
    std::vector<float> always;
    for (size_t i = 0; i < dprims.size() / 12; ++i) {
        const float* r = dprims.data() + i * 12;
        if (bits_to_int(r[3]) & 1) continue;
        float rec[20];
        memcpy(rec, r, 48);
        const uint32_t k = (uint32_t)(always.size() / 20), leaf = (uint32_t)bits_to_int(r[3]) >> 1;
        rec[5] = int_to_bits((int)i);  // own position in the primitive array = what the walk reports as the winner
        rec[6] = int_to_bits((int)k);
        memcpy(rec + 12, refleaf.data() + 8 * (size_t)leaf, 32);  // the box of its reference leaf, for the final check
        always.insert(always.end(), rec, rec + 20);
        dprims[i * 12 + 6] = int_to_bits((int)k);  // the primitive record points back at its always-list entry
    }
    return always;
}

// 5. reference-order structure: breadth-first permutation of the threaded nodes (top of the tree first -> LDS).
static inline std::vector<float> breadth_first_nodes(const std::vector<DNode>& dn, const std::vector<uint32_t>& pos_to_dn,
                                                     const std::vector<uint32_t>& sub_end) {
    const uint32_t ND = (uint32_t)dn.size(), NV = (uint32_t)pos_to_dn.size() - 1u;
    std::vector<uint32_t> depth(ND, 0);
    {
        // depth by walking positions: children of internal at pos are pos+1 (right) and sub_end[pos+1] (left)
        std::vector<uint32_t> pdepth(NV, 0);
        for (uint32_t pos = 0; pos < NV; ++pos) {
            uint32_t a = pos_to_dn[pos];
            if (!dn[a].leaf) {
                uint32_t r = pos + 1;
                if (r < NV) {
                    pdepth[r] = pdepth[pos] + 1;
                    uint32_t l = sub_end[r];
                    if (l < NV && l < sub_end[pos]) pdepth[l] = pdepth[pos] + 1;
                }
            }
            for (uint32_t k = a; k < pos_to_dn[pos + 1]; ++k) depth[k] = pdepth[pos];
        }
    }
    std::vector<uint32_t> perm(ND);  // new index -> dn index
    for (uint32_t i = 0; i < ND; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return depth[a] < depth[b]; });
    // the root must stay at index 0 (depth 0, unique) — guaranteed by the stable sort
    std::vector<uint32_t> inv(ND + 1);
    for (uint32_t i = 0; i < ND; ++i) inv[perm[i]] = i;
    inv[ND] = ND;  // terminator
    std::vector<float> dnodes((size_t)ND * 8);
    for (uint32_t i = 0; i < ND; ++i) {
        const DNode& d = dn[perm[i]];
        float* o = dnodes.data() + 8 * (size_t)i;
        memcpy(o, d.bmin, 12);
        memcpy(o + 4, d.bmax, 12);
        if (d.leaf) {  // hit link = "hold this leaf" (MPT_NODE_HOLD | first << 4 | count - 1), miss link = the next node either way
            o[3] = int_to_bits((int)(0x80000000u | (d.first * 16u + (d.count - 1u))));
            o[7] = int_to_bits((int)inv[d.hit]);
        } else {
            o[3] = int_to_bits((int)inv[d.hit]);
            o[7] = int_to_bits((int)inv[d.miss]);
        }
    }
    return dnodes;
}

// The whole conversion.  n_nodes < 2^30 and n_prims < 2^27, both non-zero (the caller has checked: the 27-bit leaf encoding).
// MPT_OK, or MPT_ERR_BAD_SCENE with the reason in err: the first fault in the reference's visit order, then the first bad prim_idx entry.
static inline int layout_scene(const float* bvh, uint64_t n_nodes, const float* prims, const float* mats, const int32_t* prim_idx,
                               uint64_t n_prims, SceneLayout& out, std::string& err) {
    std::vector<uint32_t> order, sub_end;
    if (!visit_order(bvh, (uint32_t)n_nodes, n_prims, order, sub_end, err)) return MPT_ERR_BAD_SCENE;
    out.nested = boxes_nested(bvh, order, sub_end);
    Leaves lv;
    if (!split_leaves(bvh, prims, mats, prim_idx, n_prims, order, sub_end, lv, err)) return MPT_ERR_BAD_SCENE;
    out.use_always = lv.n_spheres <= MPT_ACCEL_MAX_ALWAYS;
    out.tri_extent = lv.tri_extent;
    std::vector<mpt_accel::Item> items;
    std::vector<uint32_t> item_dn, sphere_only_dn;
    own_tree_items(lv.dn, lv.prims, out.use_always, lv.tri_extent, items, item_dn, sphere_only_dn);
    const mpt_accel::Topology topo = mpt_accel::build_topology(items);
    const std::vector<uint32_t> first_of = reorder_prims(lv.dn, lv.prims, sphere_only_dn, item_dn, topo.item_order);
    out.acc_nodes = mpt_accel::emit(topo, items, first_of);
    out.acc_depth = topo.depth;
    if (out.use_always) out.always = always_list(lv.prims, lv.refleaf);
    out.nodes = breadth_first_nodes(lv.dn, lv.pos_to_dn, sub_end);
    out.prims = std::move(lv.prims);
    out.mats = std::move(lv.mats);
    out.refleaf = std::move(lv.refleaf);
    return MPT_OK;
}

}  // namespace mpt_layout
