// lean_tail_check.cpp — lean_tail_terms (metalpathtracer_amd/csrc/mpt_lean_entry.h) on the CPU, for
// tests/test_lean_tail_cpu.py and tests/test_gpu_lean_tail.py.  A stand-alone host program: the header is included, not copied.
//
//   lean_tail_check                           the off-switch at each of its edges; the implication "the guard says certain => T's slab
//                                             test says hit and its far minimum exceeds 0.0001f" in float32 over N = 2^21 origins per
//                                             accepted box; "all passed" at the end
//   lean_tail_check terms <nodes.bin> <n_nodes> <3 hex words of the camera>
//                                             nodes.bin: the device's node array, 8 float32 words per node.  Prints:
//                                             node leaf tail_primary tlo.x tlo.y tlo.z thi.x thi.y thi.z (hex words)
//
//   g++ -O2 -std=c++17 -ffp-contract=off -Imetalpathtracer_amd/csrc tests/lean_tail/lean_tail_check.cpp -o lean_tail_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mpt_lean_entry.h"

namespace {
struct V4 {
    float x, y, z, w;
};
float as_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
uint32_t as_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
const uint32_t HOLD = MPT_LEAN_LEAF_BIT;
int failures = 0;
void check(bool ok, const char* what) {
    if (!ok) {
        printf("FAILED: %s\n", what);
        failures++;
    }
}
bool is_off(const LeanTail& t) {
    bool off = t.node == 0u && t.leaf == 0u && t.tail_primary == 0u;
    for (int a = 0; a < 3; ++a) off = off && t.tlo[a] == INFINITY && t.thi[a] == -INFINITY;
    return off;
}
V4 rec(const float p[3], uint32_t link) { return V4{p[0], p[1], p[2], as_float(link)}; }
const float ROOT_LO[3] = {-10000.0f, -20000.0f, -10000.0f}, ROOT_HI[3] = {10000.0f, 140.0f, 10000.0f};
const float SUB_LO[3] = {-8.0f, 0.0f, -9.0f}, SUB_HI[3] = {9.0f, 17.0f, 6.0f};
// the tree of a scene with hoisted spheres: node 0 the root (hit -> 1, miss -> end), node 1 the other subtree (here one leaf record,
// miss -> 2), node 2 = T, the sphere leaf (three primitives from 0, miss -> end)
std::vector<V4> tree(const float lo[3], const float hi[3]) {
    const uint32_t n = 3u;
    return {rec(ROOT_LO, 1u), rec(ROOT_HI, n), rec(SUB_LO, HOLD | (3u << 4) | 1u), rec(SUB_HI, 2u), rec(lo, HOLD | (0u << 4) | 2u), rec(hi, n)};
}

void edges() {
    const float lo[3] = {-10000.0f, -20000.0f, -10000.0f}, hi[3] = {10000.0f, 140.0f, 10000.0f}, cam[3] = {0.0f, 20.0f, 50.0f};
    const float m = MPT_LEAN_ENTRY_M;
    std::vector<V4> nd = tree(lo, hi);
    LeanTail t = lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2]);
    check(t.node == 2u && t.leaf == (HOLD | 2u) && t.tail_primary == 1u, "the accepted tree: T = 2, its leaf word, the camera inside");
    for (int a = 0; a < 3; ++a) check(t.tlo[a] == lo[a] + 2.0f * m && t.thi[a] == hi[a] - 2.0f * m && t.tlo[a] > lo[a] && t.thi[a] < hi[a], "tlo = lo + 2m, thi = hi - 2m");
    check(MPT_NODE_TAIL >= 3u && MPT_NODE_TAIL < HOLD, "the marker ends a walk and is no leaf word");
    {   // the root is a leaf record
        std::vector<V4> one = {rec(lo, HOLD | 1u), rec(hi, 1u)};
        check(is_off(lean_tail_terms(one.data(), 1u, cam[0], cam[1], cam[2])), "the root is a leaf record");
        check(is_off(lean_tail_terms(one.data(), 0u, cam[0], cam[1], cam[2])), "no nodes");
        check(is_off(lean_tail_terms((const V4*)nullptr, 0u, cam[0], cam[1], cam[2])), "no tree");
    }
    {   // T internal: the root's last child is a chain node (node 2 internal with children 3, 4)
        const uint32_t n = 5u;
        std::vector<V4> v = {rec(ROOT_LO, 1u), rec(ROOT_HI, n), rec(SUB_LO, HOLD | (3u << 4)), rec(SUB_HI, 2u), rec(lo, 3u), rec(hi, n),
                             rec(lo, HOLD | 0u), rec(hi, 4u), rec(lo, HOLD | (1u << 4)), rec(hi, n)};
        check(is_off(lean_tail_terms(v.data(), n, cam[0], cam[1], cam[2])), "T is an internal node");
    }
    {   // T = 0: A0 = 0, and a miss link back to the root
        std::vector<V4> v = tree(lo, hi);
        v[0].w = as_float(0u);
        check(is_off(lean_tail_terms(v.data(), 3u, cam[0], cam[1], cam[2])), "A0 == 0");
        v = tree(lo, hi);
        v[3].w = as_float(0u);
        check(is_off(lean_tail_terms(v.data(), 3u, cam[0], cam[1], cam[2])), "a miss link to node 0");
        v = tree(lo, hi);
        v[3].w = as_float(1u);
        check(is_off(lean_tail_terms(v.data(), 3u, cam[0], cam[1], cam[2])), "miss links that never end");
        v = tree(lo, hi);
        v[0].w = as_float(3u);
        check(is_off(lean_tail_terms(v.data(), 3u, cam[0], cam[1], cam[2])), "A0 == n_nodes");
        check(is_off(lean_tail_terms(v.data(), MPT_NODE_TAIL, cam[0], cam[1], cam[2])), "n_nodes reaches the marker");
    }
    {   // a root with one child: A0 itself is T
        std::vector<V4> v = {rec(ROOT_LO, 1u), rec(ROOT_HI, 2u), rec(lo, HOLD | 2u), rec(hi, 2u)};
        t = lean_tail_terms(v.data(), 2u, cam[0], cam[1], cam[2]);
        check(t.node == 1u && t.leaf == (HOLD | 2u), "A0 == T is accepted");
    }
    for (int a = 0; a < 3; ++a) {
        float l[3] = {lo[0], lo[1], lo[2]}, h[3] = {hi[0], hi[1], hi[2]};
        l[a] = 1.0f;
        h[a] = nextafterf(1.0f + 4.0f * m, 0.0f);
        nd = tree(l, h);
        check(is_off(lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2])), "a box thinner than 4m");
        h[a] = 1.0f + 4.0f * m;
        float c[3] = {cam[0], cam[1], cam[2]};
        c[a] = 1.0f + 2.0f * m;
        nd = tree(l, h);
        t = lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]);
        check(t.node == 2u && t.tail_primary == 1u && t.tlo[a] == t.thi[a], "a box exactly 4m thick is accepted, one origin plane inside");
        l[a] = 1.6e7f;
        h[a] = 1.7e7f;
        nd = tree(l, h);
        check(is_off(lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2])), "planes at 1.6e7, where an ulp exceeds 2m");
        l[a] = lo[a];
        h[a] = NAN;
        nd = tree(l, h);
        check(is_off(lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2])), "a NaN hi plane");
        l[a] = NAN;
        h[a] = hi[a];
        nd = tree(l, h);
        check(is_off(lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2])), "a NaN lo plane");
        l[a] = -INFINITY;
        nd = tree(l, h);
        check(is_off(lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2])), "an infinite plane");
    }
    nd = tree(lo, hi);
    t = lean_tail_terms(nd.data(), 3u, cam[0], cam[1], cam[2]);
    for (int a = 0; a < 3; ++a) {
        float c[3] = {cam[0], cam[1], cam[2]};
        c[a] = t.tlo[a];
        check(lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]).tail_primary == 1u, "camera exactly on tlo is inside");
        c[a] = nextafterf(t.tlo[a], -INFINITY);
        check(lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]).tail_primary == 0u && lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]).node == 2u,
              "camera one ulp below tlo is outside (the item stays on)");
        c[a] = t.thi[a];
        check(lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]).tail_primary == 1u, "camera exactly on thi is inside");
        c[a] = nextafterf(t.thi[a], INFINITY);
        check(lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]).tail_primary == 0u, "camera one ulp above thi is outside");
        c[a] = NAN;
        check(lean_tail_terms(nd.data(), 3u, c[0], c[1], c[2]).tail_primary == 0u, "a NaN camera is outside");
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
float uniform01() { return (float)(next_u64() >> 40) * 0x1p-24f; }
float between(float a, float b) {
    const float v = a + (b - a) * uniform01();
    return v < a ? a : (v > b ? b : v);
}
float direction_component() {
    const float sign = (next_u64() & 1u) ? -1.0f : 1.0f;
    switch (next_u64() % 10u) {
    case 0: return 0.0f;
    case 1: return -0.0f;
    case 2: return sign * as_float(1u + (uint32_t)(next_u64() % 0x7FFFFFu));   // a denormal
    case 3: return sign * 1e-30f * uniform01();                                  // tiny
    case 4: return sign * 2.0f;
    case 5: return sign * nextafterf(2.0f, 0.0f);
    case 6: return sign * ((next_u64() & 1u) ? nextafterf(2.0f, 3.0f) : INFINITY);   // past the guard's bound: such a ray is not certain
    default: return sign * uniform01();
    }
}
// the box test of closest_hit_resume (slab_hit, mpt_device.h) on T's planes with id = the IEEE 1 / d; *far_min = the minimum of the far terms
bool slab_hit(const float lo[3], const float hi[3], const float o[3], const float d[3], float best_t, float* far_min) {
    float tlo = 0.0001f, thi = best_t, fm = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const float id = 1.0f / d[a];
        const float t0 = (lo[a] - o[a]) * id, t1 = (hi[a] - o[a]) * id;
        tlo = fmaxf(tlo, id < 0.0f ? t1 : t0);
        thi = fminf(thi, id < 0.0f ? t0 : t1);
        fm = fminf(fm, id < 0.0f ? t0 : t1);
    }
    *far_min = fm;
    return thi > tlo;
}
struct Tally {
    uint64_t n, inside, certain, bad;
    float least_far;
};
Tally implication(const float lo[3], const float hi[3], uint64_t n) {
    const std::vector<V4> nd = tree(lo, hi);
    const LeanTail e = lean_tail_terms(nd.data(), 3u, 0.0f, 0.0f, 0.0f);
    Tally t = {n, 0, 0, 0, INFINITY};
    if (e.node != 2u) return t;   // (refused: the caller asserts the counts)
    for (uint64_t k = 0; k < n; ++k) {
        float o[3], d[3];
        const unsigned where = (unsigned)(next_u64() % 10u);   // 0..5 inside the shrunk box, 6 on its faces, 7 between the boxes, 8 on T's faces, 9 around it
        for (int a = 0; a < 3; ++a) {
            if (where <= 5u) o[a] = between(e.tlo[a], e.thi[a]);
            else if (where == 6u) o[a] = (next_u64() & 1u) ? e.tlo[a] : ((next_u64() & 1u) ? e.thi[a] : between(e.tlo[a], e.thi[a]));
            else if (where == 7u) o[a] = (next_u64() & 1u) ? between(lo[a], e.tlo[a]) : between(e.thi[a], hi[a]);
            else if (where == 8u) o[a] = (next_u64() & 1u) ? lo[a] : hi[a];
            else o[a] = between(lo[a] - 1.0f, hi[a] + 1.0f);
            d[a] = direction_component();
        }
        if (k % 7u == 0u) {   // a unit vector, as normalize3 leaves it
            const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (l > 0.0f && l < INFINITY)
                for (int a = 0; a < 3; ++a) d[a] /= l;
        }
        bool in = true;
        for (int a = 0; a < 3; ++a) in = in && e.tlo[a] <= o[a] && o[a] <= e.thi[a];
        const bool d_ok = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2])) <= MPT_LEAN_ENTRY_DMAX;
        t.inside += in ? 1u : 0u;
        if (!(in && d_ok)) continue;
        t.certain++;
        const float best_t = (k & 1u) ? INFINITY : nextafterf(0.0001f, 1.0f) * (1.0f + 3.0f * uniform01());   // +inf, or a t that passed `tt > 0.0001f`
        float far_min;
        const bool hit = slab_hit(lo, hi, o, d, best_t, &far_min);
        if (!(hit && far_min > 0.0001f)) t.bad++;
        if (far_min < t.least_far) t.least_far = far_min;
    }
    return t;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 7 && strcmp(argv[1], "terms") == 0) {
        const uint32_t n_nodes = (uint32_t)strtoul(argv[3], nullptr, 10);
        std::vector<V4> nd((size_t)n_nodes * 2u);
        FILE* f = fopen(argv[2], "rb");
        if (!f || fread(nd.data(), sizeof(V4), nd.size(), f) != nd.size()) {
            fprintf(stderr, "cannot read %u nodes from %s\n", n_nodes, argv[2]);
            return 2;
        }
        fclose(f);
        float cam[3];
        for (int k = 0; k < 3; ++k) cam[k] = as_float((uint32_t)strtoul(argv[4 + k], nullptr, 16));
        const LeanTail t = lean_tail_terms(nd.data(), n_nodes, cam[0], cam[1], cam[2]);
        printf("%u %08x %u %08x %08x %08x %08x %08x %08x\n", t.node, t.leaf, t.tail_primary, as_bits(t.tlo[0]), as_bits(t.tlo[1]), as_bits(t.tlo[2]), as_bits(t.thi[0]),
               as_bits(t.thi[1]), as_bits(t.thi[2]));
        return 0;
    }
    if (argc != 1) {
        fprintf(stderr, "usage: %s [terms <nodes.bin> <n_nodes> <3 hex words>]\n", argv[0]);
        return 2;
    }
    edges();
    printf("edges: %d failures\n", failures);
    const float boxes[4][2][3] = {{{-10000.0f, -20000.0f, -10000.0f}, {10000.0f, 140.0f, 10000.0f}},   // scene.xml's sphere leaf
                                  {{-1.0f, -1.0f, -1.0f}, {1.0f, 1.0f, 1.0f}},
                                  {{5.0f, -3.0f, 100.0f}, {5.0625f, 7.0f, 1000.0f}},                   // thin in x, away from the origin
                                  {{-0.25f, 1000.0f, -4000.0f}, {0.25f, 1004.0f, -3000.0f}}};
    const uint64_t N = 1ull << 21;
    for (int b = 0; b < 4; ++b) {
        const Tally t = implication(boxes[b][0], boxes[b][1], N);
        printf("box %d: %llu origins, %llu inside the shrunk box, %llu certain, %llu failures, least far term %.3e\n", b, (unsigned long long)t.n,
               (unsigned long long)t.inside, (unsigned long long)t.certain, (unsigned long long)t.bad, (double)t.least_far);
        check(t.n >= 1000000u, "at least 10^6 origins per box");
        check(2u * t.inside >= t.n, "at least half of the origins are inside the shrunk box");
        check(5u * t.certain >= t.n, "the guard says certain for a good part of them");
        check(t.bad == 0u, "guard => hit, far minimum > 0.0001f");
        check(t.least_far > 0.0001f, "least far term > 0.0001f");
    }
    if (failures == 0) printf("all passed\n");
    return failures == 0 ? 0 : 1;
}
