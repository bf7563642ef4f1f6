// lean_entry_check.cpp — lean_entry_terms (metalpathtracer_amd/csrc/mpt_lean_entry.h) on the CPU, for tests/test_lean_entry_cpu.py and
// tests/test_gpu_lean_entry.py.  A stand-alone host program: the header is included, not copied.
//
//   lean_entry_check                          the off-switch at each of its edges, then the implication "the guard says skip => the
//                                             root's slab test says hit and its far minimum exceeds 0.0001f" in float32 over N origins
//                                             per box (N = 2^21; the third line of output gives the counts); "all passed" at the end
//   lean_entry_check terms <8 hex words of node 0> <n_nodes> <3 hex words of the camera>
//                                             prints: entry entry_primary ilo.x ilo.y ilo.z ihi.x ihi.y ihi.z (floats as hex words)
//
//   g++ -O2 -std=c++17 -ffp-contract=off -Imetalpathtracer_amd/csrc tests/lean_entry/lean_entry_check.cpp -o lean_entry_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
const uint32_t HOLD = 0x80000000u;   // MPT_NODE_HOLD: the hit link of a leaf record
int failures = 0;
void check(bool ok, const char* what) {
    if (!ok) {
        printf("FAILED: %s\n", what);
        failures++;
    }
}
bool is_off(const LeanEntry& e) {
    bool off = e.entry == 0u && e.entry_primary == 0u;
    for (int a = 0; a < 3; ++a) off = off && e.ilo[a] == INFINITY && e.ihi[a] == -INFINITY;
    return off;
}
LeanEntry terms(const float lo[3], const float hi[3], uint32_t A0, uint32_t n_nodes, const float cam[3]) {
    const V4 n0 = {lo[0], lo[1], lo[2], as_float(A0)}, n1 = {hi[0], hi[1], hi[2], as_float(n_nodes)};
    return lean_entry_terms(n0, n1, n_nodes, cam[0], cam[1], cam[2]);
}

void edges() {
    const float lo[3] = {-10000.0f, -20000.0f, -10000.0f}, hi[3] = {10000.0f, 60.0f, 10000.0f}, cam[3] = {0.0f, 20.0f, 50.0f};
    const float m = MPT_LEAN_ENTRY_M;
    LeanEntry e = terms(lo, hi, 1u, 9u, cam);
    check(e.entry == 1u && e.entry_primary == 1u, "the accepted box: entry and entry_primary are A0");
    for (int a = 0; a < 3; ++a) check(e.ilo[a] == lo[a] + 2.0f * m && e.ihi[a] == hi[a] - 2.0f * m && e.ilo[a] > lo[a] && e.ihi[a] < hi[a], "ilo = lo + 2m, ihi = hi - 2m");
    check(is_off(terms(lo, hi, HOLD | (0u << 4) | 1u, 1u, cam)), "the root is a leaf record");
    check(is_off(terms(lo, hi, 9u, 9u, cam)), "A0 == n_nodes");
    check(is_off(terms(lo, hi, 0u, 9u, cam)), "A0 == 0");
    check(terms(lo, hi, 8u, 9u, cam).entry == 8u, "A0 == n_nodes - 1 is accepted");
    for (int a = 0; a < 3; ++a) {
        float l[3] = {lo[0], lo[1], lo[2]}, h[3] = {hi[0], hi[1], hi[2]};
        l[a] = 1.0f;
        h[a] = nextafterf(1.0f + 4.0f * m, 0.0f);
        check(is_off(terms(l, h, 1u, 9u, cam)), "a box thinner than 4m");
        h[a] = 1.0f + 4.0f * m;
        float c[3] = {cam[0], cam[1], cam[2]};
        c[a] = 1.0f + 2.0f * m;
        e = terms(l, h, 1u, 9u, c);
        check(e.entry == 1u && e.entry_primary == 1u && e.ilo[a] == e.ihi[a], "a box exactly 4m thick is accepted, one origin plane inside");
        l[a] = 1.6e7f;
        h[a] = 1.7e7f;
        check(is_off(terms(l, h, 1u, 9u, cam)), "planes at 1.6e7, where an ulp exceeds 2m");
        l[a] = lo[a];
        h[a] = NAN;
        check(is_off(terms(l, h, 1u, 9u, cam)), "a NaN hi plane");
        l[a] = NAN;
        h[a] = hi[a];
        check(is_off(terms(l, h, 1u, 9u, cam)), "a NaN lo plane");
        l[a] = -INFINITY;
        check(is_off(terms(l, h, 1u, 9u, cam)), "an infinite plane");
    }
    e = terms(lo, hi, 1u, 9u, cam);
    for (int a = 0; a < 3; ++a) {
        float c[3] = {cam[0], cam[1], cam[2]};
        c[a] = e.ilo[a];
        check(terms(lo, hi, 1u, 9u, c).entry_primary == 1u, "camera exactly on ilo is inside");
        c[a] = nextafterf(e.ilo[a], -INFINITY);
        check(terms(lo, hi, 1u, 9u, c).entry_primary == 0u && terms(lo, hi, 1u, 9u, c).entry == 1u, "camera one ulp below ilo is outside (bounce rays stay on)");
        c[a] = e.ihi[a];
        check(terms(lo, hi, 1u, 9u, c).entry_primary == 1u, "camera exactly on ihi is inside");
        c[a] = nextafterf(e.ihi[a], INFINITY);
        check(terms(lo, hi, 1u, 9u, c).entry_primary == 0u, "camera one ulp above ihi is outside");
        c[a] = NAN;
        check(terms(lo, hi, 1u, 9u, c).entry_primary == 0u, "a NaN camera is outside");
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
    case 6: return sign * ((next_u64() & 1u) ? nextafterf(2.0f, 3.0f) : INFINITY);   // past the guard's bound: such a ray is not skipped
    default: return sign * uniform01();
    }
}
// the trip of closest_hit_resume's box loop (mpt_device.h) on node 0 with id = the IEEE 1 / d; *far_min = the minimum of the far terms
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
    uint64_t n, inside, skipped, bad;
    float least_far;
};
Tally implication(const float lo[3], const float hi[3], uint64_t n) {
    const float cam[3] = {0.0f, 0.0f, 0.0f};
    const LeanEntry e = terms(lo, hi, 1u, 3u, cam);
    Tally t = {n, 0, 0, 0, INFINITY};
    if (e.entry != 1u) return t;   // (refused: the caller asserts the counts)
    for (uint64_t k = 0; k < n; ++k) {
        float o[3], d[3];
        const unsigned where = (unsigned)(next_u64() % 10u);   // 0..5 inside the shrunk box, 6 on its faces, 7 between the boxes, 8 on the root's faces, 9 around it
        for (int a = 0; a < 3; ++a) {
            if (where <= 5u) o[a] = between(e.ilo[a], e.ihi[a]);
            else if (where == 6u) o[a] = (next_u64() & 1u) ? e.ilo[a] : ((next_u64() & 1u) ? e.ihi[a] : between(e.ilo[a], e.ihi[a]));
            else if (where == 7u) o[a] = (next_u64() & 1u) ? between(lo[a], e.ilo[a]) : between(e.ihi[a], hi[a]);
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
        for (int a = 0; a < 3; ++a) in = in && e.ilo[a] <= o[a] && o[a] <= e.ihi[a];
        const bool d_ok = fmaxf(fmaxf(fabsf(d[0]), fabsf(d[1])), fabsf(d[2])) <= MPT_LEAN_ENTRY_DMAX;
        t.inside += in ? 1u : 0u;
        if (!(in && d_ok)) continue;
        t.skipped++;
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
    if (argc == 14 && strcmp(argv[1], "terms") == 0) {
        uint32_t w[12];
        for (int k = 0; k < 8; ++k) w[k] = (uint32_t)strtoul(argv[2 + k], nullptr, 16);
        const uint32_t n_nodes = (uint32_t)strtoul(argv[10], nullptr, 10);
        for (int k = 0; k < 3; ++k) w[8 + k] = (uint32_t)strtoul(argv[11 + k], nullptr, 16);
        const V4 n0 = {as_float(w[0]), as_float(w[1]), as_float(w[2]), as_float(w[3])}, n1 = {as_float(w[4]), as_float(w[5]), as_float(w[6]), as_float(w[7])};
        const LeanEntry e = lean_entry_terms(n0, n1, n_nodes, as_float(w[8]), as_float(w[9]), as_float(w[10]));
        printf("%u %u %08x %08x %08x %08x %08x %08x\n", e.entry, e.entry_primary, as_bits(e.ilo[0]), as_bits(e.ilo[1]), as_bits(e.ilo[2]), as_bits(e.ihi[0]),
               as_bits(e.ihi[1]), as_bits(e.ihi[2]));
        return 0;
    }
    if (argc != 1) {
        fprintf(stderr, "usage: %s [terms <8 hex words> <n_nodes> <3 hex words>]\n", argv[0]);
        return 2;
    }
    edges();
    printf("edges: %d failures\n", failures);
    const float boxes[4][2][3] = {{{-10000.0f, -20000.0f, -10000.0f}, {10000.0f, 60.0f, 10000.0f}},   // scene.xml's, with its ground sphere
                                  {{-1.0f, -1.0f, -1.0f}, {1.0f, 1.0f, 1.0f}},
                                  {{5.0f, -3.0f, 100.0f}, {5.0625f, 7.0f, 1000.0f}},                  // thin in x, away from the origin
                                  {{-0.25f, 1000.0f, -4000.0f}, {0.25f, 1004.0f, -3000.0f}}};
    const uint64_t N = 1ull << 21;
    for (int b = 0; b < 4; ++b) {
        const Tally t = implication(boxes[b][0], boxes[b][1], N);
        printf("box %d: %llu origins, %llu inside the shrunk box, %llu skipped, %llu failures, least far term %.3e\n", b, (unsigned long long)t.n,
               (unsigned long long)t.inside, (unsigned long long)t.skipped, (unsigned long long)t.bad, (double)t.least_far);
        check(t.n >= 1000000u, "at least 10^6 origins per box");
        check(2u * t.inside >= t.n, "at least half of the origins are inside the shrunk box");
        check(5u * t.skipped >= t.n, "the guard says skip for a good part of them");
        check(t.bad == 0u, "guard => hit, far minimum > 0.0001f");
        check(t.least_far > 0.0001f, "least far term > 0.0001f");
    }
    if (failures == 0) printf("all passed\n");
    return failures == 0 ? 0 : 1;
}
