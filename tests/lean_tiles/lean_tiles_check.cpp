// lean_tiles_check.cpp — the per-tile class word of the lean wave-local kernels (metalpathtracer_amd/csrc/mpt_lean_tiles.h) on the CPU.
// A stand-alone program: it builds small threaded trees in the device's layout, classifies every tile of a view and then runs a float32
// restatement of the primary path (pixel_uv, gen_primary with the IEEE division, normalize3, 1 / d, slab_hit, the sphere test) over every
// pixel of every `skip` tile with the jitters {0, 1 - 2^-24}^2, the four edge midpoints and 4096 random 24-bit pairs:
//   soundness     every chain box misses, every sphere outside `mask` is rejected, |d| <= 2 and no NaN
//   not vacuous   each case has at least the number of tiles of each class it is meant to have
//   off switches  a NaN camera, a camera outside the shrunk root / tail box, a tree without T, a chain of nine nodes, W or H that the
//                 tile counts do not cover: "general" everywhere
// `lean_tiles_check table W H nodes.bin n_nodes prims.bin n_prims <14 camera words in hex>` prints the table of that view, one word per
// line (tests/test_gpu_lean_tiles*.py compare the device's table with it).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I metalpathtracer_amd/csrc tests/lean_tiles/lean_tiles_check.cpp
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mpt_lean_tiles.h"

struct V4 {
    float x, y, z, w;
};
static float bitsf(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static const uint32_t HOLD = 0x80000000u;

struct Sph {
    float c[3], r;
};
struct Box {
    float lo[3], hi[3];
};
struct Tree {
    std::vector<V4> nodes, prims;
};
// root (node 0, internal) -> chain boxes (leaf records of one triangle each, nodes 2..) -> T (node 1, the spheres' leaf) -> end
static Tree make_tree(const std::vector<Sph>& sph, const std::vector<Box>& chain, bool with_t = true) {
    Tree t;
    const uint32_t n_nodes = 2u + (uint32_t)chain.size();
    t.nodes.resize(2 * n_nodes);
    for (const Sph& s : sph) {
        t.prims.push_back(V4{s.c[0], s.c[1], s.c[2], bitsf(0u)});
        t.prims.push_back(V4{s.r, 0.0f, 0.0f, bitsf(0u)});
        t.prims.push_back(V4{0.0f, 0.0f, 0.0f, bitsf(0u)});
    }
    Box tb = {{1e30f, 1e30f, 1e30f}, {-1e30f, -1e30f, -1e30f}};
    for (const Sph& s : sph)
        for (int a = 0; a < 3; ++a) {
            tb.lo[a] = fminf(tb.lo[a], s.c[a] - s.r);
            tb.hi[a] = fmaxf(tb.hi[a], s.c[a] + s.r);
        }
    if (sph.empty()) tb = Box{{-1.0f, -1.0f, -1.0f}, {1.0f, 1.0f, 1.0f}};
    Box rb = tb;
    for (size_t k = 0; k < chain.size(); ++k) {
        const uint32_t n = 2u + (uint32_t)k, next = k + 1 < chain.size() ? n + 1u : 1u, prim = (uint32_t)t.prims.size() / 3u;
        t.nodes[2 * n] = V4{chain[k].lo[0], chain[k].lo[1], chain[k].lo[2], bitsf(HOLD | (prim << 4))};
        t.nodes[2 * n + 1] = V4{chain[k].hi[0], chain[k].hi[1], chain[k].hi[2], bitsf(next)};
        t.prims.push_back(V4{chain[k].lo[0], chain[k].lo[1], chain[k].lo[2], bitsf(1u)});
        t.prims.push_back(V4{1.0f, 0.0f, 0.0f, bitsf(0u)});
        t.prims.push_back(V4{0.0f, 1.0f, 0.0f, bitsf(0u)});
        for (int a = 0; a < 3; ++a) {
            rb.lo[a] = fminf(rb.lo[a], chain[k].lo[a]);
            rb.hi[a] = fmaxf(rb.hi[a], chain[k].hi[a]);
        }
    }
    t.nodes[0] = V4{rb.lo[0], rb.lo[1], rb.lo[2], bitsf(chain.empty() ? 1u : 2u)};
    t.nodes[1] = V4{rb.hi[0], rb.hi[1], rb.hi[2], bitsf(n_nodes)};
    // T: the spheres' leaf record — or, without T, an internal node in its place (lean_tail_terms then finds no tail leaf)
    const uint32_t leaf = with_t && !sph.empty() ? (HOLD | (0u << 4) | ((uint32_t)sph.size() - 1u)) : 0u;
    t.nodes[2] = V4{tb.lo[0], tb.lo[1], tb.lo[2], bitsf(leaf)};
    t.nodes[3] = V4{tb.hi[0], tb.hi[1], tb.hi[2], bitsf(n_nodes)};
    return t;
}

static void norm3(float v[3]) {
    const float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int a = 0; a < 3; ++a) v[a] /= l;
}
static void cross(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// the viewport of a pinhole camera (mpt_camera_viewport's construction)
static LeanTileView make_view(const float pos[3], const float fwd[3], const float up[3], float vfov_deg, uint32_t W, uint32_t H) {
    LeanTileView v;
    const float halfH = tanf(vfov_deg * 3.14159265358979f / 180.0f * 0.5f), halfW = (float)W / (float)H * halfH;
    float w[3] = {-fwd[0], -fwd[1], -fwd[2]}, uu[3], vv[3];
    norm3(w);
    cross(up, w, uu);
    norm3(uu);
    cross(w, uu, vv);
    for (int a = 0; a < 3; ++a) {
        v.cam[a] = pos[a];
        v.vu[a] = uu[a] * (2.0f * halfW);
        v.vv[a] = -vv[a] * (2.0f * halfH);
        v.first[a] = pos[a] - w[a] - v.vu[a] * 0.5f - v.vv[a] * 0.5f;
    }
    v.W = (float)W;
    v.H = (float)H;
    v.tiles_x = (W + 7u) / 8u;
    v.tiles_y = (H + 7u) / 8u;
    return v;
}

// ---- the primary path in float32, operator for operator (mpt_kernels.h: pixel_uv, gen_primary; mpt_device.h: normalize3, slab_hit, leaf_test)
static void primary_dir(const LeanTileView& v, uint32_t px, uint32_t py, float ux, float uy, float d[3]) {
    const float uvx = ((float)px + 0.5f) / v.W, uvy = ((float)py + 0.5f) / v.H;
    const float xOff = (ux - 0.5f) / v.W, yOff = (uy - 0.5f) / v.H;
    float dir[3];
    for (int a = 0; a < 3; ++a) dir[a] = ((v.first[a] + (uvx + xOff) * v.vu[a]) + (uvy + yOff) * v.vv[a]) - v.cam[a];
    const float l2 = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
    const float inv = 1.0f / sqrtf(l2);
    for (int a = 0; a < 3; ++a) d[a] = dir[a] * inv;
}
static bool slab_hit(const V4& n0, const V4& n1, const float o[3], const float id[3], float best_t) {
    float t0 = (n0.x - o[0]) * id[0], t1 = (n1.x - o[0]) * id[0];
    float lo = fmaxf(0.0001f, id[0] < 0.0f ? t1 : t0);
    float hi = fminf(best_t, id[0] < 0.0f ? t0 : t1);
    t0 = (n0.y - o[1]) * id[1];
    t1 = (n1.y - o[1]) * id[1];
    lo = fmaxf(lo, id[1] < 0.0f ? t1 : t0);
    hi = fminf(hi, id[1] < 0.0f ? t0 : t1);
    t0 = (n0.z - o[2]) * id[2];
    t1 = (n1.z - o[2]) * id[2];
    lo = fmaxf(lo, id[2] < 0.0f ? t1 : t0);
    hi = fminf(hi, id[2] < 0.0f ? t0 : t1);
    return hi > lo;
}
static bool sphere_rejected(const V4& p0, const V4& p1, const float o[3], const float d[3]) {
    const float oc[3] = {o[0] - p0.x, o[1] - p0.y, o[2] - p0.z}, radius = p1.x;
    const float cc = (oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) - radius * radius;
    const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
    const float disc = b * b - a * cc;
    return !(!(b >= 0.0f) && disc > 0.0f);
}

struct Counts {
    uint32_t tiles = 0, general = 0, sky = 0, masked = 0, onebit = 0;
    unsigned long long rays = 0, bad = 0;
};
static uint32_t rng_state = 0x2545F491u;
static uint32_t rng24() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state >> 8;
}
static Counts check_view(const Tree& t, const LeanTileView& v, bool soundness = true) {
    Counts c;
    const uint32_t n_nodes = (uint32_t)t.nodes.size() / 2u, n_prims = (uint32_t)t.prims.size() / 3u;
    const float top = 1.0f - 0x1p-24f;
    std::vector<float> jx = {0.0f, top, 0.0f, top, 0.5f, 0.5f, 0.0f, top}, jy = {0.0f, 0.0f, top, top, 0.0f, top, 0.5f, 0.5f};
    for (int k = 0; k < 4096; ++k) {
        jx.push_back((float)rng24() * 0x1p-24f);
        jy.push_back((float)rng24() * 0x1p-24f);
    }
    for (uint32_t ty = 0; ty < v.tiles_y; ++ty)
        for (uint32_t tx = 0; tx < v.tiles_x; ++tx) {
            const uint32_t w = lean_tile_class(t.nodes.data(), n_nodes, t.prims.data(), n_prims, v, tx, ty);
            c.tiles++;
            if (!(w & MPT_LEAN_TILES_SKIP)) {
                c.general++;
                if (w != 0u) c.bad++;   // (general is the word 0)
                continue;
            }
            const uint32_t mask = w & MPT_LEAN_TILES_MASK_BITS;
            if (mask == 0u) c.sky++;
            else c.masked++;
            if (mask != 0u && (mask & (mask - 1u)) == 0u) c.onebit++;
            if (!soundness) continue;
            // the chain and T as the kernel walks them
            uint32_t A0, T = 1u;
            memcpy(&A0, &t.nodes[0].w, 4);
            uint32_t leaf;
            memcpy(&leaf, &t.nodes[2u * T].w, 4);
            const uint32_t first = (leaf & ~HOLD) >> 4, count = (leaf & 15u) + 1u;
            for (uint32_t p = 0; p < 64u; ++p)
                for (size_t q = 0; q < jx.size(); ++q) {
                    float d[3], id[3];
                    primary_dir(v, tx * 8u + (p & 7u), ty * 8u + (p >> 3), jx[q], jy[q], d);
                    c.rays++;
                    bool ok = true;
                    for (int a = 0; a < 3; ++a) {
                        ok = ok && d[a] == d[a] && fabsf(d[a]) <= MPT_LEAN_ENTRY_DMAX;
                        id[a] = 1.0f / d[a];
                    }
                    for (uint32_t n = A0; n != T && ok;) {
                        ok = !slab_hit(t.nodes[2u * n], t.nodes[2u * n + 1u], v.cam, id, INFINITY);
                        memcpy(&n, &t.nodes[2u * n + 1u].w, 4);
                    }
                    for (uint32_t k = 0; k < count && ok; ++k)
                        if (!(mask >> k & 1u)) ok = sphere_rejected(t.prims[3u * (first + k)], t.prims[3u * (first + k) + 1u], v.cam, d);
                    if (!ok) c.bad++;
                }
        }
    return c;
}

static int failures = 0;
static void expect(bool ok, const char* what, const char* name) {
    if (!ok) {
        printf("FAILED %s: %s\n", name, what);
        failures++;
    }
}
static Counts run_case(const char* name, const Tree& t, const LeanTileView& v) {
    const Counts c = check_view(t, v);
    printf("case %s: tiles %u general %u sky %u masked %u onebit %u rays %llu violations %llu\n", name, c.tiles, c.general, c.sky, c.masked,
           c.onebit, c.rays, c.bad);
    expect(c.bad == 0, "a skip tile has a ray that hits a chain box or a sphere outside the mask", name);
    return c;
}
static void run_off(const char* name, const Tree& t, const LeanTileView& v) {
    const Counts c = check_view(t, v, false);
    printf("off %s: tiles %u general %u\n", name, c.tiles, c.general);
    expect(c.tiles != 0 && c.general == c.tiles && c.bad == 0, "not general everywhere", name);
}

static int print_table(int argc, char** argv) {
    if (argc != 9 + 14) return 2;
    const uint32_t W = (uint32_t)atoi(argv[2]), H = (uint32_t)atoi(argv[3]), n_nodes = (uint32_t)atoi(argv[5]), n_prims = (uint32_t)atoi(argv[7]);
    std::vector<V4> nodes(2 * (size_t)n_nodes), prims(3 * (size_t)n_prims);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(nodes.data(), 32, n_nodes, f) != n_nodes) return 3;
    fclose(f);
    f = fopen(argv[6], "rb");
    if (!f || fread(prims.data(), 48, n_prims, f) != n_prims) return 3;
    fclose(f);
    float w[14];
    for (int k = 0; k < 14; ++k) w[k] = bitsf((uint32_t)strtoul(argv[9 + k], nullptr, 16));
    LeanTileView v;
    for (int a = 0; a < 3; ++a) {
        v.cam[a] = w[a];
        v.first[a] = w[3 + a];
        v.vu[a] = w[6 + a];
        v.vv[a] = w[9 + a];
    }
    v.W = w[12];
    v.H = w[13];
    v.tiles_x = (W + 7u) / 8u;
    v.tiles_y = (H + 7u) / 8u;
    (void)argv[8];
    for (uint32_t ty = 0; ty < v.tiles_y; ++ty)
        for (uint32_t tx = 0; tx < v.tiles_x; ++tx) printf("%08x\n", lean_tile_class(nodes.data(), n_nodes, prims.data(), n_prims, v, tx, ty));
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "table") == 0) return print_table(argc, argv);
    // scene.xml: the ground, the sphere at y = 100, the light, and the mesh's top box (bunny.obj x 10 at (-25, 0, 0))
    const std::vector<Sph> spheres = {{{0.0f, -10000.0f, 0.0f}, 10000.0f}, {{0.0f, 100.0f, 0.0f}, 40.0f}, {{0.0f, 20.0f, 0.0f}, 10.0f}};
    const Box mesh = {{-31.92f, -0.15f, -6.99f}, {-16.39f, 15.23f, 5.06f}};
    const Tree scene = make_tree(spheres, {mesh});
    const float pos[3] = {0.0f, 20.0f, 50.0f}, fwd[3] = {0.0f, 0.0f, -1.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    {
        const Counts c = run_case("default_70x45", scene, make_view(pos, fwd, up, 60.0f, 70, 45));
        expect(c.tiles == 54 && 5 * c.sky >= c.tiles, "fewer than a fifth of the 54 tiles are sky tiles", "default_70x45");
        expect(c.onebit >= 1, "no skip tile with a one-bit mask", "default_70x45");
    }
    {   // d.x = 0 in the centre column (64 wide: uvx + xOff = 0.5 is reached between pixels 31 and 32)
        const Counts c = run_case("default_64x64", scene, make_view(pos, fwd, up, 60.0f, 64, 64));
        expect(c.tiles == 64 && c.sky >= 8 && c.masked >= 8, "the centre-column case has too few skip tiles", "default_64x64");
    }
    {   // the horizon through the middle of a tile row: pitched so that it crosses row 20 of 45
        const float f2[3] = {0.0f, -0.03f, -1.0f};
        const Counts c = run_case("horizon_row", scene, make_view(pos, f2, up, 60.0f, 70, 45));
        expect(c.sky >= 9 && c.onebit >= 9 && c.general >= 1, "the horizon case lacks a class", "horizon_row");
    }
    {   // straight up and straight down
        const float fu[3] = {0.0f, 1.0f, 0.0f}, fd[3] = {0.0f, -1.0f, 0.0f}, upz[3] = {0.0f, 0.0f, -1.0f};
        const Counts cu = run_case("straight_up", scene, make_view(pos, fu, upz, 60.0f, 70, 45));
        expect(cu.sky >= 1 && cu.masked >= 1, "looking up: sky tiles and tiles of the y = 100 sphere expected", "straight_up");
        const Counts cd = run_case("straight_down", scene, make_view(pos, fd, upz, 60.0f, 70, 45));
        expect(cd.sky == 0 && cd.onebit >= 27, "looking down: at least half of the tiles see the ground alone", "straight_down");
    }
    {   // the y = 100 sphere in view
        const float f2[3] = {0.0f, 0.9f, -1.0f};
        const Counts c = run_case("sphere100_in_view", scene, make_view(pos, f2, up, 60.0f, 70, 45));
        expect(c.onebit >= 4 && c.sky >= 4, "the y = 100 sphere's tiles are missing", "sphere100_in_view");
    }
    {   // a lone triangle in the sky: a second chain node
        const Box tri = {{10.0f, 40.0f, -5.0f}, {14.0f, 44.0f, -4.0f}};
        const Counts c = run_case("triangle_in_sky", make_tree(spheres, {mesh, tri}), make_view(pos, fwd, up, 60.0f, 70, 45));
        expect(c.sky >= 9 && c.general >= 2, "the second chain node changes nothing", "triangle_in_sky");
    }
    {   // eight chain nodes: still on
        std::vector<Box> ch(8, mesh);
        const Counts c = run_case("chain_of_8", make_tree(spheres, ch), make_view(pos, fwd, up, 60.0f, 70, 45));
        expect(5 * c.sky >= c.tiles, "a chain of eight nodes must be accepted", "chain_of_8");
    }
    // ---- off switches
    {
        LeanTileView v = make_view(pos, fwd, up, 60.0f, 70, 45);
        LeanTileView n = v;
        n.cam[1] = NAN;
        run_off("nan_camera", scene, n);
        n = v;
        n.vu[0] = NAN;
        run_off("nan_viewport", scene, n);
        // above the sphere leaf's box (y <= 140) but inside the root's, which a tall chain box stretches to y = 400: entry_primary is set,
        // tail_primary is not
        const float above[3] = {0.0f, 200.0f, 50.0f};
        const Box tall = {{-60.0f, 0.0f, -60.0f}, {60.0f, 400.0f, 60.0f}};
        const Tree tall_scene = make_tree(spheres, {mesh, tall});
        {
            const LeanTileView va = make_view(above, fwd, up, 60.0f, 70, 45);
            const LeanEntry e = lean_entry_terms(tall_scene.nodes[0], tall_scene.nodes[1], 4u, va.cam[0], va.cam[1], va.cam[2]);
            const LeanTail tt = lean_tail_terms(tall_scene.nodes.data(), 4u, va.cam[0], va.cam[1], va.cam[2]);
            expect(e.entry_primary != 0u && tt.node != 0u && tt.tail_primary == 0u, "the camera is not inside the root box alone", "camera_outside_tail_box");
            run_off("camera_outside_tail_box", tall_scene, va);
        }
        const float far_[3] = {0.0f, 20.0f, 20000.0f};
        run_off("camera_outside_root_box", scene, make_view(far_, fwd, up, 60.0f, 70, 45));
        run_off("tree_without_T", make_tree(spheres, {mesh}, false), v);
        run_off("no_spheres", make_tree({}, {mesh}), v);
        std::vector<Box> ch(9, mesh);
        run_off("chain_of_9", make_tree(spheres, ch), v);
        n = v;
        n.W = 72.0f;   // a width the nine tile columns cover, but H below does not fit its rows
        n.H = 49.0f;
        run_off("size_not_covered", scene, n);
        n = v;
        n.W = 69.5f;
        run_off("width_not_whole", scene, n);
        n = v;
        n.tiles_x = 8u;
        run_off("too_few_tile_columns", scene, n);
    }
    printf(failures ? "FAILED (%d)\n" : "all passed\n", failures);
    return failures ? 1 : 0;
}
