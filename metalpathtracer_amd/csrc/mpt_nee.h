// mpt_nee.h — next-event estimation inside the path loop (included by mpt_hip.hip after mpt_direct.h):
//   k_nee<WALK>   one lane per pixel: the pixel's samples in turn, a light sample with a shadow ray at every Lambert vertex, the light a
//                 bounce finds weighted against it (power heuristic), the HDR sum updated in registers in sample order
//   k_nee_cone<WALK>  the same render with a sphere light sampled in the cone it subtends (MPT_LIGHT_SAMPLING_CONE): its light sample and
//                 the weight of a sphere light a bounce finds change, nothing else; both kernels are nee_render<WALK, CONE>
//   the round     its pieces, written once: the pinned pass constants (nee_consts), the lane's pixel and path state, regeneration,
//                 the closest-hit step, the weight of an emitter a bounce finds (nee_emitter_weight), the MIS-weighted factor of a
//                 light sample (nee_light_factor), the shadow step, the clamped sample value, the totals.  nee_render,
//                 nee_adaptive_render (mpt_nee_adaptive.h) and nee_ris_render (mpt_ris.h) are loops over them; the shading of a
//                 round (sky, material, the three BSDF branches) stands in each loop, because as a shared piece it rescheduled them
// The estimator is specified exactly in include/mpt.h (mpt_nee_params) and restated in numpy in tests/nee_ref.py; DESIGN.md §17 has the
// lane mapping, the registers, the measured times and how the pieces are passed so that the three renders compile to the registers
// they had as three bodies.  Nothing here edits a kernel or a device function of the plain render: the walks
// (closest_hit_resume, closest_hit_ordered, any_hit_ref, any_hit_own), finish_hit, the Philox block and the light table are the tested ones.
// The tile prologue and the shadow walk's dispatch are mpt_ao.h's (tile_walk, any_hit), the light sample is mpt_direct.h's (table_search,
// light_sample): what is written here is the path loop, the MIS weights and the weight of an emitter a bounce finds.
#pragma once
#include "mpt_direct.h"

struct NeePass {
    float4* sum;                 // the HDR sum (W * H rgba): read once and written once per pixel
    unsigned long long* totals;  // += paths, closest-hit queries, shadow rays, shadow rays occluded (one atomic each per wave that has any)
    const float4* lights;        // the light table of mpt_direct.h: MPT_LIGHT_F4 float4 per light, ascending caller id
    const float* cdf;
    const int32_t* ids;          // the caller ids of the table's lights (ascending): what an emitter a bounce hits is looked up in
    uint32_t n_lights;
    F3 cam, first, vu, vv;
    float fW, fH;                // uniforms.screenSize, as gen_primary divides by it
    uint32_t W, H;
    uint32_t sample_begin, sample_count;
    uint32_t seed_lo, seed_hi;
    int32_t bsdf_mode, max_depth;
    uint32_t primitive_count;    // uniforms.primitiveCount (the material guard of shade_bounce)
    float clamp;                 // per-sample, per-channel upper clamp (+inf: none)
};

// Lane mapping.  The tile grid of k_ao / k_direct: a workgroup of four waves takes a 16 x 16 pixel block, each wave one 8 x 8 tile, ONE
// LANE PER PIXEL.  A lane runs its pixel's samples one after the other with path regeneration: a lane whose path has ended starts its
// next sample at the head of the next round, so the wave stays full until its pixels run out of samples, and leaves when no lane holds a
// ray.  A round is one closest-hit walk for the lanes that hold a ray, the shading of what they found, and one any-hit walk for the
// lanes whose vertex drew a light sample (skipped when there is none).  The pixel's running sum lives in the lane's registers from
// the first round to the last: no result slots, no resolve, no atomics on the image, and no value depends on which lane has which pixel.

// ---- the pieces of the round: nee_render below, nee_adaptive_render (mpt_nee_adaptive.h) and nee_ris_render (mpt_ris.h) are loops over these
// How values cross a piece's boundary decides the registers and the schedule of the renders (DESIGN.md §17 "One round"): a piece takes
// values and returns values — the pass by value into nee_consts only, the path never by reference, no flag inside a struct — and the
// renders compute and initialise in the order their one body did.

// What the rounds and the end need from the pass, in VECTOR registers (an empty asm makes the value opaque, as in k_direct): the two
// walks hold the scalar file.  The camera goes with them: a regeneration needs its fourteen words in any round.
struct NeeConsts {
    float4* sum;
    const float4* lights;
    const float* cdf;
    const int32_t* ids;
    uint32_t last, sample_begin, prim_count, search_steps;
    int32_t bsdf_mode, max_depth;
    float clamp_hi, fW, fH;
    F3 cam, first, vu, vv;
    uint32_t have_lights;
    uint32_t seed_lo, seed_hi;   // not pinned: Philox's key, which lives in scalar registers
};
__device__ __forceinline__ NeeConsts nee_consts(NeePass P) {   // (the pass by value, the pins on locals: either way else moves the renders' registers)
    float4* sum = P.sum;
    const float4* lights = P.lights;
    const float* cdf = P.cdf;
    const int32_t* ids = P.ids;
    uint32_t last = P.n_lights - 1u, sample_begin = P.sample_begin, prim_count = P.primitive_count;
    uint32_t search_steps = table_search_steps(P.n_lights);
    int32_t bsdf_mode = P.bsdf_mode, max_depth = P.max_depth;
    float clamp_hi = P.clamp, fW = P.fW, fH = P.fH;
    F3 cam = P.cam, first = P.first, vu = P.vu, vv = P.vv;
    uint32_t have_lights = P.n_lights != 0u ? 1u : 0u;
    asm volatile("" : "+v"(sum), "+v"(lights), "+v"(cdf), "+v"(ids), "+v"(last), "+v"(sample_begin), "+v"(prim_count), "+v"(search_steps));
    asm volatile("" : "+v"(bsdf_mode), "+v"(max_depth), "+v"(clamp_hi), "+v"(fW), "+v"(fH), "+v"(have_lights));
    asm volatile("" : "+v"(cam.x), "+v"(cam.y), "+v"(cam.z), "+v"(first.x), "+v"(first.y), "+v"(first.z));
    asm volatile("" : "+v"(vu.x), "+v"(vu.y), "+v"(vu.z), "+v"(vv.x), "+v"(vv.y), "+v"(vv.z));
    return NeeConsts{sum, lights, cdf, ids, last, sample_begin, prim_count, search_steps, bsdf_mode, max_depth, clamp_hi, fW, fH, cam, first, vu, vv,
                     have_lights, P.seed_lo, P.seed_hi};
}
// The lane's pixel: (tx0 + lane % 8, ty0 + lane / 8) of the wave's tile.
struct NeePixel {
    uint32_t px, py;
    bool inside;
    uint32_t pixel;              // 0 outside the image
};
__device__ __forceinline__ NeePixel nee_pixel(const TileWalk& T, uint32_t W, uint32_t H) {
    NeePixel X;
    X.px = T.tx0 + (T.lane & 7u);
    X.py = T.ty0 + (T.lane >> 3);
    X.inside = X.px < W && X.py < H;
    X.pixel = X.inside ? X.py * W + X.px : 0u;
    return X;
}
// The lane's running path.  has_ray and sampled stay plain flags of the render, and the struct is never passed by reference: either
// moves the registers of the renders (DESIGN.md §17 "One round").
struct NeePath {
    uint32_t sample;             // Philox counter word 1 of the running path
    F3 o, d, thr, L;
    float La, pb;                // pb: the bounce's pdf at the vertex before, per solid angle
    uint32_t b;
};
// Path regeneration: sample `s` of the pixel (uvx, uvy: its pixel_uv) starts with the primary ray of gen_primary (philox).
__device__ __forceinline__ NeePath nee_regenerate(const NeeConsts& K, uint32_t pixel, float uvx, float uvy, uint32_t s) {
    NeePath p;
    p.sample = K.sample_begin + s;
    const U4 r = philox4x32_10<true>(pixel, p.sample, 0xFFFFFFFFu, 0u, K.seed_lo, K.seed_hi);
    const float xOff = (u01(r.x) - 0.5f) / K.fW, yOff = (u01(r.y) - 0.5f) / K.fH;
    const F3 dir = (K.first + (uvx + xOff) * K.vu + (uvy + yOff) * K.vv) - K.cam;
    p.o = K.cam;
    p.d = normalize3(dir);
    p.thr = f3(1.0f, 1.0f, 1.0f);
    p.L = f3(0.0f, 0.0f, 0.0f);
    p.La = 0.0f;
    p.pb = 0.0f;
    p.b = 0u;
    return p;
}
// The closest hit of the lanes that hold a ray: the ordered walk, or closest_hit with the idle lanes done before the first node.
struct NeeHit {
    float t;
    int prim;                    // < 0: the sky
};
template <int WALK>
__device__ __forceinline__ NeeHit nee_closest(const SceneDev& sc, const AccelDev& ac, const TileWalk& T, F3 o, F3 d, bool has_ray, WorkCount& wc) {
    float t;
    int prim;
    if (WALK == MPT_AO_OWN) {
        uint32_t flags;
        closest_hit_ordered<false>(ac, sc, T.lds, T.st, o, d, has_ray, t, prim, flags, wc);
    } else {
        uint32_t node = has_ray ? 0u : sc.n_nodes;
        t = INFINITY;
        prim = -1;
        closest_hit_resume<false, WALK == MPT_AO_REF_ALL_LDS, false>(sc, T.lds, o, d, node, t, prim, 0xFFFFFFFFu, wc);
    }
    return NeeHit{t, prim};
}
// The weight of the light a bounce found (primitive h, at t along d from o): in full, unless the vertex before drew a light sample that
// could have found it too — then the power heuristic of the bounce's pdf pb against the sample's, both per solid angle.
template <bool CONE>
__device__ __forceinline__ float nee_emitter_weight(const NeeConsts& K, const HitInfo& h, F3 o, F3 d, float t, float pb) {
    float w = 1.0f;
    // the smallest k with id <= ids[k]
    const uint32_t lo = table_search(K.last, K.search_steps, [&](uint32_t mid) { return h.orig_id <= K.ids[mid]; });
    if (K.ids[lo] == h.orig_id) {
        const float4 L0 = K.lights[MPT_LIGHT_F4 * lo], L3 = K.lights[MPT_LIGHT_F4 * lo + 3u];
        if (L0.w != 0.0f || h.front) {   // (a sphere emits outward only where it is sampled)
            if (!CONE || L0.w != 0.0f) {
                const float cos_l = -dot3(h.normal, d);
                const float pl = (t * t) / (cos_l * L3.w);
                const float q = pl / pb;
                w = 1.0f / (1.0f + q * q);
            } else {   // the solid-angle pdf of the cone from this ray's origin: neither t nor cos_l enters
                const float4 L1 = K.lights[MPT_LIGHT_F4 * lo + 1u];
                float dc2, omc, J;
                if (cone_cap(f3(L0.x, L0.y, L0.z) - o, L1.x, L3.w, dc2, omc, J)) {
                    const float q = 1.0f / (J * pb);
                    w = 1.0f / (1.0f + q * q);
                }
            }
        }
    }
    return w;
}
// The estimator's factor of a light sample drawn at a Lambert vertex, times its weight against the bounce's pdf cos_s / pi (power
// heuristic), both per solid angle.  The only copy: the one draw below and every candidate of ris_pick<CONE, true> (mpt_ris.h).
template <bool CONE>
__device__ __forceinline__ float nee_light_factor(LightSample ls) {
    if (!CONE || ls.tri) {
        const float g = (ls.cos_s * ls.cos_l) / ls.d2;
        const float pl = ls.d2 / (ls.cos_l * ls.inv_pdf);
        const float q = (ls.cos_s * 0.31830987f) / pl;
        return (g * ls.inv_pdf) * (1.0f / (1.0f + q * q));
    }
    const float q = (ls.cos_s * 0.31830987f) * ls.J;
    return (ls.cos_s * ls.J) * (1.0f / (1.0f + q * q));
}
// The shadow rays of this round's vertices, from the bounce rays' origins o (the walk is skipped when no lane has one): the path's L
// with what arrived.
template <int WALK>
__device__ __forceinline__ F3 nee_shadow_step(const SceneDev& sc, const AccelDev& ac, const TileWalk& T, F3 o, F3 L, bool shadow, F3 wi, float tmax, F3 C,
                                              unsigned long long& n_shadow, unsigned long long& n_occluded) {
    if (__ballot(shadow) == 0ull) return L;   // (wave-uniform)
    const bool hit = any_hit<WALK>(sc, ac, T, o, wi, tmax, shadow);
    if (shadow) {
        n_shadow += 1ull;
        if (hit) {
            n_occluded += 1ull;
        } else {
            L.x += C.x;
            L.y += C.y;
            L.z += C.z;
        }
    }
    return L;
}
// The per-sample value of a path that has ended: clamped (rgb), with the clamped alpha.
__device__ __forceinline__ float4 nee_sample_value(const NeeConsts& K, F3 L, float La) {
    return make_float4(L.x > 0.0f ? fminf(L.x, K.clamp_hi) : 0.0f, L.y > 0.0f ? fminf(L.y, K.clamp_hi) : 0.0f,
                       L.z > 0.0f ? fminf(L.z, K.clamp_hi) : 0.0f, clamp01(La));
}
// The wave's four counters into the pass's totals: one atomic each, for those that are not zero.
__device__ __forceinline__ void nee_add_totals(unsigned long long* totals, uint32_t lane, uint32_t paths, unsigned long long n_rays,
                                               unsigned long long n_shadow, unsigned long long n_occluded) {
    unsigned long long n_paths = paths;
    for (int off = 32; off > 0; off >>= 1) {
        n_paths += __shfl_down(n_paths, off);
        n_rays += __shfl_down(n_rays, off);
        n_shadow += __shfl_down(n_shadow, off);
        n_occluded += __shfl_down(n_occluded, off);
    }
    if (lane == 0u) {
        if (n_paths != 0ull) atomicAdd(totals, n_paths);
        if (n_rays != 0ull) atomicAdd(totals + 1, n_rays);
        if (n_shadow != 0ull) atomicAdd(totals + 2, n_shadow);
        if (n_occluded != 0ull) atomicAdd(totals + 3, n_occluded);
    }
}

// ---- k_nee: every pixel takes the pass's sample count, one light sample per Lambert vertex ----------------------------------------------
// The shading of a round — the sky, the material, the three BSDF branches — stands in each of the three renders: as a shared piece,
// by reference or by value, it rescheduled them (k_nee_adaptive_cone 2.6 % slower on the MI355X; DESIGN.md §17 "One round").
template <int WALK, bool CONE>
__device__ __forceinline__ void nee_render(SceneDev sc, AccelDev ac, NeePass P) {
    const TileWalk T = tile_walk<WALK>(sc, ac);
    if (T.tx0 >= P.W || T.ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const NeePixel X = nee_pixel(T, P.W, P.H);
    const NeeConsts K = nee_consts(P);
    const float uvx = ((float)X.px + 0.5f) / K.fW, uvy = ((float)X.py + 0.5f) / K.fH;   // pixel_uv of gen_primary
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (X.inside) acc = K.sum[X.pixel];
    const uint32_t N = X.inside ? P.sample_count : 0u;
    uint32_t s = 0u;             // samples of this pixel started so far
    NeePath p;                   // (initialised in the order the registers were first allotted in: see the header's note)
    p.sample = 0u;
    bool has_ray = false;
    p.o = f3(1.0f, 1.0f, 1.0f), p.d = f3(1.0f, 1.0f, 1.0f), p.thr = f3(1.0f, 1.0f, 1.0f), p.L = f3(0.0f, 0.0f, 0.0f);
    p.La = 0.0f, p.pb = 0.0f;
    p.b = 0u;
    bool sampled = false;
    uint32_t n_paths = 0u;
    unsigned long long n_rays = 0ull, n_shadow = 0ull, n_occluded = 0ull;
    WorkCount wc = {};
    for (;;) {
        if (!has_ray && s < N) {
            p = nee_regenerate(K, X.pixel, uvx, uvy, s);
            sampled = false;
            has_ray = true;
            s += 1u;
            n_paths += 1u;
        }
        if (__ballot(has_ray) == 0ull) break;   // (wave-uniform: every pixel of the tile has its samples)
        const NeeHit hit = nee_closest<WALK>(sc, ac, T, p.o, p.d, has_ray, wc);
        bool shadow = false, ended = false;
        F3 wi = f3(1.0f, 1.0f, 1.0f), C = f3(0.0f, 0.0f, 0.0f);
        float tmax = 0.0f;
        if (has_ray) {
            n_rays += 1ull;
            if (hit.prim < 0) {   // the sky of shade_bounce: never sampled as a light, always in full
                const F3 ud = normalize3(p.d);
                const float tt = 0.5f * (ud.y + 1.0f);
                const F3 sky = f3(1.0f + (0.6f - 1.0f) * tt, 1.0f + (0.7f - 1.0f) * tt, 1.0f + (1.0f - 1.0f) * tt);
                p.L.x += p.thr.x * sky.x;
                p.L.y += p.thr.y * sky.y;
                p.L.z += p.thr.z * sky.z;
                p.La += 1.0f;
                ended = true;
            } else {
                const U4 rb = philox4x32_10<true>(X.pixel, p.sample, p.b, 0u, K.seed_lo, K.seed_hi);
                const HitInfo h = finish_hit(sc, T.lds, p.o, p.d, hit.t, hit.prim);
                if ((uint32_t)h.orig_id >= K.prim_count) {
                    ended = true;
                } else {
                    float4 m0, m1;
                    if ((uint32_t)h.mat < sc.n_lds_mats) {
                        const LdsNodes q = T.lds + sc.lds_mat_off + 2u * (uint32_t)h.mat;
                        const v4f a0 = q[0], a1 = q[1];
                        m0 = make_float4(a0.x, a0.y, a0.z, a0.w);
                        m1 = make_float4(a1.x, a1.y, a1.z, a1.w);
                    } else {
                        m0 = sc.mats[2 * h.mat];
                        m1 = sc.mats[2 * h.mat + 1];
                    }
                    const float mtype = m0.w, power = m1.w;
                    if (power > 0.0f || mtype == 2.0f) {
                        float w = 1.0f;
                        if (sampled) w = nee_emitter_weight<CONE>(K, h, p.o, p.d, hit.t, p.pb);
                        p.L.x += ((p.thr.x * m1.x) * power) * w;
                        p.L.y += ((p.thr.y * m1.y) * power) * w;
                        p.L.z += ((p.thr.z * m1.z) * power) * w;
                        p.La += power;
                    }
                    F3 nd;
                    bool through = false;
                    if (K.bsdf_mode == 0 || mtype == 0.0f) {   // a Lambert vertex: the bounce of shade_bounce and a light p.sample
                        const float z = 2.0f * u01(rb.x) - 1.0f;
                        float sn, cs;
                        sincos_2pi(u01(rb.y), sn, cs);
                        const float rr = sqrtf(1.0f - z * z);
                        nd = normalize3(h.normal + f3(rr * cs, rr * sn, z));
                        const F3 on = h.point + 0.0001f * h.normal;
                        const bool attempt = K.have_lights != 0u && (int)(p.b + 1u) < K.max_depth;
                        if (attempt) {   // the p.sample of k_direct, with n = h.normal and p.o = on, from the block with word 3 = 1
                            const U4 r = philox4x32_10<true>(X.pixel, p.sample, p.b, 1u, K.seed_lo, K.seed_hi);
                            const float u = u01(r.x);
                            const uint32_t k = table_search(K.last, K.search_steps, [&](uint32_t mid) { return u < K.cdf[mid]; });
                            const LightSample ls = light_sample<CONE>(K.lights, k, on, h.normal, u01(r.y), u01(r.z));
                            wi = ls.wi;
                            shadow = ls.ok;
                            tmax = ls.dist * 0.9990234375f;
                            const float m = nee_light_factor<CONE>(ls);
                            C = f3(((p.thr.x * m0.x) * 0.31830987f) * (ls.Le.x * m), ((p.thr.y * m0.y) * 0.31830987f) * (ls.Le.y * m),
                                   ((p.thr.z * m0.z) * 0.31830987f) * (ls.Le.z * m));
                        }
                        sampled = attempt;
                        p.pb = dot3(h.normal, nd) * 0.31830987f;
                    } else if (mtype < 0.0f) {   // shade_bounce's mirror and dielectric, unchanged: no light p.sample
                        nd = normalize3(reflect3(p.d, h.normal));
                        sampled = false;
                    } else {
                        const float ri = h.front ? 1.0f / mtype : mtype;
                        nd = mirror_angle(ri, h.normal, p.d, u01(rb.z)) ? reflect3(p.d, h.normal) : refract3(p.d, h.normal, ri);
                        nd = normalize3(nd);
                        through = dot3(nd, h.normal) < 0.0f;
                        sampled = false;
                    }
                    p.o = through ? h.point - 0.0001f * h.normal : h.point + 0.0001f * h.normal;
                    p.d = nd;
                    p.thr.x *= m0.x;
                    p.thr.y *= m0.y;
                    p.thr.z *= m0.z;
                    p.b += 1u;
                    ended = !((int)p.b < K.max_depth);
                }
            }
        }
        p.L = nee_shadow_step<WALK>(sc, ac, T, p.o, p.L, shadow, wi, tmax, C, n_shadow, n_occluded);
        if (ended) {   // the per-sample value joins the running sum, in sample order
            const float4 val = nee_sample_value(K, p.L, p.La);
            acc.x += val.x;
            acc.y += val.y;
            acc.z += val.z;
            acc.w += val.w;
            has_ray = false;
            p.o = f3(1.0f, 1.0f, 1.0f);
            p.d = f3(1.0f, 1.0f, 1.0f);
        }
    }
    if (X.inside) K.sum[X.pixel] = acc;
    nee_add_totals(P.totals, T.lane, n_paths, n_rays, n_shadow, n_occluded);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee(SceneDev sc, AccelDev ac, NeePass P) {
    nee_render<WALK, false>(sc, ac, P);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee_cone(SceneDev sc, AccelDev ac, NeePass P) {
    nee_render<WALK, true>(sc, ac, P);
}
