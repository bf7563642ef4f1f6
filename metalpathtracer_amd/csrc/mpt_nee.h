// mpt_nee.h — next-event estimation inside the path loop (included by mpt_hip.hip after mpt_direct.h):
//   k_nee<WALK>   one lane per pixel: the pixel's samples in turn, a light sample with a shadow ray at every Lambert vertex, the light a
//                 bounce finds weighted against it (power heuristic), the HDR sum updated in registers in sample order
//   k_nee_cone<WALK>  the same render with a sphere light sampled in the cone it subtends (MPT_LIGHT_SAMPLING_CONE): its light sample and
//                 the weight of a sphere light a bounce finds change, nothing else; both kernels are nee_render<WALK, CONE>
// The estimator is specified exactly in include/mpt.h (mpt_nee_params) and restated in numpy in tests/nee_ref.py; DESIGN.md §17 has the
// lane mapping, the registers and the measured times.  Nothing here edits a kernel or a device function of the plain render: the walks
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
template <int WALK, bool CONE>
__device__ __forceinline__ void nee_render(SceneDev sc, AccelDev ac, NeePass P) {
    const TileWalk T = tile_walk<WALK>(sc, ac);
    const LdsNodes lds = T.lds;
    const uint32_t lane = T.lane, tx0 = T.tx0, ty0 = T.ty0;
    if (tx0 >= P.W || ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const uint32_t px = tx0 + (lane & 7u), py = ty0 + (lane >> 3);
    const bool inside = px < P.W && py < P.H;
    const uint32_t pixel = inside ? py * P.W + px : 0u;
    // What the rounds and the end need from the pass goes into VECTOR registers (an empty asm makes the value opaque, as in k_direct):
    // the two walks hold the scalar file.  The camera goes with them: a regeneration needs its fourteen words in any round.
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
    const float uvx = ((float)px + 0.5f) / fW, uvy = ((float)py + 0.5f) / fH;   // pixel_uv of gen_primary
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside) acc = sum[pixel];
    const uint32_t N = inside ? P.sample_count : 0u;
    uint32_t s = 0u;             // samples of this pixel started so far
    uint32_t sample = 0u;        // Philox counter word 1 of the running path
    bool has_ray = false;
    F3 o = f3(1.0f, 1.0f, 1.0f), d = f3(1.0f, 1.0f, 1.0f), thr = f3(1.0f, 1.0f, 1.0f), L = f3(0.0f, 0.0f, 0.0f);
    float La = 0.0f, pb = 0.0f;
    uint32_t b = 0u;
    bool sampled = false;
    uint32_t n_paths = 0u;
    unsigned long long n_rays = 0ull, n_shadow = 0ull, n_occluded = 0ull;
    WorkCount wc = {};
    for (;;) {
        if (!has_ray && s < N) {   // path regeneration: the primary ray of gen_primary (philox)
            sample = sample_begin + s;
            const U4 r = philox4x32_10<true>(pixel, sample, 0xFFFFFFFFu, 0u, P.seed_lo, P.seed_hi);
            const float xOff = (u01(r.x) - 0.5f) / fW, yOff = (u01(r.y) - 0.5f) / fH;
            const F3 dir = (first + (uvx + xOff) * vu + (uvy + yOff) * vv) - cam;
            o = cam;
            d = normalize3(dir);
            thr = f3(1.0f, 1.0f, 1.0f);
            L = f3(0.0f, 0.0f, 0.0f);
            La = 0.0f;
            pb = 0.0f;
            b = 0u;
            sampled = false;
            has_ray = true;
            s += 1u;
            n_paths += 1u;
        }
        if (__ballot(has_ray) == 0ull) break;   // (wave-uniform: every pixel of the tile has its samples)
        float t;
        int prim;
        if (WALK == MPT_AO_OWN) {
            uint32_t flags;
            closest_hit_ordered<false>(ac, sc, lds, T.st, o, d, has_ray, t, prim, flags, wc);
        } else {   // closest_hit, with the lanes that hold no ray done before the first node
            uint32_t node = has_ray ? 0u : sc.n_nodes;
            t = INFINITY;
            prim = -1;
            closest_hit_resume<false, WALK == MPT_AO_REF_ALL_LDS, false>(sc, lds, o, d, node, t, prim, 0xFFFFFFFFu, wc);
        }
        bool shadow = false, ended = false;
        F3 wi = f3(1.0f, 1.0f, 1.0f), C = f3(0.0f, 0.0f, 0.0f);
        float tmax = 0.0f;
        if (has_ray) {
            n_rays += 1ull;
            if (prim < 0) {   // the sky of shade_bounce: never sampled as a light, always in full
                const F3 ud = normalize3(d);
                const float tt = 0.5f * (ud.y + 1.0f);
                const F3 sky = f3(1.0f + (0.6f - 1.0f) * tt, 1.0f + (0.7f - 1.0f) * tt, 1.0f + (1.0f - 1.0f) * tt);
                L.x += thr.x * sky.x;
                L.y += thr.y * sky.y;
                L.z += thr.z * sky.z;
                La += 1.0f;
                ended = true;
            } else {
                const U4 rb = philox4x32_10<true>(pixel, sample, b, 0u, P.seed_lo, P.seed_hi);
                const HitInfo h = finish_hit(sc, lds, o, d, t, prim);
                if ((uint32_t)h.orig_id >= prim_count) {
                    ended = true;
                } else {
                    float4 m0, m1;
                    if ((uint32_t)h.mat < sc.n_lds_mats) {
                        const LdsNodes q = lds + sc.lds_mat_off + 2u * (uint32_t)h.mat;
                        const v4f a0 = q[0], a1 = q[1];
                        m0 = make_float4(a0.x, a0.y, a0.z, a0.w);
                        m1 = make_float4(a1.x, a1.y, a1.z, a1.w);
                    } else {
                        m0 = sc.mats[2 * h.mat];
                        m1 = sc.mats[2 * h.mat + 1];
                    }
                    const float mtype = m0.w, power = m1.w;
                    if (power > 0.0f || mtype == 2.0f) {
                        // the light a bounce found: in full, unless the vertex before drew a light sample that could have found it too
                        float w = 1.0f;
                        if (sampled) {
                            // the smallest k with id <= ids[k]
                            const uint32_t lo = table_search(last, search_steps, [&](uint32_t mid) { return h.orig_id <= ids[mid]; });
                            if (ids[lo] == h.orig_id) {
                                const float4 L0 = lights[MPT_LIGHT_F4 * lo], L3 = lights[MPT_LIGHT_F4 * lo + 3u];
                                if (L0.w != 0.0f || h.front) {   // (a sphere emits outward only where it is sampled)
                                    if (!CONE || L0.w != 0.0f) {
                                        const float cos_l = -dot3(h.normal, d);
                                        const float pl = (t * t) / (cos_l * L3.w);
                                        const float q = pl / pb;
                                        w = 1.0f / (1.0f + q * q);
                                    } else {   // the solid-angle pdf of the cone from this ray's origin: neither t nor cos_l enters
                                        const float4 L1 = lights[MPT_LIGHT_F4 * lo + 1u];
                                        float dc2, omc, J;
                                        if (cone_cap(f3(L0.x, L0.y, L0.z) - o, L1.x, L3.w, dc2, omc, J)) {
                                            const float q = 1.0f / (J * pb);
                                            w = 1.0f / (1.0f + q * q);
                                        }
                                    }
                                }
                            }
                        }
                        L.x += ((thr.x * m1.x) * power) * w;
                        L.y += ((thr.y * m1.y) * power) * w;
                        L.z += ((thr.z * m1.z) * power) * w;
                        La += power;
                    }
                    F3 nd;
                    bool through = false;
                    if (bsdf_mode == 0 || mtype == 0.0f) {   // a Lambert vertex: the bounce of shade_bounce and a light sample
                        const float z = 2.0f * u01(rb.x) - 1.0f;
                        float sn, cs;
                        sincos_2pi(u01(rb.y), sn, cs);
                        const float rr = sqrtf(1.0f - z * z);
                        nd = normalize3(h.normal + f3(rr * cs, rr * sn, z));
                        const F3 on = h.point + 0.0001f * h.normal;
                        const bool attempt = have_lights != 0u && (int)(b + 1u) < max_depth;
                        if (attempt) {   // the sample of k_direct, with n = h.normal and o = on, from the block with word 3 = 1
                            const U4 r = philox4x32_10<true>(pixel, sample, b, 1u, P.seed_lo, P.seed_hi);
                            const float u = u01(r.x);
                            const uint32_t k = table_search(last, search_steps, [&](uint32_t mid) { return u < cdf[mid]; });
                            const LightSample ls = light_sample<CONE>(lights, k, on, h.normal, u01(r.y), u01(r.z));
                            wi = ls.wi;
                            shadow = ls.ok;
                            tmax = ls.dist * 0.9990234375f;
                            // the sample's factor times its weight against the bounce's pdf (power heuristic), both per solid angle
                            float m;
                            if (!CONE || ls.tri) {
                                const float g = (ls.cos_s * ls.cos_l) / ls.d2;
                                const float pl = ls.d2 / (ls.cos_l * ls.inv_pdf);
                                const float q = (ls.cos_s * 0.31830987f) / pl;
                                m = (g * ls.inv_pdf) * (1.0f / (1.0f + q * q));
                            } else {
                                const float q = (ls.cos_s * 0.31830987f) * ls.J;
                                m = (ls.cos_s * ls.J) * (1.0f / (1.0f + q * q));
                            }
                            C = f3(((thr.x * m0.x) * 0.31830987f) * (ls.Le.x * m), ((thr.y * m0.y) * 0.31830987f) * (ls.Le.y * m),
                                   ((thr.z * m0.z) * 0.31830987f) * (ls.Le.z * m));
                        }
                        sampled = attempt;
                        pb = dot3(h.normal, nd) * 0.31830987f;
                    } else if (mtype < 0.0f) {   // shade_bounce's mirror and dielectric, unchanged: no light sample
                        nd = normalize3(reflect3(d, h.normal));
                        sampled = false;
                    } else {
                        const float ri = h.front ? 1.0f / mtype : mtype;
                        nd = mirror_angle(ri, h.normal, d, u01(rb.z)) ? reflect3(d, h.normal) : refract3(d, h.normal, ri);
                        nd = normalize3(nd);
                        through = dot3(nd, h.normal) < 0.0f;
                        sampled = false;
                    }
                    o = through ? h.point - 0.0001f * h.normal : h.point + 0.0001f * h.normal;
                    d = nd;
                    thr.x *= m0.x;
                    thr.y *= m0.y;
                    thr.z *= m0.z;
                    b += 1u;
                    ended = !((int)b < max_depth);
                }
            }
        }
        if (__ballot(shadow) != 0ull) {   // (wave-uniform) the shadow rays of this round's vertices, from the bounce rays' origins
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
        }
        if (ended) {   // the per-sample value joins the running sum, in sample order
            acc.x += L.x > 0.0f ? fminf(L.x, clamp_hi) : 0.0f;
            acc.y += L.y > 0.0f ? fminf(L.y, clamp_hi) : 0.0f;
            acc.z += L.z > 0.0f ? fminf(L.z, clamp_hi) : 0.0f;
            acc.w += clamp01(La);
            has_ray = false;
            o = f3(1.0f, 1.0f, 1.0f);
            d = f3(1.0f, 1.0f, 1.0f);
        }
    }
    if (inside) sum[pixel] = acc;
    unsigned long long n_paths64 = n_paths;
    for (int off = 32; off > 0; off >>= 1) {
        n_paths64 += __shfl_down(n_paths64, off);
        n_rays += __shfl_down(n_rays, off);
        n_shadow += __shfl_down(n_shadow, off);
        n_occluded += __shfl_down(n_occluded, off);
    }
    if (lane == 0u) {
        if (n_paths64 != 0ull) atomicAdd(P.totals, n_paths64);
        if (n_rays != 0ull) atomicAdd(P.totals + 1, n_rays);
        if (n_shadow != 0ull) atomicAdd(P.totals + 2, n_shadow);
        if (n_occluded != 0ull) atomicAdd(P.totals + 3, n_occluded);
    }
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee(SceneDev sc, AccelDev ac, NeePass P) {
    nee_render<WALK, false>(sc, ac, P);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee_cone(SceneDev sc, AccelDev ac, NeePass P) {
    nee_render<WALK, true>(sc, ac, P);
}
