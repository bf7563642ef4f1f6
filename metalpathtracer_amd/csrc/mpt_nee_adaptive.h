// mpt_nee_adaptive.h — adaptive sampling over the NEE estimator, decided per tile ON THE DEVICE (included by mpt_hip.hip after mpt_nee.h
// and mpt_adaptive.h; the contract is mpt_render_nee_adaptive's in include/mpt.h, DESIGN.md §18 has the lane mapping and the measurements):
//   k_nee_adaptive<WALK>        k_nee's render — one wave per 8 x 8 tile, one lane per pixel, the pixel's sum in registers — with the second
//                               moments beside the sum, a sample quota per tile that follows mpt_render_adaptive's schedule, and the stopping
//                               rule of k_adaptive_eval applied by the wave itself whenever its tile holds the quota: one launch, no host passes
//   k_nee_adaptive_cone<WALK>   the same with MPT_LIGHT_SAMPLING_CONE; both are nee_adaptive_render<WALK, CONE>
// nee_render (mpt_nee.h) is not edited and not shared: its generated code stays what it is.  The round below is ITS round, statement for
// statement — the estimator is specified once in include/mpt.h (mpt_nee_params) and both loops are held to it bit for bit by the tests
// (tests/test_gpu_nee.py for k_nee, tests/test_gpu_nee_adaptive.py for this one, against k_nee's own per-sample values).  What differs is
// marked [A]: the moments, the quota in place of the sample count, the decision where k_nee leaves, and what is written at the end.
#pragma once
#include "mpt_nee.h"
#include "mpt_adaptive.h"

struct NeeAdaptivePass {
    NeePass nee;                 // k_nee's pass: sum = the CLEARED HDR sum (written, never read), sample_count = N, the most a tile gets
    float4* m2;                  // the cleared moments buffer (W * H rgba): written once per pixel
    uint32_t* tile_count;        // row-major by tile, tiles_x per row: the samples every pixel of the tile holds at the end
    uint32_t tiles_x;
    uint32_t min_samples, batch; // the schedule: n_0 = min(min_samples, N), n_{k+1} = min(n_k + batch, N)
    float threshold, floor;      // the stopping rule's, widened to double where it is applied (as the host widens them for k_adaptive_eval)
};

template <int WALK, bool CONE>
__device__ __forceinline__ void nee_adaptive_render(SceneDev sc, AccelDev ac, NeeAdaptivePass A) {
    const NeePass& P = A.nee;
    const TileWalk T = tile_walk<WALK>(sc, ac);
    const LdsNodes lds = T.lds;
    const uint32_t lane = T.lane, tx0 = T.tx0, ty0 = T.ty0;
    if (tx0 >= P.W || ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const uint32_t px = tx0 + (lane & 7u), py = ty0 + (lane >> 3);
    const bool inside = px < P.W && py < P.H;
    const uint32_t pixel = inside ? py * P.W + px : 0u;
    // k_nee's pass constants in VECTOR registers (the two walks hold the scalar file), and [A] the five of the schedule and the rule
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
    uint32_t n_max = P.sample_count, batch = A.batch;
    uint32_t quota = A.min_samples < n_max ? A.min_samples : n_max;   // [A] samples the tile's pixels get before the next decision
    float threshold = A.threshold, floor_l = A.floor;
    asm volatile("" : "+v"(sum), "+v"(lights), "+v"(cdf), "+v"(ids), "+v"(last), "+v"(sample_begin), "+v"(prim_count), "+v"(search_steps));
    asm volatile("" : "+v"(bsdf_mode), "+v"(max_depth), "+v"(clamp_hi), "+v"(fW), "+v"(fH), "+v"(have_lights));
    asm volatile("" : "+v"(cam.x), "+v"(cam.y), "+v"(cam.z), "+v"(first.x), "+v"(first.y), "+v"(first.z));
    asm volatile("" : "+v"(vu.x), "+v"(vu.y), "+v"(vu.z), "+v"(vv.x), "+v"(vv.y), "+v"(vv.z));
    asm volatile("" : "+v"(n_max), "+v"(batch), "+v"(quota), "+v"(threshold), "+v"(floor_l));
    const float uvx = ((float)px + 0.5f) / fW, uvy = ((float)py + 0.5f) / fH;   // pixel_uv of gen_primary
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // [A] the host cleared the sum: nothing to read
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // [A] the second moments of the samples in acc
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
        if (!has_ray && inside && s < quota) {   // path regeneration: the primary ray of gen_primary (philox); [A] up to the quota
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
        if (__ballot(has_ray) == 0ull) {
            // [A] (wave-uniform) no lane holds a ray and none could start one: every pixel of the tile inside the image holds exactly
            // `quota` samples, in acc and m.  k_adaptive_eval's rule, on registers; the maximum reaches every lane, so all decide alike.
            double err = 0.0;
            if (inside) err = adaptive_pixel_error(acc, m.w, quota, (double)floor_l);
            err = adaptive_tile_error(err);
            const bool more = err > (double)threshold && quota < n_max;
            if (__ballot(more) == 0ull) break;
            quota = batch < n_max - quota ? quota + batch : n_max;   // min(quota + batch, N) without the 32-bit overflow
            continue;
        }
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
                            float mw;
                            if (!CONE || ls.tri) {
                                const float g = (ls.cos_s * ls.cos_l) / ls.d2;
                                const float pl = ls.d2 / (ls.cos_l * ls.inv_pdf);
                                const float q = (ls.cos_s * 0.31830987f) / pl;
                                mw = (g * ls.inv_pdf) * (1.0f / (1.0f + q * q));
                            } else {
                                const float q = (ls.cos_s * 0.31830987f) * ls.J;
                                mw = (ls.cos_s * ls.J) * (1.0f / (1.0f + q * q));
                            }
                            C = f3(((thr.x * m0.x) * 0.31830987f) * (ls.Le.x * mw), ((thr.y * m0.y) * 0.31830987f) * (ls.Le.y * mw),
                                   ((thr.z * m0.z) * 0.31830987f) * (ls.Le.z * mw));
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
        if (ended) {   // the per-sample value joins the running sum and [A] the moments, in sample order
            const float4 v = make_float4(L.x > 0.0f ? fminf(L.x, clamp_hi) : 0.0f, L.y > 0.0f ? fminf(L.y, clamp_hi) : 0.0f,
                                         L.z > 0.0f ? fminf(L.z, clamp_hi) : 0.0f, clamp01(La));
            acc.x += v.x;
            acc.y += v.y;
            acc.z += v.z;
            acc.w += v.w;
            add_moments(m, v);
            has_ray = false;
            o = f3(1.0f, 1.0f, 1.0f);
            d = f3(1.0f, 1.0f, 1.0f);
        }
    }
    if (inside) {   // [A] the tile is done: its pixels hold `quota` samples each
        sum[pixel] = acc;
        A.m2[pixel] = m;
    }
    if (lane == 0u) A.tile_count[(ty0 >> 3) * A.tiles_x + (tx0 >> 3)] = quota;
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
// Registers.  The moments, the quota and the rule's constants put the reference-order instantiations at 137 VGPRs where k_nee has 107:
// past 128, three waves per SIMD instead of four, and this render lives on its waves in flight (measured, DESIGN.md §18: 1.21x the
// time of k_nee for the same samples, before any batch boundary).  NEE_ADAPTIVE_WAVES asks the compiler for k_nee's four: it keeps
// them in 128 VGPRs and spills 9 (cone: 10) cold ones to 40 (44) bytes of scratch per lane — 1.02x.  The own-tree instantiation
// has 163 with or without it and stays at three, as its k_nee sibling does at 134.
#define NEE_ADAPTIVE_WAVES(WALK) __attribute__((amdgpu_waves_per_eu((WALK) == MPT_AO_OWN ? 3 : 4, (WALK) == MPT_AO_OWN ? 3 : 4)))
template <int WALK>
__global__ __launch_bounds__(256) NEE_ADAPTIVE_WAVES(WALK) void k_nee_adaptive(SceneDev sc, AccelDev ac, NeeAdaptivePass A) {
    nee_adaptive_render<WALK, false>(sc, ac, A);
}
template <int WALK>
__global__ __launch_bounds__(256) NEE_ADAPTIVE_WAVES(WALK) void k_nee_adaptive_cone(SceneDev sc, AccelDev ac, NeeAdaptivePass A) {
    nee_adaptive_render<WALK, true>(sc, ac, A);
}
