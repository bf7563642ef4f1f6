// mpt_nee_adaptive.h — adaptive sampling over the NEE estimator, decided per tile ON THE DEVICE (included by mpt_hip.hip after mpt_nee.h
// and mpt_adaptive.h; the contract is mpt_render_nee_adaptive's in include/mpt.h, DESIGN.md §18 has the lane mapping and the measurements):
//   k_nee_adaptive<WALK>        k_nee's render — one wave per 8 x 8 tile, one lane per pixel, the pixel's sum in registers — with the second
//                               moments beside the sum, a sample quota per tile that follows mpt_render_adaptive's schedule, and the stopping
//                               rule of k_adaptive_eval applied by the wave itself whenever its tile holds the quota: one launch, no host passes
//   k_nee_adaptive_cone<WALK>   the same with MPT_LIGHT_SAMPLING_CONE; both are nee_adaptive_render<WALK, CONE>
// The round is k_nee's, from the pieces of mpt_nee.h (the shading stands in the loop, as in k_nee: see there): this header has the pass,
// the loop and the two kernels.  The loop has the quota in place of the sample count, the tile's decision where k_nee leaves, the
// moments beside the sum, and the moments and the tile's count written at the end.  The estimator is specified once in include/mpt.h (mpt_nee_params); tests/test_gpu_nee.py holds k_nee to it
// bit for bit and tests/test_gpu_nee_adaptive.py this render to k_nee's own per-sample values.
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
    const TileWalk T = tile_walk<WALK>(sc, ac);
    if (T.tx0 >= A.nee.W || T.ty0 >= A.nee.H) return;   // (wave-uniform: the tile lies outside the image)
    // k_nee's pass constants, and beside them in VECTOR registers the five of the schedule and the rule
    const NeePixel X = nee_pixel(T, A.nee.W, A.nee.H);
    const NeeConsts K = nee_consts(A.nee);
    uint32_t n_max = A.nee.sample_count, batch = A.batch;
    uint32_t quota = A.min_samples < n_max ? A.min_samples : n_max;   // samples the tile's pixels get before the next decision
    float threshold = A.threshold, floor_l = A.floor;
    asm volatile("" : "+v"(n_max), "+v"(batch), "+v"(quota), "+v"(threshold), "+v"(floor_l));
    const float uvx = ((float)X.px + 0.5f) / K.fW, uvy = ((float)X.py + 0.5f) / K.fH;   // pixel_uv of gen_primary
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // the host cleared the sum: nothing to read
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // the second moments of the samples in acc
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
        if (!has_ray && X.inside && s < quota) {   // up to the quota
            p = nee_regenerate(K, X.pixel, uvx, uvy, s);
            sampled = false;
            has_ray = true;
            s += 1u;
            n_paths += 1u;
        }
        if (__ballot(has_ray) == 0ull) {
            // (wave-uniform) no lane holds a ray and none could start one: every pixel of the tile inside the image holds exactly
            // `quota` samples, in acc and m.  k_adaptive_eval's rule, on registers; the maximum reaches every lane, so all decide alike.
            double err = 0.0;
            if (X.inside) err = adaptive_pixel_error(acc, m.w, quota, (double)floor_l);
            err = adaptive_tile_error(err);
            const bool more = err > (double)threshold && quota < n_max;
            if (__ballot(more) == 0ull) break;
            quota = batch < n_max - quota ? quota + batch : n_max;   // min(quota + batch, N) without the 32-bit overflow
            continue;
        }
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
                            const float mw = nee_light_factor<CONE>(ls);
                            C = f3(((p.thr.x * m0.x) * 0.31830987f) * (ls.Le.x * mw), ((p.thr.y * m0.y) * 0.31830987f) * (ls.Le.y * mw),
                                   ((p.thr.z * m0.z) * 0.31830987f) * (ls.Le.z * mw));
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
        if (ended) {   // the per-sample value joins the running sum and the moments, in sample order
            const float4 val = nee_sample_value(K, p.L, p.La);
            acc.x += val.x;
            acc.y += val.y;
            acc.z += val.z;
            acc.w += val.w;
            add_moments(m, val);
            has_ray = false;
            p.o = f3(1.0f, 1.0f, 1.0f);
            p.d = f3(1.0f, 1.0f, 1.0f);
        }
    }
    if (X.inside) {   // the tile is done: its pixels hold `quota` samples each
        K.sum[X.pixel] = acc;
        A.m2[X.pixel] = m;
    }
    if (T.lane == 0u) A.tile_count[(T.ty0 >> 3) * A.tiles_x + (T.tx0 >> 3)] = quota;
    nee_add_totals(A.nee.totals, T.lane, n_paths, n_rays, n_shadow, n_occluded);
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
