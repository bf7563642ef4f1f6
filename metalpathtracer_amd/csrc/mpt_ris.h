// mpt_ris.h — resampled light sampling (RIS) in the direct pass and in the NEE render (included by mpt_hip.hip after mpt_nee.h; the
// contract is the "light candidates" section of include/mpt.h, tests/ris_ref.py restates it in numpy, DESIGN.md §19 has the registers
// and the measurements):
//   ris_pick<CONE, NEE>        M candidates drawn as the one sample of k_direct / k_nee is drawn, each weighted by the light it would
//                              deliver unshadowed, one kept in a streaming reservoir of one
//   k_direct_ris<WALK>, k_direct_ris_cone<WALK>   k_direct's pass with the round's sample picked that way: one shadow ray per round, as before
//   k_nee_ris<WALK>, k_nee_ris_cone<WALK>         k_nee's render with the vertex's light sample picked that way
// The host launches these for mpt_set_light_candidates(m >= 2) only: m = 1 launches k_direct / k_nee themselves.  The direct kernels are
// direct_pass<WALK, CONE, true> (mpt_direct.h), whose round calls ris_pick; the render is a loop over the pieces of k_nee's round
// (mpt_nee.h) whose shading only notes the vertex; the pick follows it, for all the wave's vertices together, with the contribution
// finished before the walk.
#pragma once
#include "mpt_nee.h"

struct DirectRisPass {
    DirectPass d;                // k_direct's pass
    uint32_t M;                  // candidates per sample, 2..MPT_LIGHT_CANDIDATES_MAX (wave-uniform: the candidate loop is a uniform loop)
};
struct NeeRisPass {
    NeePass nee;                 // k_nee's pass
    uint32_t M;
};

// What the candidate loop leaves: the shadow ray of the candidate it kept and the estimator's factor Le_y * Fy, Fy = (wsum / M) / l_y.
struct RisPick {
    F3 wi;
    float tmax;
    F3 C;                        // (Le_y.r Fy, Le_y.g Fy, Le_y.b Fy)
    bool taken;                  // false: no candidate counted — the sample is skipped
};
// Candidates j = 0 .. M-1 from the blocks philox(c0, c1, c2, c3 + j) at the point o with the normal n; a lane with active == false takes
// none.  NEE: the candidate's factor carries its power-heuristic weight against the bounce's pdf (nee_light_factor), else it is the
// direct pass's (direct_light_factor).  The reservoir is wsum, wi, dist, Le and l; r.w, which the one sample leaves unused, decides the replacement.
// (declared ahead in mpt_direct.h for direct_pass: keep the two signatures in step)
template <bool CONE, bool NEE>
__device__ __forceinline__ RisPick ris_pick(const float4* lights, const float* cdf, uint32_t last, uint32_t search_steps, uint32_t M, uint32_t c0,
                                            uint32_t c1, uint32_t c2, uint32_t c3, uint32_t seed_lo, uint32_t seed_hi, F3 o, F3 n, bool active) {
    float wsum = 0.0f, y_dist = 0.0f, y_l = 1.0f;
    F3 y_wi = f3(1.0f, 1.0f, 1.0f), y_Le = f3(0.0f, 0.0f, 0.0f);
    bool taken = false;
    for (uint32_t j = 0; j < M; ++j) {
        const U4 r = philox4x32_10<true>(c0, c1, c2, c3 + j, seed_lo, seed_hi);
        const float u = u01(r.x);   // the smallest k with u < cdf[k]
        const uint32_t k = table_search(last, search_steps, [&](uint32_t mid) { return u < cdf[mid]; });
        const LightSample ls = light_sample<CONE>(lights, k, o, n, u01(r.y), u01(r.z));
        float fac;
        if (!NEE) {
            fac = direct_light_factor<CONE>(ls);
        } else {
            fac = nee_light_factor<CONE>(ls);
        }
        const float l = (0.2126f * ls.Le.x + 0.7152f * ls.Le.y) + 0.0722f * ls.Le.z;
        const float w = l * fac;
        if (active && ls.ok && w > 0.0f && w < INFINITY) {   // the candidate counts (a NaN does not)
            wsum = wsum + w;
            if (!taken || u01(r.w) * wsum < w) {
                y_wi = ls.wi;
                y_dist = ls.dist;
                y_Le = ls.Le;
                y_l = l;
            }
            taken = true;
        }
    }
    RisPick p;
    p.wi = y_wi;
    p.tmax = y_dist * 0.9990234375f;
    const float Fy = (wsum / (float)M) / y_l;
    p.C = f3(y_Le.x * Fy, y_Le.y * Fy, y_Le.z * Fy);
    p.taken = taken;
    return p;
}

// ---- the direct pass: direct_pass of mpt_direct.h with the round's sample picked --------------------------------------------------------
template <int WALK>
__global__ __launch_bounds__(256) void k_direct_ris(SceneDev sc, AccelDev ac, DirectRisPass R) {
    direct_pass<WALK, false, true>(sc, ac, R.d, R.M);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_direct_ris_cone(SceneDev sc, AccelDev ac, DirectRisPass R) {
    direct_pass<WALK, true, true>(sc, ac, R.d, R.M);
}

// ---- the NEE render: nee_render's loop with the vertex's light sample picked ------------------------------------------------------------
template <int WALK, bool CONE>
__device__ __forceinline__ void nee_ris_render(SceneDev sc, AccelDev ac, NeeRisPass R) {
    const TileWalk T = tile_walk<WALK>(sc, ac);
    if (T.tx0 >= R.nee.W || T.ty0 >= R.nee.H) return;   // (wave-uniform: the tile lies outside the image)
    // k_nee's pass constants, and the candidate count with them in a VECTOR register
    const NeePixel X = nee_pixel(T, R.nee.W, R.nee.H);
    const NeeConsts K = nee_consts(R.nee);
    uint32_t Mv = R.M;
    asm volatile("" : "+v"(Mv));
    const float uvx = ((float)X.px + 0.5f) / K.fW, uvy = ((float)X.py + 0.5f) / K.fH;   // pixel_uv of gen_primary
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (X.inside) acc = K.sum[X.pixel];
    const uint32_t N = X.inside ? R.nee.sample_count : 0u;
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
        bool ended = false;
        bool attempt = false;        // this lane's vertex draws a light sample: the candidate loop below runs for it
        F3 on = f3(1.0f, 1.0f, 1.0f), nn = f3(0.0f, 0.0f, 1.0f), ta = f3(0.0f, 0.0f, 0.0f);   // its point, its normal, (thr * albedo) / pi
        uint32_t vb = 0u;            // ... and its bounce index (Philox counter word 2)
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
                        attempt = K.have_lights != 0u && (int)(p.b + 1u) < K.max_depth;
                        if (attempt) { // the candidates are drawn behind the shading, by all the wave's vertices together
                            on = h.point + 0.0001f * h.normal;
                            nn = h.normal;
                            ta = f3((p.thr.x * m0.x) * 0.31830987f, (p.thr.y * m0.y) * 0.31830987f, (p.thr.z * m0.z) * 0.31830987f);
                            vb = p.b;
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
        bool shadow = false;
        F3 wi = f3(1.0f, 1.0f, 1.0f), C = f3(0.0f, 0.0f, 0.0f);
        float tmax = 0.0f;
        if (__ballot(attempt) != 0ull) {   // (wave-uniform) the pick of M candidates from the blocks (pixel, sample, b, 1 + j), j ascending
            const uint32_t M = __builtin_amdgcn_readfirstlane(Mv);
            const RisPick y = ris_pick<CONE, true>(K.lights, K.cdf, K.last, K.search_steps, M, X.pixel, p.sample, vb, 1u, K.seed_lo, K.seed_hi, on, nn,
                                                   attempt);
            shadow = y.taken;
            wi = y.wi;
            tmax = y.tmax;
            C = f3(ta.x * y.C.x, ta.y * y.C.y, ta.z * y.C.z);
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
    nee_add_totals(R.nee.totals, T.lane, n_paths, n_rays, n_shadow, n_occluded);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee_ris(SceneDev sc, AccelDev ac, NeeRisPass R) {
    nee_ris_render<WALK, false>(sc, ac, R);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee_ris_cone(SceneDev sc, AccelDev ac, NeeRisPass R) {
    nee_ris_render<WALK, true>(sc, ac, R);
}
