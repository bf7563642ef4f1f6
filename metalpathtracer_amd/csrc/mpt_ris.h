// mpt_ris.h — resampled light sampling (RIS) in the direct pass and in the NEE render (included by mpt_hip.hip after mpt_nee.h; the
// contract is the "light candidates" section of include/mpt.h, tests/ris_ref.py restates it in numpy, DESIGN.md §19 has the registers
// and the measurements):
//   ris_pick<CONE, NEE>        M candidates drawn as the one sample of k_direct / k_nee is drawn, each weighted by the light it would
//                              deliver unshadowed, one kept in a streaming reservoir of one
//   k_direct_ris<WALK>, k_direct_ris_cone<WALK>   k_direct's pass with the round's sample picked that way: one shadow ray per round, as before
//   k_nee_ris<WALK>, k_nee_ris_cone<WALK>         k_nee's render with the vertex's light sample picked that way
// The host launches these for mpt_set_light_candidates(m >= 2) only: m = 1 launches k_direct / k_nee themselves, whose code is not edited
// and not shared (direct_pass and nee_render keep their generated code).  The two bodies below are THEIR bodies, statement for statement;
// what differs is marked [R]: the pick in place of the one sample, and the contribution finished before the walk.
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
// none.  NEE: the candidate's factor carries its power-heuristic weight against the bounce's pdf (nee_render's m), else it is the
// direct pass's fac.  The reservoir is wsum, wi, dist, Le and l; r.w, which the one sample leaves unused, decides the replacement.
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
            fac = !CONE || ls.tri ? ((ls.cos_s * ls.cos_l) / ls.d2) * ls.inv_pdf : ls.cos_s * ls.J;
        } else if (!CONE || ls.tri) {
            const float g = (ls.cos_s * ls.cos_l) / ls.d2;
            const float pl = ls.d2 / (ls.cos_l * ls.inv_pdf);
            const float q = (ls.cos_s * 0.31830987f) / pl;
            fac = (g * ls.inv_pdf) * (1.0f / (1.0f + q * q));
        } else {
            const float q = (ls.cos_s * 0.31830987f) * ls.J;
            fac = (ls.cos_s * ls.J) * (1.0f / (1.0f + q * q));
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

// ---- the direct pass (direct_pass of mpt_direct.h, with [R]) --------------------------------------------------------------------------
template <int WALK, bool CONE>
__device__ __forceinline__ void direct_ris_pass(SceneDev sc, AccelDev ac, DirectRisPass R) {
    const DirectPass& P = R.d;
    const TileWalk T = tile_walk<WALK>(sc, ac);
    const uint32_t lane = T.lane, tx0 = T.tx0, ty0 = T.ty0;
    if (tx0 >= P.W || ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    F3 o = f3(1.0f, 1.0f, 1.0f), n = f3(0.0f, 0.0f, 0.0f), albedo = f3(0.0f, 0.0f, 0.0f);
    uint32_t pixel = 0u;
    bool surface = false;
    {
        const uint32_t px = tx0 + (lane & 7u), py = ty0 + (lane >> 3);
        if (px < P.W && py < P.H) {
            pixel = py * P.W + px;
            const float4 g = P.nc[pixel];
            const float4 a = P.ad[pixel];
            surface = g.w == 0.0f;
            if (surface) {
                n = f3(g.x, g.y, g.z);
                o = guide_origin(P, px, py, a.w, n);
                albedo = f3(a.x, a.y, a.z);
            } else {
                P.out[pixel] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                P.traced()[pixel] = 0u;
                P.unoccluded()[pixel] = 0u;
            }
        }
    }
    const uint32_t n_surface = (uint32_t)__popcll(__ballot(surface));
    if (n_surface == 0u) return;   // (wave-uniform: nothing to shade in this tile)
    // the pass constants of a round in VECTOR registers, as in direct_pass: the walks hold the scalar file
    float4* out = P.out;
    const float4* lights = P.lights;
    const float* cdf = P.cdf;
    uint32_t n_pixels = P.n_pixels, N = P.sample_count, sample_begin = P.sample_begin, last = P.n_lights - 1u;
    asm volatile("" : "+v"(out), "+v"(lights), "+v"(cdf), "+v"(n_pixels), "+v"(N), "+v"(sample_begin), "+v"(last));
    uint32_t n_traced = 0u, n_unoccluded = 0u;
    F3 S = f3(0.0f, 0.0f, 0.0f);
    const uint32_t search_steps = __builtin_amdgcn_readfirstlane(table_search_steps(P.n_lights));
    const uint32_t M = __builtin_amdgcn_readfirstlane(R.M);   // [R]
    const uint32_t rounds = P.n_lights != 0u ? P.sample_count : 0u;   // (no lights: nothing to sample, every surface pixel is black)
    for (uint32_t s = 0; s < rounds; ++s) {
        // [R] the round's sample: the pick of M candidates, its contribution finished here so that wi, tmax and C cross the walk
        const RisPick y = ris_pick<CONE, false>(lights, cdf, last, search_steps, M, pixel, sample_begin + s, 0xFFFFFFFDu, 0u, P.seed_lo,
                                                P.seed_hi, o, n, surface);
        const bool live = y.taken;
        if (__ballot(live) == 0ull) continue;   // (wave-uniform)
        const bool hit = any_hit<WALK>(sc, ac, T, o, y.wi, y.tmax, live);
        if (live) {
            n_traced += 1u;
            if (!hit) {
                n_unoccluded += 1u;
                S = S + y.C;
            }
        }
    }
    if (surface) {
        const float fN = (float)N;
        out[pixel] = make_float4((albedo.x * 0.31830987f) * (S.x / fN), (albedo.y * 0.31830987f) * (S.y / fN), (albedo.z * 0.31830987f) * (S.z / fN), 1.0f);
        ((uint32_t*)(out + n_pixels))[pixel] = n_traced;                // (DirectPass::traced, unoccluded)
        ((uint32_t*)(out + n_pixels))[n_pixels + pixel] = n_unoccluded;
    }
    for (int off = 32; off > 0; off >>= 1) {
        n_traced += (uint32_t)__shfl_down((int)n_traced, off);
        n_unoccluded += (uint32_t)__shfl_down((int)n_unoccluded, off);
    }
    if (lane == 0u) {
        atomicAdd(P.totals(), (unsigned long long)n_surface);
        if (n_traced != 0u) atomicAdd(P.totals() + 1, (unsigned long long)n_traced);
        if (n_unoccluded != 0u) atomicAdd(P.totals() + 2, (unsigned long long)n_unoccluded);
    }
}
template <int WALK>
__global__ __launch_bounds__(256) void k_direct_ris(SceneDev sc, AccelDev ac, DirectRisPass R) {
    direct_ris_pass<WALK, false>(sc, ac, R);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_direct_ris_cone(SceneDev sc, AccelDev ac, DirectRisPass R) {
    direct_ris_pass<WALK, true>(sc, ac, R);
}

// ---- the NEE render (nee_render of mpt_nee.h, with [R]) -------------------------------------------------------------------------------
template <int WALK, bool CONE>
__device__ __forceinline__ void nee_ris_render(SceneDev sc, AccelDev ac, NeeRisPass R) {
    const NeePass& P = R.nee;
    const TileWalk T = tile_walk<WALK>(sc, ac);
    const LdsNodes lds = T.lds;
    const uint32_t lane = T.lane, tx0 = T.tx0, ty0 = T.ty0;
    if (tx0 >= P.W || ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const uint32_t px = tx0 + (lane & 7u), py = ty0 + (lane >> 3);
    const bool inside = px < P.W && py < P.H;
    const uint32_t pixel = inside ? py * P.W + px : 0u;
    // k_nee's pass constants in VECTOR registers (the two walks hold the scalar file), and [R] the candidate count with them
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
    uint32_t Mv = R.M;
    asm volatile("" : "+v"(sum), "+v"(lights), "+v"(cdf), "+v"(ids), "+v"(last), "+v"(sample_begin), "+v"(prim_count), "+v"(search_steps));
    asm volatile("" : "+v"(bsdf_mode), "+v"(max_depth), "+v"(clamp_hi), "+v"(fW), "+v"(fH), "+v"(have_lights), "+v"(Mv));
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
        bool ended = false;
        bool attempt = false;        // [R] this lane's vertex draws a light sample: the candidate loop below runs for it
        F3 on = f3(1.0f, 1.0f, 1.0f), nn = f3(0.0f, 0.0f, 1.0f), ta = f3(0.0f, 0.0f, 0.0f);   // [R] its point, its normal, (thr * albedo) / pi
        uint32_t vb = 0u;            // [R] ... and its bounce index (Philox counter word 2)
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
                        attempt = have_lights != 0u && (int)(b + 1u) < max_depth;
                        if (attempt) {   // [R] the candidates are drawn behind the shading, by all the wave's vertices together
                            on = h.point + 0.0001f * h.normal;
                            nn = h.normal;
                            ta = f3((thr.x * m0.x) * 0.31830987f, (thr.y * m0.y) * 0.31830987f, (thr.z * m0.z) * 0.31830987f);
                            vb = b;
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
        bool shadow = false;
        F3 wi = f3(1.0f, 1.0f, 1.0f), C = f3(0.0f, 0.0f, 0.0f);
        float tmax = 0.0f;
        if (__ballot(attempt) != 0ull) {   // (wave-uniform) [R] the pick of M candidates from the blocks (pixel, sample, b, 1 + j), j ascending
            const uint32_t M = __builtin_amdgcn_readfirstlane(Mv);
            const RisPick y = ris_pick<CONE, true>(lights, cdf, last, search_steps, M, pixel, sample, vb, 1u, P.seed_lo, P.seed_hi, on, nn, attempt);
            shadow = y.taken;
            wi = y.wi;
            tmax = y.tmax;
            C = f3(ta.x * y.C.x, ta.y * y.C.y, ta.z * y.C.z);
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
__global__ __launch_bounds__(256) void k_nee_ris(SceneDev sc, AccelDev ac, NeeRisPass R) {
    nee_ris_render<WALK, false>(sc, ac, R);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_nee_ris_cone(SceneDev sc, AccelDev ac, NeeRisPass R) {
    nee_ris_render<WALK, true>(sc, ac, R);
}
