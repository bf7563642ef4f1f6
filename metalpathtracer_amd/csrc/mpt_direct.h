// mpt_direct.h — direct lighting over the first-hit guide buffers (included by mpt_hip.hip after mpt_anyhit.h):
//   k_light_collect   one thread per device primitive: the emissive ones are appended to a list (the host sorts it into the light table)
//   k_direct<WALK>    per surface pixel, N points on the lights drawn by power, one shadow ray each through an any-hit walk
//   k_direct_cone<WALK>  the same pass with a sphere light sampled in the cone it subtends (MPT_LIGHT_SAMPLING_CONE); both kernels are
//                     direct_pass<WALK, CONE, false>, which differ in the sphere sample alone
//   direct_pass<WALK, CONE, RIS>   the pass, written once: the prologue over the guide buffers, the rounds, the image, the counts and the
//                     totals; RIS = true is k_direct_ris / k_direct_ris_cone (mpt_ris.h), whose round takes ris_pick's sample for the one draw
//   table_search, light_sample<CONE>   one sample of the light table — the selection, the point or direction on the light, the skip
//                     predicate — for direct_pass, the NEE round (mpt_nee.h) and ris_pick: the only copy
//   direct_light_factor<CONE>      the estimator's factor of such a sample, for direct_pass and ris_pick<CONE, false>
// The pass is specified exactly in include/mpt.h (mpt_direct_params) and restated in numpy in tests/direct_ref.py; DESIGN.md §16 has the
// table, the lane mapping and the registers.
#pragma once
#include "mpt_anyhit.h"
#include "mpt_ao.h"

#define MPT_LIGHT_F4 4u   // float4 per light: (v0 | c, type) (e1 | r 0 0, 0) (e2 | 0, 0) (Le, inv_pdf); type 1 triangle, 0 sphere

// A primitive is a light iff its material has emissionPower > 0 (the guide pass's class 1).  Appends (geometry, Le = emission * power)
// in the table's record layout, with the caller's primitive id in the unused last word of the second float4 (the host takes it out).
// `counter` counts every emissive primitive; entries beyond `cap` are not written.
__global__ __launch_bounds__(256) void k_light_collect(const float4* prims, const float4* mats, uint32_t n_prims, uint32_t cap, uint32_t* counter,
                                                       float4* list) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_prims) return;
    const float4 p0 = prims[3 * (size_t)i], p1 = prims[3 * (size_t)i + 1], p2 = prims[3 * (size_t)i + 2];
    const float4 m1 = mats[2 * (size_t)__float_as_int(p1.w) + 1];
    if (!(m1.w > 0.0f)) return;
    const uint32_t k = atomicAdd(counter, 1u);
    if (k >= cap) return;
    const bool tri = prim_type(p0) == 1;
    float4* r = list + (size_t)MPT_LIGHT_F4 * k;
    r[0] = make_float4(p0.x, p0.y, p0.z, tri ? 1.0f : 0.0f);
    r[1] = make_float4(p1.x, tri ? p1.y : 0.0f, tri ? p1.z : 0.0f, p2.w);
    r[2] = make_float4(p2.x, p2.y, p2.z, 0.0f);
    r[3] = make_float4(m1.x * m1.w, m1.y * m1.w, m1.z * m1.w, 0.0f);
}

// ---- a sphere light sampled by solid angle (MPT_LIGHT_SAMPLING_CONE; include/mpt.h has the rule, tests/cone_ref.py restates it) ----------
// The cap a point sees of the sphere (c, r), from w = c - o: false unless the point lies outside (a NaN: false).  omc = 1 - cos(theta_max)
// without cancellation; J = the reciprocal of the solid-angle pdf, the selection of the light included (inv_pdf = 4 pi r^2 / p_k).
__device__ __forceinline__ bool cone_cap(F3 w, float r, float inv_pdf, float& dc2, float& omc, float& J) {
    dc2 = dot3(w, w);
    const float r2 = r * r;
    const float s2 = r2 / dc2;
    const float cm = sqrtf(1.0f - s2);
    omc = s2 / (1.0f + cm);
    J = omc * (inv_pdf / ((2.0f * r) * r));
    return dc2 > r2;
}
// The direction drawn uniformly in that cone from (u1, u2), in the frame of Duff et al. 2017 around wc = w / |w|, and the distance to the
// near intersection with the sphere: r^2 - dc^2 sin^2(theta) as a product of factors that do not cancel at the cone's edge.
__device__ __forceinline__ void cone_sample(F3 w, float dc2, float omc, float u1, float u2, F3& wi, float& dist) {
    const float k = u1 * omc;
    const float ct = 1.0f - k;
    const float st = sqrtf(k * (2.0f - k));
    float sn, cs;
    sincos_2pi(u2, sn, cs);
    const float dc = sqrtf(dc2);
    const F3 wc = w * mpt_rcp(dc);
    const float sg = wc.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sg + wc.z);
    const float b = (wc.x * wc.y) * a;
    const F3 t1 = f3(1.0f + ((sg * wc.x) * wc.x) * a, sg * b, -(sg * wc.x));
    const F3 t2 = f3(b, sg + (wc.y * wc.y) * a, -wc.y);
    wi = normalize3(((st * cs) * t1 + (st * sn) * t2) + ct * wc);
    dist = dc * ct - sqrtf(dc2 * ((omc * (1.0f - u1)) * ((2.0f - omc) - k)));
}

// ---- one sample of the light table: what k_direct and k_nee (and their cone variants) draw at a vertex, written once -----------------
// The smallest k in [0, last] with below(k), for a predicate that is false up to some k and true from it on (true at `last`): a binary
// search of the same length, table_search_steps(last + 1), in every lane.  Serves u < cdf[k] and id <= ids[k].
__device__ __forceinline__ uint32_t table_search_steps(uint32_t n) { return n > 1u ? 32u - (uint32_t)__builtin_clz(n - 1u) : 0u; }   // ceil(log2(n))
template <class Below>
__device__ __forceinline__ uint32_t table_search(uint32_t last, uint32_t steps, Below below) {
    uint32_t lo = 0u, hi = last;
    for (uint32_t step = 0; step < steps; ++step) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool b = below(mid);
        const bool open = lo < hi;
        hi = open && b ? mid : hi;
        lo = open && !b ? mid + 1u : lo;
    }
    return lo;
}
// Light k sampled from the point o with the normal n by (ua, ub).  A triangle, and a sphere unless CONE: a point p of its area —
// d2 = |p - o|^2, cos_l at the light; the estimator's factor is (cos_s cos_l / d2) inv_pdf.  CONE, a sphere: a direction of the cone it
// subtends — the factor is cos_s J (d2 and cos_l are the triangle branch's and mean nothing).  ok: the sample can carry light (a NaN: false).
struct LightSample {
    F3 wi;                       // unit direction towards the light
    float dist;                  // ... and the distance to it along wi
    float cos_s, cos_l, d2, J;   // cos_s = n . wi
    float inv_pdf;               // the record's: area / p_k
    F3 Le;
    bool tri, ok;
};
template <bool CONE>
__device__ __forceinline__ LightSample light_sample(const float4* lights, uint32_t k, F3 o, F3 n, float ua, float ub) {
    const float4 L0 = lights[MPT_LIGHT_F4 * k], L1 = lights[MPT_LIGHT_F4 * k + 1u], L2 = lights[MPT_LIGHT_F4 * k + 2u],
                 L3 = lights[MPT_LIGHT_F4 * k + 3u];
    LightSample s;
    s.tri = L0.w != 0.0f;
    s.Le = f3(L3.x, L3.y, L3.z);
    s.inv_pdf = L3.w;
    s.J = 0.0f;
    // a point of the triangle ...
    float a = ua, b = ub;
    if (a + b > 1.0f) {
        a = 1.0f - a;
        b = 1.0f - b;
    }
    const F3 e1 = f3(L1.x, L1.y, L1.z), e2 = f3(L2.x, L2.y, L2.z), c = f3(L0.x, L0.y, L0.z);
    const F3 pt = (c + a * e1) + b * e2;
    const F3 ng = normalize3(cross3(e1, e2));
    if (!CONE) {
        // ... or of the sphere
        const float z = 2.0f * ua - 1.0f;
        float sn, cs;
        sincos_2pi(ub, sn, cs);
        const float rr = sqrtf(1.0f - z * z);
        const F3 ns = f3(rr * cs, rr * sn, z);
        const F3 ps = c + L1.x * ns;
        const F3 nl = s.tri ? ng : ns;
        const F3 p = s.tri ? pt : ps;
        const F3 v = p - o;
        s.d2 = dot3(v, v);
        s.dist = sqrtf(s.d2);
        s.wi = v * mpt_rcp(s.dist);
        s.cos_s = dot3(n, s.wi);
        const float dl = dot3(nl, s.wi);
        s.cos_l = s.tri ? fabsf(dl) : -dl;
        s.ok = s.d2 > 0.0f && s.cos_s > 0.0f && s.cos_l > 0.0f;
    } else {
        // ... or a direction of the cone the sphere subtends
        const F3 vt = pt - o;
        s.d2 = dot3(vt, vt);
        const float dist_t = sqrtf(s.d2);
        const F3 wi_t = vt * mpt_rcp(dist_t);
        const float cos_t = dot3(n, wi_t);
        s.cos_l = fabsf(dot3(ng, wi_t));
        const F3 w = c - o;
        float dc2, omc, dist_c;
        const bool outside = cone_cap(w, L1.x, L3.w, dc2, omc, s.J);
        F3 wi_c;
        cone_sample(w, dc2, omc, ua, ub, wi_c, dist_c);
        const float cos_c = dot3(n, wi_c);
        s.wi = s.tri ? wi_t : wi_c;
        s.dist = s.tri ? dist_t : dist_c;
        s.cos_s = s.tri ? cos_t : cos_c;
        s.ok = s.cos_s > 0.0f && (s.tri ? s.d2 > 0.0f && s.cos_l > 0.0f : outside && dist_c > 0.0f);
    }
    return s;
}

struct DirectPass {
    const float4* ad;            // (albedo, t)
    const float4* nc;            // (normal facing the ray, class)
    float4* out;                 // ONE block: [0, n) rgba, then n uint32 traced, n uint32 unoccluded, then three 64-bit totals:
    uint32_t n_pixels;           //   += surface pixels, += rays traced, += rays not occluded (one atomic each per wave that has any)
    __host__ __device__ uint32_t* traced() const { return (uint32_t*)(out + n_pixels); }
    __host__ __device__ uint32_t* unoccluded() const { return traced() + n_pixels; }
    __host__ __device__ unsigned long long* totals() const { return (unsigned long long*)(unoccluded() + n_pixels); }
    const float4* lights;        // MPT_LIGHT_F4 float4 per light, ascending caller id
    const float* cdf;            // cdf[n_lights - 1] = 1
    uint32_t n_lights;
    F3 cam, first, vu, vv;
    float fW, fH;
    uint32_t W, H;
    uint32_t sample_begin, sample_count;
    uint32_t seed_lo, seed_hi;
};

// The estimator's factor of a light sample: (cos_s cos_l / d2) inv_pdf for a point of an area, cos_s J for a direction of a cone.  The only
// copy: direct_pass forms it for its one draw, ris_pick<CONE, false> (mpt_ris.h) for every candidate.
template <bool CONE>
__device__ __forceinline__ float direct_light_factor(LightSample ls) {   // (by value: by reference the cone kernels come out with another register count)
    return !CONE || ls.tri ? ((ls.cos_s * ls.cos_l) / ls.d2) * ls.inv_pdf : ls.cos_s * ls.J;
}
// (mpt_ris.h, which is included after mpt_nee.h and this header: the round's sample of k_direct_ris)
struct RisPick;
template <bool CONE, bool NEE>
__device__ __forceinline__ RisPick ris_pick(const float4* lights, const float* cdf, uint32_t last, uint32_t search_steps, uint32_t M, uint32_t c0,
                                            uint32_t c1, uint32_t c2, uint32_t c3, uint32_t seed_lo, uint32_t seed_hi, F3 o, F3 n, bool active);

// Lane mapping.  A workgroup of four waves takes a 16 x 16 pixel block, each wave one 8 x 8 tile of it (as k_ao), ONE LANE PER PIXEL, and
// a round per sample: all 64 lanes trace sample s of their own pixels together.  The shadow rays of neighbouring pixels towards a handful
// of lights start next to each other and point the same way, so a round's walk is coherent as it is, and a pixel's sum runs in sample
// order in its one lane: no cross-lane work.  A round in which no lane has a ray skips the walk; a tile without a surface pixel
// returns after writing its constants.  The table is fetched per lane from global memory (it is small and stays in L2).
// CONE: a sphere light is sampled by cone_cap / cone_sample (light_sample<true>); a triangle light, the selection and everything else are the same.
// RIS: the round's sample is not the one draw but ris_pick's choice among `candidates` draws (k_direct_ris, mpt_ris.h): one shadow ray per
// round as before, and the prologue over the guide buffers, the image, the counts and the totals are these for both.
template <int WALK, bool CONE, bool RIS>
__device__ __forceinline__ void direct_pass(SceneDev sc, AccelDev ac, DirectPass P, uint32_t candidates) {
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
    // What a round or the end needs from the pass goes into VECTOR registers (an empty asm makes the value opaque, as in k_ao): the walks
    // hold the scalar file.
    float4* out = P.out;
    const float4* lights = P.lights;
    const float* cdf = P.cdf;
    uint32_t n_pixels = P.n_pixels, N = P.sample_count, sample_begin = P.sample_begin, last = P.n_lights - 1u;
    asm volatile("" : "+v"(out), "+v"(lights), "+v"(cdf), "+v"(n_pixels), "+v"(N), "+v"(sample_begin), "+v"(last));
    uint32_t n_traced = 0u, n_unoccluded = 0u;
    F3 S = f3(0.0f, 0.0f, 0.0f);
    // (the count is wave-uniform and stays in the scalar file: formed from n_lights - 1, which `last` above has put in a vector register,
    // it would follow it there and take a vector register across the walk; the candidate loop is a uniform loop)
    const uint32_t search_steps = __builtin_amdgcn_readfirstlane(table_search_steps(P.n_lights));
    const uint32_t M = RIS ? __builtin_amdgcn_readfirstlane(candidates) : 1u;
    const uint32_t rounds = P.n_lights != 0u ? P.sample_count : 0u;   // (no lights: nothing to sample, every surface pixel is black)
    for (uint32_t s = 0; s < rounds; ++s) {
        // the round's sample: its shadow ray (wi, tmax), whether the lane traces it, and what it adds where the ray arrives
        F3 wi, C;
        float tmax, fac = 0.0f;
        bool live;
        LightSample ls;   // (the one draw: not used under RIS)
        if constexpr (RIS) {   // the pick of M candidates, its contribution finished here so that wi, tmax and C cross the walk
            const auto y = ris_pick<CONE, false>(lights, cdf, last, search_steps, M, pixel, sample_begin + s, 0xFFFFFFFDu, 0u, P.seed_lo,
                                                 P.seed_hi, o, n, surface);
            wi = y.wi;
            tmax = y.tmax;
            C = y.C;
            live = y.taken;
        } else {
            const U4 r = philox4x32_10<true>(pixel, sample_begin + s, 0xFFFFFFFDu, 0u, P.seed_lo, P.seed_hi);
            const float u = u01(r.x);   // the smallest k with u < cdf[k] (u < 1 = cdf[last])
            const uint32_t k = table_search(last, search_steps, [&](uint32_t mid) { return u < cdf[mid]; });
            ls = light_sample<CONE>(lights, k, o, n, u01(r.y), u01(r.z));
            // the sample's factor: CONE forms it here, so one value crosses the walk; AREA forms it behind the walk, for the rays that arrive
            if (CONE) fac = direct_light_factor<CONE>(ls);
            wi = ls.wi;
            tmax = ls.dist * 0.9990234375f;
            live = surface && ls.ok;
        }
        if (__ballot(live) == 0ull) continue;   // (wave-uniform)
        const bool hit = any_hit<WALK>(sc, ac, T, o, wi, tmax, live);
        if (live) {
            n_traced += 1u;
            if (!hit) {
                n_unoccluded += 1u;
                if constexpr (!RIS) {
                    if (!CONE) fac = direct_light_factor<CONE>(ls);
                    C = f3(ls.Le.x * fac, ls.Le.y * fac, ls.Le.z * fac);
                }
                S = S + C;
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
__global__ __launch_bounds__(256) void k_direct(SceneDev sc, AccelDev ac, DirectPass P) {
    direct_pass<WALK, false, false>(sc, ac, P, 1u);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_direct_cone(SceneDev sc, AccelDev ac, DirectPass P) {
    direct_pass<WALK, true, false>(sc, ac, P, 1u);
}
