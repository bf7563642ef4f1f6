// mpt_direct.h — direct lighting over the first-hit guide buffers (included by mpt_hip.hip after mpt_anyhit.h):
//   k_light_collect   one thread per device primitive: the emissive ones are appended to a list (the host sorts it into the light table)
//   k_direct<WALK>    per surface pixel, N points on the lights drawn by power, one shadow ray each through an any-hit walk
//   k_direct_cone<WALK>  the same pass with a sphere light sampled in the cone it subtends (MPT_LIGHT_SAMPLING_CONE); both kernels are
//                     direct_pass<WALK, CONE>, which differ in the sphere sample alone
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

// Lane mapping.  A workgroup of four waves takes a 16 x 16 pixel block, each wave one 8 x 8 tile of it (as k_ao), ONE LANE PER PIXEL, and
// a round per sample: all 64 lanes trace sample s of their own pixels together.  The shadow rays of neighbouring pixels towards a handful
// of lights start next to each other and point the same way, so a round's walk is coherent as it is, and a pixel's sum runs in sample
// order in its one lane: no cross-lane work.  A round in which no lane has a ray skips the walk; a tile without a surface pixel
// returns after writing its constants.  The table is fetched per lane from global memory (it is small and stays in L2).
// CONE: a sphere light is sampled by cone_cap / cone_sample; a triangle light, the selection and everything else are the same.
template <int WALK, bool CONE>
__device__ __forceinline__ void direct_pass(SceneDev sc, AccelDev ac, DirectPass P) {
    extern __shared__ float4 lds_raw[];
    if (WALK == MPT_AO_OWN) ot_stage(sc, ac, lds_raw);
    else stage_nodes(sc, lds_raw);
    const LdsNodes lds = (LdsNodes)lds_raw;
    OtStack st = {};
    if (WALK == MPT_AO_OWN) st = ot_stack(ac, lds_raw, 0u);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tx0 = blockIdx.x * MPT_DN_TILE + (wave & 1u) * 8u, ty0 = blockIdx.y * MPT_DN_TILE + (wave >> 1) * 8u;
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
                const float uvx = ((float)px + 0.5f) / P.fW, uvy = ((float)py + 0.5f) / P.fH;
                const F3 dv = (P.first + uvx * P.vu + uvy * P.vv) - P.cam;
                const F3 dc = dv * (1.0f / sqrtf(dot3(dv, dv)));   // normalize3, with the division written out (the lanes diverge here)
                n = f3(g.x, g.y, g.z);
                o = (P.cam + a.w * dc) + 0.0001f * n;   // the origin of the bounce ray, exactly as k_ao forms it
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
    const uint32_t search_steps = P.n_lights > 1u ? 32u - (uint32_t)__builtin_clz(P.n_lights - 1u) : 0u;   // ceil(log2(n_lights))
    const uint32_t rounds = P.n_lights != 0u ? P.sample_count : 0u;   // (no lights: nothing to sample, every surface pixel is black)
    for (uint32_t s = 0; s < rounds; ++s) {
        const U4 r = philox4x32_10<true>(pixel, sample_begin + s, 0xFFFFFFFDu, 0u, P.seed_lo, P.seed_hi);
        // the smallest k with u < cdf[k] (u < 1 = cdf[last]): a binary search of the same length in every lane
        const float u = u01(r.x);
        uint32_t lo = 0u, hi = last;
        for (uint32_t step = 0; step < search_steps; ++step) {
            const uint32_t mid = (lo + hi) >> 1;
            const bool below = u < cdf[mid];
            const bool open = lo < hi;
            hi = open && below ? mid : hi;
            lo = open && !below ? mid + 1u : lo;
        }
        const float4 L0 = lights[MPT_LIGHT_F4 * lo], L1 = lights[MPT_LIGHT_F4 * lo + 1u], L2 = lights[MPT_LIGHT_F4 * lo + 2u],
                     L3 = lights[MPT_LIGHT_F4 * lo + 3u];
        const bool tri = L0.w != 0.0f;
        const float ua = u01(r.y), ub = u01(r.z);
        // a point of the triangle ...
        float a = ua, b = ub;
        if (a + b > 1.0f) {
            a = 1.0f - a;
            b = 1.0f - b;
        }
        const F3 e1 = f3(L1.x, L1.y, L1.z), e2 = f3(L2.x, L2.y, L2.z), c = f3(L0.x, L0.y, L0.z);
        const F3 pt = (c + a * e1) + b * e2;
        const F3 ng = normalize3(cross3(e1, e2));
        F3 wi;
        float d2, dist, cos_s, cos_l, fac = 0.0f;
        bool live;
        if (!CONE) {
            // ... or of the sphere
            const float z = 2.0f * ua - 1.0f;
            float sn, cs;
            sincos_2pi(ub, sn, cs);
            const float rr = sqrtf(1.0f - z * z);
            const F3 ns = f3(rr * cs, rr * sn, z);
            const F3 ps = c + L1.x * ns;
            const F3 nl = tri ? ng : ns;
            const F3 p = tri ? pt : ps;
            const F3 v = p - o;
            d2 = dot3(v, v);
            dist = sqrtf(d2);
            wi = v * mpt_rcp(dist);
            cos_s = dot3(n, wi);
            const float dl = dot3(nl, wi);
            cos_l = tri ? fabsf(dl) : -dl;
            live = surface && d2 > 0.0f && cos_s > 0.0f && cos_l > 0.0f;   // (a NaN skips)
        } else {
            // ... or a direction of the cone the sphere subtends; the sample's factor is formed here, so one value crosses the walk
            const F3 vt = pt - o;
            d2 = dot3(vt, vt);
            const float dist_t = sqrtf(d2);
            const F3 wi_t = vt * mpt_rcp(dist_t);
            const float cos_t = dot3(n, wi_t);
            cos_l = fabsf(dot3(ng, wi_t));
            const float g = (cos_t * cos_l) / d2;
            const F3 w = c - o;
            float dc2, omc, J, dist_c;
            const bool outside = cone_cap(w, L1.x, L3.w, dc2, omc, J);
            F3 wi_c;
            cone_sample(w, dc2, omc, ua, ub, wi_c, dist_c);
            const float cos_c = dot3(n, wi_c);
            wi = tri ? wi_t : wi_c;
            dist = tri ? dist_t : dist_c;
            cos_s = tri ? cos_t : cos_c;
            fac = tri ? g * L3.w : cos_c * J;
            live = surface && cos_s > 0.0f && (tri ? d2 > 0.0f && cos_l > 0.0f : outside && dist_c > 0.0f);   // (a NaN skips)
        }
        if (__ballot(live) == 0ull) continue;   // (wave-uniform)
        const float tmax = dist * 0.9990234375f;
        bool hit;
        if (WALK == MPT_AO_OWN) {
            uint32_t flags;
            hit = any_hit_own(ac, sc, lds, st, o, wi, tmax, live, flags);
        } else {
            hit = any_hit_ref<WALK == MPT_AO_REF_ALL_LDS>(sc, lds, o, wi, tmax, live);
        }
        if (live) {
            n_traced += 1u;
            if (!hit) {
                n_unoccluded += 1u;
                float w = fac;
                if (!CONE) {
                    const float g = (cos_s * cos_l) / d2;
                    w = g * L3.w;
                }
                S = S + f3(L3.x * w, L3.y * w, L3.z * w);
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
    direct_pass<WALK, false>(sc, ac, P);
}
template <int WALK>
__global__ __launch_bounds__(256) void k_direct_cone(SceneDev sc, AccelDev ac, DirectPass P) {
    direct_pass<WALK, true>(sc, ac, P);
}
