// mpt_restir.h — spatial reservoir reuse (ReSTIR) in the direct pass (included by mpt_hip.hip after mpt_ris.h; the contract is the
// "spatial reservoir reuse" section of include/mpt.h, tests/restir_ref.py restates it in numpy, DESIGN.md §20 has the registers):
//   restir_pick                 ris_pick<false, false>'s candidate loop, remembering what a reservoir stores: the light, the two uniforms
//                               the kept candidate was formed from, and its factor
//   k_restir_initial<WALK>      step A of a round: every surface pixel's reservoir of one, kept only if its shadow ray arrives
//   k_restir_merge<WALK, UNBIASED>   steps B-E of the round: the merge with the neighbours' reservoirs, the final ray, the
//                               normalisation (UNBIASED: one correction ray per accepted neighbour) and the contribution
// Two kernels per round, because a round's reservoirs must all exist before any pixel merges; the host launches the pair once per
// sample.  Both keep direct_pass's mapping (mpt_direct.h): a 16 x 16 block per workgroup, a wave per 8 x 8 tile, a lane per pixel, the
// scene staged by tile_walk.  A pixel's sum S, its two counts and the totals live in global memory across the rounds (the host zeroes
// them before the first), so S runs in sample order.
#pragma once
#include "mpt_ris.h"

#define MPT_RESTIR_WORD2 0xFFFFFFFCu   // Philox counter word 2 of a neighbour draw: nobody else's (the light sample has ...FD, AO ...FE, the jitter ...FF)
enum { MPT_RS_SURFACE = 0, MPT_RS_INITIAL, MPT_RS_FINAL, MPT_RS_CORRECTION, MPT_RS_UNOCCLUDED, MPT_RS_ACCEPTED, MPT_RS_FROM_NEIGHBOUR, MPT_RS_TOTALS };
// The totals are kept MPT_RS_SLOTS times, a workgroup adding to the copy of its index, each copy on a 128-byte line of its own; the host
// sums the copies.  A call is 2 N launches of up to seven atomics per wave: on ONE set of addresses they serialise in the L2 and were
// most of the call's time.
#define MPT_RS_SLOTS 64u
#define MPT_RS_SLOT_WORDS 16u
#define MPT_RS_TOTAL_WORDS (MPT_RS_SLOTS * MPT_RS_SLOT_WORDS)

// A reservoir in memory: two uint4 per pixel, (k, ua, ub, wsum) (fac, flags, 0, 0), floats by their bits; flags bit 0 = holds,
// bit 1 = the pixel's own sample (set in the pick of step B only).  An EMPTY reservoir is all zeros.
struct RestirPass {
    const float4* ad;            // (albedo, t)
    const float4* nc;            // (normal facing the ray, class)
    float4* out;                 // ONE block, as DirectPass::out: [0, n) rgba, n uint32 traced, n uint32 unoccluded, then MPT_RS_TOTAL_WORDS 64-bit words of totals
    uint32_t n_pixels;
    __host__ __device__ uint32_t* traced() const { return (uint32_t*)(out + n_pixels); }
    __host__ __device__ uint32_t* unoccluded() const { return traced() + n_pixels; }
    __host__ __device__ unsigned long long* totals() const { return (unsigned long long*)(unoccluded() + n_pixels); }
    float4* S;                   // the running sum of a pixel's rounds (w unused)
    uint4* initial;              // the round's reservoirs after step A
    uint4* pick;                 // the pick of step B, written by the last round alone (mpt_read_restir_reservoirs)
    const float4* lights;        // the light table, as DirectPass
    const float* cdf;
    uint32_t n_lights;
    F3 cam, first, vu, vv;
    float fW, fH;
    uint32_t W, H;
    uint32_t sample_begin, sample_count;
    uint32_t seed_lo, seed_hi;
    uint32_t round;              // 0 .. sample_count - 1: this launch is sample sample_begin + round
    uint32_t M, K, R;            // candidates, neighbours, radius
    float normal_threshold, depth_tolerance;
};

// ris_pick<false, false> (mpt_ris.h) with the kept candidate's (k, ua, ub, fac) remembered.  The loop runs for M = 1 too.
struct RestirPick {
    uint32_t k;
    float ua, ub, wsum, fac;
    F3 wi;
    float tmax;
    bool taken;
};
__device__ __forceinline__ RestirPick restir_pick(const float4* lights, const float* cdf, uint32_t last, uint32_t search_steps, uint32_t M, uint32_t c0,
                                                  uint32_t c1, uint32_t seed_lo, uint32_t seed_hi, F3 o, F3 n, bool active) {
    RestirPick p;
    p.k = 0u;
    p.ua = p.ub = p.wsum = p.fac = 0.0f;
    p.wi = f3(1.0f, 1.0f, 1.0f);
    p.taken = false;
    float y_dist = 0.0f;
    for (uint32_t j = 0; j < M; ++j) {
        const U4 r = philox4x32_10<true>(c0, c1, 0xFFFFFFFDu, j, seed_lo, seed_hi);
        const float u = u01(r.x);   // the smallest k with u < cdf[k]
        const uint32_t k = table_search(last, search_steps, [&](uint32_t mid) { return u < cdf[mid]; });
        const float ua = u01(r.y), ub = u01(r.z);
        const LightSample ls = light_sample<false>(lights, k, o, n, ua, ub);
        const float fac = direct_light_factor<false>(ls);
        const float l = (0.2126f * ls.Le.x + 0.7152f * ls.Le.y) + 0.0722f * ls.Le.z;
        const float w = l * fac;
        if (active && ls.ok && w > 0.0f && w < INFINITY) {   // the candidate counts (a NaN does not)
            p.wsum = p.wsum + w;
            if (!p.taken || u01(r.w) * p.wsum < w) {
                p.k = k;
                p.ua = ua;
                p.ub = ub;
                p.fac = fac;
                p.wi = ls.wi;
                y_dist = ls.dist;
            }
            p.taken = true;
        }
    }
    p.tmax = y_dist * 0.9990234375f;
    return p;
}

// What both kernels start from: the lane's pixel of the wave's tile and, at a surface pixel, the point its shadow rays leave from.
struct RestirPixel {
    uint32_t px, py, pixel;
    bool inside, surface;
    F3 o, n, albedo;
    float t;
};
__device__ __forceinline__ RestirPixel restir_pixel(const RestirPass& P, const TileWalk& T) {
    RestirPixel X;
    X.px = T.tx0 + (T.lane & 7u), X.py = T.ty0 + (T.lane >> 3);
    X.inside = X.px < P.W && X.py < P.H;
    X.pixel = 0u;
    X.surface = false;
    X.o = f3(1.0f, 1.0f, 1.0f), X.n = f3(0.0f, 0.0f, 0.0f), X.albedo = f3(0.0f, 0.0f, 0.0f);
    X.t = 0.0f;
    if (X.inside) {
        X.pixel = X.py * P.W + X.px;
        const float4 g = P.nc[X.pixel];
        const float4 a = P.ad[X.pixel];
        X.surface = g.w == 0.0f;
        if (X.surface) {
            X.n = f3(g.x, g.y, g.z);
            X.o = guide_origin(P, X.px, X.py, a.w, X.n);
            X.albedo = f3(a.x, a.y, a.z);
            X.t = a.w;
        }
    }
    return X;
}
// a wave's sum of a per-lane count, added to total `which` by lane 0 when there is anything to add
__device__ __forceinline__ void restir_total(const RestirPass& P, uint32_t lane, int which, uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_down((int)v, off);
    const uint32_t slot = (blockIdx.y * gridDim.x + blockIdx.x) & (MPT_RS_SLOTS - 1u);
    if (lane == 0u && v != 0u) atomicAdd(P.totals() + slot * MPT_RS_SLOT_WORDS + which, (unsigned long long)v);
}

// ---- step A: the round's initial reservoirs ---------------------------------------------------------------------------------------------
template <int WALK>
__global__ __launch_bounds__(256) void k_restir_initial(SceneDev sc, AccelDev ac, RestirPass P) {
    const TileWalk T = tile_walk<WALK>(sc, ac);
    if (T.tx0 >= P.W || T.ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const RestirPixel X = restir_pixel(P, T);
    // what the end needs from the pass, in VECTOR registers (as direct_pass: the walk holds the scalar file)
    uint4* initial = P.initial;
    uint32_t* traced = P.traced();
    asm volatile("" : "+v"(initial), "+v"(traced));
    RestirPick y;
    y.k = 0u;
    y.ua = y.ub = y.wsum = y.fac = 0.0f;
    bool holds = false, live = false;
    if (P.n_lights != 0u && __ballot(X.surface) != 0ull) {   // (wave-uniform: no lights or no surface pixel, every reservoir of the tile is EMPTY)
        const uint32_t search_steps = __builtin_amdgcn_readfirstlane(table_search_steps(P.n_lights));
        const uint32_t M = __builtin_amdgcn_readfirstlane(P.M);
        y = restir_pick(P.lights, P.cdf, P.n_lights - 1u, search_steps, M, X.pixel, P.sample_begin + P.round, P.seed_lo, P.seed_hi, X.o, X.n, X.surface);
        live = y.taken;
        if (__ballot(live) != 0ull) {   // (wave-uniform)
            const bool hit = any_hit<WALK>(sc, ac, T, X.o, y.wi, y.tmax, live);
            holds = live && !hit;
        }
    }
    if (X.inside) {
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
        if (holds) {
            a = make_uint4(y.k, __float_as_uint(y.ua), __float_as_uint(y.ub), __float_as_uint(y.wsum));
            b = make_uint4(__float_as_uint(y.fac), 1u, 0u, 0u);
        }
        initial[2u * (size_t)X.pixel] = a;
        initial[2u * (size_t)X.pixel + 1u] = b;
        if (live) {
            traced[X.pixel] += 1u;
            if (holds) traced[P.n_pixels + X.pixel] += 1u;   // (RestirPass::unoccluded)
        }
    }
    if (P.round == 0u) restir_total(P, T.lane, MPT_RS_SURFACE, X.surface ? 1u : 0u);
    restir_total(P, T.lane, MPT_RS_INITIAL, live ? 1u : 0u);
    restir_total(P, T.lane, MPT_RS_UNOCCLUDED, holds ? 1u : 0u);
}

// ---- steps B-E: merge, final ray, normalisation, contribution ------------------------------------------------------------------------------
// Neighbour i of the lane's pixel in this round: the offset from the block philox(pixel, s, MPT_RESTIR_WORD2, i), and r.z for the take.
struct RestirTap {
    int qx, qy;
    bool off_centre;
    float uz;
};
__device__ __forceinline__ RestirTap restir_tap(const RestirPass& P, const RestirPixel& X, uint32_t s, uint32_t i, int R, float span) {
    const U4 r = philox4x32_10<true>(X.pixel, s, MPT_RESTIR_WORD2, i, P.seed_lo, P.seed_hi);
    const int dx = min((int)(u01(r.x) * span), 2 * R) - R, dy = min((int)(u01(r.y) * span), 2 * R) - R;
    RestirTap t;
    t.qx = (int)X.px + dx;
    t.qy = (int)X.py + dy;
    t.off_centre = dx != 0 || dy != 0;
    t.uz = u01(r.z);
    return t;
}
template <int WALK, bool UNBIASED>
__global__ __launch_bounds__(256) void k_restir_merge(SceneDev sc, AccelDev ac, RestirPass P) {
    const TileWalk T = tile_walk<WALK>(sc, ac);
    if (T.tx0 >= P.W || T.ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const RestirPixel X = restir_pixel(P, T);
    const bool last_round = P.round + 1u == P.sample_count;
    if (X.inside && !X.surface && last_round) P.out[X.pixel] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);   // (its counts are the host's zeros)
    if (__ballot(X.surface) == 0ull) return;   // (wave-uniform: nothing to shade in this tile)
    float4* out = P.out;
    float4* Sg = P.S;
    asm volatile("" : "+v"(out), "+v"(Sg));
    const uint32_t s = P.sample_begin + P.round;
    const uint32_t K = __builtin_amdgcn_readfirstlane(P.K);
    const int R = (int)P.R;
    const float span = (float)(2 * R + 1);
    // step B: the pixel's own reservoir, then the neighbours'
    bool held = false, own = false;
    uint32_t yk = 0u, accepted = 0u, n_accepted = 0u;
    float yua = 0.0f, yub = 0.0f, yfac = 0.0f, Wp = 0.0f;
    if (X.surface && P.n_lights != 0u) {
        const uint4 a = P.initial[2u * (size_t)X.pixel], b = P.initial[2u * (size_t)X.pixel + 1u];
        if (b.y & 1u) {
            held = own = true;
            yk = a.x, yua = __uint_as_float(a.y), yub = __uint_as_float(a.z), Wp = __uint_as_float(a.w), yfac = __uint_as_float(b.x);
        }
        for (uint32_t i = 0; i < K; ++i) {
            const RestirTap t = restir_tap(P, X, s, i, R, span);
            if (!(t.off_centre && t.qx >= 0 && t.qx < (int)P.W && t.qy >= 0 && t.qy < (int)P.H)) continue;
            const uint32_t q = (uint32_t)t.qy * P.W + (uint32_t)t.qx;
            const float4 g = P.nc[q];
            const float tq = P.ad[q].w;
            if (!(g.w == 0.0f && dot3(X.n, f3(g.x, g.y, g.z)) >= P.normal_threshold && fabsf(tq - X.t) <= P.depth_tolerance * X.t)) continue;
            accepted |= 1u << i;
            n_accepted += 1u;
            const uint4 qa = P.initial[2u * (size_t)q], qb = P.initial[2u * (size_t)q + 1u];
            if (!(qb.y & 1u)) continue;
            // q's sample seen from this pixel: the same light_sample with another (o, n)
            const float ua = __uint_as_float(qa.y), ub = __uint_as_float(qa.z);
            const LightSample ls = light_sample<false>(P.lights, qa.x, X.o, X.n, ua, ub);
            const float fac = direct_light_factor<false>(ls);
            const float w = __uint_as_float(qa.w) * (fac / __uint_as_float(qb.x));
            if (ls.ok && w > 0.0f && w < INFINITY) {
                Wp = Wp + w;
                if (!held || t.uz * Wp < w) {
                    yk = qa.x, yua = ua, yub = ub, yfac = fac;
                    own = false;
                }
                held = true;
            }
        }
    }
    if (held && last_round) {   // (an empty pick is the host's zeros)
        P.pick[2u * (size_t)X.pixel] = make_uint4(yk, __float_as_uint(yua), __float_as_uint(yub), __float_as_uint(Wp));
        P.pick[2u * (size_t)X.pixel + 1u] = make_uint4(__float_as_uint(yfac), own ? 3u : 1u, 0u, 0u);
    }
    uint32_t n_final = 0u, n_correction = 0u, n_unoccluded = 0u, c = 1u;
    F3 Le = f3(0.0f, 0.0f, 0.0f);
    bool go = held;   // the round goes on to the normalisation
    if (__ballot(held) != 0ull) {   // (wave-uniform)
        // step C: y from this pixel, and its ray unless the pixel's own step A has traced it
        F3 wi = f3(1.0f, 1.0f, 1.0f);
        float tmax = 0.0f;
        if (held) {
            const LightSample ly = light_sample<false>(P.lights, yk, X.o, X.n, yua, yub);
            wi = ly.wi;
            tmax = ly.dist * 0.9990234375f;
            Le = ly.Le;
        }
        const bool fin = held && !own;
        if (__ballot(fin) != 0ull) {   // (wave-uniform)
            const bool hit = any_hit<WALK>(sc, ac, T, X.o, wi, tmax, fin);
            if (fin) {
                n_final = 1u;
                if (hit) go = false;
                else n_unoccluded += 1u;
            }
        }
        // step D: which of the accepted neighbours could have produced y — one any_hit per neighbour index over the whole wave
        if (__ballot(go && accepted != 0u) != 0ull) {   // (wave-uniform)
            for (uint32_t i = 0; i < K; ++i) {
                bool live = false;
                F3 oq = f3(1.0f, 1.0f, 1.0f), wq = f3(1.0f, 1.0f, 1.0f);
                float tq_max = 0.0f;
                if (go && ((accepted >> i) & 1u) != 0u) {
                    const RestirTap t = restir_tap(P, X, s, i, R, span);
                    const uint32_t q = (uint32_t)t.qy * P.W + (uint32_t)t.qx;
                    const float4 g = P.nc[q];
                    const F3 nq = f3(g.x, g.y, g.z);
                    oq = guide_origin(P, (uint32_t)t.qx, (uint32_t)t.qy, P.ad[q].w, nq);
                    const LightSample ls = light_sample<false>(P.lights, yk, oq, nq, yua, yub);
                    const float fac = direct_light_factor<false>(ls);
                    live = ls.ok && fac > 0.0f && fac < INFINITY;
                    wq = ls.wi;
                    tq_max = ls.dist * 0.9990234375f;
                }
                if constexpr (UNBIASED) {
                    if (__ballot(live) == 0ull) continue;   // (wave-uniform)
                    const bool hit = any_hit<WALK>(sc, ac, T, oq, wq, tq_max, live);
                    if (live) {
                        n_correction += 1u;
                        if (!hit) {
                            n_unoccluded += 1u;
                            c += 1u;
                        }
                    }
                } else {
                    if (live) c += 1u;
                }
            }
        }
    }
    // step E, and the end of the round
    if (X.surface) {
        float4 S = Sg[X.pixel];
        if (go) {
            const float l = (0.2126f * Le.x + 0.7152f * Le.y) + 0.0722f * Le.z;
            const float Fy = (Wp / (float)(P.M * c)) / l;
            S.x = S.x + Le.x * Fy;
            S.y = S.y + Le.y * Fy;
            S.z = S.z + Le.z * Fy;
            Sg[X.pixel] = S;
        }
        if (last_round) {
            const float fN = (float)P.sample_count;
            out[X.pixel] = make_float4((X.albedo.x * 0.31830987f) * (S.x / fN), (X.albedo.y * 0.31830987f) * (S.y / fN),
                                       (X.albedo.z * 0.31830987f) * (S.z / fN), 1.0f);
        }
        const uint32_t n_traced = n_final + n_correction;
        if (n_traced != 0u) ((uint32_t*)(out + P.n_pixels))[X.pixel] += n_traced;                        // (RestirPass::traced, unoccluded)
        if (n_unoccluded != 0u) ((uint32_t*)(out + P.n_pixels))[P.n_pixels + X.pixel] += n_unoccluded;
    }
    restir_total(P, T.lane, MPT_RS_FINAL, n_final);
    restir_total(P, T.lane, MPT_RS_CORRECTION, n_correction);
    restir_total(P, T.lane, MPT_RS_UNOCCLUDED, n_unoccluded);
    restir_total(P, T.lane, MPT_RS_ACCEPTED, n_accepted);
    restir_total(P, T.lane, MPT_RS_FROM_NEIGHBOUR, held && !own ? 1u : 0u);
}
