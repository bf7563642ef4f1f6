// mpt_restir_temporal.h — temporal reservoir reuse in the direct pass over a camera path (included by mpt_hip.hip after mpt_restir.h; the
// contract is the "temporal reservoir reuse" section of include/mpt.h, tests/restir_temporal_ref.py restates it in numpy, DESIGN.md §21
// has the registers):
//   k_restir_temporal<WALK, UNBIASED>   steps T-E of a frame: the tap into the previous frame's reservoirs (the reprojection of
//                               k_tp_reproject, one nearest pixel), the merge with the pixel's own reservoir, the final ray, the
//                               normalisation (UNBIASED: one correction ray from last frame's point) and the new reservoir
// Step A of the frame is k_restir_initial (mpt_restir.h) as it is, launched before this kernel on the same RestirPass with round 0 of a
// one-sample range that begins at the frame number.  The mapping is direct_pass's: a 16 x 16 block per workgroup, a wave per 8 x 8 tile,
// a lane per pixel, the scene staged by tile_walk.  The reprojection and the three 16-byte gathers of a tap are per lane; each of the two
// rays is one any_hit over the wave behind a ballot.
#pragma once
#include "mpt_restir.h"

#define MPT_RESTIR_TEMPORAL_WORD2 0xFFFFFFFBu   // Philox counter word 2 of the take of step B: nobody else's (...FC is the spatial neighbour draw)

// A camera as guide_origin takes it ("any pass with a camera"): the history's, for the point frame f-1 shaded at a pixel
struct RestirCamera {
    F3 cam, first, vu, vv;
    float fW, fH;
};

// A temporal reservoir in memory: two uint4 per pixel, (k, ua, ub, wsum) (fac, flags, Mh, 0) — RestirPass's with the count Mh of the
// candidates it stands for.  A reservoir that does not hold is zeros but for Mh; a pixel that is no surface has Mh = 0 too.
struct RestirTemporalPass {
    RestirPass base;             // the frame as k_restir_initial sees it: initial = this frame's reservoirs after step A, round = 0,
                                 // sample_begin = the frame number, sample_count = 1; S and pick are unused
    const uint4* res_in;         // the previous frame's reservoirs and its guide, at the history's camera — unused by MPT_TP_NONE
    const float4* guide_in;
    uint4* res_out;              // this frame's reservoirs and its guide (the current guide, packed as k_tp_pack packs it)
    float4* guide_out;
    uint32_t mode;               // MPT_TP_NONE, MPT_TP_SAME or MPT_TP_MOVED (mpt_temporal.h)
    uint32_t cap;                // C * m: the most a history may count for
    RestirCamera cam_h;          // the history's camera, and from it as TpFrame:
    F3 nn, fc;                   // nn = cross(vu', vv'), fc = first' - cam',
    float fcnn, uu, vvl;         // dot(fc, nn), dot(vu', vu'), dot(vv', vv')
};

template <int WALK, bool UNBIASED>
__global__ __launch_bounds__(256) void k_restir_temporal(SceneDev sc, AccelDev ac, RestirTemporalPass TP) {
    const RestirPass& P = TP.base;
    const TileWalk T = tile_walk<WALK>(sc, ac);
    if (T.tx0 >= P.W || T.ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    const RestirPixel X = restir_pixel(P, T);
    if (X.inside) {
        const float4 g = P.nc[X.pixel];
        TP.guide_out[X.pixel] = make_float4(g.x, g.y, g.z, g.w == 2.0f ? MPT_TP_MISS_T : P.ad[X.pixel].w);
        if (!X.surface) {   // (its counts are the host's zeros)
            P.out[X.pixel] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
            TP.res_out[2u * (size_t)X.pixel] = make_uint4(0u, 0u, 0u, 0u);
            TP.res_out[2u * (size_t)X.pixel + 1u] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (__ballot(X.surface) == 0ull) return;   // (wave-uniform: nothing to shade in this tile)
    float4* out = P.out;
    uint4* res_out = TP.res_out;
    asm volatile("" : "+v"(out), "+v"(res_out));
    const uint32_t M = P.M;
    // step B.1: the pixel's own reservoir
    bool held = false, own = false;
    uint32_t yk = 0u;
    float yua = 0.0f, yub = 0.0f, yfac = 0.0f, Wp = 0.0f;
    if (X.surface) {
        const uint4 a = P.initial[2u * (size_t)X.pixel], b = P.initial[2u * (size_t)X.pixel + 1u];
        if (b.y & 1u) {
            held = own = true;
            yk = a.x, yua = __uint_as_float(a.y), yub = __uint_as_float(a.z), Wp = __uint_as_float(a.w), yfac = __uint_as_float(b.x);
        }
    }
    // step T: the one tap into the previous frame, then the rest of step B
    bool accepted = false;
    int qx = 0, qy = 0;
    uint32_t Mc = 0u;
    if (X.surface && TP.mode != MPT_TP_NONE) {
        bool tap = false;
        if (TP.mode == MPT_TP_SAME) {
            qx = (int)X.px, qy = (int)X.py;
            tap = true;
        } else {
            const float uvx = ((float)X.px + 0.5f) / P.fW, uvy = ((float)X.py + 0.5f) / P.fH;
            const F3 dv = (P.first + uvx * P.vu + uvy * P.vv) - P.cam;
            const F3 d = dv * (1.0f / sqrtf(tp_dot(dv, dv)));
            const F3 r = (P.cam + X.t * d) - TP.cam_h.cam;
            const float s = TP.fcnn / tp_dot(r, TP.nn);
            const F3 q3 = s * r - TP.fc;
            const float u = tp_dot(q3, TP.cam_h.vu) / TP.uu, v = tp_dot(q3, TP.cam_h.vv) / TP.vvl;
            const float fx = u * P.fW - 0.5f, fy = v * P.fH - 0.5f;
            if (s > 0.0f && s < __builtin_inff() && fx >= -1.0f && fx < P.fW && fy >= -1.0f && fy < P.fH) {   // (a NaN fails here, before any conversion)
                qx = (int)floorf(fx + 0.5f), qy = (int)floorf(fy + 0.5f);
                if (qx >= 0 && qx < (int)P.W && qy >= 0 && qy < (int)P.H) {
                    const float4 gq = TP.guide_in[(size_t)qy * P.W + (size_t)qx];
                    const float rl = sqrtf(tp_dot(r, r));
                    tap = gq.w < __builtin_inff() && fabsf(gq.w - rl) <= P.depth_tolerance * rl && tp_dot(X.n, F3{gq.x, gq.y, gq.z}) >= P.normal_threshold;
                }
            }
        }
        if (tap) {
            const size_t q = (size_t)qy * P.W + (size_t)qx;
            const uint4 qb = TP.res_in[2u * q + 1u];
            const uint32_t Mh = qb.z;
            if (Mh != 0u) {
                accepted = true;
                Mc = min(Mh, TP.cap);
                if (qb.y & 1u) {
                    // q's sample seen from this pixel: the same light_sample with another (o, n)
                    const uint4 qa = TP.res_in[2u * q];
                    const float ua = __uint_as_float(qa.y), ub = __uint_as_float(qa.z);
                    const LightSample ls = light_sample<false>(P.lights, qa.x, X.o, X.n, ua, ub);
                    const float fac = direct_light_factor<false>(ls);
                    const float w = (__uint_as_float(qa.w) * (fac / __uint_as_float(qb.x))) * ((float)Mc / (float)Mh);
                    if (ls.ok && w > 0.0f && w < INFINITY) {
                        Wp = Wp + w;
                        if (!held || u01(philox4x32_10<true>(X.pixel, P.sample_begin, MPT_RESTIR_TEMPORAL_WORD2, 0u, P.seed_lo, P.seed_hi).z) * Wp < w) {
                            yk = qa.x, yua = ua, yub = ub, yfac = fac;
                            own = false;
                        }
                        held = true;
                    }
                }
            }
        }
    }
    uint32_t n_final = 0u, n_correction = 0u, n_unoccluded = 0u, Z = M;
    F3 Le = f3(0.0f, 0.0f, 0.0f);
    bool go = held;   // the frame goes on to the normalisation
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
        // step D: could last frame's point at q have produced y?  (the history guide is read again, not kept across the walk)
        if (__ballot(go && accepted) != 0ull) {   // (wave-uniform)
            bool live = false;
            F3 oq = f3(1.0f, 1.0f, 1.0f), wq = f3(1.0f, 1.0f, 1.0f);
            float tq_max = 0.0f;
            if (go && accepted) {
                const float4 gq = TP.guide_in[(size_t)qy * P.W + (size_t)qx];
                const F3 nq = f3(gq.x, gq.y, gq.z);
                oq = guide_origin(TP.cam_h, (uint32_t)qx, (uint32_t)qy, gq.w, nq);
                const LightSample ls = light_sample<false>(P.lights, yk, oq, nq, yua, yub);
                const float fac = direct_light_factor<false>(ls);
                live = ls.ok && fac > 0.0f && fac < INFINITY;
                wq = ls.wi;
                tq_max = ls.dist * 0.9990234375f;
            }
            if constexpr (UNBIASED) {
                if (__ballot(live) != 0ull) {   // (wave-uniform)
                    const bool hit = any_hit<WALK>(sc, ac, T, oq, wq, tq_max, live);
                    if (live) {
                        n_correction = 1u;
                        if (!hit) {
                            n_unoccluded += 1u;
                            Z += Mc;
                        }
                    }
                }
            } else {
                if (live) Z += Mc;
            }
        }
    }
    // step E: the contribution and the frame's reservoir
    if (X.surface) {
        const uint32_t Mnew = M + (accepted ? Mc : 0u);
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, Mnew, 0u);
        F3 S = f3(0.0f, 0.0f, 0.0f);
        if (go) {
            const float l = (0.2126f * Le.x + 0.7152f * Le.y) + 0.0722f * Le.z;
            const float Fy = (Wp / (float)Z) / l;
            S = f3(Le.x * Fy, Le.y * Fy, Le.z * Fy);
            a = make_uint4(yk, __float_as_uint(yua), __float_as_uint(yub), __float_as_uint(Wp * ((float)Mnew / (float)Z)));
            b = make_uint4(__float_as_uint(yfac), own ? 3u : 1u, Mnew, 0u);
        }
        out[X.pixel] = make_float4((X.albedo.x * 0.31830987f) * (S.x / 1.0f), (X.albedo.y * 0.31830987f) * (S.y / 1.0f),
                                   (X.albedo.z * 0.31830987f) * (S.z / 1.0f), 1.0f);
        res_out[2u * (size_t)X.pixel] = a;
        res_out[2u * (size_t)X.pixel + 1u] = b;
        const uint32_t n_traced = n_final + n_correction;
        if (n_traced != 0u) ((uint32_t*)(out + P.n_pixels))[X.pixel] += n_traced;                        // (RestirPass::traced, unoccluded)
        if (n_unoccluded != 0u) ((uint32_t*)(out + P.n_pixels))[P.n_pixels + X.pixel] += n_unoccluded;
    }
    restir_total(P, T.lane, MPT_RS_FINAL, n_final);
    restir_total(P, T.lane, MPT_RS_CORRECTION, n_correction);
    restir_total(P, T.lane, MPT_RS_UNOCCLUDED, n_unoccluded);
    restir_total(P, T.lane, MPT_RS_ACCEPTED, accepted ? 1u : 0u);   // (mpt_restir_temporal_info: history_accepted, samples_from_history)
    restir_total(P, T.lane, MPT_RS_FROM_NEIGHBOUR, held && !own ? 1u : 0u);
}
