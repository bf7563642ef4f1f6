// mpt_ao.h — ambient occlusion over the first-hit guide buffers (included by mpt_hip.hip after mpt_anyhit.h):
//   k_ao<WALK>   per surface pixel, N Lambert-distributed shadow rays from the bounce ray's origin through an any-hit walk
// and what the per-tile shadow-ray kernels (k_ao, k_direct, k_nee and the cone variants) start from, written once:
//   tile_walk<WALK>      the scene image staged in LDS, the own tree's stack, the wave's 8 x 8 tile
//   any_hit<WALK>        the one dispatch to any_hit_own / any_hit_ref<ALL_LDS>
//   guide_origin         the bounce ray's origin at a surface pixel of the guide buffers
// The pass is specified exactly in include/mpt.h (mpt_ao_params) and restated in numpy in tests/ao_ref.py; DESIGN.md §15 has the layout,
// the lane mapping and the measured times.
#pragma once
#include "mpt_anyhit.h"

enum { MPT_AO_REF = 0, MPT_AO_REF_ALL_LDS = 1, MPT_AO_OWN = 2 };   // WALK: which tree, and whether all of it is in LDS

// A workgroup of four waves takes a 16 x 16 pixel block, each wave one 8 x 8 tile of it (as k_dn_guide): (tx0, ty0) is the tile's first
// pixel.  Every wave stages, also one whose tile lies outside the image (the callers return after this, wave-uniformly).
struct TileWalk {
    LdsNodes lds;
    OtStack st;
    uint32_t lane, tx0, ty0;
};
template <int WALK>
__device__ __forceinline__ TileWalk tile_walk(const SceneDev& sc, const AccelDev& ac) {
    extern __shared__ float4 lds_raw[];
    if (WALK == MPT_AO_OWN) ot_stage(sc, ac, lds_raw);
    else stage_nodes(sc, lds_raw);
    TileWalk T = {};
    T.lds = (LdsNodes)lds_raw;
    if (WALK == MPT_AO_OWN) T.st = ot_stack(ac, lds_raw, 0u);
    const uint32_t wave = threadIdx.x >> 6;
    T.lane = threadIdx.x & 63u;
    T.tx0 = blockIdx.x * MPT_DN_TILE + (wave & 1u) * 8u;
    T.ty0 = blockIdx.y * MPT_DN_TILE + (wave >> 1) * 8u;
    return T;
}
template <int WALK>
__device__ __forceinline__ bool any_hit(const SceneDev& sc, const AccelDev& ac, const TileWalk& T, F3 o, F3 d, float tmax, bool live) {
    if (WALK == MPT_AO_OWN) {
        uint32_t flags;
        return any_hit_own(ac, sc, T.lds, T.st, o, d, tmax, live, flags);
    }
    return any_hit_ref<WALK == MPT_AO_REF_ALL_LDS>(sc, T.lds, o, d, tmax, live);
}
// The origin of the bounce ray (shade_bounce) at pixel (px, py) of the guide buffers: t = ad.w, n = the normal of nc; P: any pass with a camera.
template <class Pass>
__device__ __forceinline__ F3 guide_origin(const Pass& P, uint32_t px, uint32_t py, float t, F3 n) {
    const float uvx = ((float)px + 0.5f) / P.fW, uvy = ((float)py + 0.5f) / P.fH;
    const F3 dv = (P.first + uvx * P.vu + uvy * P.vv) - P.cam;
    const F3 dc = dv * (1.0f / sqrtf(dot3(dv, dv)));   // normalize3, with the division written out (the lanes diverge here)
    const F3 hitp = P.cam + t * dc;
    return hitp + 0.0001f * n;
}

struct AoPass {
    const float4* ad;            // (albedo, t)
    const float4* nc;            // (normal facing the ray, class)
    float* out;                  // ONE block (one base pointer in scalar registers instead of three):
    uint32_t n_pixels;           //   [0, n)   ao = (N - count) / N, 1 for a pixel that is no surface
                                 //   [n, 2n)  the counts (uint32), 0 for a pixel that is no surface
                                 //   then two 64-bit totals: += surface pixels, += occluded rays (one atomic each per wave that has any)
    __host__ __device__ float* ao() const { return out; }
    __host__ __device__ uint32_t* occluded() const { return (uint32_t*)out + n_pixels; }
    __host__ __device__ unsigned long long* totals() const { return (unsigned long long*)(out + 2u * (size_t)n_pixels); }
    F3 cam, first, vu, vv;
    float fW, fH;
    uint32_t W, H;
    uint32_t sample_begin, sample_count;
    uint32_t group_log2;         // a pixel's samples sit in 2^group_log2 adjacent lanes: min(N, 64) rounded down to a power of two
    float tmax;                  // radius, or +inf
    uint32_t seed_lo, seed_hi;
};

// Lane mapping.  A workgroup of four waves takes a 16 x 16 pixel block, each wave one 8 x 8 tile of it (as k_dn_guide).  With G = 2^group_log2
// lanes per pixel a wave holds 64 / G pixels of its tile at a time — consecutive pixels of the tile's row-major order, so a wave's origins
// lie next to each other — and walks the tile in G chunks; a chunk takes ceil(N / G) rounds, in which lane l of a pixel's group traces
// sample round * G + l.  The count of a pixel is the popcount of its group's bits of the round's ballot, summed over the rounds: no atomics,
// and whatever the mapping, the same N rays per pixel are counted.  A chunk without a surface pixel traces nothing.  A pixel that is
// no surface gets ao = 1, occluded = 0 from the lane that prepared it.
template <int WALK>
__global__ __launch_bounds__(256) void k_ao(SceneDev sc, AccelDev ac, AoPass P) {
    const TileWalk T = tile_walk<WALK>(sc, ac);
    const uint32_t lane = T.lane, tx0 = T.tx0, ty0 = T.ty0;
    if (tx0 >= P.W || ty0 >= P.H) return;   // (wave-uniform: the tile lies outside the image)
    // every lane first prepares ONE pixel of the tile — its class, its normal and the origin of its rays — and the chunks below fetch
    // a pixel's values from the lane that holds them (ds_bpermute): the camera is not needed beyond this point
    float ox = 1.0f, oy = 1.0f, oz = 1.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    uint32_t my_pixel = 0u;
    bool my_surface = false;
    {
        const uint32_t px = tx0 + (lane & 7u), py = ty0 + (lane >> 3);
        if (px < P.W && py < P.H) {
            const uint32_t i = py * P.W + px;
            my_pixel = i;
            const float4 g = P.nc[i];
            const float t = P.ad[i].w;
            my_surface = g.w == 0.0f;
            if (my_surface) {
                const F3 n = f3(g.x, g.y, g.z);
                const F3 o = guide_origin(P, px, py, t, n);
                ox = o.x, oy = o.y, oz = o.z;
                nx = n.x, ny = n.y, nz = n.z;
            } else {
                P.occluded()[i] = 0u;
                P.ao()[i] = 1.0f;
            }
        }
    }
    const uint32_t n_surface = (uint32_t)__popcll(__ballot(my_surface));
    if (n_surface == 0u) return;   // (wave-uniform: nothing to trace in this tile)
    const uint32_t gl = P.group_log2, G = 1u << gl, per_chunk = 64u >> gl;
    const uint32_t slot = lane >> gl, sl = lane & (G - 1u);
    const uint32_t rounds = (P.sample_count + G - 1u) >> gl;
    // What a round or the end of a chunk needs from the pass goes into VECTOR registers (an empty asm makes the value opaque, as in
    // philox4x32_10): the walks below hold the scalar file — scene, tree, exec masks of five nested loops — and the own-tree variant
    // spilled scalar registers with these four in it.
    float* out = P.out;
    uint32_t n_pixels = P.n_pixels, N = P.sample_count, sample_begin = P.sample_begin;
    asm volatile("" : "+v"(out), "+v"(n_pixels), "+v"(N), "+v"(sample_begin));
    uint32_t n_occluded = 0u;
    for (uint32_t chunk = 0; chunk < G; ++chunk) {
        const uint32_t p = chunk * per_chunk + slot;
        const bool surface = __shfl((int)my_surface, (int)p) != 0;
        if (__ballot(surface) == 0ull) continue;   // (wave-uniform)
        const F3 o = f3(__shfl(ox, (int)p), __shfl(oy, (int)p), __shfl(oz, (int)p));
        const F3 n = f3(__shfl(nx, (int)p), __shfl(ny, (int)p), __shfl(nz, (int)p));
        const uint32_t pixel = (uint32_t)__shfl((int)my_pixel, (int)p);
        uint32_t count = 0u;
        for (uint32_t round = 0; round < rounds; ++round) {
            const uint32_t s = (round << gl) + sl;
            const bool live = surface && s < N;
            const U4 r = philox4x32_10<true>(pixel, sample_begin + s, 0xFFFFFFFEu, 0u, P.seed_lo, P.seed_hi);
            const float uz = u01(r.x), uphi = u01(r.y);
            const float z = 2.0f * uz - 1.0f;
            float sn, cs;
            sincos_2pi(uphi, sn, cs);
            const float rr = sqrtf(1.0f - z * z);
            const F3 dir = normalize3(n + f3(rr * cs, rr * sn, z));   // the Lambert direction (PathTracing.h:252-254)
            const bool hit = any_hit<WALK>(sc, ac, T, o, dir, P.tmax, live);
            // the group's G bits of the ballot: shifted down to bit 0, then up until the bits of the groups above fall off
            const unsigned long long mine = (__ballot(hit && live) >> (slot << gl)) << (64u - G);
            count += (uint32_t)__popcll(mine);
        }
        if (surface && sl == 0u) {
            ((uint32_t*)out)[n_pixels + pixel] = count;   // (AoPass::occluded, ao)
            out[pixel] = (float)(N - count) / (float)N;
            n_occluded += count;
        }
    }
    for (int off = 32; off > 0; off >>= 1) n_occluded += (uint32_t)__shfl_down((int)n_occluded, off);
    if (lane == 0u && n_surface != 0u) {
        atomicAdd(P.totals(), (unsigned long long)n_surface);
        if (n_occluded != 0u) atomicAdd(P.totals() + 1, (unsigned long long)n_occluded);
    }
}
