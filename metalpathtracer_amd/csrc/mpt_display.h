// mpt_display.h — the display stage (included by mpt_hip.hip after mpt_adaptive.h):
//   k_dp_histogram   256-bin histogram of the source's luminance, four bins per octave (auto-exposure only)
//   k_dp_exposure    one wave: prefix sum, key bin, target, smoothing -> the scale k_dp_present and the host read
//   k_dp_present     exposure, tone curve, table encoding -> one RGBA8 word per pixel, and the count of clipped pixels
// The stage is specified exactly in include/mpt.h (mpt_display_params) and restated in numpy in tests/display_ref.py; DESIGN.md §14
// has the layout and the measured times.  Only + - * / and comparisons, one IEEE operation each (-ffp-contract=off); the bins come
// from the bits of the luminance and the code from comparisons with a committed table (mpt_display_table.h): no pow, exp or log
// runs here, so the device and numpy agree bit for bit.
#pragma once
#include "mpt_display_table.h"

#define MPT_DP_BINS 256u
#define MPT_DP_BIN_FIRST 380u   // float_bits(2^-32) >> 21
#define MPT_DP_BIN_LAST 635u    // the quarter octave below 2^32 ... and everything above it
#define MPT_DP_V_MAX 65504.0f
#define MPT_DP_NO_BIN 0xFFFFFFFFu

enum { MPT_DP_SRC_RAW = 0,     // c = the source's float4
       MPT_DP_SRC_DIV = 1,     // c = the HDR sum / samples
       MPT_DP_SRC_TILE = 2 };  // c = the HDR sum / (float)count of the pixel's 8 x 8 tile, 0 where the count is 0

// What k_dp_exposure leaves for k_dp_present and the host: the first 32 bytes are mpt_display_info; `kept` is the auto scale the next
// call smooths from (have_kept = 0: none).
struct DpState {
    float scale, auto_scale;
    uint32_t key_bin, _pad;
    unsigned long long counted, clipped;
    float kept;
    uint32_t have_kept;
};

struct DpSource {
    const float4* color;
    const uint32_t* tile_count;   // MPT_DP_SRC_TILE: samples per tile, row-major, tiles_x per row
    uint32_t n, W, tiles_x;       // n = W * H pixels
    float samples;                // MPT_DP_SRC_DIV
};

__device__ __forceinline__ float dp_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

template <int SRC>
__device__ __forceinline__ float4 dp_load(const DpSource& S, uint32_t i) {
    const float4 c = S.color[i];
    if (SRC == MPT_DP_SRC_DIV) return make_float4(c.x / S.samples, c.y / S.samples, c.z / S.samples, c.w);
    if (SRC == MPT_DP_SRC_TILE) {
        const uint32_t y = i / S.W, x = i - y * S.W;
        const uint32_t cnt = S.tile_count[(y >> 3) * S.tiles_x + (x >> 3)];
        if (cnt == 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float f = (float)cnt;
        return make_float4(c.x / f, c.y / f, c.z / f, c.w);
    }
    return c;
}

// Linear pixel index, grid-stride: a wave reads 1 KB contiguously per trip.  The workgroup counts into 1 KB of LDS and flushes
// the bins it touched with one global add each; counts are integers, so the result does not depend on the order of the adds.
// AGG: a sky or a wall puts all 64 lanes in one bin, 64 same-address LDS adds.  The lanes that share the first counted lane's bin
// are added by that lane alone (one ballot, one popcount); the others add for themselves.
template <int SRC, bool AGG>
__global__ __launch_bounds__(256) void k_dp_histogram(DpSource S, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[MPT_DP_BINS];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * 256u;
    // (every lane of a wave takes the same number of trips: the ballots below are over whole waves)
    for (uint32_t base = blockIdx.x * 256u; base < S.n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool counted = false;
        uint32_t b = 0;
        if (i < S.n) {
            const float4 c = dp_load<SRC>(S, i);
            const float l = dp_lum(c.x, c.y, c.z);
            counted = l > 0.0f && l < __builtin_inff();
            const uint32_t e = __float_as_uint(l) >> 21;
            b = min(max(e, MPT_DP_BIN_FIRST), MPT_DP_BIN_LAST) - MPT_DP_BIN_FIRST;
        }
        if (AGG) {
            const unsigned long long todo = __ballot(counted);
            if (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const uint32_t lb = (uint32_t)__shfl((int)b, leader);
                const bool same = counted && b == lb;
                const unsigned long long group = __ballot(same);
                if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&bins[lb], (uint32_t)__popcll(group));
                else if (counted && !same) atomicAdd(&bins[b], 1u);
            }
        } else if (counted) {
            atomicAdd(&bins[b], 1u);
        }
    }
    __syncthreads();
    const uint32_t v = bins[threadIdx.x];
    if (v) atomicAdd(&hist[threadIdx.x], v);
}

struct DpExposure {
    float exposure, key, adaptation;   // resolved by the host: exposure > 0, key > 0, adaptation in (0, 1) or 0 = none
    uint32_t percentile;               // 1..100
    int32_t auto_exposure;
};

// One wave: lane i owns bins 4 i .. 4 i + 3.
__global__ __launch_bounds__(64) void k_dp_exposure(const uint32_t* __restrict__ hist, DpExposure E, DpState* __restrict__ st) {
    const uint32_t lane = threadIdx.x;
    if (!E.auto_exposure) {   // (the kept auto scale stays as it is)
        if (lane == 0) {
            st->scale = E.exposure * 1.0f;
            st->auto_scale = 1.0f;
            st->key_bin = MPT_DP_NO_BIN;
            st->_pad = 0;
            st->counted = 0;
            st->clipped = 0;
        }
        return;
    }
    const uint4 h = ((const uint4*)hist)[lane];
    const uint32_t own = (h.x + h.y) + (h.z + h.w);   // (at most W * H < 2^31)
    uint32_t inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= (uint32_t)d) inc += up;
    }
    const uint32_t N = (uint32_t)__shfl((int)inc, 63);
    const unsigned long long need = (unsigned long long)N * E.percentile;
    // the smallest bin of this lane with cum(b) * 100 >= N * percentile, or 4 if it has none
    const unsigned long long c0 = inc - own + h.x, c1 = c0 + h.y, c2 = c1 + h.z, c3 = c2 + h.w;
    const uint32_t k = c0 * 100ull >= need ? 0u : c1 * 100ull >= need ? 1u : c2 * 100ull >= need ? 2u : c3 * 100ull >= need ? 3u : 4u;
    const unsigned long long found = __ballot(k < 4u);   // (never empty: the last lane's c3 is N and percentile <= 100)
    const int first = __ffsll((long long)found) - 1;
    const uint32_t key_bin = 4u * (uint32_t)first + (uint32_t)__shfl((int)k, first);
    if (lane == 0) {
        float auto_scale = 1.0f;
        uint32_t kb = MPT_DP_NO_BIN;
        if (N != 0) {
            kb = key_bin;
            const float edge = __uint_as_float((kb + MPT_DP_BIN_FIRST) << 21);
            const float target = E.key / edge;
            const float p = st->kept;
            auto_scale = st->have_kept && E.adaptation > 0.0f ? p + (target - p) * E.adaptation : target;
        }
        st->kept = auto_scale;
        st->have_kept = 1;
        st->scale = E.exposure * auto_scale;
        st->auto_scale = auto_scale;
        st->key_bin = kb;
        st->_pad = 0;
        st->counted = N;
        st->clipped = 0;
    }
}

struct DpTone {
    const float* table;   // the 255 thresholds of the transfer function (device memory)
    float ww;             // REINHARD: white * white
};

template <int TONE>
__device__ __forceinline__ float dp_curve(float c, float scale, float ww) {
    const float x = c * scale;
    float v = x > 0.0f ? x : 0.0f;   // (a NaN becomes 0)
    v = v < MPT_DP_V_MAX ? v : MPT_DP_V_MAX;
    if (TONE == MPT_TONE_REINHARD) return (v * (1.0f + v / ww)) / (1.0f + v);
    if (TONE == MPT_TONE_ACES) return (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f);
    return v;
}

// The number of thresholds <= y, y in [0, 1]: eight steps over T[1..255] (index k - 1), no branch.  Step s reads at most
// index 255 - s.
__device__ __forceinline__ uint32_t dp_code(const float* T, float y) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t s = 128; s; s >>= 1) c += T[c + s - 1] <= y ? s : 0u;
    return c;
}

template <int TONE>
__device__ __forceinline__ uint32_t dp_pixel(const float* T, float4 c, float scale, float ww, bool& clipped) {
    const float r = dp_curve<TONE>(c.x, scale, ww), g = dp_curve<TONE>(c.y, scale, ww), b = dp_curve<TONE>(c.z, scale, ww);
    clipped = r >= 1.0f || g >= 1.0f || b >= 1.0f;
    const uint32_t cr = dp_code(T, r < 1.0f ? r : 1.0f), cg = dp_code(T, g < 1.0f ? g : 1.0f), cb = dp_code(T, b < 1.0f ? b : 1.0f);
    return cr | cg << 8 | cb << 16 | 255u << 24;
}

// PX = 1: one pixel per thread, 4-byte stores (256 B per wave).  PX = 4: four consecutive pixels per thread, one 16-byte store (the
// last thread of an image whose size is no multiple of four stores its pixels one by one).  Both give the same bytes.
template <int SRC, int TONE, int PX>
__global__ __launch_bounds__(256) void k_dp_present(DpSource S, DpTone P, DpState* __restrict__ st, uint32_t* __restrict__ out) {
    __shared__ float T[256];
    T[threadIdx.x] = threadIdx.x < 255u ? P.table[threadIdx.x] : __builtin_inff();
    const float scale = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(st->scale)));
    __syncthreads();
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)PX;
    uint32_t n_clipped = 0;
    if (PX == 1) {
        bool clip = false;
        if (i0 < S.n) out[i0] = dp_pixel<TONE>(T, dp_load<SRC>(S, i0), scale, P.ww, clip);
        n_clipped = (uint32_t)__popcll(__ballot(clip));
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
        bool clip[4] = {false, false, false, false};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + (uint32_t)j < S.n) w[j] = dp_pixel<TONE>(T, dp_load<SRC>(S, i0 + (uint32_t)j), scale, P.ww, clip[j]);
        if (i0 + 3u < S.n) {
            *(uint4*)(out + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (i0 + (uint32_t)j < S.n) out[i0 + (uint32_t)j] = w[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) n_clipped += (uint32_t)__popcll(__ballot(clip[j]));
    }
    if ((threadIdx.x & 63u) == 0 && n_clipped) atomicAdd(&st->clipped, (unsigned long long)n_clipped);
}

template <bool AGG>
static const void* dp_histogram_kernel_of(int src) {
    return src == MPT_DP_SRC_RAW ? (const void*)k_dp_histogram<MPT_DP_SRC_RAW, AGG>
           : src == MPT_DP_SRC_DIV ? (const void*)k_dp_histogram<MPT_DP_SRC_DIV, AGG> : (const void*)k_dp_histogram<MPT_DP_SRC_TILE, AGG>;
}
static const void* dp_histogram_kernel(int src, bool agg) { return agg ? dp_histogram_kernel_of<true>(src) : dp_histogram_kernel_of<false>(src); }

template <int SRC, int PX>
static const void* dp_present_kernel_of(int tone) {
    return tone == MPT_TONE_CLAMP ? (const void*)k_dp_present<SRC, MPT_TONE_CLAMP, PX>
           : tone == MPT_TONE_REINHARD ? (const void*)k_dp_present<SRC, MPT_TONE_REINHARD, PX> : (const void*)k_dp_present<SRC, MPT_TONE_ACES, PX>;
}
template <int PX>
static const void* dp_present_kernel_px(int src, int tone) {
    return src == MPT_DP_SRC_RAW ? dp_present_kernel_of<MPT_DP_SRC_RAW, PX>(tone)
           : src == MPT_DP_SRC_DIV ? dp_present_kernel_of<MPT_DP_SRC_DIV, PX>(tone) : dp_present_kernel_of<MPT_DP_SRC_TILE, PX>(tone);
}
static const void* dp_present_kernel(int src, int tone, int px) { return px == 4 ? dp_present_kernel_px<4>(src, tone) : dp_present_kernel_px<1>(src, tone); }
