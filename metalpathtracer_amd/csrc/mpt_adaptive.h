// mpt_adaptive.h — device side of adaptive sampling (mpt_render_adaptive; the contract is in include/mpt.h).
//
// After every pass the host runs k_adaptive_eval over the tiles that pass rendered (one wave64 per tile, lane = pixel, as in the
// trace kernels) and compacts the tiles it flags into the next pass's tile list with hipcub::DeviceSelect::Flagged, which keeps
// the order of the full tile table (ensure_tile_order's mix of cheap and expensive tiles).  Lists hold x | y << 16 as the table does.
#pragma once

#include <hipcub/hipcub.hpp>

struct AdaptiveEval {
    const uint32_t* list;     // tiles the last pass rendered (x | y << 16)
    uint32_t n_list;
    const float4* sum;        // HDR sum and second moments (W x H, row-major)
    const float4* m2;
    uint32_t width, height, tiles_x;
    uint32_t n, n_max;        // samples every listed tile holds now; the most any tile gets (N)
    double threshold, luminance_floor;
    uint32_t* tile_count;     // row-major by tile: the count of every listed tile is written
    uint8_t* flag;            // per list entry: 1 = the tile stays active
};

// Luminance weights of dn_lum / add_moments (float constants, evaluated in double).
__device__ __forceinline__ double adaptive_lum(float r, float g, float b) {
    return ((double)0.2126f * (double)r + (double)0.7152f * (double)g) + (double)0.0722f * (double)b;
}

// The stopping rule per pixel, written once (k_adaptive_eval below and the NEE render that decides in the wave, mpt_nee_adaptive.h):
// the relative standard error of the mean luminance of a pixel that holds n_samples samples, from its float32 sum and the luminance
// moment m2.w, in double precision.
__device__ __forceinline__ double adaptive_pixel_error(const float4& s4, float m2w, uint32_t n_samples, double luminance_floor) {
    const double n = (double)n_samples;
    const double s = adaptive_lum(s4.x, s4.y, s4.z);
    const double mean = s / n;
    const double var = fmax(0.0, ((double)m2w - s * mean) / (n - 1.0));
    return sqrt(var / n) / fmax(mean, luminance_floor);
}
// The tile's error: the maximum over the wave's lanes (cross-lane shuffles; every lane gets it).
__device__ __forceinline__ double adaptive_tile_error(double err) {
    for (int off = 32; off > 0; off >>= 1) err = fmax(err, __shfl_xor(err, off));
    return err;
}

// One wave64 per list entry.  err = sqrt(var / n) / max(mean, floor) per pixel inside the image (0 outside), the tile's error is the
// wave maximum; lane 0 writes the tile's count and whether it stays active (error > threshold and n < N).
__global__ __launch_bounds__(256) void k_adaptive_eval(AdaptiveEval a) {
    const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (e >= a.n_list) return;   // (wave-uniform)
    const uint32_t xy = a.list[e], tx = xy & 0xFFFFu, ty = xy >> 16;
    const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
    double err = 0.0;
    if (px < a.width && py < a.height) {
        const size_t i = (size_t)py * a.width + px;
        const float4 s4 = a.sum[i], q4 = a.m2[i];
        err = adaptive_pixel_error(s4, q4.w, a.n, a.luminance_floor);
    }
    err = adaptive_tile_error(err);
    if (lane == 0u) {
        a.tile_count[(size_t)ty * a.tiles_x + tx] = a.n;
        a.flag[e] = err > a.threshold && a.n < a.n_max ? 1u : 0u;
    }
}
