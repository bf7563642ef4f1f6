// mpt_wl_lean.h — when the lean wave-local trace kernels (k_wavelocal_lean*, mpt_kernels.h) may run a pass, and the constants their
// integer arithmetic needs.  Pure host code (no HIP): mpt_hip.hip calls it in select_trace_kernel (a step of run_pass), tests/wl_lean/ compiles it alone.
//
// The lean kernels are the step loop of k_wavelocal with the render mode decided at compile time (Philox RNG, Lambert bounce, no work
// counters) and with every index computed by full-rate 24-bit instructions instead of 32 x 32 and 64-bit multiplies.  The instruction
// forms and what each needs (u24 = an operand of v_mul_u32_u24 / v_mad_u32_u24 / v_mul_hi_u32_u24: only its low 24 bits are read; the
// 32-bit forms return the low 32 bits of the product):
//
//   primitive record   off = i * 48 (u24 x const), i < n_prims                        n_prims <= 2^24  (then off < 48 * 2^24 < 2^32)
//   pixel index        py * width + px (u24 x u24 + u32), the value is < width*height width, height < 2^24, width * height <= 2^32
//   tile of a path     T = tl * nranks + rank (u24 x u24 + u32), T < N                N = tiles_x * tiles_y <= 2^24, nranks < 2^24
//   tile row           ty = (T * tile_mul) >> 24 in 32 bits, tile_mul = ceil(2^24 / tiles_x), e = tile_mul * tiles_x - 2^24:
//                      T * tile_mul / 2^24 = T / tiles_x + T * e / (tiles_x * 2^24), and the floor is that of T / tiles_x while
//                      T * e < 2^24 (the fraction of T / tiles_x is at most 1 - 1 / tiles_x)
//                                                                                     (N - 1) * e < 2^24, (N - 1) * tile_mul < 2^32,
//                                                                                     tiles_x >= 2 (tile_mul < 2^24)
//   tile column        tx = T - ty * tiles_x (u24 x u24)                              covered by N <= 2^24
//   sample of a path   chunk = path >> 6 < C = n_tiles * S (this rank's tiles)        C <= 2^24, S < 2^24
//                      S = 2^k: shift and mask.  Otherwise tl = (chunk * s_mul) >> s_shift with the 48-bit product of two u24
//                      (v_mul_u32_u24 + v_mul_hi_u32_u24), s_shift <= 47 the largest shift with s_mul = ceil(2^s_shift / S) < 2^24,
//                      e = s_mul * S - 2^s_shift: exact while chunk * e < 2^s_shift, as above      (C - 1) * e < 2^s_shift
//                      s = chunk - tl * S (u24 x u24)
//
// Everything else (ring addressing, path ids) is shifts and adds in both kernels.  A pass that fails any line runs the generic kernels.
#pragma once
#include <stdint.h>

#define MPT_WL_LEAN_TILE_SHIFT 24u

struct WlLean {
    uint32_t tile_mul;          // T / tiles_x = (T * tile_mul) >> MPT_WL_LEAN_TILE_SHIFT
    uint32_t s_mul, s_shift;    // S not a power of two: chunk / S = (chunk * s_mul) >> s_shift; else 0, 0
};

// rng: MPT_RNG_* (1 = Philox), bsdf: MPT_BSDF_* (0 = Lambert); count: the pass counts its work (MPT_FLAG_COUNT);
// tile_magic: PassParams::tile_magic (!= 0: the rank's k-th tile is tile k * nranks + rank in row-major order, no table)
static inline bool wl_lean_ok(uint64_t n_prims, uint64_t n_tiles, uint64_t tiles_x, uint64_t width, uint64_t height, uint64_t nranks, uint64_t S,
                              uint32_t tile_magic, int rng, int bsdf, bool count, WlLean* out) {
    const uint64_t M24 = 1ull << 24, M32 = 1ull << 32;
    if (rng != 1 || bsdf != 0 || count || tile_magic == 0u) return false;
    if (n_prims > M24) return false;
    if (width == 0 || height == 0 || width >= M24 || height >= M24 || width * height > M32) return false;
    if (tiles_x < 2 || tiles_x != (width + 7) / 8 || nranks == 0 || nranks >= M24) return false;
    const uint64_t N = tiles_x * ((height + 7) / 8);
    if (N > M24 || n_tiles == 0 || n_tiles > N) return false;
    WlLean w = {0u, 0u, 0u};
    {
        const uint64_t m = (M24 + tiles_x - 1) / tiles_x, e = m * tiles_x - M24;
        if ((N - 1) * e >= M24 || (N - 1) * m >= M32) return false;
        w.tile_mul = (uint32_t)m;
    }
    if (S == 0 || S >= M24 || n_tiles * S > M24) return false;
    if ((S & (S - 1)) != 0) {
        uint32_t sh = 47;
        while (((1ull << sh) + S - 1) / S >= M24) --sh;     // (S >= 3: 2^25 / 3 < 2^24, so sh >= 25)
        const uint64_t m = ((1ull << sh) + S - 1) / S, e = m * S - (1ull << sh);
        if ((n_tiles * S - 1) * e >= (1ull << sh)) return false;
        w.s_mul = (uint32_t)m;
        w.s_shift = sh;
    }
    if (out) *out = w;
    return true;
}
