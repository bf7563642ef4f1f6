// lean_tiles_harness.hip — "a skip tile's rays miss the chain and the spheres outside its mask" on the device, for
// tests/test_gpu_lean_tiles_device.py: the class word of mpt_lean_tiles.h against the product's own gen_primary<true>, mpt_rcp3, slab_hit
// and leaf_test<.., LEAN, PRIMARY>.  Test infrastructure only: the functions are the product's, included, not copied — so this file is
// built with the product's -ffp-contract=off and include paths.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Imetalpathtracer_amd/csrc -shared \
//         tests/lean_tiles/lean_tiles_harness.hip -o tests/lean_tiles/_build/libleantiles.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpt.h"
#include "mpt_accel.h"
#include "mpt_device.h"
#include "mpt_own.h"
#include "mpt_kernels.h"

namespace {
enum { LT_OK = 0, LT_ERR_ARG = -1, LT_ERR_HIP = -2 };
#define LT_SAMPLES 4096u   // per pixel: 64 x 4096 = 2^18 primary rays per tile

// One workgroup of 256 per tile.  out[0] += skip tiles, out[1] += rays of skip tiles, out[2] += rays that hit a chain box, a sphere outside
// the mask, or have a NaN or |d| > 2, out[3] += rays of skip tiles that hit a sphere of the mask (so the masks are not simply full).
__global__ __launch_bounds__(256) void k_tile_violations(const float4* nodes, uint32_t n_nodes, const float4* prims, uint32_t n_prims, LeanTileView view,
                                                         uint32_t width, uint32_t seed, unsigned long long* out) {
    const uint32_t tx = blockIdx.x % view.tiles_x, ty = blockIdx.x / view.tiles_x;
    const uint32_t word = lean_tile_class(nodes, n_nodes, prims, n_prims, view, tx, ty);
    if ((word & MPT_LEAN_TILES_SKIP) == 0u) return;   // (the whole workgroup)
    const LeanEntry e = lean_entry_terms(nodes[0], nodes[1], n_nodes, view.cam[0], view.cam[1], view.cam[2]);
    const LeanTail t = lean_tail_terms(nodes, n_nodes, view.cam[0], view.cam[1], view.cam[2]);
    const uint32_t enc = t.leaf & ~MPT_NODE_HOLD, first = enc >> 4, count = (enc & 15u) + 1u;
    PassParams pp = {};
    pp.width = width;
    pp.sp.rng_mode = 1;
    pp.sp.seed_lo = seed;
    pp.sp.seed_hi = 0u;
    pp.scene.nodes = nodes;
    pp.scene.prims = prims;
    pp.scene.n_nodes = n_nodes;
    pp.scene.n_prims = n_prims;   // (nothing staged: every record comes from global memory, with the camera terms load_prim computes)
    CamView cv;
    cv.cam = f3(view.cam[0], view.cam[1], view.cam[2]);
    cv.first = f3(view.first[0], view.first[1], view.first[2]);
    cv.vu = f3(view.vu[0], view.vu[1], view.vu[2]);
    cv.vv = f3(view.vv[0], view.vv[1], view.vv[2]);
    cv.W = view.W;
    cv.H = view.H;
    cv.rW = cdiv_recip(view.W);
    cv.rH = cdiv_recip(view.H);
    const uint32_t p = threadIdx.x & 63u, px = tx * 8u + (p & 7u), py = ty * 8u + (p >> 3);
    float uvx, uvy;
    pixel_uv(cv, px, py, uvx, uvy);
    WorkCount wc = {};
    unsigned long long bad = 0ull, lit = 0ull;
    for (uint32_t s = threadIdx.x >> 6; s < LT_SAMPLES; s += 4u) {   // (every lane of a wave makes every trip: the ballots inside are whole)
        PathState ps;
        PathRngDev g;
        gen_primary<true>(pp, cv, px, py, uvx, uvy, s, ps, g);
        bool ok = ps.d.x == ps.d.x && ps.d.y == ps.d.y && ps.d.z == ps.d.z && fmaxf(fmaxf(fabsf(ps.d.x), fabsf(ps.d.y)), fabsf(ps.d.z)) <= MPT_LEAN_ENTRY_DMAX;
        float idx, idy, idz;
        mpt_rcp3(ps.d.x, ps.d.y, ps.d.z, idx, idy, idz);
        for (uint32_t n = e.entry_primary; n != t.node; n = __float_as_uint(nodes[2u * n + 1u].w))
            if (slab_hit(nodes[2u * n], nodes[2u * n + 1u], ps.o, idx, idy, idz, INFINITY)) ok = false;
        bool in_mask = false;
        for (uint32_t k = 0; k < count; ++k) {
            float best_t = INFINITY;
            int best_prim = -1;
            leaf_test<false, true, true>(pp.scene, nullptr, first + k, 1u, ps.o, ps.d, best_t, best_prim, wc);
            if (best_prim >= 0) {
                if ((word >> k & 1u) == 0u) ok = false;
                else in_mask = true;
            }
        }
        bad += ok ? 0ull : 1ull;
        lit += in_mask ? 1ull : 0ull;
    }
    for (int off = 32; off > 0; off >>= 1) {
        bad += __shfl_down(bad, off);
        lit += __shfl_down(lit, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (threadIdx.x == 0u) atomicAdd(out + 0, 1ull);
        atomicAdd(out + 1, 64ull * (LT_SAMPLES / 4u));
        if (bad) atomicAdd(out + 2, bad);
        if (lit) atomicAdd(out + 3, lit);
    }
}

template <typename T>
struct Dev {   // a device array, freed on every exit path
    T* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
};
}  // namespace

// nodes: n_nodes x 8 words, prims: n_prims x 12 words (the device's arrays as mpt_read_scene_array returns them); cam: the fourteen camera
// words (position, first pixel, viewport u, viewport v, W, H); out: four counters (k_tile_violations)
extern "C" int lean_tiles_violations(const float* nodes, uint32_t n_nodes, const float* prims, uint32_t n_prims, const float* cam, uint32_t width,
                                     uint32_t height, uint32_t seed, unsigned long long* out) {
    if (!nodes || !prims || !cam || !out || n_nodes == 0u || n_nodes > (1u << 20) || n_prims == 0u || n_prims > (1u << 20) || width == 0u ||
        height == 0u || width > 4096u || height > 4096u)
        return LT_ERR_ARG;
    LeanTileView v;
    for (int a = 0; a < 3; ++a) {
        v.cam[a] = cam[a];
        v.first[a] = cam[3 + a];
        v.vu[a] = cam[6 + a];
        v.vv[a] = cam[9 + a];
    }
    v.W = cam[12];
    v.H = cam[13];
    v.tiles_x = (width + 7u) / 8u;
    v.tiles_y = (height + 7u) / 8u;
    Dev<float4> d_n, d_p;
    Dev<unsigned long long> d_o;
    if (!d_n.alloc(2 * (size_t)n_nodes) || !d_p.alloc(3 * (size_t)n_prims) || !d_o.alloc(4)) return LT_ERR_HIP;
    if (hipMemcpy(d_n.p, nodes, 32 * (size_t)n_nodes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_p.p, prims, 48 * (size_t)n_prims, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_o.p, 0, 32) != hipSuccess)
        return LT_ERR_HIP;
    hipLaunchKernelGGL(k_tile_violations, dim3(v.tiles_x * v.tiles_y), dim3(256), 0, 0, (const float4*)d_n.p, n_nodes, (const float4*)d_p.p, n_prims, v, width, seed, d_o.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LT_ERR_HIP;
    return hipMemcpy(out, d_o.p, 32, hipMemcpyDeviceToHost) == hipSuccess ? LT_OK : LT_ERR_HIP;
}
