// lean_entry_harness.hip — "the entry guard implies the root's box test" on the device, for tests/test_gpu_lean_entry_device.py: the
// guard of the lean wave-local kernels (mpt_lean_entry.h, as wavelocal_body evaluates it) and the product's own box-trip expression
// (slab_hit, mpt_device.h) with the reciprocals of mpt_rcp3.  Test infrastructure only: the functions are the product's, included, not
// copied — so this file is built with the product's -ffp-contract=off and include paths.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Imetalpathtracer_amd/csrc -shared \
//         tests/lean_entry/lean_entry_harness.hip -o tests/lean_entry/_build/libleanentry.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpt.h"
#include "mpt_accel.h"
#include "mpt_device.h"
#include "mpt_own.h"
#include "mpt_kernels.h"

namespace {
enum { LE_OK = 0, LE_ERR_ARG = -1, LE_ERR_HIP = -2 };

// sample i: origin o[3i..], direction d[3i..], best_t[i].  flags[i]: bit 0 = the guard says skip, bit 1 = the box trip on node 0 says
// hit, bit 2 = the minimum of the trip's far terms exceeds 0.0001f
__global__ void k_entry_implication(float4 n0, float4 n1, uint32_t n_nodes, const float* o, const float* d, const float* best_t, uint32_t n, uint32_t* flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const uint32_t j = live ? i : 0u;   // (every lane of a wave takes part in mpt_rcp3's ballot)
    const F3 ro = f3(o[3 * j], o[3 * j + 1], o[3 * j + 2]), rd = f3(d[3 * j], d[3 * j + 1], d[3 * j + 2]);
    const LeanEntry e = lean_entry_terms(n0, n1, n_nodes, 0.0f, 0.0f, 0.0f);
    const bool d_ok = fmaxf(fmaxf(fabsf(rd.x), fabsf(rd.y)), fabsf(rd.z)) <= MPT_LEAN_ENTRY_DMAX;
    const bool in = e.ilo[0] <= ro.x && ro.x <= e.ihi[0] && e.ilo[1] <= ro.y && ro.y <= e.ihi[1] && e.ilo[2] <= ro.z && ro.z <= e.ihi[2];
    const bool nan_d = rd.x != rd.x || rd.y != rd.y || rd.z != rd.z;   // (the walk's own rule comes first: such a ray tests nothing)
    const bool skip = e.entry != 0u && in && d_ok && !nan_d;
    float idx, idy, idz;
    mpt_rcp3(rd.x, rd.y, rd.z, idx, idy, idz);
    const bool hit = slab_hit(n0, n1, ro, idx, idy, idz, best_t[j]);
    const float fx = idx < 0.0f ? (n0.x - ro.x) * idx : (n1.x - ro.x) * idx, fy = idy < 0.0f ? (n0.y - ro.y) * idy : (n1.y - ro.y) * idy,
                fz = idz < 0.0f ? (n0.z - ro.z) * idz : (n1.z - ro.z) * idz;
    const bool far_ok = fminf(fminf(fx, fy), fz) > 0.0001f;
    if (live) flags[i] = (skip ? 1u : 0u) | (hit ? 2u : 0u) | (far_ok ? 4u : 0u);
}

template <typename T>
struct Dev {   // a device array, freed on every exit path
    T* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
};
}  // namespace

// node0: the eight words of node 0 (lo, A0, hi, B0); o, d: n x 3 floats; best_t: n floats; flags: n words out
extern "C" int lean_entry_implication(const float* node0, uint32_t n_nodes, const float* o, const float* d, const float* best_t, uint32_t n, uint32_t* flags) {
    if (!node0 || !o || !d || !best_t || !flags || n == 0u || n > (1u << 26)) return LE_ERR_ARG;
    Dev<float> d_o, d_d, d_t;
    Dev<uint32_t> d_f;
    if (!d_o.alloc(3 * (size_t)n) || !d_d.alloc(3 * (size_t)n) || !d_t.alloc(n) || !d_f.alloc(n)) return LE_ERR_HIP;
    if (hipMemcpy(d_o.p, o, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_d.p, d, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_t.p, best_t, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess)
        return LE_ERR_HIP;
    const float4 n0 = make_float4(node0[0], node0[1], node0[2], node0[3]), n1 = make_float4(node0[4], node0[5], node0[6], node0[7]);
    hipLaunchKernelGGL(k_entry_implication, dim3((n + 255u) / 256u), dim3(256), 0, 0, n0, n1, n_nodes, (const float*)d_o.p, (const float*)d_d.p, (const float*)d_t.p, n, d_f.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LE_ERR_HIP;
    return hipMemcpy(flags, d_f.p, 4 * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? LE_OK : LE_ERR_HIP;
}
