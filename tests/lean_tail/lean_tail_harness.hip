// lean_tail_harness.hip — "the tail guard implies T's box test" on the device, for tests/test_gpu_lean_tail_device.py: the guard of the
// lean wave-local kernels' tail leaf (mpt_lean_entry.h, as closest_hit_resume evaluates it) against the product's own box-trip
// expression (slab_hit, mpt_device.h) with the reciprocals of mpt_rcp3.  Test infrastructure only: the functions are the product's,
// included, not copied — so this file is built with the product's -ffp-contract=off and include paths.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Imetalpathtracer_amd/csrc -shared \
//         tests/lean_tail/lean_tail_harness.hip -o tests/lean_tail/_build/libleantail.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpt.h"
#include "mpt_accel.h"
#include "mpt_device.h"
#include "mpt_own.h"
#include "mpt_kernels.h"

namespace {
enum { LT_OK = 0, LT_ERR_ARG = -1, LT_ERR_HIP = -2 };

// sample i: origin o[3i..], direction d[3i..], best_t[i].  flags[i]: bit 0 = the guard says certain, bit 1 = the box test of T says
// hit, bit 2 = the minimum of the test's far terms exceeds 0.0001f.  flags[n] = T as lean_tail_terms finds it.
__global__ void k_tail_implication(const float4* nodes, uint32_t n_nodes, const float* o, const float* d, const float* best_t, uint32_t n, uint32_t* flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const uint32_t j = live ? i : 0u;   // (every lane of a wave takes part in mpt_rcp3's ballot)
    const F3 ro = f3(o[3 * j], o[3 * j + 1], o[3 * j + 2]), rd = f3(d[3 * j], d[3 * j + 1], d[3 * j + 2]);
    const LeanTail t = lean_tail_terms(nodes, n_nodes, 0.0f, 0.0f, 0.0f);
    if (i == 0u) flags[n] = t.node;
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 n0 = none, n1 = none;
    if (t.node != 0u) {
        n0 = nodes[2u * t.node];
        n1 = nodes[2u * t.node + 1u];
    }
    const bool d_ok = fmaxf(fmaxf(fabsf(rd.x), fabsf(rd.y)), fabsf(rd.z)) <= MPT_LEAN_ENTRY_DMAX;
    const bool in = t.tlo[0] <= ro.x && ro.x <= t.thi[0] && t.tlo[1] <= ro.y && ro.y <= t.thi[1] && t.tlo[2] <= ro.z && ro.z <= t.thi[2];
    const bool nan_d = rd.x != rd.x || rd.y != rd.y || rd.z != rd.z;   // (the walk's own rule comes first: such a ray never holds the marker)
    const bool certain = t.node != 0u && in && d_ok && !nan_d;
    float idx, idy, idz;
    mpt_rcp3(rd.x, rd.y, rd.z, idx, idy, idz);
    const bool hit = slab_hit(n0, n1, ro, idx, idy, idz, best_t[j]);
    const float fx = idx < 0.0f ? (n0.x - ro.x) * idx : (n1.x - ro.x) * idx, fy = idy < 0.0f ? (n0.y - ro.y) * idy : (n1.y - ro.y) * idy,
                fz = idz < 0.0f ? (n0.z - ro.z) * idz : (n1.z - ro.z) * idz;
    const bool far_ok = fminf(fminf(fx, fy), fz) > 0.0001f;
    if (live) flags[i] = (certain ? 1u : 0u) | (hit ? 2u : 0u) | (far_ok ? 4u : 0u);
}

template <typename T>
struct Dev {   // a device array, freed on every exit path
    T* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
};
}  // namespace

// nodes: n_nodes x 8 words (lo, hit link, hi, miss link); o, d: n x 3 floats; best_t: n floats; flags: n + 1 words out
extern "C" int lean_tail_implication(const float* nodes, uint32_t n_nodes, const float* o, const float* d, const float* best_t, uint32_t n, uint32_t* flags) {
    if (!nodes || !o || !d || !best_t || !flags || n == 0u || n > (1u << 26) || n_nodes == 0u || n_nodes > (1u << 20)) return LT_ERR_ARG;
    Dev<float> d_o, d_d, d_t;
    Dev<float4> d_n;
    Dev<uint32_t> d_f;
    if (!d_o.alloc(3 * (size_t)n) || !d_d.alloc(3 * (size_t)n) || !d_t.alloc(n) || !d_f.alloc((size_t)n + 1) || !d_n.alloc(2 * (size_t)n_nodes)) return LT_ERR_HIP;
    if (hipMemcpy(d_o.p, o, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_d.p, d, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_t.p, best_t, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_n.p, nodes, 32 * (size_t)n_nodes, hipMemcpyHostToDevice) != hipSuccess)
        return LT_ERR_HIP;
    hipLaunchKernelGGL(k_tail_implication, dim3((n + 255u) / 256u), dim3(256), 0, 0, (const float4*)d_n.p, n_nodes, (const float*)d_o.p, (const float*)d_d.p, (const float*)d_t.p, n, d_f.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LT_ERR_HIP;
    return hipMemcpy(flags, d_f.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost) == hipSuccess ? LT_OK : LT_ERR_HIP;
}
