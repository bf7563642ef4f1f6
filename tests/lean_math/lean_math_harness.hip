// lean_math_harness.hip — the short arithmetic forms of the lean wave-local kernels (mpt_device.h: sqrt_core, normalize3<true>,
// cdiv_chain) behind C entry points, for tests/test_gpu_lean_math.py.  Test infrastructure only: the functions are the product's,
// included, not copied — so this file is built with the product's -ffp-contract=off and include paths.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Imetalpathtracer_amd/csrc -shared \
//         tests/lean_math/lean_math_harness.hip -o tests/lean_math/_build/libleanmath.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "mpt.h"
#include "mpt_accel.h"
#include "mpt_device.h"
#include "mpt_own.h"
#include "mpt_kernels.h"

namespace {
enum { LM_OK = 0, LM_ERR_ARG = -1, LM_ERR_HIP = -2 };

__device__ __forceinline__ bool same_bits(float fa, float fb) {   // (two NaNs are the same answer)
    const uint32_t a = __float_as_uint(fa), b = __float_as_uint(fb);
    return a == b || ((a & 0x7FFFFFFFu) > 0x7F800000u && (b & 0x7FFFFFFFu) > 0x7F800000u);
}
__device__ __forceinline__ void wave_add4(unsigned long long* out, unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d) {
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
        c += __shfl_down(c, off);
        d += __shfl_down(d, off);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (a) atomicAdd(out + 0, a);
        if (b) atomicAdd(out + 1, b);
        if (c) atomicAdd(out + 2, c);
        if (d) atomicAdd(out + 3, d);
    }
}
// All 2^32 operands (the host launches 65536 x 256: a stride that divides 2^32).
// WHAT 0: sqrt_core(x) against sqrtf(x); "in" = sqrt_core_exact(x).   WHAT 1: inv_len_core(x) against 1.0f / sqrtf(x); "in" = norm_core_exact(x).
// out = {mismatches in, operands in, mismatches out, operands out}
template <int WHAT>
__global__ void k_all_operands(unsigned long long* out) {
    unsigned long long bad_in = 0, n_in = 0, bad_out = 0, n_out = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t bits = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t it = 0; it < (uint32_t)(0x100000000ull / stride); ++it, bits += stride) {
        const float x = __uint_as_float(bits);
        const bool in = WHAT == 0 ? sqrt_core_exact(x) : norm_core_exact(x);
        const bool same = WHAT == 0 ? same_bits(sqrt_core(x), sqrtf(x)) : same_bits(inv_len_core(x), 1.0f / sqrtf(x));
        if (in) {
            n_in++;
            bad_in += same ? 0u : 1u;
        } else {
            n_out++;
            bad_out += same ? 0u : 1u;
        }
    }
    wave_add4(out, bad_in, n_in, bad_out, n_out);
}
// bad[blockIdx.y] = numerators k 2^-24 - 0.5 (all 2^24) for which cdiv_chain differs from x / W[blockIdx.y]
__global__ void k_cdiv_many(const float* W, uint32_t* bad) {
    uint32_t n = cdiv_mismatches(W[blockIdx.y], blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(bad + blockIdx.y, n);
}
// one wave per workgroup of 64: the wave-uniform guards see exactly the 64 operands the caller put together
template <bool LEAN>
__global__ void k_normalize(const float* v, float* o) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const F3 r = normalize3<LEAN>(f3(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
    o[3 * i] = r.x;
    o[3 * i + 1] = r.y;
    o[3 * i + 2] = r.z;
}

template <typename T>
struct Dev {   // a device array, freed on every exit path
    T* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
};

template <int WHAT>
int all_operands(uint64_t* out4) {
    if (!out4) return LM_ERR_ARG;
    Dev<unsigned long long> d;
    if (!d.alloc(4) || hipMemset(d.p, 0, 32) != hipSuccess) return LM_ERR_HIP;
    hipLaunchKernelGGL(k_all_operands<WHAT>, dim3(65536), dim3(256), 0, 0, d.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LM_ERR_HIP;
    return hipMemcpy(out4, d.p, 32, hipMemcpyDeviceToHost) == hipSuccess ? LM_OK : LM_ERR_HIP;
}

// in: n_in floats per item group, out: two arrays (lean, reference) of n_out floats; n_waves waves of 64 items
template <typename KL, typename KR>
int two_ways(const float* in, size_t n_in, float* lean_out, float* ref_out, size_t n_out, uint32_t n_waves, KL lean, KR ref) {
    if (!in || !lean_out || !ref_out || n_waves == 0u) return LM_ERR_ARG;
    Dev<float> d_in, d_a, d_b;
    if (!d_in.alloc(n_in) || !d_a.alloc(n_out) || !d_b.alloc(n_out)) return LM_ERR_HIP;
    if (hipMemcpy(d_in.p, in, n_in * 4, hipMemcpyHostToDevice) != hipSuccess) return LM_ERR_HIP;
    hipLaunchKernelGGL(lean, dim3(n_waves), dim3(64), 0, 0, (const float*)d_in.p, d_a.p);
    hipLaunchKernelGGL(ref, dim3(n_waves), dim3(64), 0, 0, (const float*)d_in.p, d_b.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LM_ERR_HIP;
    if (hipMemcpy(lean_out, d_a.p, n_out * 4, hipMemcpyDeviceToHost) != hipSuccess) return LM_ERR_HIP;
    return hipMemcpy(ref_out, d_b.p, n_out * 4, hipMemcpyDeviceToHost) == hipSuccess ? LM_OK : LM_ERR_HIP;
}
}  // namespace

extern "C" int lean_math_sqrt_all(uint64_t* out4) { return all_operands<0>(out4); }
extern "C" int lean_math_inv_len_all(uint64_t* out4) { return all_operands<1>(out4); }

// bad[i] = mismatches of the constant-division chain against x / W[i] over all 2^24 numerators
extern "C" int lean_math_cdiv(const float* W, uint32_t n, uint32_t* bad) {
    if (!W || !bad || n == 0u || n > 65535u) return LM_ERR_ARG;
    Dev<float> d_w;
    Dev<uint32_t> d_bad;
    if (!d_w.alloc(n) || !d_bad.alloc(n)) return LM_ERR_HIP;
    if (hipMemcpy(d_w.p, W, n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_bad.p, 0, n * 4) != hipSuccess) return LM_ERR_HIP;
    hipLaunchKernelGGL(k_cdiv_many, dim3(64, n), dim3(256), 0, 0, (const float*)d_w.p, d_bad.p);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LM_ERR_HIP;
    return hipMemcpy(bad, d_bad.p, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? LM_OK : LM_ERR_HIP;
}

// n_waves waves of 64 vectors (xyz) each, every wave on its own: normalize3<true> into lean_out, normalize3<false> into ref_out
extern "C" int lean_math_normalize(const float* xyz, uint32_t n_waves, float* lean_out, float* ref_out) {
    return two_ways(xyz, (size_t)n_waves * 192, lean_out, ref_out, (size_t)n_waves * 192, n_waves, k_normalize<true>, k_normalize<false>);
}
