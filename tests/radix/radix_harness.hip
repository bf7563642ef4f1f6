// radix_harness.hip — the builders' radix sort (mpt_radix.h) and material hash (mpt_devbuild.h k_mat_hash) behind a C entry point each, for
// tests/test_gpu_radix.py and tests/test_gpu_materials.py.  Test infrastructure only: the kernels are the product's, included, not copied.
//
// radix_harness_sort sorts device copies of the caller's pairs on a stream of its own, with a Scratch over a pool of the call's own for the sort's
// temporaries, and puts RADIX_GUARD words of a known pattern behind each of the four pair buffers: a word of them that changed is an
// error of its own (RADIX_ERR_GUARD), whatever the sorted arrays look like.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Imetalpathtracer_amd/csrc -shared \
//         tests/radix/radix_harness.hip -o tests/radix/_build/libradixharness.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mpt.h"
#include "mpt_accel.h"
#include "mpt_device.h"
#include "mpt_own.h"
#include "mpt_kernels.h"
#include "mpt_lbvh.h"
#include "mpt_devbuild.h"

namespace {
constexpr uint32_t RADIX_GUARD = 1024u;   // words behind every pair buffer
enum { RADIX_OK = 0, RADIX_ERR_ARG = -1, RADIX_ERR_HIP = -2, RADIX_ERR_SORT = -3, RADIX_ERR_GUARD = -4 };

hipStream_t g_stream = nullptr;
bool stream_ready() { return g_stream || hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking) == hipSuccess; }

inline uint32_t guard_word(int buffer, uint32_t k) { return 0xA5C30000u ^ ((uint32_t)buffer << 12) ^ k; }

struct DevWords {   // a device array of n + RADIX_GUARD words, freed on every exit path
    uint32_t* p = nullptr;
    ~DevWords() { if (p) hipFree(p); }
};
}  // namespace

extern "C" int radix_harness_sort(const uint32_t* keys, const uint32_t* vals, uint32_t n, int passes, uint32_t* keys_out, uint32_t* vals_out,
                                  int* in_second) {
    if (!keys || !vals || !keys_out || !vals_out || !in_second || n == 0u || passes < 1 || passes > 4) return RADIX_ERR_ARG;
    if (!stream_ready()) return RADIX_ERR_HIP;
    const size_t words = (size_t)n + RADIX_GUARD;
    DevWords d[4];   // keys, vals, keys2, vals2
    std::vector<uint32_t> h(words);
    for (int b = 0; b < 4; ++b) {
        if (hipMalloc((void**)&d[b].p, words * 4) != hipSuccess) return RADIX_ERR_HIP;
        const uint32_t* src = b == 0 ? keys : b == 1 ? vals : nullptr;
        for (uint32_t i = 0; i < n; ++i) h[i] = src ? src[i] : 0xDEADBEEFu;   // (the second pair starts as something no test sorts)
        for (uint32_t k = 0; k < RADIX_GUARD; ++k) h[n + k] = guard_word(b, k);
        if (hipMemcpyAsync(d[b].p, h.data(), words * 4, hipMemcpyHostToDevice, g_stream) != hipSuccess) return RADIX_ERR_HIP;
        if (hipStreamSynchronize(g_stream) != hipSuccess) return RADIX_ERR_HIP;   // (h is filled again for the next buffer)
    }
    bool second = false;
    {
        mpt_build::ScratchPool pool;   // (freed with the call)
        mpt_build::Scratch sc(pool);
        mpt_radix::RadixTemp T;
        if (mpt_radix::radix_reserve(sc, n, g_stream, T) != hipSuccess) return RADIX_ERR_HIP;
        const hipError_t e = mpt_radix::radix_sort_pairs(g_stream, T, d[0].p, d[1].p, d[2].p, d[3].p, n, passes, &second);
        if (hipStreamSynchronize(g_stream) != hipSuccess || e != hipSuccess) return RADIX_ERR_SORT;
    }
    int rc = RADIX_OK;
    for (int b = 0; b < 4; ++b) {
        if (hipMemcpy(h.data(), d[b].p, words * 4, hipMemcpyDeviceToHost) != hipSuccess) return RADIX_ERR_HIP;
        for (uint32_t k = 0; k < RADIX_GUARD; ++k)
            if (h[n + k] != guard_word(b, k)) rc = RADIX_ERR_GUARD;
        if (b == (second ? 2 : 0)) std::copy(h.begin(), h.begin() + n, keys_out);
        if (b == (second ? 3 : 1)) std::copy(h.begin(), h.begin() + n, vals_out);
    }
    *in_second = second ? 1 : 0;
    return rc;
}

// keys_out[i] = the 64-bit hash k_mat_hash gives material row i (mats: n rows of 8 floats)
extern "C" int radix_harness_mat_hash(const float* mats, uint32_t n, uint64_t* keys_out) {
    if (!mats || !keys_out || n == 0u) return RADIX_ERR_ARG;
    if (!stream_ready()) return RADIX_ERR_HIP;
    float4* d_mats = nullptr;
    unsigned long long* d_keys = nullptr;
    uint32_t* d_ids = nullptr;
    int rc = RADIX_ERR_HIP;
    if (hipMalloc((void**)&d_mats, (size_t)n * 32) == hipSuccess && hipMalloc((void**)&d_keys, (size_t)n * 8) == hipSuccess &&
        hipMalloc((void**)&d_ids, (size_t)n * 4) == hipSuccess &&
        hipMemcpyAsync(d_mats, mats, (size_t)n * 32, hipMemcpyHostToDevice, g_stream) == hipSuccess) {
        const uint32_t B = 256u;
        hipLaunchKernelGGL(mpt_devbuild::k_mat_hash, dim3((n + B - 1u) / B), dim3(B), 0, g_stream, (const float4*)d_mats, n, d_keys, (uint32_t*)nullptr, 0u,
                           d_ids);
        if (hipGetLastError() == hipSuccess && hipMemcpyAsync(keys_out, d_keys, (size_t)n * 8, hipMemcpyDeviceToHost, g_stream) == hipSuccess &&
            hipStreamSynchronize(g_stream) == hipSuccess)
            rc = RADIX_OK;
    }
    hipFree(d_mats);
    hipFree(d_keys);
    hipFree(d_ids);
    return rc;
}
