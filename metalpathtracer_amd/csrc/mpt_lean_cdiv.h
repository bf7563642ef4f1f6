// mpt_lean_cdiv.h — the per-context record of whether the lean wave-local kernels' division by the image's width and height is exact at
// the context's size.  Pure host code (no HIP): mpt_hip.hip calls it in select_trace_kernel (a step of run_pass) with the device check, tests/lean_math/ compiles it
// alone with the check stubbed.
//
// gen_primary<true> divides the sub-pixel jitter x = k 2^-24 - 0.5 by W and H with cdiv_chain (mpt_device.h): five instructions that are
// the compiler's division wherever its range handling does nothing.  Whether that holds for a given (W, H) is MEASURED on the device, over
// all 2^24 numerators (k_lean_cdiv_check, mpt_kernels.h), the first time a context is about to run a lean kernel at that size; the answer
// is kept until the size changes (mpt_resize, mpt_set_uniforms — never inside a render).  A size that fails, or whose check could not
// run, renders with the generic kernels.
#pragma once
#include <stdint.h>

struct LeanCdivCache {
    float W = 0.0f, H = 0.0f;   // the pair the answer below is for
    bool valid = false, ok = false;
    uint64_t checks = 0;        // device checks made (tests)
};

// check(W, H, &mismatches) runs the device check and returns false when it could not run.
template <typename Check>
static inline bool lean_cdiv_ok(LeanCdivCache& c, float W, float H, Check&& check) {
    if (!(W == W) || !(H == H)) return false;   // (a NaN size equals nothing, itself included: no check, the generic kernels)
    if (c.valid && c.W == W && c.H == H) return c.ok;
    uint32_t mismatches = 0;
    const bool ran = check(W, H, &mismatches);
    c.W = W;
    c.H = H;
    c.valid = true;
    c.ok = ran && mismatches == 0u;
    c.checks++;
    return c.ok;
}
