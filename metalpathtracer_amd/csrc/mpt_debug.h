// mpt_debug.h — the mpt_debug_* entry points of the diagnostics builds (-DMPT_OT_TIMES, -DMPT_CLOCK_STAMP, -DMPT_DEBUG_WAVE_TIMES; read by
// tools/gpu_ot_times.py, gpu_clock.py, gpu_wave_times.py); a product build compiles none of them.  Host code only: mpt_hip.hip includes it once, last.
#pragma once

#ifdef MPT_OT_TIMES
extern "C" int mpt_debug_ot_times(unsigned long long* out40, int reset) {   // [0,24) g_ot_times, [24,40) g_ot_walk
    hipError_t e = hipMemcpyFromSymbol(out40, HIP_SYMBOL(g_ot_times), 24 * 8);
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out40 + 24, HIP_SYMBOL(g_ot_walk), 16 * 8);
    if (e == hipSuccess && reset) {
        unsigned long long z[24] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_ot_times), z, sizeof z);
        if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_ot_walk), z, 16 * 8);
    }
    return (int)e;
}
#endif

#ifdef MPT_CLOCK_STAMP
extern "C" int mpt_debug_clock(unsigned long long* out2, int reset) {   // sums over waves: shader cycles, 100 MHz ticks
    hipError_t e = hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_clock), 16);
    if (e == hipSuccess && reset) {
        unsigned long long z[2] = {};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_clock), z, 16);
    }
    return (int)e;
}
#endif

#ifdef MPT_DEBUG_WAVE_TIMES
static mpt_ctx* g_dbg_ctx = nullptr;
extern "C" void mpt_debug_bind(mpt_ctx* ctx) { g_dbg_ctx = ctx; }
extern "C" int mpt_debug_reset() {   // zero the diagnostics block behind lane 0's rings
    mpt_ctx* ctx = g_dbg_ctx;
    const Lane& L = ctx->lane[0];
    if (!L.ring.base) return -1;
    const size_t off = L.ring_waves * MPT_WL_LEVELS * MPT_WL_RING;
    return (int)hipMemset((char*)L.ring.tv() + off * 16, 0, L.ring_waves * 128 + 1024);
}
extern "C" int mpt_debug_wave_times(unsigned long long* out, int n) {
    mpt_ctx* ctx = g_dbg_ctx;
    const Lane& L = ctx->lane[0];
    const size_t off = L.ring_waves * MPT_WL_LEVELS * MPT_WL_RING;
    return (int)hipMemcpy(out, (const char*)L.ring.tv() + off * 16, (size_t)n * 128 + 1024, hipMemcpyDeviceToHost);
}
#endif
