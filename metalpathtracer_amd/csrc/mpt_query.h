// mpt_query.h — host side of the ray queries behind the C ABI (include/mpt.h): closest hit (mpt_trace_rays, mpt_trace_rays_ordered) and
// any hit (mpt_trace_occluded) for rays the caller brings, their timing hook (mpt_time_trace) and the known-answer kernels (mpt_kat_*).
// Host code only: mpt_hip.hip includes it once, behind mpt_post.h.  Every call here is three things: its argument checks, the WalkViews
// of the tree that answers (walk_views, mpt_hip.hip) and one launch inside a DeviceCall.  None of them calls wait_impl: they only read
// the scene, which cannot change while a render is in flight.
#pragma once

// ---- shared: the device side of one call ---------------------------------------------------------------------------------------------
// Buffers that live as long as the call, filled and read back on ctx->stream (stage_in / scratch / copy_out of mpt_post.h): in() is a
// device copy of a host array, out() a buffer a kernel fills, run() the launch, hipGetLastError, the outputs' copies and ONE
// synchronise.  The first failure is kept in rc; nothing is launched after one.
struct DeviceCall {
    mpt_ctx* ctx;
    int rc;
    std::vector<DevMem<>> bufs;
    struct Out {
        void* host;
        const void* dev;
        size_t bytes;
    };
    std::vector<Out> outs;
    explicit DeviceCall(mpt_ctx* c) : ctx(c), rc(select_device()) {}
    int select_device() {
        HIPCHK(hipSetDevice(ctx->device));
        return MPT_OK;
    }
    // `count` items of a host array on the device; no host array, no buffer: a null pointer (the kernels' convention for "no tmax")
    template <class T>
    const T* in(const T* host, size_t count) {
        bufs.emplace_back();
        if (!rc) rc = stage_in(ctx, bufs.back(), host, count * sizeof(T));
        return (const T*)bufs.back().get();
    }
    // `count` items for a kernel to fill, read back into `host` by run() (a null `host`: an output the caller did not ask for, or scratch)
    template <class T>
    T* out(T* host, size_t count) {
        bufs.emplace_back();
        if (!rc) rc = scratch(ctx, count * sizeof(T), {&bufs.back()});
        outs.push_back({host, bufs.back().get(), count * sizeof(T)});
        return (T*)bufs.back().get();
    }
    // launch: enqueues on ctx->stream; it may return a status
    template <class F>
    int run(F&& launch) {
        if (rc) return rc;
        if constexpr (std::is_void<decltype(launch())>::value) launch();
        else if ((rc = launch())) return rc;
        HIPCHK(hipGetLastError());
        for (const Out& o : outs)
            if ((rc = copy_out(ctx, o.host, o.dev, o.bytes))) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return MPT_OK;
    }
};
static dim3 blocks_of_256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// The rays of a query on the device — origins, directions, and tmax if the caller gave one (tmax = NULL: no limit, a null pointer on
// the device too) — and the outputs the call asked for.  The two launch functions take a WalkViews and run the kernel it names,
// one ray per lane in workgroups of 256: what the untimed calls launch once, mpt_time_trace launches in turn.
struct RayBatch : DeviceCall {
    uint32_t n;
    const float *o, *d, *tmax;
    float *t = nullptr, *normal = nullptr;   // closest hit
    int32_t *prim = nullptr, *front = nullptr;
    uint8_t* occ = nullptr;                  // any hit
    uint32_t* flags = nullptr;               // the own tree's re-trace flags (either)
    RayBatch(mpt_ctx* c, const float* o_, const float* d_, const float* tmax_, uint64_t n_)
        : DeviceCall(c), n((uint32_t)n_), o(in(o_, 3 * n_)), d(in(d_, 3 * n_)), tmax(in(tmax_, n_)) {}
    void closest_out(float* t_, int32_t* prim_, float* normal_, int32_t* front_) {
        t = out(t_, n);
        prim = out(prim_, n);
        normal = out(normal_, 3 * (size_t)n);
        front = out(front_, n);
    }
};
static void launch_closest(const WalkViews& v, const RayBatch& b) {
    if (v.which == MPT_AO_OWN)
        hipLaunchKernelGGL(k_trace_rays_ordered, blocks_of_256(b.n), dim3(256), v.lds, b.ctx->stream, v.sc, v.ac, b.o, b.d, b.n, b.t, b.prim, b.normal, b.front, b.flags);
    else
        hipLaunchKernelGGL(k_trace_rays, blocks_of_256(b.n), dim3(256), v.lds, b.ctx->stream, v.sc, b.o, b.d, b.n, b.t, b.prim, b.normal, b.front);
}
static void launch_occluded(const WalkViews& v, const RayBatch& b) {
    if (v.which == MPT_AO_OWN)
        hipLaunchKernelGGL(k_occluded_own, blocks_of_256(b.n), dim3(256), v.lds, b.ctx->stream, v.sc, v.ac, b.o, b.d, b.tmax, b.n, b.occ, b.flags);
    else if (v.which == MPT_AO_REF_ALL_LDS)
        hipLaunchKernelGGL(k_occluded_ref<true>, blocks_of_256(b.n), dim3(256), v.lds, b.ctx->stream, v.sc, b.o, b.d, b.tmax, b.n, b.occ);
    else
        hipLaunchKernelGGL(k_occluded_ref<false>, blocks_of_256(b.n), dim3(256), v.lds, b.ctx->stream, v.sc, b.o, b.d, b.tmax, b.n, b.occ);
}

// ---- closest hit ---------------------------------------------------------------------------------------------------------------------
extern "C" int mpt_trace_rays(mpt_ctx* ctx, const float* o, const float* d, uint64_t n, float* t_out, int32_t* prim_out, float* normal_out, int32_t* front_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !o || !d || !t_out || !prim_out || !normal_out || !front_out || n == 0 || n > (1ull << 30))
            return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
        if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
        WalkViews v;
        const int rc = walk_views(ctx, false, 0, 256u, v);
        if (rc) return rc;
        RayBatch b(ctx, o, d, nullptr, n);
        b.closest_out(t_out, prim_out, normal_out, front_out);
        return b.run([&] { launch_closest(v, b); });
    });
}
extern "C" int mpt_trace_rays_ordered(mpt_ctx* ctx, const float* o, const float* d, uint64_t n, float* t_out, int32_t* prim_out, float* normal_out, int32_t* front_out, uint32_t* flags_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !o || !d || !t_out || !prim_out || !normal_out || !front_out || !flags_out || n == 0 || n > (1ull << 22))
            return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument (at most 2^22 rays per call)");
        if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
        if (!ctx->acc_ok) return fail(ctx, MPT_ERR_BAD_SCENE, "closest-first walk unavailable for this scene: " + ctx->acc_why);
        WalkViews v;
        const int rc = walk_views(ctx, true, 0, 256u, v);
        if (rc) return rc;
        RayBatch b(ctx, o, d, nullptr, n);
        b.closest_out(t_out, prim_out, normal_out, front_out);
        b.flags = b.out(flags_out, n);
        return b.run([&] { launch_closest(v, b); });
    });
}

// ---- shadow rays (mpt_anyhit.h; the specification is in include/mpt.h) ---------------------------------------------------------------
extern "C" int mpt_trace_occluded(mpt_ctx* ctx, const float* o, const float* d, const float* tmax, uint64_t n, int32_t walk, uint8_t* occluded_out,
                                  uint32_t* flags_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !o || !d || !occluded_out || n == 0 || n > (1ull << 22) || !walk_valid(walk))
            return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument (at most 2^22 rays per call, walk = MPT_WALK_*)");
        if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
        WalkViews v;
        const int rc = walk_views(ctx, resolve_walk(ctx, walk) == 1, 0, 256u, v);
        if (rc) return rc;
        RayBatch b(ctx, o, d, tmax, n);
        b.occ = b.out(occluded_out, n);
        b.flags = b.out(flags_out, n);
        return b.run([&]() -> int {
            if (v.which != MPT_AO_OWN) HIPCHK(hipMemsetAsync(b.flags, 0, n * 4, ctx->stream));   // (the reference walk flags nothing)
            launch_occluded(v, b);
            return MPT_OK;
        });
    });
}

// Measurement hook (tools/ao_timing.py): the four one-ray-per-lane kernels on the SAME rays, uploaded once, launched in turn — closest hit
// in reference order (k_trace_rays), any hit in reference order, closest hit through the own tree (k_trace_rays_ordered), any hit through
// the own tree — `warmup` untimed rounds, then `reps` rounds with a pair of HIP events around every launch.  ms_out: [reps][4]; the
// own tree's two columns are 0 for a scene it cannot be used for.
extern "C" int mpt_time_trace(mpt_ctx* ctx, const float* o, const float* d, const float* tmax, uint64_t n, uint32_t warmup, uint32_t reps, double* ms_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !o || !d || !ms_out || n == 0 || n > (1ull << 22) || reps == 0 || reps > 1000u || warmup > 1000u)
            return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument (at most 2^22 rays, 1..1000 repetitions)");
        if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
        WalkViews v[2];   // reference order, own tree
        int rc = walk_views(ctx, false, 0, 256u, v[0]);
        if (rc || (ctx->acc_ok && (rc = walk_views(ctx, true, 0, 256u, v[1])))) return rc;
        RayBatch b(ctx, o, d, tmax, n);
        b.closest_out(nullptr, nullptr, nullptr, nullptr);   // (what the kernels write stays on the device)
        b.occ = b.out((uint8_t*)nullptr, n);
        b.flags = b.out((uint32_t*)nullptr, n);
        Event e0, e1;
        return b.run([&]() -> int {
            HIPCHK(e0.create(hipEventCreate));
            HIPCHK(e1.create(hipEventCreate));
            for (uint32_t r = 0; r < warmup + reps; ++r)
                for (int kind = 0; kind < 4; ++kind) {
                    double* slot = r >= warmup ? ms_out + 4 * (size_t)(r - warmup) + kind : nullptr;
                    if (kind >= 2 && !ctx->acc_ok) {
                        if (slot) *slot = 0.0;
                        continue;
                    }
                    HIPCHK(hipEventRecord(e0.get(), ctx->stream));
                    if (kind & 1) launch_occluded(v[kind >> 1], b);
                    else launch_closest(v[kind >> 1], b);
                    HIPCHK(hipGetLastError());
                    HIPCHK(hipEventRecord(e1.get(), ctx->stream));
                    HIPCHK(hipEventSynchronize(e1.get()));
                    float ms = 0.0f;
                    HIPCHK(hipEventElapsedTime(&ms, e0.get(), e1.get()));
                    if (slot) *slot = (double)ms;
                }
            return MPT_OK;
        });
    });
}

// ---- known-answer kernels of the device arithmetic (mpt_kernels.h); an argument error sets no text -------------------------------------
extern "C" int mpt_kat_pcg(mpt_ctx* ctx, const uint32_t* seeds, uint64_t n, uint32_t* h, float* f) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !seeds || !h || !f || n == 0 || n > (1u << 28)) return MPT_ERR_INVALID_ARG;
        DeviceCall c(ctx);
        const uint32_t* d_seeds = c.in(seeds, n);
        uint32_t* d_h = c.out(h, n);
        float* d_f = c.out(f, n);
        return c.run([&] { hipLaunchKernelGGL(k_kat_pcg, blocks_of_256(n), dim3(256), 0, ctx->stream, d_seeds, (uint32_t)n, d_h, d_f); });
    });
}
extern "C" int mpt_kat_philox(mpt_ctx* ctx, const uint32_t* ctr, const uint32_t* key, uint64_t n, uint32_t* o) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !ctr || !key || !o || n == 0 || n > (1u << 26)) return MPT_ERR_INVALID_ARG;
        DeviceCall c(ctx);
        const uint32_t *d_ctr = c.in(ctr, 4 * n), *d_key = c.in(key, 2 * n);
        uint32_t* d_o = c.out(o, 4 * n);
        return c.run([&] { hipLaunchKernelGGL(k_kat_philox, blocks_of_256(n), dim3(256), 0, ctx->stream, d_ctr, d_key, (uint32_t)n, d_o); });
    });
}
extern "C" int mpt_kat_sincos(mpt_ctx* ctx, const float* u, uint64_t n, float* s, float* c_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !u || !s || !c_out || n == 0 || n > (1u << 28)) return MPT_ERR_INVALID_ARG;
        DeviceCall c(ctx);
        const float* d_u = c.in(u, n);
        float *d_s = c.out(s, n), *d_c = c.out(c_out, n);
        return c.run([&] { hipLaunchKernelGGL(k_kat_sincos, blocks_of_256(n), dim3(256), 0, ctx->stream, d_u, (uint32_t)n, d_s, d_c); });
    });
}
extern "C" int mpt_kat_rcp(mpt_ctx* ctx, uint64_t* out4) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !out4) return MPT_ERR_INVALID_ARG;
        const uint64_t zero[4] = {0, 0, 0, 0};
        DeviceCall c(ctx);
        const uint64_t* d_zero = c.in(zero, 4);
        uint64_t* d_out = c.out(out4, 4);
        return c.run([&] {
            (void)hipMemcpyAsync(d_out, d_zero, sizeof zero, hipMemcpyDeviceToDevice, ctx->stream);   // (an error shows in hipGetLastError of run)
            hipLaunchKernelGGL(k_kat_rcp, dim3(65536), dim3(256), 0, ctx->stream, (unsigned long long*)d_out);
        });
    });
}
