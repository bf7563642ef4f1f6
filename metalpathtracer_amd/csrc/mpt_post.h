// mpt_post.h — host side of the post-processing stages behind the C ABI (include/mpt.h): the guide pass and the denoiser
// (mpt_denoise.h), ambient occlusion (mpt_ao.h), temporal accumulation (mpt_temporal.h), SVGF (mpt_svgf.h) and the display stage
// (mpt_display.h).  Host code only: mpt_hip.hip includes it once, below `guarded`; the states the stages own are declared there, in
// front of mpt_ctx.  What the stages have in common comes first and is written once; a new stage calls it and adds its own section.
#pragma once

// ---- shared: launch geometry and the camera key -------------------------------------------------------------------------------------
// one workgroup of 256 threads per MPT_DN_TILE x MPT_DN_TILE pixels: the grid of every per-tile kernel of the stages
static dim3 tile_grid(uint32_t W, uint32_t H) { return dim3((W + MPT_DN_TILE - 1) / MPT_DN_TILE, (H + MPT_DN_TILE - 1) / MPT_DN_TILE); }
// LDS bytes of an a-trous level that stages its tile and the 2-step halo (32 bytes per pixel); 0 = the step is too wide, the level
// reads its taps from global memory (the <false> kernels)
static size_t atrous_lds_bytes(uint32_t step) {
    const uint32_t T = MPT_DN_TILE + 4u * step;
    return step <= MPT_DN_LDS_MAX_STEP ? (size_t)T * T * 32u : 0u;
}
// The camera fields a frame's guides depend on, compared bit for bit (GuideState::cam, History::cam) ...
static void guide_key(const mpt_uniforms& u, float k[14]) {
    memcpy(k, u.cameraPosition, 12);
    memcpy(k + 3, u.viewportU, 12);
    memcpy(k + 6, u.viewportV, 12);
    memcpy(k + 9, u.firstPixelPosition, 12);
    memcpy(k + 12, u.screenSize, 8);
}
// ... and its four vectors as the kernels take them
enum { KEY_CAM = 0, KEY_VU = 1, KEY_VV = 2, KEY_FIRST = 3 };
static F3 key_f3(const float key[14], int which) { return F3{key[3 * which], key[3 * which + 1], key[3 * which + 2]}; }

// A pass's camera, size, sample range and seeds from a camera key and any params struct that names them (AoPass, DirectPass, NeePass)
template <class Pass, class Params>
static void pass_frame(Pass& P, const float key[14], uint32_t W, uint32_t H, const Params& p) {
    P.cam = key_f3(key, KEY_CAM);
    P.vu = key_f3(key, KEY_VU);
    P.vv = key_f3(key, KEY_VV);
    P.first = key_f3(key, KEY_FIRST);
    P.fW = (float)W;
    P.fH = (float)H;
    P.W = W;
    P.H = H;
    P.sample_begin = p.sample_begin;
    P.sample_count = p.sample_count;
    P.seed_lo = p.seed_lo;
    P.seed_hi = p.seed_hi;
}
// The launch of a per-tile shadow-ray kernel (mpt_ao.h: tile_walk) on ctx->stream: k = its three instantiations in the order of MPT_AO_*,
// of which `walk` (MPT_WALK_*) and the scene pick one — the own tree, or the reference-order tree wholly or partly in LDS.
template <class Pass>
using WalkKernel = void (*)(SceneDev, AccelDev, Pass);
template <class Pass>
static int tile_walk_launch(mpt_ctx* ctx, uint32_t W, uint32_t H, int32_t walk, const WalkKernel<Pass> k[3], const Pass& P) {
    WalkViews v;
    const int rc = walk_views(ctx, resolve_walk(ctx, walk) == 1, 0, 256u, v);
    if (rc) return rc;
    hipLaunchKernelGGL(k[v.which], tile_grid(W, H), dim3(256), v.lds, ctx->stream, v.sc, v.ac, P);
    HIPCHK(hipGetLastError());
    return MPT_OK;
}

// ---- shared: the device side of an image hook ---------------------------------------------------------------------------------------
// The mpt_*_image hooks run a stage on host arrays of any size and touch no state of the context: their device buffers are locals
// that free themselves, filled and read back on ctx->stream.
static bool bad_image_size(uint32_t W, uint32_t H) { return W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 31); }
// a device copy of a host array, the copy enqueued; no host array, no buffer (d.get() stays null: a hook's "no history")
template <class T>
static int stage_in(mpt_ctx* ctx, DevMem<T>& d, const void* host, size_t bytes) {
    if (!host) return MPT_OK;
    HIPCHK(d.alloc(bytes));
    HIPCHK(hipMemcpyAsync(d.get(), host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return MPT_OK;
}
// buffers of `bytes` each that the kernels fill (a stage's own, too)
template <class T>
static int scratch(mpt_ctx* ctx, size_t bytes, std::initializer_list<DevMem<T>*> bufs) {
    for (DevMem<T>* b : bufs) HIPCHK(b->alloc(bytes));
    return MPT_OK;
}
// device -> host array, enqueued (the caller synchronises once, behind its last copy); an output the caller did not ask for is skipped
static int copy_out(mpt_ctx* ctx, void* host, const void* dev, size_t bytes) {
    if (host) HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return MPT_OK;
}

// ---- shared: the colour a stage of the context works on -----------------------------------------------------------------------------
// In two steps.  check_source runs BEFORE wait_impl: a refused call changes nothing and waits for nothing.  `last`: the largest
// MPT_DISPLAY_* the stage takes (the other stages take SUM and FRAME).
static_assert(MPT_DISPLAY_SUM == MPT_DENOISE_SUM && MPT_DISPLAY_FRAME == MPT_DENOISE_FRAME, "one source check for every stage");
static int check_source(mpt_ctx* ctx, const char* stage, int32_t source, uint32_t samples, int32_t last = MPT_DENOISE_FRAME) {
    if (source < MPT_DENOISE_SUM || source > last) return fail(ctx, MPT_ERR_INVALID_ARG, std::string("bad ") + stage + " source");
    if (source == MPT_DENOISE_SUM && samples == 0) return fail(ctx, MPT_ERR_INVALID_ARG, std::string(stage) + " of the sum with samples = 0");
    return MPT_OK;
}
// pick_source runs AFTER wait_impl: only then the sum is complete and cur_target names the frame drawn last.
struct Source {
    const float4* color;
    float samples;   // the divisor of `color` (1 for a frame: x / 1 is x)
};
static Source pick_source(const mpt_ctx* ctx, int32_t source, uint32_t samples) {
    const bool sum = source == MPT_DENOISE_SUM;
    return {sum ? ctx->d_sum : ctx->d_accum[ctx->cur_target].get(), sum ? (float)samples : 1.0f};
}

// ---- shared: what a stage keeps, and how it is read -----------------------------------------------------------------------------------
// The validity rule of History, DisplayState and AoState: written in the scene and at the size the context has now.  A stage sets
// `epoch` to 0 before its launches and to guide_epoch only after they succeeded, on buffers of W x H, so a valid state has its buffers.
template <class S>
static bool stage_valid(const mpt_ctx* ctx, const S& s) {
    return s.epoch != 0 && s.epoch == ctx->guide_epoch && s.W == ctx->W && s.H == ctx->H;
}
// What a stage has to show: the buffer mpt_read_* copies and mpt_*_buffer hands out, and what to say when there is none (p == null).
struct StageResult {
    void* p;
    uint64_t bytes;
    const char* why;
};
static StageResult stage_result(const mpt_ctx* ctx, bool ready, void* p, uint32_t bytes_per_pixel, const char* why) {
    return {ready ? p : nullptr, (uint64_t)ctx->W * ctx->H * bytes_per_pixel, why};
}
static StageResult dn_result(const mpt_ctx* c) { return stage_result(c, c->dn.valid, c->dn.out.get(), 16, "no mpt_denoise result at this size"); }
static StageResult tp_result(const mpt_ctx* c) { return stage_result(c, stage_valid(c, c->tp), c->tp.hist[c->tp.cur].get(), 16, "no temporal history"); }
static StageResult sv_result(const mpt_ctx* c) { return stage_result(c, stage_valid(c, c->sv), c->sv.out.get(), 16, "no svgf state"); }
static StageResult dp_result(const mpt_ctx* c) {
    return stage_result(c, stage_valid(c, c->dp) && c->dp.shown, c->dp.out.get(), 4, "no mpt_display result");
}
static StageResult ao_result(const mpt_ctx* c) {
    return stage_result(c, stage_valid(c, c->ao), c->ao.out.get(), 4, "no mpt_ambient_occlusion result for this scene and size");
}
typedef StageResult (*ResultOf)(const mpt_ctx*);
static int need(mpt_ctx* ctx, const StageResult& r) { return r.p ? (int)MPT_OK : fail(ctx, MPT_ERR_NOT_READY, r.why); }
// mpt_read_*: no wait_impl — a result is complete on ctx->stream, whatever renders are still in flight
static int read_result(mpt_ctx* ctx, ResultOf of, void* host) {
    if (!ctx || !host) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    const StageResult r = of(ctx);
    int rc = need(ctx, r);
    if (rc || (rc = copy_out(ctx, host, r.p, r.bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
// mpt_*_buffer: called outside `guarded` (nothing here allocates or throws, and a queued render does not move a result)
static int result_buffer(mpt_ctx* ctx, ResultOf of, void** p, uint64_t* bytes) {
    if (!ctx || !p) return MPT_ERR_INVALID_ARG;
    const StageResult r = of(ctx);
    if (!r.p) return need(ctx, r);
    *p = r.p;
    if (bytes) *bytes = r.bytes;
    return MPT_OK;
}

// ---- shared: a reprojected history (temporal accumulation, SVGF) ------------------------------------------------------------------
static bool history_fits(const mpt_ctx* ctx, const History& h) { return h.hist[0] && h.W == ctx->W && h.H == ctx->H; }
// The fields TpFrame and SvFrame share, for a pass that reads h's current side and writes the other
template <class Frame>
static Frame history_frame(const History& h, Source src, const float4* ad, const float4* nc) {
    Frame T = {};
    T.color = src.color;
    T.samples = src.samples;
    T.ad = ad;
    T.nc = nc;
    T.hist_in = h.hist[h.cur].get();
    T.guide_in = h.guide[h.cur].get();
    T.hist_out = h.hist[h.cur ^ 1].get();
    T.guide_out = h.guide[h.cur ^ 1].get();
    T.n_reset = h.n_reset.get();
    T.W = h.W;
    T.H = h.H;
    return T;
}
// The end of a pass: its reset count comes back — the one host wait of the pass — into either info struct
template <class Info>
static int history_counts(mpt_ctx* ctx, const History& h, Info* out) {
    unsigned long long n_reset = 0;
    HIPCHK(hipMemcpyAsync(&n_reset, h.n_reset.get(), 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (out) {
        out->pixels_reset = n_reset;
        out->pixels_reprojected = (uint64_t)h.W * h.H - n_reset;
    }
    return MPT_OK;
}
// One accumulate call on the context's history `h`: buffers at the context's size, then pass(key, key_h) — the current camera's key
// and the history's, null when there is no valid history — from the current side into the other.  Nothing is kept if the pass fails;
// after it, its output is the history.
template <class Pass>
static int history_accumulate(mpt_ctx* ctx, History& h, Pass&& pass) {
    const bool have = stage_valid(ctx, h);
    int rc;
    if (!history_fits(ctx, h)) {
        h.W = h.H = 0;
        h.epoch = 0;
        if ((rc = scratch(ctx, (size_t)ctx->W * ctx->H * 16, {&h.hist[0], &h.hist[1], &h.guide[0], &h.guide[1]}))) return rc;
        HIPCHK(h.n_reset.alloc(8));
        h.W = ctx->W;
        h.H = ctx->H;
        h.cur = 0;
    }
    float key[14];
    guide_key(ctx->u, key);
    h.epoch = 0;
    if ((rc = pass(key, have ? h.cam : nullptr))) return rc;
    h.cur ^= 1;
    h.epoch = ctx->guide_epoch;
    memcpy(h.cam, key, sizeof key);
    return MPT_OK;
}

// One call of a stage that keeps a per-pixel result with 64-bit totals behind it (AoState, DirectState): the buffer at the context's
// size, launch(key, out) at the current camera's key between a pair of events, then the totals — the one host wait — and the epoch.
template <class State, class Launch>
static int stage_run(mpt_ctx* ctx, State& s, size_t out_bytes, unsigned long long* totals, size_t n_totals, float* ms, Launch&& launch) {
    if (!s.out || s.W != ctx->W || s.H != ctx->H) {
        s = State{};
        HIPCHK(s.out.alloc(out_bytes));
        s.W = ctx->W;
        s.H = ctx->H;
    }
    s.epoch = 0;
    float key[14];
    guide_key(ctx->u, key);
    Event e0, e1;
    HIPCHK(e0.create(hipEventCreate));
    HIPCHK(e1.create(hipEventCreate));
    HIPCHK(hipEventRecord(e0.get(), ctx->stream));
    const int rc = launch(key, s.out.get());
    if (rc) return rc;
    HIPCHK(hipEventRecord(e1.get(), ctx->stream));
    HIPCHK(hipMemcpyAsync(totals, (const char*)s.out.get() + out_bytes - n_totals * 8, n_totals * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s.epoch = ctx->guide_epoch;
    if (ms) HIPCHK(hipEventElapsedTime(ms, e0.get(), e1.get()));
    return MPT_OK;
}

// ---- guide pass and denoiser (mpt_denoise.h; the specification is in include/mpt.h) ------------------------------------------------
struct DnSigmas {
    int iterations;
    float sl, sn, sz;
};
static int dn_resolve(mpt_ctx* ctx, const mpt_denoise_params* p, DnSigmas& r) {
    if (p->iterations > MPT_DENOISE_MAX_ITERATIONS) return fail(ctx, MPT_ERR_INVALID_ARG, "denoise iterations > 8");
    r.iterations = p->iterations < 0 ? MPT_DENOISE_DEFAULT_ITERATIONS : p->iterations;
    r.sl = p->sigma_luminance > 0.0f ? p->sigma_luminance : MPT_DENOISE_DEFAULT_SIGMA_LUMINANCE;
    r.sn = p->sigma_normal > 0.0f ? p->sigma_normal : MPT_DENOISE_DEFAULT_SIGMA_NORMAL;
    r.sz = p->sigma_depth > 0.0f ? p->sigma_depth : MPT_DENOISE_DEFAULT_SIGMA_DEPTH;
    return MPT_OK;
}
// N levels on ctx->stream: level 0 demodulates src.color / src.samples, level N-1 remodulates into `out`; x[2] are the ping-pong buffers.
static int dn_filter(mpt_ctx* ctx, uint32_t W, uint32_t H, Source src, const float4* ad, const float4* guide, const DevMem<float4> x[2],
                     const DnSigmas& sg, float4* out) {
    const uint32_t n = W * H;
    if (sg.iterations == 0) {
        hipLaunchKernelGGL(k_dn_copy, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, src.color, src.samples, n, out);
        HIPCHK(hipGetLastError());
        return MPT_OK;
    }
    for (int i = 0; i < sg.iterations; ++i) {
        const bool first = i == 0, last = i == sg.iterations - 1;
        DnLevel L;
        L.color = src.color;
        L.ad = ad;
        L.guide = guide;
        L.xin = first ? nullptr : x[(i - 1) & 1].get();
        L.xout = last ? out : x[i & 1].get();
        L.W = W;
        L.H = H;
        L.step = 1u << i;
        L.samples = src.samples;
        L.sigma_n = sg.sn;
        L.sigma_z = sg.sz;
        L.sigma_l = sg.sl * ldexpf(1.0f, -i);
        const size_t lds = atrous_lds_bytes(L.step);
        const void* k = lds ? dn_level_kernel<true>(first, last) : dn_level_kernel<false>(first, last);
        void* args[] = {&L};
        HIPCHK(hipLaunchKernel(k, tile_grid(W, H), dim3(256), args, lds, ctx->stream));
    }
    return MPT_OK;
}
static int ensure_dn_buffers(mpt_ctx* ctx) {
    GuideState& g = ctx->gd;
    if (ctx->dn.out && g.W == ctx->W && g.H == ctx->H) return MPT_OK;
    g.W = g.H = 0;
    g.built = 0;
    ctx->dn.valid = false;
    const size_t n = (size_t)ctx->W * ctx->H;
    const int rc = scratch(ctx, n * 16, {&g.ad, &g.nc, &g.packed, &ctx->dn.x[0], &ctx->dn.x[1], &ctx->dn.out});
    if (rc) return rc;
    HIPCHK(g.prim.alloc(n * 4));
    g.W = ctx->W;
    g.H = ctx->H;
    return MPT_OK;
}
// The guide pass, when the guides are stale: one thread per pixel, 16 x 16 pixels per workgroup of four 8 x 8 tiles, the top of the
// tree staged in LDS as k_trace_rays does (the reference-order walk: it returns what the closest-first walk returns).
static int refresh_guides(mpt_ctx* ctx) {
    if (!ctx->have_scene || !ctx->have_uniforms || !ctx->W) return fail(ctx, MPT_ERR_NOT_READY, "scene, uniforms or size not set");
    if ((uint32_t)ctx->u.screenSize[0] != ctx->W || (uint32_t)ctx->u.screenSize[1] != ctx->H)
        return fail(ctx, MPT_ERR_INVALID_ARG, "uniforms.screenSize does not match mpt_resize");
    int rc = ensure_dn_buffers(ctx);
    if (rc) return rc;
    GuideState& g = ctx->gd;
    float key[14];
    guide_key(ctx->u, key);
    if (g.built == ctx->guide_epoch && memcmp(key, g.cam, sizeof key) == 0) return MPT_OK;
    hipLaunchKernelGGL(k_dn_guide, tile_grid(ctx->W, ctx->H), dim3(256), ref_lds_bytes(ctx), ctx->stream, scene_dev(ctx), key_f3(key, KEY_CAM),
                       key_f3(key, KEY_FIRST), key_f3(key, KEY_VU), key_f3(key, KEY_VV), ctx->u.screenSize[0], ctx->u.screenSize[1], ctx->W, ctx->H,
                       g.ad.get(), g.nc.get(), g.prim.get(), g.packed.get());
    HIPCHK(hipGetLastError());
    g.built = ctx->guide_epoch;
    memcpy(g.cam, key, sizeof key);
    return MPT_OK;
}
// What a stage of the context starts with, once its arguments are accepted: the renders in flight collected (a failed mpt_render_async
// is reported here; the sum is complete afterwards) and the guides of the current frame
static int settle_and_guide(mpt_ctx* ctx) {
    const int rc = wait_impl(ctx);
    return rc ? rc : refresh_guides(ctx);
}
static int read_aovs_impl(mpt_ctx* ctx, float* ad, float* nc, int32_t* prim) {
    if (!ctx || !ad || !nc) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    int rc = settle_and_guide(ctx);
    if (rc) return rc;
    const size_t n = (size_t)ctx->W * ctx->H;
    if ((rc = copy_out(ctx, ad, ctx->gd.ad.get(), n * 16)) || (rc = copy_out(ctx, nc, ctx->gd.nc.get(), n * 16)) ||
        (rc = copy_out(ctx, prim, ctx->gd.prim.get(), n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
// mpt_denoise and mpt_denoise_temporal: `src` through the context's guides into dn.out; no result while a launch may have failed
static int dn_run(mpt_ctx* ctx, Source src, const DnSigmas& sg) {
    ctx->dn.valid = false;
    const int rc = dn_filter(ctx, ctx->W, ctx->H, src, ctx->gd.ad.get(), ctx->gd.packed.get(), ctx->dn.x, sg, ctx->dn.out.get());
    if (rc) return rc;
    ctx->dn.valid = true;
    return MPT_OK;
}
static int denoise_impl(mpt_ctx* ctx, const mpt_denoise_params* p) {
    if (!ctx || !p) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    DnSigmas sg;
    int rc = dn_resolve(ctx, p, sg);
    if (rc || (rc = check_source(ctx, "denoise", p->source, p->samples)) || (rc = settle_and_guide(ctx))) return rc;
    return dn_run(ctx, pick_source(ctx, p->source, p->samples), sg);
}
static int denoise_temporal_impl(mpt_ctx* ctx, const mpt_denoise_params* p) {
    if (!ctx || !p) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    DnSigmas sg;
    int rc = dn_resolve(ctx, p, sg);
    if (rc || (rc = need(ctx, tp_result(ctx))) || (rc = settle_and_guide(ctx))) return rc;
    return dn_run(ctx, Source{(const float4*)tp_result(ctx).p, 1.0f}, sg);
}
static int denoise_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* color, const float* ad, const float* nc,
                              const mpt_denoise_params* p, float* out) {
    if (!ctx || !color || !ad || !nc || !p || !out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    DnSigmas sg;
    int rc = dn_resolve(ctx, p, sg);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    DevMem<float4> d_c, d_ad, d_nc, d_g, d_x[2], d_o;
    if ((rc = scratch(ctx, n * 16, {&d_g, &d_x[0], &d_x[1], &d_o})) || (rc = stage_in(ctx, d_c, color, n * 16)) ||
        (rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16)))
        return rc;
    hipLaunchKernelGGL(k_dn_pack, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_ad.get(), d_nc.get(), (uint32_t)n, d_g.get());
    HIPCHK(hipGetLastError());
    if ((rc = dn_filter(ctx, W, H, Source{d_c.get(), 1.0f}, d_ad.get(), d_g.get(), d_x, sg, d_o.get())) || (rc = copy_out(ctx, out, d_o.get(), n * 16)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
extern "C" int mpt_read_aovs(mpt_ctx* ctx, float* albedo_depth, float* normal_class, int32_t* prim) {
    return guarded(ctx, [&] { return read_aovs_impl(ctx, albedo_depth, normal_class, prim); });
}
extern "C" int mpt_denoise(mpt_ctx* ctx, const mpt_denoise_params* p) {
    return guarded(ctx, [&] { return denoise_impl(ctx, p); });
}
extern "C" int mpt_denoise_temporal(mpt_ctx* ctx, const mpt_denoise_params* p) {
    return guarded(ctx, [&] { return denoise_temporal_impl(ctx, p); });
}
extern "C" int mpt_read_denoised(mpt_ctx* ctx, float* rgba) {
    return guarded(ctx, [&] { return read_result(ctx, dn_result, rgba); });
}
extern "C" int mpt_denoised_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, dn_result, p, bytes); }
extern "C" int mpt_denoise_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* color, const float* albedo_depth, const float* normal_class,
                                 const mpt_denoise_params* p, float* out) {
    return guarded(ctx, [&] { return denoise_image_impl(ctx, w, h, color, albedo_depth, normal_class, p, out); });
}

// ---- ambient occlusion (mpt_ao.h; the specification is in include/mpt.h) -------------------------------------------------------------
static int ao_check(mpt_ctx* ctx, const mpt_ao_params* p) {
    if (!p) return fail(ctx, MPT_ERR_INVALID_ARG, "null ambient-occlusion params");
    if (p->sample_count == 0 || p->sample_count > MPT_AO_MAX_SAMPLES) return fail(ctx, MPT_ERR_INVALID_ARG, "ambient occlusion: sample_count outside 1..1024");
    if (p->radius != p->radius) return fail(ctx, MPT_ERR_INVALID_ARG, "ambient occlusion: the radius is NaN");
    if (!walk_valid(p->walk)) return fail(ctx, MPT_ERR_INVALID_ARG, "ambient occlusion: bad walk");
    return MPT_OK;
}
// One pass on ctx->stream over guides on the device, at the camera `key`; out: ao_out_bytes(W * H).
static int ao_launch(mpt_ctx* ctx, uint32_t W, uint32_t H, const float4* ad, const float4* nc, const float key[14], const mpt_ao_params* p, float* out) {
    AoPass P = {};
    P.ad = ad;
    P.nc = nc;
    P.out = out;
    P.n_pixels = W * H;
    HIPCHK(hipMemsetAsync(P.totals(), 0, 16, ctx->stream));
    pass_frame(P, key, W, H, *p);
    uint32_t gl = 0;
    while (gl < 6u && (2u << gl) <= p->sample_count) ++gl;   // min(N, 64) rounded down to a power of two
    P.group_log2 = gl;
    P.tmax = p->radius > 0.0f ? p->radius : INFINITY;
    static const WalkKernel<AoPass> k[3] = {k_ao<MPT_AO_REF>, k_ao<MPT_AO_REF_ALL_LDS>, k_ao<MPT_AO_OWN>};
    return tile_walk_launch(ctx, W, H, p->walk, k, P);
}
static size_t ao_out_bytes(size_t n_pixels) { return n_pixels * 8 + 16; }
static int ambient_occlusion_impl(mpt_ctx* ctx, const mpt_ao_params* p, mpt_ao_info* out) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    int rc = ao_check(ctx, p);
    if (rc || (rc = settle_and_guide(ctx))) return rc;
    unsigned long long totals[2] = {0, 0};
    float ms = 0.0f;
    rc = stage_run(ctx, ctx->ao, ao_out_bytes((size_t)ctx->W * ctx->H), totals, 2, out ? &ms : nullptr, [&](const float* key, float* o) {
        return ao_launch(ctx, ctx->W, ctx->H, ctx->gd.ad.get(), ctx->gd.nc.get(), key, p, o);
    });
    if (rc) return rc;
    if (out) {
        out->pixels_surface = totals[0];
        out->rays = totals[0] * p->sample_count;
        out->rays_occluded = totals[1];
        out->device_ms = (double)ms;
    }
    return MPT_OK;
}
// (ao, then the optional counts behind it: two copies and one wait, so not read_result)
static int read_ao_impl(mpt_ctx* ctx, float* ao, uint32_t* occluded) {
    if (!ctx || !ao) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    const StageResult r = ao_result(ctx);
    int rc = need(ctx, r);
    if (rc || (rc = copy_out(ctx, ao, r.p, r.bytes)) || (rc = copy_out(ctx, occluded, (const char*)r.p + r.bytes, r.bytes))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int ao_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* ad, const float* nc, const mpt_uniforms* cam, const mpt_ao_params* p,
                         float* ao_out, uint32_t* occ_out) {
    if (!ctx || !ad || !nc || !cam || !ao_out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    int rc = ao_check(ctx, p);
    if (rc) return rc;
    if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    DevMem<float4> d_ad, d_nc;
    DevMem<float> d_out;
    HIPCHK(d_out.alloc(ao_out_bytes(n)));
    if ((rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16))) return rc;
    float key[14];
    guide_key(*cam, key);
    if ((rc = ao_launch(ctx, W, H, d_ad.get(), d_nc.get(), key, p, d_out.get())) || (rc = copy_out(ctx, ao_out, d_out.get(), n * 4)) ||
        (rc = copy_out(ctx, occ_out, d_out.get() + n, n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
extern "C" int mpt_ambient_occlusion(mpt_ctx* ctx, const mpt_ao_params* p, mpt_ao_info* out) {
    return guarded(ctx, [&] { return ambient_occlusion_impl(ctx, p, out); });
}
extern "C" int mpt_read_ao(mpt_ctx* ctx, float* ao, uint32_t* occluded) {
    return guarded(ctx, [&] { return read_ao_impl(ctx, ao, occluded); });
}
extern "C" int mpt_ao_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, ao_result, p, bytes); }
extern "C" int mpt_ao_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* albedo_depth, const float* normal_class, const mpt_uniforms* cam,
                            const mpt_ao_params* p, float* ao_out, uint32_t* occluded_out) {
    return guarded(ctx, [&] { return ao_image_impl(ctx, w, h, albedo_depth, normal_class, cam, p, ao_out, occluded_out); });
}

// ---- direct lighting (mpt_direct.h; the specification is in include/mpt.h) -----------------------------------------------------------
// The light table of the scene in place, built when stale: k_light_collect appends the emissive primitives of the device arrays, the host
// sorts them by caller id, weighs them in float64 and uploads the table.  Nothing is kept of a build that fails.
static int ensure_lights(mpt_ctx* ctx) {
    if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
    if (ctx->lights.built) return MPT_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevMem<uint32_t> d_count;
    HIPCHK(d_count.alloc(4));
    HIPCHK(hipMemsetAsync(d_count.get(), 0, 4, ctx->stream));
    const uint32_t cap = (uint32_t)std::min<uint64_t>(ctx->n_prims, MPT_LIGHTS_MAX);
    DevMem<float4> d_list;
    HIPCHK(d_list.alloc((size_t)std::max(cap, 1u) * MPT_LIGHT_F4 * 16));
    hipLaunchKernelGGL(k_light_collect, dim3((ctx->n_prims + 255u) / 256u), dim3(256), 0, ctx->stream, (const float4*)ctx->d_prims, (const float4*)ctx->d_mats,
                       ctx->n_prims, cap, d_count.get(), d_list.get());
    HIPCHK(hipGetLastError());
    uint32_t seen = 0;
    HIPCHK(hipMemcpyAsync(&seen, d_count.get(), 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (seen > MPT_LIGHTS_MAX) return fail(ctx, MPT_ERR_BAD_SCENE, "more than MPT_LIGHTS_MAX (65536) emissive primitives: " + std::to_string(seen));
    std::vector<float> list((size_t)seen * 16);
    if (seen) HIPCHK(hipMemcpy(list.data(), d_list.get(), list.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> order(seen);
    for (uint32_t i = 0; i < seen; ++i) order[i] = i;
    auto id_of = [&](uint32_t i) {
        int32_t id;
        memcpy(&id, &list[(size_t)i * 16 + 7], 4);
        return id;
    };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return id_of(a) < id_of(b); });
    LightState t;
    std::vector<double> lum, csum;
    double C = 0.0;
    for (uint32_t i : order) {
        const float* r = &list[(size_t)i * 16];
        const bool tri = r[3] != 0.0f;
        double A;
        if (tri) {
            const double ax = r[4], ay = r[5], az = r[6], bx = r[8], by = r[9], bz = r[10];
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            A = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        } else {
            const double rad = r[4];
            A = ((4.0 * 3.14159265358979323846) * rad) * rad;
        }
        const double l = (0.2126 * (double)r[12] + 0.7152 * (double)r[13]) + 0.0722 * (double)r[14];
        const double Wk = A * l;
        if (!(std::isfinite(Wk) && Wk != 0.0)) continue;
        C += Wk;
        csum.push_back(C);
        lum.push_back(l);
        t.ids.push_back(id_of(i));
        t.h_rec.insert(t.h_rec.end(), r, r + 16);
        t.h_rec[t.h_rec.size() - 16 + 7] = 0.0f;   // (the id travelled here)
        (tri ? t.n_tri : t.n_sph)++;
    }
    const uint32_t n = t.n();
    t.h_cdf.resize(n);
    for (uint32_t k = 0; k < n; ++k) {
        t.h_cdf[k] = k + 1 == n ? 1.0f : (float)(csum[k] / C);
        t.h_rec[(size_t)k * 16 + 15] = (float)(C / lum[k]);
    }
    if (n) {
        HIPCHK(t.rec.alloc((size_t)n * 64));
        HIPCHK(t.cdf.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(t.rec.get(), t.h_rec.data(), (size_t)n * 64, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t.cdf.get(), t.h_cdf.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIPCHK(t.d_ids.alloc((size_t)n * 4));
        HIPCHK(hipMemcpy(t.d_ids.get(), t.ids.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    t.seen = seen;
    t.built = true;
    ctx->lights = std::move(t);
    return MPT_OK;
}
static int light_info_impl(mpt_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    int rc = wait_impl(ctx);
    if (rc || (rc = ensure_lights(ctx))) return rc;
    const LightState& t = ctx->lights;
    out[0] = t.n();
    out[1] = t.seen;
    out[2] = t.n_tri;
    out[3] = t.n_sph;
    return MPT_OK;
}
static int read_lights_impl(mpt_ctx* ctx, uint32_t capacity, int32_t* prim_id, float* records, float* cdf, uint32_t* n_out) {
    if (!ctx || !n_out) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    int rc = wait_impl(ctx);
    if (rc || (rc = ensure_lights(ctx))) return rc;
    const LightState& t = ctx->lights;
    const size_t m = std::min(capacity, t.n());
    if (prim_id && m) memcpy(prim_id, t.ids.data(), m * 4);
    if (records && m) memcpy(records, t.h_rec.data(), m * 64);
    if (cdf && m) memcpy(cdf, t.h_cdf.data(), m * 4);
    *n_out = t.n();
    return MPT_OK;
}
static int direct_check(mpt_ctx* ctx, const mpt_direct_params* p) {
    if (!p) return fail(ctx, MPT_ERR_INVALID_ARG, "null direct-lighting params");
    if (p->sample_count == 0 || p->sample_count > MPT_DIRECT_MAX_SAMPLES) return fail(ctx, MPT_ERR_INVALID_ARG, "direct lighting: sample_count outside 1..1024");
    if (!walk_valid(p->walk)) return fail(ctx, MPT_ERR_INVALID_ARG, "direct lighting: bad walk");
    return MPT_OK;
}
static size_t direct_out_bytes(size_t n_pixels) { return n_pixels * 24 + 24; }
// One pass on ctx->stream over guides on the device, at the camera `key`, with the (built) light table; out: direct_out_bytes(W * H).
static int direct_launch(mpt_ctx* ctx, uint32_t W, uint32_t H, const float4* ad, const float4* nc, const float key[14], const mpt_direct_params* p, float4* out) {
    DirectPass P = {};
    P.ad = ad;
    P.nc = nc;
    P.out = out;
    P.n_pixels = W * H;
    HIPCHK(hipMemsetAsync(P.totals(), 0, 24, ctx->stream));
    P.lights = ctx->lights.rec.get();
    P.cdf = ctx->lights.cdf.get();
    P.n_lights = ctx->lights.n();
    pass_frame(P, key, W, H, *p);
    static const WalkKernel<DirectPass> area[3] = {k_direct<MPT_AO_REF>, k_direct<MPT_AO_REF_ALL_LDS>, k_direct<MPT_AO_OWN>},
                                        cone[3] = {k_direct_cone<MPT_AO_REF>, k_direct_cone<MPT_AO_REF_ALL_LDS>, k_direct_cone<MPT_AO_OWN>};
    const bool use_cone = ctx->light_sampling == MPT_LIGHT_SAMPLING_CONE;
    if (ctx->light_candidates == 1u) return tile_walk_launch(ctx, W, H, p->walk, use_cone ? cone : area, P);   // today's kernels, bit for bit
    // the same pass with every sample resampled from the candidates (mpt_ris.h)
    static const WalkKernel<DirectRisPass> ris_area[3] = {k_direct_ris<MPT_AO_REF>, k_direct_ris<MPT_AO_REF_ALL_LDS>, k_direct_ris<MPT_AO_OWN>},
                                           ris_cone[3] = {k_direct_ris_cone<MPT_AO_REF>, k_direct_ris_cone<MPT_AO_REF_ALL_LDS>,
                                                          k_direct_ris_cone<MPT_AO_OWN>};
    const DirectRisPass R = {P, ctx->light_candidates};
    return tile_walk_launch(ctx, W, H, p->walk, use_cone ? ris_cone : ris_area, R);
}
static StageResult di_result(const mpt_ctx* c) {
    return stage_result(c, stage_valid(c, c->di), c->di.out.get(), 16, "no mpt_direct_lighting result for this scene and size");
}
static int direct_lighting_impl(mpt_ctx* ctx, const mpt_direct_params* p, mpt_direct_info* out) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    int rc = direct_check(ctx, p);
    if (rc || (rc = settle_and_guide(ctx)) || (rc = ensure_lights(ctx))) return rc;
    unsigned long long totals[3] = {0, 0, 0};
    float ms = 0.0f;
    rc = stage_run(ctx, ctx->di, direct_out_bytes((size_t)ctx->W * ctx->H), totals, 3, out ? &ms : nullptr, [&](const float* key, float4* o) {
        return direct_launch(ctx, ctx->W, ctx->H, ctx->gd.ad.get(), ctx->gd.nc.get(), key, p, o);
    });
    if (rc) return rc;
    if (out) {
        out->pixels_surface = totals[0];
        out->rays = totals[1];
        out->rays_occluded = totals[1] - totals[2];
        out->lights = ctx->lights.n();
        out->device_ms = (double)ms;
    }
    return MPT_OK;
}
// (rgba, then the optional counts behind it: up to three copies and one wait, so not read_result)
static int read_direct_impl(mpt_ctx* ctx, float* rgba, uint32_t* traced, uint32_t* unoccluded) {
    if (!ctx || !rgba) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    const StageResult r = di_result(ctx);
    int rc = need(ctx, r);
    const size_t n = (size_t)ctx->W * ctx->H;
    if (rc || (rc = copy_out(ctx, rgba, r.p, r.bytes)) || (rc = copy_out(ctx, traced, (const char*)r.p + n * 16, n * 4)) ||
        (rc = copy_out(ctx, unoccluded, (const char*)r.p + n * 20, n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int direct_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* ad, const float* nc, const mpt_uniforms* cam, const mpt_direct_params* p,
                             float* rgba_out, uint32_t* traced_out, uint32_t* unocc_out) {
    if (!ctx || !ad || !nc || !cam || !rgba_out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    int rc = direct_check(ctx, p);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = ensure_lights(ctx))) return rc;
    const size_t n = (size_t)W * H;
    DevMem<float4> d_ad, d_nc, d_out;
    HIPCHK(d_out.alloc(direct_out_bytes(n)));
    if ((rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16))) return rc;
    float key[14];
    guide_key(*cam, key);
    const char* o = (const char*)d_out.get();
    if ((rc = direct_launch(ctx, W, H, d_ad.get(), d_nc.get(), key, p, d_out.get())) || (rc = copy_out(ctx, rgba_out, o, n * 16)) ||
        (rc = copy_out(ctx, traced_out, o + n * 16, n * 4)) || (rc = copy_out(ctx, unocc_out, o + n * 20, n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
extern "C" int mpt_light_info(mpt_ctx* ctx, uint64_t out[4]) {
    return guarded(ctx, [&] { return light_info_impl(ctx, out); });
}
extern "C" int mpt_read_lights(mpt_ctx* ctx, uint32_t capacity, int32_t* prim_id, float* records, float* cdf, uint32_t* n_out) {
    return guarded(ctx, [&] { return read_lights_impl(ctx, capacity, prim_id, records, cdf, n_out); });
}
extern "C" int mpt_direct_lighting(mpt_ctx* ctx, const mpt_direct_params* p, mpt_direct_info* out) {
    return guarded(ctx, [&] { return direct_lighting_impl(ctx, p, out); });
}
extern "C" int mpt_read_direct(mpt_ctx* ctx, float* rgba, uint32_t* traced, uint32_t* unoccluded) {
    return guarded(ctx, [&] { return read_direct_impl(ctx, rgba, traced, unoccluded); });
}
extern "C" int mpt_direct_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, di_result, p, bytes); }
extern "C" int mpt_direct_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* albedo_depth, const float* normal_class, const mpt_uniforms* cam,
                                const mpt_direct_params* p, float* rgba_out, uint32_t* traced_out, uint32_t* unoccluded_out) {
    return guarded(ctx, [&] { return direct_image_impl(ctx, w, h, albedo_depth, normal_class, cam, p, rgba_out, traced_out, unoccluded_out); });
}

// ---- spatial reservoir reuse (mpt_restir.h; the specification is in include/mpt.h) ---------------------------------------------------
struct RestirResolved {
    uint32_t M, K, R;
    float normal_thr, depth_tol;
};
// The argument checks, in front of wait_impl: a refused call changes nothing and waits for nothing.
static int restir_check(mpt_ctx* ctx, const mpt_restir_params* p, RestirResolved& r) {
    if (!p) return fail(ctx, MPT_ERR_INVALID_ARG, "null restir params");
    if (p->sample_count == 0 || p->sample_count > MPT_DIRECT_MAX_SAMPLES) return fail(ctx, MPT_ERR_INVALID_ARG, "restir: sample_count outside 1..1024");
    if (!walk_valid(p->walk)) return fail(ctx, MPT_ERR_INVALID_ARG, "restir: bad walk");
    if (p->mode != MPT_RESTIR_UNBIASED && p->mode != MPT_RESTIR_BIASED) return fail(ctx, MPT_ERR_INVALID_ARG, "restir: bad mode");
    if (p->neighbours > MPT_RESTIR_MAX_NEIGHBOURS) return fail(ctx, MPT_ERR_INVALID_ARG, "restir: neighbours > 16");
    if (p->radius > MPT_RESTIR_MAX_RADIUS) return fail(ctx, MPT_ERR_INVALID_ARG, "restir: radius > 64");
    if (p->normal_threshold != p->normal_threshold || p->depth_tolerance != p->depth_tolerance)
        return fail(ctx, MPT_ERR_INVALID_ARG, "restir: a threshold is NaN");
    if (ctx->light_sampling == MPT_LIGHT_SAMPLING_CONE)
        return fail(ctx, MPT_ERR_INVALID_ARG, "restir: lights are sampled by area only (mpt_set_light_sampling is MPT_LIGHT_SAMPLING_CONE)");
    r.M = ctx->light_candidates;   // (read at the start)
    r.K = p->neighbours;
    r.R = p->radius ? p->radius : MPT_RESTIR_DEFAULT_RADIUS;
    r.normal_thr = p->normal_threshold > 0.0f ? p->normal_threshold : MPT_RESTIR_DEFAULT_NORMAL_THRESHOLD;
    r.depth_tol = p->depth_tolerance > 0.0f ? p->depth_tolerance : MPT_RESTIR_DEFAULT_DEPTH_TOLERANCE;
    return MPT_OK;
}
static size_t restir_out_bytes(size_t n_pixels) { return n_pixels * 24 + MPT_RS_TOTAL_WORDS * 8; }
static size_t restir_res_bytes(size_t n_pixels) { return n_pixels * 32; }
// The rounds on ctx->stream over guides on the device, at the camera `key`, with the (built) light table: the sums, the counts, the
// totals and the picks zeroed, then k_restir_initial and k_restir_merge once per sample.  out: restir_out_bytes(W * H); S: 16 bytes per
// pixel; initial, pick: restir_res_bytes(W * H).
static int restir_launch(mpt_ctx* ctx, uint32_t W, uint32_t H, const float4* ad, const float4* nc, const float key[14], const mpt_restir_params* p,
                         const RestirResolved& r, float4* out, float4* S, uint4* initial, uint4* pick) {
    RestirPass P = {};
    const size_t n = (size_t)W * H;
    P.ad = ad;
    P.nc = nc;
    P.out = out;
    P.n_pixels = W * H;
    P.S = S;
    P.initial = initial;
    P.pick = pick;
    HIPCHK(hipMemsetAsync(P.traced(), 0, n * 8 + MPT_RS_TOTAL_WORDS * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(S, 0, n * 16, ctx->stream));
    HIPCHK(hipMemsetAsync(pick, 0, restir_res_bytes(n), ctx->stream));
    P.lights = ctx->lights.rec.get();
    P.cdf = ctx->lights.cdf.get();
    P.n_lights = ctx->lights.n();
    pass_frame(P, key, W, H, *p);
    P.M = r.M;
    P.K = r.K;
    P.R = r.R;
    P.normal_threshold = r.normal_thr;
    P.depth_tolerance = r.depth_tol;
    static const WalkKernel<RestirPass> initial_k[3] = {k_restir_initial<MPT_AO_REF>, k_restir_initial<MPT_AO_REF_ALL_LDS>, k_restir_initial<MPT_AO_OWN>},
                                        unbiased[3] = {k_restir_merge<MPT_AO_REF, true>, k_restir_merge<MPT_AO_REF_ALL_LDS, true>,
                                                       k_restir_merge<MPT_AO_OWN, true>},
                                        biased[3] = {k_restir_merge<MPT_AO_REF, false>, k_restir_merge<MPT_AO_REF_ALL_LDS, false>,
                                                     k_restir_merge<MPT_AO_OWN, false>};
    for (uint32_t round = 0; round < p->sample_count; ++round) {
        P.round = round;
        int rc = tile_walk_launch(ctx, W, H, p->walk, initial_k, P);
        if (rc || (rc = tile_walk_launch(ctx, W, H, p->walk, p->mode == MPT_RESTIR_UNBIASED ? unbiased : biased, P))) return rc;
    }
    return MPT_OK;
}
static StageResult rs_result(const mpt_ctx* c) {
    return stage_result(c, stage_valid(c, c->rs), c->rs.out.get(), 16, "no mpt_direct_restir result for this scene and size");
}
static int direct_restir_impl(mpt_ctx* ctx, const mpt_restir_params* p, mpt_restir_info* out) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    RestirResolved r;
    int rc = restir_check(ctx, p, r);
    if (rc || (rc = settle_and_guide(ctx)) || (rc = ensure_lights(ctx))) return rc;
    std::vector<unsigned long long> slots(MPT_RS_TOTAL_WORDS, 0ull);   // the totals, MPT_RS_SLOTS times (mpt_restir.h)
    float ms = 0.0f;
    const size_t n = (size_t)ctx->W * ctx->H;
    rc = stage_run(ctx, ctx->rs, restir_out_bytes(n), slots.data(), MPT_RS_TOTAL_WORDS, out ? &ms : nullptr, [&](const float* key, float4* o) -> int {
        RestirState& s = ctx->rs;
        if (!s.S) {   // (stage_run has made a fresh state of this size)
            HIPCHK(s.S.alloc(n * 16));
            HIPCHK(s.res[0].alloc(restir_res_bytes(n)));
            HIPCHK(s.res[1].alloc(restir_res_bytes(n)));
        }
        return restir_launch(ctx, ctx->W, ctx->H, ctx->gd.ad.get(), ctx->gd.nc.get(), key, p, r, o, s.S.get(), s.res[0].get(), s.res[1].get());
    });
    if (rc) return rc;
    if (out) {
        unsigned long long totals[MPT_RS_TOTALS] = {};
        for (uint32_t s = 0; s < MPT_RS_SLOTS; ++s)
            for (int k = 0; k < MPT_RS_TOTALS; ++k) totals[k] += slots[s * MPT_RS_SLOT_WORDS + k];
        const unsigned long long traced = totals[MPT_RS_INITIAL] + totals[MPT_RS_FINAL] + totals[MPT_RS_CORRECTION];
        out->pixels_surface = totals[MPT_RS_SURFACE];
        out->rays_initial = totals[MPT_RS_INITIAL];
        out->rays_final = totals[MPT_RS_FINAL];
        out->rays_correction = totals[MPT_RS_CORRECTION];
        out->rays_occluded = traced - totals[MPT_RS_UNOCCLUDED];
        out->neighbours_accepted = totals[MPT_RS_ACCEPTED];
        out->samples_from_neighbours = totals[MPT_RS_FROM_NEIGHBOUR];
        out->lights = ctx->lights.n();
        out->device_ms = (double)ms;
    }
    return MPT_OK;
}
static int read_restir_impl(mpt_ctx* ctx, float* rgba, uint32_t* traced, uint32_t* unoccluded) {
    if (!ctx || !rgba) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    const StageResult r = rs_result(ctx);
    int rc = need(ctx, r);
    const size_t n = (size_t)ctx->W * ctx->H;
    if (rc || (rc = copy_out(ctx, rgba, r.p, r.bytes)) || (rc = copy_out(ctx, traced, (const char*)r.p + n * 16, n * 4)) ||
        (rc = copy_out(ctx, unoccluded, (const char*)r.p + n * 20, n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
// six of a reservoir's eight words per pixel (RestirPass: the last two are padding)
static int read_restir_reservoirs_impl(mpt_ctx* ctx, int32_t which, uint32_t* out) {
    if (!ctx || !out || (which != 0 && which != 1)) return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_read_restir_reservoirs: null argument or which not 0 or 1");
    int rc = need(ctx, rs_result(ctx));
    if (rc) return rc;
    const size_t n = (size_t)ctx->W * ctx->H;
    std::vector<uint32_t> words(n * 8);
    HIPCHK(hipMemcpyAsync(words.data(), ctx->rs.res[which].get(), n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) memcpy(out + 6 * i, &words[8 * i], 24);
    return MPT_OK;
}
static int restir_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* ad, const float* nc, const mpt_uniforms* cam, const mpt_restir_params* p,
                             float* rgba_out, uint32_t* traced_out, uint32_t* unocc_out) {
    if (!ctx || !ad || !nc || !cam || !rgba_out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    RestirResolved r;
    int rc = restir_check(ctx, p, r);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = ensure_lights(ctx))) return rc;
    const size_t n = (size_t)W * H;
    DevMem<float4> d_ad, d_nc, d_out, d_S;
    DevMem<uint4> d_res[2];
    HIPCHK(d_out.alloc(restir_out_bytes(n)));
    HIPCHK(d_S.alloc(n * 16));
    HIPCHK(d_res[0].alloc(restir_res_bytes(n)));
    HIPCHK(d_res[1].alloc(restir_res_bytes(n)));
    if ((rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16))) return rc;
    float key[14];
    guide_key(*cam, key);
    const char* o = (const char*)d_out.get();
    if ((rc = restir_launch(ctx, W, H, d_ad.get(), d_nc.get(), key, p, r, d_out.get(), d_S.get(), d_res[0].get(), d_res[1].get())) ||
        (rc = copy_out(ctx, rgba_out, o, n * 16)) || (rc = copy_out(ctx, traced_out, o + n * 16, n * 4)) ||
        (rc = copy_out(ctx, unocc_out, o + n * 20, n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
extern "C" int mpt_direct_restir(mpt_ctx* ctx, const mpt_restir_params* p, mpt_restir_info* out) {
    return guarded(ctx, [&] { return direct_restir_impl(ctx, p, out); });
}
extern "C" int mpt_read_restir(mpt_ctx* ctx, float* rgba, uint32_t* traced, uint32_t* unoccluded) {
    return guarded(ctx, [&] { return read_restir_impl(ctx, rgba, traced, unoccluded); });
}
extern "C" int mpt_restir_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, rs_result, p, bytes); }
extern "C" int mpt_restir_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* albedo_depth, const float* normal_class, const mpt_uniforms* cam,
                                const mpt_restir_params* p, float* rgba_out, uint32_t* traced_out, uint32_t* unoccluded_out) {
    return guarded(ctx, [&] { return restir_image_impl(ctx, w, h, albedo_depth, normal_class, cam, p, rgba_out, traced_out, unoccluded_out); });
}
extern "C" int mpt_read_restir_reservoirs(mpt_ctx* ctx, int32_t which, uint32_t* out) {
    return guarded(ctx, [&] { return read_restir_reservoirs_impl(ctx, which, out); });
}

// ---- temporal accumulation (mpt_temporal.h; the specification is in include/mpt.h) ---------------------------------------------
struct TpResolved {
    float max_history, depth_tol, normal_thr, min_weight;
};
// (the reprojection parameters of SVGF's step A are these too: mpt_svgf_params names them alike)
template <class Params>
static int tp_resolve(mpt_ctx* ctx, const char* stage, const Params* p, TpResolved& r) {
    if (p->depth_tolerance != p->depth_tolerance || p->normal_threshold != p->normal_threshold || p->min_weight != p->min_weight)
        return fail(ctx, MPT_ERR_INVALID_ARG, std::string(stage) + ": a tolerance is NaN");
    r.max_history = (float)(p->max_history ? p->max_history : MPT_TEMPORAL_DEFAULT_MAX_HISTORY);
    r.depth_tol = p->depth_tolerance > 0.0f ? p->depth_tolerance : MPT_TEMPORAL_DEFAULT_DEPTH_TOLERANCE;
    r.normal_thr = p->normal_threshold > 0.0f ? p->normal_threshold : MPT_TEMPORAL_DEFAULT_NORMAL_THRESHOLD;
    r.min_weight = p->min_weight > 0.0f ? p->min_weight : MPT_TEMPORAL_DEFAULT_MIN_WEIGHT;
    return MPT_OK;
}
// The per-frame constants of k_tp_reproject / k_sv_reproject from the two cameras' guide_key, by the expressions of include/mpt.h in
// float32.  key_h = nullptr: no history.  Returns the MPT_TP_* mode of the kernel.
template <class Frame>
static int tp_frame_constants(Frame& T, const float key[14], const float* key_h, const TpResolved& r) {
    T.fW = (float)T.W;
    T.fH = (float)T.H;
    T.cam = key_f3(key, KEY_CAM);
    T.vu = key_f3(key, KEY_VU);
    T.vv = key_f3(key, KEY_VV);
    T.first = key_f3(key, KEY_FIRST);
    T.depth_tol = r.depth_tol;
    T.normal_thr = r.normal_thr;
    T.min_weight = r.min_weight;
    T.max_history = r.max_history;
    int mode = MPT_TP_NONE;
    if (key_h) {
        mode = memcmp(key, key_h, 14 * sizeof(float)) == 0 ? MPT_TP_SAME : MPT_TP_MOVED;
        T.cam_h = key_f3(key_h, KEY_CAM);
        T.vu_h = key_f3(key_h, KEY_VU);
        T.vv_h = key_f3(key_h, KEY_VV);
        const F3 a = T.vu_h, b = T.vv_h;
        T.nn = F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
        T.fc = F3{key_h[9] - key_h[0], key_h[10] - key_h[1], key_h[11] - key_h[2]};
        T.fcnn = tp_dot(T.fc, T.nn);
        T.uu = tp_dot(T.vu_h, T.vu_h);
        T.vvl = tp_dot(T.vv_h, T.vv_h);
    }
    return mode;
}
// One pass on ctx->stream from h's current side into the other, then the wait for its counts
static int tp_launch(mpt_ctx* ctx, const History& h, Source src, const float4* ad, const float4* nc, const float key[14], const float* key_h,
                     const TpResolved& r, mpt_temporal_info* out) {
    TpFrame T = history_frame<TpFrame>(h, src, ad, nc);
    const int mode = tp_frame_constants(T, key, key_h, r);
    HIPCHK(hipMemsetAsync(T.n_reset, 0, 8, ctx->stream));
    void* args[] = {&T};
    HIPCHK(hipLaunchKernel(tp_kernel(mode), tile_grid(T.W, T.H), dim3(256), args, 0, ctx->stream));
    return history_counts(ctx, h, out);
}
static int temporal_accumulate_impl(mpt_ctx* ctx, const mpt_temporal_params* p, mpt_temporal_info* out) {
    if (!ctx || !p) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    TpResolved r;
    int rc = check_source(ctx, "temporal accumulation", p->source, p->samples);
    if (rc || (rc = tp_resolve(ctx, "temporal accumulation", p, r)) || (rc = settle_and_guide(ctx))) return rc;
    const Source src = pick_source(ctx, p->source, p->samples);
    return history_accumulate(ctx, ctx->tp, [&](const float* key, const float* key_h) {
        return tp_launch(ctx, ctx->tp, src, ctx->gd.ad.get(), ctx->gd.nc.get(), key, key_h, r, out);
    });
}
static int temporal_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* color, const float* ad, const float* nc, const mpt_uniforms* cam,
                               const float* hist_h, const float* ad_h, const float* nc_h, const mpt_uniforms* cam_h,
                               const mpt_temporal_params* p, float* hist_out, mpt_temporal_info* out) {
    if (!ctx || !color || !ad || !nc || !cam || !p || !hist_out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    if (hist_h && (!ad_h || !nc_h || !cam_h)) return fail(ctx, MPT_ERR_INVALID_ARG, "a history without its guides or camera");
    TpResolved r;
    int rc = tp_resolve(ctx, "temporal accumulation", p, r);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    History h;   // side 0: the caller's history (none: null buffers), side 1: the result
    h.W = W;
    h.H = H;
    DevMem<float4> d_c, d_ad, d_nc, d_adh, d_nch;
    if ((rc = scratch(ctx, n * 16, {&h.hist[1], &h.guide[1]}))) return rc;
    HIPCHK(h.n_reset.alloc(8));
    if ((rc = stage_in(ctx, d_c, color, n * 16)) || (rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16))) return rc;
    float key[14], key_h[14];
    guide_key(*cam, key);
    if (hist_h) {
        if ((rc = scratch(ctx, n * 16, {&h.guide[0]})) || (rc = stage_in(ctx, h.hist[0], hist_h, n * 16)) ||
            (rc = stage_in(ctx, d_adh, ad_h, n * 16)) || (rc = stage_in(ctx, d_nch, nc_h, n * 16)))
            return rc;
        hipLaunchKernelGGL(k_tp_pack, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_adh.get(), d_nch.get(), (uint32_t)n, h.guide[0].get());
        HIPCHK(hipGetLastError());
        guide_key(*cam_h, key_h);
    }
    if ((rc = tp_launch(ctx, h, Source{d_c.get(), 1.0f}, d_ad.get(), d_nc.get(), key, hist_h ? key_h : nullptr, r, out)) ||
        (rc = copy_out(ctx, hist_out, h.hist[1].get(), n * 16)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
// mpt_temporal_reset, mpt_svgf_reset: lets go of a state of the context once nothing on the stream uses it any more
template <class State>
static int reset_state(mpt_ctx* ctx, State mpt_ctx::*state) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->*state = State{};
    return MPT_OK;
}
extern "C" int mpt_temporal_accumulate(mpt_ctx* ctx, const mpt_temporal_params* p, mpt_temporal_info* out) {
    return guarded(ctx, [&] { return temporal_accumulate_impl(ctx, p, out); });
}
extern "C" int mpt_read_temporal(mpt_ctx* ctx, float* rgba) {
    return guarded(ctx, [&] { return read_result(ctx, tp_result, rgba); });
}
extern "C" int mpt_temporal_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, tp_result, p, bytes); }
extern "C" int mpt_temporal_reset(mpt_ctx* ctx) {
    return guarded(ctx, [&] { return reset_state(ctx, &mpt_ctx::tp); });
}
extern "C" int mpt_temporal_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* color, const float* albedo_depth_cur, const float* normal_class_cur,
                                  const mpt_uniforms* cam_cur, const float* history_prev, const float* albedo_depth_prev, const float* normal_class_prev,
                                  const mpt_uniforms* cam_prev, const mpt_temporal_params* p, float* history_out, mpt_temporal_info* out) {
    return guarded(ctx, [&] {
        return temporal_image_impl(ctx, w, h, color, albedo_depth_cur, normal_class_cur, cam_cur, history_prev, albedo_depth_prev, normal_class_prev,
                                   cam_prev, p, history_out, out);
    });
}

// ---- temporal reservoir reuse (mpt_restir_temporal.h; the specification is in include/mpt.h) -----------------------------------------
// The spatial call's frame-to-frame counterpart.  It stands here, behind temporal accumulation, because it takes the camera arithmetic,
// k_tp_pack and reset_state from there; the reservoirs, the totals and the result block are the spatial call's (restir_*_bytes, MPT_RS_*).
struct RtResolved {
    uint32_t M, C;
    float normal_thr, depth_tol;
};
// The argument checks, in front of wait_impl: a refused call changes nothing and waits for nothing.
static int rt_check(mpt_ctx* ctx, const mpt_restir_temporal_params* p, RtResolved& r) {
    if (!p) return fail(ctx, MPT_ERR_INVALID_ARG, "null restir temporal params");
    if (!walk_valid(p->walk)) return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: bad walk");
    if (p->mode != MPT_RESTIR_UNBIASED && p->mode != MPT_RESTIR_BIASED) return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: bad mode");
    if (p->max_history > MPT_RESTIR_TEMPORAL_MAX_HISTORY) return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: max_history > 1024");
    if (p->normal_threshold != p->normal_threshold || p->depth_tolerance != p->depth_tolerance)
        return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: a threshold is NaN");
    if (ctx->light_sampling == MPT_LIGHT_SAMPLING_CONE)
        return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: lights are sampled by area only (mpt_set_light_sampling is MPT_LIGHT_SAMPLING_CONE)");
    r.M = ctx->light_candidates;   // (read at the start)
    r.C = p->max_history ? p->max_history : MPT_RESTIR_TEMPORAL_DEFAULT_HISTORY;
    r.normal_thr = p->normal_threshold > 0.0f ? p->normal_threshold : MPT_RESTIR_DEFAULT_NORMAL_THRESHOLD;
    r.depth_tol = p->depth_tolerance > 0.0f ? p->depth_tolerance : MPT_RESTIR_DEFAULT_DEPTH_TOLERANCE;
    return MPT_OK;
}
// One frame on ctx->stream over guides on the device, at the camera `key`, with the (built) light table: the counts and the totals
// zeroed, then k_restir_initial and k_restir_temporal.  key_h = nullptr: no history (res_in and guide_in are not read).  out:
// restir_out_bytes(W * H); initial, res_in, res_out: restir_res_bytes(W * H); the guides 16 bytes per pixel.
static int rt_launch(mpt_ctx* ctx, uint32_t W, uint32_t H, const float4* ad, const float4* nc, const float key[14], const float* key_h,
                     const mpt_restir_temporal_params* p, const RtResolved& r, float4* out, uint4* initial, const uint4* res_in, const float4* guide_in,
                     uint4* res_out, float4* guide_out) {
    RestirTemporalPass T = {};
    RestirPass& P = T.base;
    const size_t n = (size_t)W * H;
    P.ad = ad;
    P.nc = nc;
    P.out = out;
    P.n_pixels = W * H;
    P.initial = initial;
    HIPCHK(hipMemsetAsync(P.traced(), 0, n * 8 + MPT_RS_TOTAL_WORDS * 8, ctx->stream));
    P.lights = ctx->lights.rec.get();
    P.cdf = ctx->lights.cdf.get();
    P.n_lights = ctx->lights.n();
    const struct {
        uint32_t sample_begin, sample_count, seed_lo, seed_hi;
    } range = {p->frame, 1u, p->seed_lo, p->seed_hi};   // the frame is round 0 of a one-sample range that begins at its number
    pass_frame(P, key, W, H, range);
    P.M = r.M;
    P.normal_threshold = r.normal_thr;
    P.depth_tolerance = r.depth_tol;
    T.res_in = res_in;
    T.guide_in = guide_in;
    T.res_out = res_out;
    T.guide_out = guide_out;
    T.cap = r.C * r.M;
    T.mode = MPT_TP_NONE;
    if (key_h) {   // (by the expressions of tp_frame_constants)
        T.mode = memcmp(key, key_h, 14 * sizeof(float)) == 0 ? MPT_TP_SAME : MPT_TP_MOVED;
        T.cam_h = RestirCamera{key_f3(key_h, KEY_CAM), key_f3(key_h, KEY_FIRST), key_f3(key_h, KEY_VU), key_f3(key_h, KEY_VV), (float)W, (float)H};
        const F3 a = T.cam_h.vu, b = T.cam_h.vv;
        T.nn = F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
        T.fc = F3{key_h[9] - key_h[0], key_h[10] - key_h[1], key_h[11] - key_h[2]};
        T.fcnn = tp_dot(T.fc, T.nn);
        T.uu = tp_dot(a, a);
        T.vvl = tp_dot(b, b);
    }
    static const WalkKernel<RestirPass> initial_k[3] = {k_restir_initial<MPT_AO_REF>, k_restir_initial<MPT_AO_REF_ALL_LDS>, k_restir_initial<MPT_AO_OWN>};
    static const WalkKernel<RestirTemporalPass> unbiased[3] = {k_restir_temporal<MPT_AO_REF, true>, k_restir_temporal<MPT_AO_REF_ALL_LDS, true>,
                                                               k_restir_temporal<MPT_AO_OWN, true>},
                                                biased[3] = {k_restir_temporal<MPT_AO_REF, false>, k_restir_temporal<MPT_AO_REF_ALL_LDS, false>,
                                                             k_restir_temporal<MPT_AO_OWN, false>};
    int rc = tile_walk_launch(ctx, W, H, p->walk, initial_k, P);
    if (rc || (rc = tile_walk_launch(ctx, W, H, p->walk, p->mode == MPT_RESTIR_UNBIASED ? unbiased : biased, T))) return rc;
    return MPT_OK;
}
// mpt_restir_temporal_info from the totals, MPT_RS_SLOTS times (mpt_restir.h)
static void rt_info(const mpt_ctx* ctx, const unsigned long long* slots, float ms, mpt_restir_temporal_info* out) {
    unsigned long long totals[MPT_RS_TOTALS] = {};
    for (uint32_t s = 0; s < MPT_RS_SLOTS; ++s)
        for (int k = 0; k < MPT_RS_TOTALS; ++k) totals[k] += slots[s * MPT_RS_SLOT_WORDS + k];
    const unsigned long long traced = totals[MPT_RS_INITIAL] + totals[MPT_RS_FINAL] + totals[MPT_RS_CORRECTION];
    out->pixels_surface = totals[MPT_RS_SURFACE];
    out->rays_initial = totals[MPT_RS_INITIAL];
    out->rays_final = totals[MPT_RS_FINAL];
    out->rays_correction = totals[MPT_RS_CORRECTION];
    out->rays_occluded = traced - totals[MPT_RS_UNOCCLUDED];
    out->history_accepted = totals[MPT_RS_ACCEPTED];
    out->samples_from_history = totals[MPT_RS_FROM_NEIGHBOUR];
    out->pixels_reset = totals[MPT_RS_SURFACE] - totals[MPT_RS_ACCEPTED];
    out->lights = ctx->lights.n();
    out->device_ms = (double)ms;
}
static StageResult rt_result(const mpt_ctx* c) {
    return stage_result(c, stage_valid(c, c->rt), c->rt.out.get(), 16, "no mpt_direct_restir_temporal result for this scene and size");
}
static int direct_restir_temporal_impl(mpt_ctx* ctx, const mpt_restir_temporal_params* p, mpt_restir_temporal_info* out) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    RtResolved r;
    int rc = rt_check(ctx, p, r);
    if (rc || (rc = settle_and_guide(ctx)) || (rc = ensure_lights(ctx))) return rc;
    RestirTemporalState& s = ctx->rt;
    const bool have = stage_valid(ctx, s);   // (asked before stage_run, which marks the state as being written)
    float key_h[14];
    memcpy(key_h, s.cam, sizeof key_h);
    std::vector<unsigned long long> slots(MPT_RS_TOTAL_WORDS, 0ull);
    float ms = 0.0f;
    const size_t n = (size_t)ctx->W * ctx->H;
    rc = stage_run(ctx, s, restir_out_bytes(n), slots.data(), MPT_RS_TOTAL_WORDS, out ? &ms : nullptr, [&](const float* key, float4* o) -> int {
        if (!s.initial) {   // (stage_run has made a fresh state of this size)
            int arc = scratch(ctx, restir_res_bytes(n), {&s.initial, &s.res[0], &s.res[1]});
            if (arc || (arc = scratch(ctx, n * 16, {&s.guide[0], &s.guide[1]}))) return arc;
            s.cur = 0;
        }
        return rt_launch(ctx, ctx->W, ctx->H, ctx->gd.ad.get(), ctx->gd.nc.get(), key, have ? key_h : nullptr, p, r, o, s.initial.get(),
                         s.res[s.cur].get(), s.guide[s.cur].get(), s.res[s.cur ^ 1].get(), s.guide[s.cur ^ 1].get());
    });
    if (rc) return rc;
    s.cur ^= 1;   // the frame's reservoirs are the history
    guide_key(ctx->u, s.cam);
    if (out) rt_info(ctx, slots.data(), ms, out);
    return MPT_OK;
}
static int read_restir_temporal_impl(mpt_ctx* ctx, float* rgba, uint32_t* traced, uint32_t* unoccluded) {
    if (!ctx || !rgba) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    const StageResult r = rt_result(ctx);
    int rc = need(ctx, r);
    const size_t n = (size_t)ctx->W * ctx->H;
    if (rc || (rc = copy_out(ctx, rgba, r.p, r.bytes)) || (rc = copy_out(ctx, traced, (const char*)r.p + n * 16, n * 4)) ||
        (rc = copy_out(ctx, unoccluded, (const char*)r.p + n * 20, n * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
// seven of a reservoir's eight words per pixel (RestirTemporalPass: the last one is padding), after the wait
static int rt_words_out(mpt_ctx* ctx, const uint4* res, size_t n, uint32_t* out) {
    std::vector<uint32_t> words(n * 8);
    HIPCHK(hipMemcpyAsync(words.data(), res, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) memcpy(out + 7 * i, &words[8 * i], 28);
    return MPT_OK;
}
static int read_restir_temporal_reservoirs_impl(mpt_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_read_restir_temporal_reservoirs: null argument");
    const int rc = need(ctx, rt_result(ctx));
    if (rc) return rc;
    return rt_words_out(ctx, ctx->rt.res[ctx->rt.cur].get(), (size_t)ctx->W * ctx->H, out);
}
static int restir_temporal_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* ad, const float* nc, const mpt_uniforms* cam, const float* ad_h,
                                      const float* nc_h, const mpt_uniforms* cam_h, const uint32_t* res_h, const mpt_restir_temporal_params* p,
                                      float* rgba_out, uint32_t* traced_out, uint32_t* unocc_out, uint32_t* res_out, mpt_restir_temporal_info* out) {
    if (!ctx || !ad || !nc || !cam || !rgba_out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    if (res_h && (!ad_h || !nc_h || !cam_h)) return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: reservoirs without their guides or camera");
    RtResolved r;
    int rc = rt_check(ctx, p, r);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = ensure_lights(ctx))) return rc;
    const size_t n = (size_t)W * H;
    std::vector<uint32_t> words;
    if (res_h) {   // seven words per pixel -> the two uint4; a light the table does not have would be read out of bounds
        words.assign(n * 8, 0u);
        for (size_t i = 0; i < n; ++i) {
            memcpy(&words[8 * i], res_h + 7 * i, 28);
            if ((words[8 * i + 5] & 1u) && words[8 * i] >= ctx->lights.n())
                return fail(ctx, MPT_ERR_INVALID_ARG, "restir temporal: a reservoir holds a light the table does not have");
        }
    }
    DevMem<float4> d_ad, d_nc, d_adh, d_nch, d_out, d_guide[2];
    DevMem<uint4> d_initial, d_res[2];
    HIPCHK(d_out.alloc(restir_out_bytes(n)));
    if ((rc = scratch(ctx, restir_res_bytes(n), {&d_initial, &d_res[1]})) || (rc = scratch(ctx, n * 16, {&d_guide[1]})) ||
        (rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16)))
        return rc;
    float key[14], key_h[14];
    guide_key(*cam, key);
    if (res_h) {
        if ((rc = scratch(ctx, n * 16, {&d_guide[0]})) || (rc = stage_in(ctx, d_res[0], words.data(), n * 32)) ||
            (rc = stage_in(ctx, d_adh, ad_h, n * 16)) || (rc = stage_in(ctx, d_nch, nc_h, n * 16)))
            return rc;
        hipLaunchKernelGGL(k_tp_pack, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_adh.get(), d_nch.get(), (uint32_t)n, d_guide[0].get());
        HIPCHK(hipGetLastError());
        guide_key(*cam_h, key_h);
    }
    Event e0, e1;
    HIPCHK(e0.create(hipEventCreate));
    HIPCHK(e1.create(hipEventCreate));
    HIPCHK(hipEventRecord(e0.get(), ctx->stream));
    if ((rc = rt_launch(ctx, W, H, d_ad.get(), d_nc.get(), key, res_h ? key_h : nullptr, p, r, d_out.get(), d_initial.get(), d_res[0].get(),
                        d_guide[0].get(), d_res[1].get(), d_guide[1].get())))
        return rc;
    HIPCHK(hipEventRecord(e1.get(), ctx->stream));
    const char* o = (const char*)d_out.get();
    std::vector<unsigned long long> slots(MPT_RS_TOTAL_WORDS, 0ull);
    if ((rc = copy_out(ctx, rgba_out, o, n * 16)) || (rc = copy_out(ctx, traced_out, o + n * 16, n * 4)) ||
        (rc = copy_out(ctx, unocc_out, o + n * 20, n * 4)) || (rc = copy_out(ctx, slots.data(), o + n * 24, MPT_RS_TOTAL_WORDS * 8)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (res_out && (rc = rt_words_out(ctx, d_res[1].get(), n, res_out))) return rc;
    if (out) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, e0.get(), e1.get()));
        rt_info(ctx, slots.data(), ms, out);
    }
    return MPT_OK;
}
extern "C" int mpt_direct_restir_temporal(mpt_ctx* ctx, const mpt_restir_temporal_params* p, mpt_restir_temporal_info* out) {
    return guarded(ctx, [&] { return direct_restir_temporal_impl(ctx, p, out); });
}
extern "C" int mpt_read_restir_temporal(mpt_ctx* ctx, float* rgba, uint32_t* traced, uint32_t* unoccluded) {
    return guarded(ctx, [&] { return read_restir_temporal_impl(ctx, rgba, traced, unoccluded); });
}
extern "C" int mpt_restir_temporal_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, rt_result, p, bytes); }
extern "C" int mpt_read_restir_temporal_reservoirs(mpt_ctx* ctx, uint32_t* out) {
    return guarded(ctx, [&] { return read_restir_temporal_reservoirs_impl(ctx, out); });
}
extern "C" int mpt_restir_temporal_reset(mpt_ctx* ctx) {
    return guarded(ctx, [&] { return reset_state(ctx, &mpt_ctx::rt); });
}
extern "C" int mpt_restir_temporal_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* albedo_depth_cur, const float* normal_class_cur,
                                         const mpt_uniforms* cam_cur, const float* albedo_depth_prev, const float* normal_class_prev,
                                         const mpt_uniforms* cam_prev, const uint32_t* reservoirs_prev, const mpt_restir_temporal_params* p,
                                         float* rgba_out, uint32_t* traced_out, uint32_t* unoccluded_out, uint32_t* reservoirs_out,
                                         mpt_restir_temporal_info* out) {
    return guarded(ctx, [&] {
        return restir_temporal_image_impl(ctx, w, h, albedo_depth_cur, normal_class_cur, cam_cur, albedo_depth_prev, normal_class_prev, cam_prev,
                                          reservoirs_prev, p, rgba_out, traced_out, unoccluded_out, reservoirs_out, out);
    });
}

// ---- SVGF (mpt_svgf.h; the specification is in include/mpt.h) -------------------------------------------------------------------
struct SvResolved {
    TpResolved tp;
    int iterations, feedback;
    float sl, sn, sz;
};
static int sv_resolve(mpt_ctx* ctx, const mpt_svgf_params* p, SvResolved& r) {
    const int rc = tp_resolve(ctx, "svgf", p, r.tp);
    if (rc) return rc;
    if (p->sigma_luminance != p->sigma_luminance || p->sigma_normal != p->sigma_normal || p->sigma_depth != p->sigma_depth)
        return fail(ctx, MPT_ERR_INVALID_ARG, "svgf: a sigma is NaN");
    if (p->iterations > MPT_DENOISE_MAX_ITERATIONS) return fail(ctx, MPT_ERR_INVALID_ARG, "svgf iterations > 8");
    r.iterations = p->iterations < 0 ? MPT_SVGF_DEFAULT_ITERATIONS : p->iterations;
    r.sl = p->sigma_luminance > 0.0f ? p->sigma_luminance : MPT_SVGF_DEFAULT_SIGMA_LUMINANCE;
    r.sn = p->sigma_normal > 0.0f ? p->sigma_normal : MPT_SVGF_DEFAULT_SIGMA_NORMAL;
    r.sz = p->sigma_depth > 0.0f ? p->sigma_depth : MPT_SVGF_DEFAULT_SIGMA_DEPTH;
    r.feedback = p->feedback < 0 ? MPT_SVGF_DEFAULT_FEEDBACK : p->feedback != 0;
    return MPT_OK;
}
// Steps A, B, C on ctx->stream, then one wait for the counts.  Step A goes from s's current side into the other, which is what B and C
// read; dn_guide: the denoiser's packed guide of the current frame; s.xv[0] = (X, V_0), s.xv[1], s.xv[2] the ping-pong; s.out: the frame.
static int sv_run(mpt_ctx* ctx, const SvgfState& s, Source src, const float4* ad, const float4* nc, const float4* dn_guide, const float key[14],
                  const float* key_h, const SvResolved& r, mpt_svgf_info* out) {
    SvFrame T = history_frame<SvFrame>(s, src, ad, nc);
    T.mom_in = s.mom[s.cur].get();
    T.mom_out = s.mom[s.cur ^ 1].get();
    const int mode = tp_frame_constants(T, key, key_h, r.tp);
    const uint32_t W = T.W, H = T.H, n = W * H;
    HIPCHK(hipMemsetAsync(T.n_reset, 0, 8, ctx->stream));
    const dim3 grid = tile_grid(W, H);
    {
        void* args[] = {&T};
        HIPCHK(hipLaunchKernel(sv_reproject_kernel(mode), grid, dim3(256), args, 0, ctx->stream));
    }
    SvVariance S = {T.hist_out, T.mom_out, dn_guide, s.xv[0].get(), W, H, r.sn, r.sz};
    hipLaunchKernelGGL(k_sv_variance, grid, dim3(256), 0, ctx->stream, S);
    HIPCHK(hipGetLastError());
    if (r.iterations == 0) {
        hipLaunchKernelGGL(k_sv_modulate, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)T.hist_out, T.ad, dn_guide, n, s.out.get());
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < r.iterations; ++i) {
        const bool last = i == r.iterations - 1;
        SvLevel L;
        L.xin = s.xv[i == 0 ? 0 : 1 + ((i - 1) & 1)].get();
        L.guide = dn_guide;
        L.ad = T.ad;
        L.hist = T.hist_out;
        L.xout = last ? s.out.get() : s.xv[1 + (i & 1)].get();
        L.feedback = i == 0 && r.feedback ? T.hist_out : nullptr;
        L.W = W;
        L.H = H;
        L.step = 1u << i;
        L.sigma_n = r.sn;
        L.sigma_z = r.sz;
        L.sigma_l = r.sl;
        const size_t lds = atrous_lds_bytes(L.step);
        const void* k = lds ? sv_level_kernel<true>(last) : sv_level_kernel<false>(last);
        void* args[] = {&L};
        HIPCHK(hipLaunchKernel(k, grid, dim3(256), args, lds, ctx->stream));
    }
    return history_counts(ctx, s, out);
}
// what SvgfState adds to its History, W x H each
static int sv_own_buffers(mpt_ctx* ctx, SvgfState& s, size_t n) {
    const int rc = scratch(ctx, n * 16, {&s.xv[0], &s.xv[1], &s.xv[2], &s.out});
    if (rc) return rc;
    HIPCHK(s.mom[1].alloc(n * 8));
    return MPT_OK;
}
static int svgf_accumulate_impl(mpt_ctx* ctx, const mpt_svgf_params* p, mpt_svgf_info* out) {
    if (!ctx || !p) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    SvResolved r;
    int rc = check_source(ctx, "svgf accumulation", p->source, p->samples);
    if (rc || (rc = sv_resolve(ctx, p, r)) || (rc = settle_and_guide(ctx))) return rc;
    SvgfState& sv = ctx->sv;
    if (!history_fits(ctx, sv)) {   // its own buffers first: the history's, made by history_accumulate, complete the state
        sv.W = sv.H = 0;
        sv.epoch = 0;
        if ((rc = sv_own_buffers(ctx, sv, (size_t)ctx->W * ctx->H))) return rc;
        HIPCHK(sv.mom[0].alloc((size_t)ctx->W * ctx->H * 8));
    }
    const Source src = pick_source(ctx, p->source, p->samples);
    return history_accumulate(ctx, sv, [&](const float* key, const float* key_h) {
        return sv_run(ctx, sv, src, ctx->gd.ad.get(), ctx->gd.nc.get(), ctx->gd.packed.get(), key, key_h, r, out);
    });
}
// The last step of a read-back of `s`: the wait for the copies enqueued before, with (M1, M2) of `side` and (X, V_0) of the device
// as the (M1, M2, V_0, 0) the readers return when `out` is asked for
static int sv_read_moments(mpt_ctx* ctx, const SvgfState& s, int side, float* out) {
    const size_t n = (size_t)s.W * s.H;
    std::vector<float> mom(out ? n * 2 : 0), x0(out ? n * 4 : 0);
    int rc;
    if (out && ((rc = copy_out(ctx, mom.data(), s.mom[side].get(), n * 8)) || (rc = copy_out(ctx, x0.data(), s.xv[0].get(), n * 16)))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; out && i < n; ++i) {
        out[4 * i + 0] = mom[2 * i];
        out[4 * i + 1] = mom[2 * i + 1];
        out[4 * i + 2] = x0[4 * i + 3];
        out[4 * i + 3] = 0.0f;
    }
    return MPT_OK;
}
static int svgf_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* color, const float* ad, const float* nc, const mpt_uniforms* cam,
                           const float* hist_h, const float* mom_h, const float* ad_h, const float* nc_h, const mpt_uniforms* cam_h,
                           const mpt_svgf_params* p, float* hist_out, float* mv_out, float* filtered_out, mpt_svgf_info* out) {
    if (!ctx || !color || !ad || !nc || !cam || !p || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    if (hist_h && (!mom_h || !ad_h || !nc_h || !cam_h)) return fail(ctx, MPT_ERR_INVALID_ARG, "a history without its moments, guides or camera");
    SvResolved r;
    int rc = sv_resolve(ctx, p, r);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)W * H;
    SvgfState s;   // side 0: the caller's history (none: null buffers), side 1: the result
    s.W = W;
    s.H = H;
    DevMem<float4> d_c, d_ad, d_nc, d_g, d_adh, d_nch;
    if ((rc = scratch(ctx, n * 16, {&d_g, &s.hist[1], &s.guide[1]})) || (rc = sv_own_buffers(ctx, s, n))) return rc;
    HIPCHK(s.n_reset.alloc(8));
    if ((rc = stage_in(ctx, d_c, color, n * 16)) || (rc = stage_in(ctx, d_ad, ad, n * 16)) || (rc = stage_in(ctx, d_nc, nc, n * 16))) return rc;
    const dim3 lin((uint32_t)((n + 255) / 256));
    hipLaunchKernelGGL(k_dn_pack, lin, dim3(256), 0, ctx->stream, d_ad.get(), d_nc.get(), (uint32_t)n, d_g.get());
    HIPCHK(hipGetLastError());
    float key[14], key_h[14];
    guide_key(*cam, key);
    if (hist_h) {
        if ((rc = scratch(ctx, n * 16, {&s.guide[0]})) || (rc = stage_in(ctx, s.hist[0], hist_h, n * 16)) || (rc = stage_in(ctx, s.mom[0], mom_h, n * 8)) ||
            (rc = stage_in(ctx, d_adh, ad_h, n * 16)) || (rc = stage_in(ctx, d_nch, nc_h, n * 16)))
            return rc;
        hipLaunchKernelGGL(k_sv_pack, lin, dim3(256), 0, ctx->stream, d_adh.get(), d_nch.get(), (uint32_t)n, s.guide[0].get());
        HIPCHK(hipGetLastError());
        guide_key(*cam_h, key_h);
    }
    if ((rc = sv_run(ctx, s, Source{d_c.get(), 1.0f}, d_ad.get(), d_nc.get(), d_g.get(), key, hist_h ? key_h : nullptr, r, out)) ||
        (rc = copy_out(ctx, hist_out, s.hist[1].get(), n * 16)) || (rc = copy_out(ctx, filtered_out, s.out.get(), n * 16)))
        return rc;
    return sv_read_moments(ctx, s, 1, mv_out);
}
static int read_svgf_state_impl(mpt_ctx* ctx, float* history, float* moments_variance) {
    if (!ctx || !history || !moments_variance) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    int rc = need(ctx, sv_result(ctx));
    if (rc) return rc;
    const SvgfState& sv = ctx->sv;
    if ((rc = copy_out(ctx, history, sv.hist[sv.cur].get(), (size_t)sv.W * sv.H * 16))) return rc;
    return sv_read_moments(ctx, sv, sv.cur, moments_variance);
}
extern "C" int mpt_svgf_accumulate(mpt_ctx* ctx, const mpt_svgf_params* p, mpt_svgf_info* out) {
    return guarded(ctx, [&] { return svgf_accumulate_impl(ctx, p, out); });
}
extern "C" int mpt_read_svgf(mpt_ctx* ctx, float* rgba) {
    return guarded(ctx, [&] { return read_result(ctx, sv_result, rgba); });
}
extern "C" int mpt_svgf_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, sv_result, p, bytes); }
extern "C" int mpt_read_svgf_state(mpt_ctx* ctx, float* history, float* moments_variance) {
    return guarded(ctx, [&] { return read_svgf_state_impl(ctx, history, moments_variance); });
}
extern "C" int mpt_svgf_reset(mpt_ctx* ctx) {
    return guarded(ctx, [&] { return reset_state(ctx, &mpt_ctx::sv); });
}
extern "C" int mpt_svgf_image(mpt_ctx* ctx, uint32_t w, uint32_t h, const float* color, const float* albedo_depth_cur, const float* normal_class_cur,
                              const mpt_uniforms* cam_cur, const float* history_prev, const float* moments_prev, const float* albedo_depth_prev,
                              const float* normal_class_prev, const mpt_uniforms* cam_prev, const mpt_svgf_params* p, float* history_out,
                              float* moments_variance_out, float* filtered_out, mpt_svgf_info* out) {
    return guarded(ctx, [&] {
        return svgf_image_impl(ctx, w, h, color, albedo_depth_cur, normal_class_cur, cam_cur, history_prev, moments_prev, albedo_depth_prev,
                               normal_class_prev, cam_prev, p, history_out, moments_variance_out, filtered_out, out);
    });
}

// ---- display (mpt_display.h; the specification is in include/mpt.h) --------------------------------------------------------------
static_assert(sizeof(mpt_display_info) == 32 && offsetof(DpState, kept) == 32, "DpState begins with mpt_display_info");
struct DpResolved {
    DpExposure E;
    float ww;   // REINHARD's white * white
};
static int dp_resolve(mpt_ctx* ctx, const mpt_display_params* p, DpResolved& r) {
    if (!p) return fail(ctx, MPT_ERR_INVALID_ARG, "null display params");
    if (p->tone < MPT_TONE_CLAMP || p->tone > MPT_TONE_ACES) return fail(ctx, MPT_ERR_INVALID_ARG, "bad tone curve");
    if (p->transfer < MPT_TRANSFER_SRGB || p->transfer > MPT_TRANSFER_LINEAR) return fail(ctx, MPT_ERR_INVALID_ARG, "bad transfer function");
    if (p->percentile > 100u) return fail(ctx, MPT_ERR_INVALID_ARG, "display percentile above 100");
    if (p->exposure != p->exposure || p->white != p->white || p->key != p->key || p->adaptation != p->adaptation)
        return fail(ctx, MPT_ERR_INVALID_ARG, "a display parameter is NaN");
    const float white = p->white > 0.0f ? p->white : 4.0f;
    r.ww = white * white;
    r.E.exposure = p->exposure > 0.0f ? p->exposure : 1.0f;
    r.E.key = p->key > 0.0f ? p->key : 0.18f;
    r.E.adaptation = p->adaptation > 0.0f && p->adaptation < 1.0f ? p->adaptation : 0.0f;
    r.E.percentile = p->percentile ? p->percentile : 50u;
    r.E.auto_exposure = p->auto_exposure != 0;
    return MPT_OK;
}
// W x H pixels of `color` as they are (MPT_DP_SRC_RAW)
static DpSource dp_source(const float4* color, uint32_t W, uint32_t H) {
    DpSource S = {};
    S.color = color;
    S.n = W * H;
    S.W = W;
    S.tiles_x = (W + 7) / 8;
    S.samples = 1.0f;
    return S;
}
// histogram (auto-exposure only) -> exposure -> present, back to back on the context's stream; the host reads the 32-byte result once
static int dp_run(mpt_ctx* ctx, DpSource S, int src_kind, const mpt_display_params* p, const DpResolved& r, uint32_t* hist, DpState* st,
                  const float* tables, uint32_t* out_words, mpt_display_info* info) {
    if (r.E.auto_exposure) {
        HIPCHK(hipMemsetAsync(hist, 0, MPT_DP_BINS * 4, ctx->stream));
        const uint32_t blocks = std::min<uint32_t>((S.n + 255u) / 256u, (uint32_t)std::max(1, ctx->prop.multiProcessorCount) * 8u);
        void* args[] = {&S, &hist};
        HIPCHK(hipLaunchKernel(dp_histogram_kernel(src_kind, ctx->dp_hist_agg), dim3(blocks), dim3(256), args, 0, ctx->stream));
    }
    DpExposure E = r.E;
    hipLaunchKernelGGL(k_dp_exposure, dim3(1), dim3(64), 0, ctx->stream, (const uint32_t*)hist, E, st);
    HIPCHK(hipGetLastError());
    DpTone P = {tables + (size_t)p->transfer * 255, r.ww};
    const uint32_t per_block = 256u * (uint32_t)ctx->dp_px;
    void* args[] = {&S, &P, &st, &out_words};
    HIPCHK(hipLaunchKernel(dp_present_kernel(src_kind, p->tone, ctx->dp_px), dim3((S.n + per_block - 1u) / per_block), dim3(256), args, 0, ctx->stream));
    mpt_display_info got = {};
    HIPCHK(hipMemcpyAsync(&got, st, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (info) *info = got;
    return MPT_OK;
}
// the buffers of a display pass over n pixels: `out`, `hist`, `st` and the tables, uploaded (hist and st are not cleared here)
static int dp_make_buffers(mpt_ctx* ctx, DisplayState& d, uint32_t n) {
    HIPCHK(d.out.alloc(((size_t)n * 4 + 15) & ~(size_t)15));
    HIPCHK(d.hist.alloc(MPT_DP_BINS * 4));
    HIPCHK(d.st.alloc(sizeof(DpState)));
    HIPCHK(d.tables.alloc(sizeof MPT_DISPLAY_TABLE));
    HIPCHK(hipMemcpy(d.tables.get(), MPT_DISPLAY_TABLE, sizeof MPT_DISPLAY_TABLE, hipMemcpyHostToDevice));
    return MPT_OK;
}
static int display_impl(mpt_ctx* ctx, const mpt_display_params* p, mpt_display_info* out) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    DpResolved r;
    int rc = dp_resolve(ctx, p, r);
    if (rc || (rc = check_source(ctx, "display", p->source, p->samples, MPT_DISPLAY_ADAPTIVE))) return rc;
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    // the stage whose result is shown (none: the sum or the frame)
    const int32_t of = p->source;
    const ResultOf shown = of == MPT_DISPLAY_DENOISED ? dn_result : of == MPT_DISPLAY_TEMPORAL ? tp_result : of == MPT_DISPLAY_SVGF ? sv_result : nullptr;
    if (shown && (rc = need(ctx, shown(ctx)))) return rc;
    if (p->source == MPT_DISPLAY_ADAPTIVE && !ctx->ad.tile_count) return fail(ctx, MPT_ERR_NOT_READY, "no adaptive render at this size");
    if ((rc = wait_impl(ctx))) return rc;   // (the display stage reads no guides)
    HIPCHK(hipSetDevice(ctx->device));
    if (!stage_valid(ctx, ctx->dp)) {   // the first call, or the first after a scene call: the buffers are made whole before they replace the old ones
        HIPCHK(hipStreamSynchronize(ctx->stream));
        DisplayState d;
        if ((rc = dp_make_buffers(ctx, d, ctx->W * ctx->H))) return rc;
        HIPCHK(hipMemset(d.hist.get(), 0, MPT_DP_BINS * 4));
        HIPCHK(hipMemset(d.st.get(), 0, sizeof(DpState)));
        d.W = ctx->W;
        d.H = ctx->H;
        d.epoch = ctx->guide_epoch;
        ctx->dp = std::move(d);
    }
    DisplayState& dp = ctx->dp;
    DpSource S = dp_source(ctx->d_sum, ctx->W, ctx->H);
    int kind = MPT_DP_SRC_RAW;
    if (shown) {
        S.color = (const float4*)shown(ctx).p;
    } else if (p->source == MPT_DISPLAY_ADAPTIVE) {
        S.tile_count = ctx->ad.tile_count.get();
        kind = MPT_DP_SRC_TILE;
    } else {
        const Source src = pick_source(ctx, p->source, p->samples);
        S.color = src.color;
        S.samples = src.samples;
        if (p->source == MPT_DISPLAY_SUM) kind = MPT_DP_SRC_DIV;
    }
    dp.shown = false;
    if ((rc = dp_run(ctx, S, kind, p, r, dp.hist.get(), dp.st.get(), dp.tables.get(), dp.out.get(), out))) return rc;
    dp.shown = true;
    return MPT_OK;
}
static int display_image_impl(mpt_ctx* ctx, uint32_t W, uint32_t H, const float* color, const mpt_display_params* p, const float* prev_auto_scale,
                              uint8_t* rgba8_out, uint32_t* histogram_out, mpt_display_info* out) {
    if (!ctx || !color || !rgba8_out || bad_image_size(W, H)) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    DpResolved r;
    int rc = dp_resolve(ctx, p, r);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = W * H;
    DevMem<float4> d_c;
    DisplayState d;
    if ((rc = dp_make_buffers(ctx, d, n))) return rc;
    DpState st0 = {};
    if (prev_auto_scale) {
        st0.kept = *prev_auto_scale;
        st0.have_kept = 1;
    }
    if ((rc = stage_in(ctx, d_c, color, (size_t)n * 16))) return rc;
    HIPCHK(hipMemcpyAsync(d.st.get(), &st0, sizeof st0, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d.hist.get(), 0, MPT_DP_BINS * 4, ctx->stream));
    if ((rc = dp_run(ctx, dp_source(d_c.get(), W, H), MPT_DP_SRC_RAW, p, r, d.hist.get(), d.st.get(), d.tables.get(), d.out.get(), out)) ||
        (rc = copy_out(ctx, rgba8_out, d.out.get(), (size_t)n * 4)) || (rc = copy_out(ctx, histogram_out, d.hist.get(), MPT_DP_BINS * 4)))
        return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
// (the histogram of the frame mpt_read_display returns: ready when that one is)
static int read_display_histogram_impl(mpt_ctx* ctx, uint32_t out[256]) {
    if (!ctx || !out) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
    int rc = need(ctx, dp_result(ctx));
    if (rc || (rc = copy_out(ctx, out, ctx->dp.hist.get(), MPT_DP_BINS * 4))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
extern "C" int mpt_display(mpt_ctx* ctx, const mpt_display_params* p, mpt_display_info* out) {
    return guarded(ctx, [&] { return display_impl(ctx, p, out); });
}
extern "C" int mpt_read_display(mpt_ctx* ctx, uint8_t* rgba8) {
    return guarded(ctx, [&] { return read_result(ctx, dp_result, rgba8); });
}
extern "C" int mpt_display_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) { return result_buffer(ctx, dp_result, p, bytes); }
extern "C" int mpt_read_display_histogram(mpt_ctx* ctx, uint32_t out[256]) {
    return guarded(ctx, [&] { return read_display_histogram_impl(ctx, out); });
}
extern "C" int mpt_display_reset(mpt_ctx* ctx) {
    return guarded(ctx, [&]() -> int {
        if (!ctx) return MPT_ERR_INVALID_ARG;
        if (!stage_valid(ctx, ctx->dp)) return MPT_OK;   // (nothing kept)
        HIPCHK(hipMemsetAsync((char*)ctx->dp.st.get() + offsetof(DpState, kept), 0, sizeof(DpState) - offsetof(DpState, kept), ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return MPT_OK;
    });
}
extern "C" int mpt_display_table(int transfer, float out[255]) {
    if (!out || transfer < MPT_TRANSFER_SRGB || transfer > MPT_TRANSFER_LINEAR) return MPT_ERR_INVALID_ARG;
    memcpy(out, MPT_DISPLAY_TABLE[transfer], sizeof MPT_DISPLAY_TABLE[transfer]);
    return MPT_OK;
}
extern "C" int mpt_display_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* color, const mpt_display_params* p,
                                 const float* prev_auto_scale, uint8_t* rgba8_out, uint32_t* histogram_out, mpt_display_info* out) {
    return guarded(ctx, [&] { return display_image_impl(ctx, width, height, color, p, prev_auto_scale, rgba8_out, histogram_out, out); });
}
