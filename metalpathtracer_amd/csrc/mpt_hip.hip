// mpt_hip.hip — host side of the C ABI (include/mpt.h) of the MI355X path-tracing hot path: context and resource
// management, upload of a scene (its conversion into the device layout — threaded breadth-first BVH, leaf-ordered
// primitives, de-duplicated materials — is pure host code in mpt_scene_layout.h), pass scheduling and kernel launches.
// The kernels themselves are in mpt_kernels.h, their building blocks in mpt_device.h; the host side of the
// post-processing stages is mpt_post.h, the ray queries mpt_query.h, the RCCL reduce mpt_comm.h, all included below.
//
// One mpt_render = one pass per <= 2^30 paths: k_begin_pass, ONE k_wavelocal launch (default pipeline; the global
// wavefront launches k_step + k_advance per bounce generation instead), k_resolve_sum, one host synchronisation.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).  gfx950 only.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <map>
#include <memory>
#include <exception>
#include <string>
#include <type_traits>
#include <vector>

#include "mpt.h"
#include "mpt_accel.h"
#include "mpt_scene_layout.h"
#include "mpt_env.h"
#include "mpt_device.h"
#include "mpt_own.h"

#include "mpt_kernels.h"
#include "mpt_lean_cdiv.h"
#include "mpt_lbvh.h"
#include "mpt_devbuild.h"
#include "mpt_ordered.h"
#include "mpt_denoise.h"
#include "mpt_temporal.h"
#include "mpt_svgf.h"
#include "mpt_adaptive.h"
#include "mpt_display.h"
#include "mpt_anyhit.h"
#include "mpt_ao.h"
#include "mpt_direct.h"
#include "mpt_nee.h"
#include "mpt_nee_adaptive.h"
#include "mpt_ris.h"
#include "mpt_restir.h"
#include "mpt_restir_temporal.h"

// =====================================================================================================
// host side of the C ABI
// =====================================================================================================
// Everything one in-flight render owns.  A context has two lanes so that consecutive renders overlap: the next
// render's trace kernel fills the CUs that the previous one's tail (and its resolve) leave idle (measured with two
// contexts: +11 % at 1080p x 256 spp, +15 % for a 1/8 tile shard).  Resolves are chained in submission order, so the
// HDR sum is bit-identical to the serial schedule.
// Box-test trips granted per step of ring 0..LEVELS-2 (the last ring runs to completion).  Rounds 1-3 (five rings), scene.xml at
// 1080p x 256 spp: 8/20/50/125 -> 29.3 ms, 8/24/72/inf -> 30.4, 8/16/32/64 -> 30.2, 8/16/32/inf -> 31.8, 8/12/24/48 -> 31.3.
// Round 4 (two rings, mpt_kernels.h): only ring 0's budget is left — 6 / 8 / 12 / 16 / 24: 17.01 / 16.88 / 17.11 / 17.49 / 18.26 ms.
static WaveBudgets default_budgets() {
    WaveBudgets w;
    const uint32_t ladder[] = {8, 20, 50, 125, 300, 700, 1600};
    for (uint32_t k = 0; k < MPT_WL_LEVELS; ++k) {
        w.b[k] = k + 1 < MPT_WL_LEVELS && k < 7 ? ladder[k] : MPT_WL_NO_BUDGET;
        // a step of ring 1.. also ends once fewer than 24 of its 64 lanes are still traversing (the stragglers are
        // parked and regrouped): 29.9 -> 28.5 ms; 16 or 32 lanes are about as good, 8 is not, ring 0 is better without
        // (round 3, five rings, no carry rule.  The lean kernels, whose values are their own constants — mpt_lds_cfg.h — end a ring-0 step
        //  below 8 lanes: swept again on them, profiles/r28_ring0_rule.txt.  The generic kernels were not swept and keep 0.)
        w.min_active[k] = k == 0 ? 0 : 24;
    }
    return w;
}

// Node-loop trips a step of tree-walk ring M_k may make before its unfinished rays are parked in M_k+1 (MPT_OT_BUDGETS),
// and the number of lanes that must still be walking for a step to go on (MPT_OT_MIN_ACTIVE).
static OtBudgets default_ot_budgets() {
    OtBudgets b;
    // Round 5: a walk step of ring M0 (and a walk made in place by a top-test step) ends when fewer than 24 of its lanes still walk,
    // or after 32 trips of the node loop; a step of the last ring when fewer than 32 do.  Until round 4 the first rule did not exist
    // (16 trips and out, whoever was still walking): a trip budget cuts a step short while most of its lanes are still busy and sends
    // them through a ring for nothing, a utilisation rule ends it when it has become wasteful.  Same-box sweep (gpurun_out/r05/s10, s11:
    // budgets 16 .. 1000 x minimum lanes 0 .. 40 x 24 / 32), (16; 0, 24) -> (32; 24, 32): 8 / 20 bunnies 43.6 -> 42.8 / 55.1 -> 53.9 ms,
    // the 1 M-triangle shard of configs[4] 117.2 -> 113.2; no trip budget at all (1000; 24, 32) is the same within 0.1 %; a budget
    // WITHOUT the rule is far worse than before (32; 0, 24: 64.9 ms on bunny x20).  Rounds 2-3: 4,10 -> 29.3 / 123 ms, 16,48 -> 27.4 / 111.
    const uint32_t ladder[] = {32, 96, 240, 600, 1500};
    for (uint32_t k = 0; k < MPT_OT_MLEVELS; ++k) {
        b.trips[k] = k + 1 < MPT_OT_MLEVELS && k < 5 ? ladder[k] : 0x7FFFFFFFu;
        b.min_active[k] = k + 1 < MPT_OT_MLEVELS ? 24 : 32;
    }
    b.inplace_min = 48;   // bunny x20 256 spp: never 74.9 ms, 56 72.6, 48 72.8, 40 73.1, 32 73.7, 24 74.4; scene.xml 25.96 / 25.6 / 25.6 / 25.7 / 25.9 / 26.6
    return b;
}

using mpt_own::DevMem;
using mpt_own::Event;
using mpt_own::HostMem;
using mpt_own::Stream;

// What a lane's class table was built from: the scene (guide_epoch: bumped by every scene call and every resize, and the node array), the camera as
// the kernels read it, the image and its tile grid, and the number of words (tiles + the pass's rank count)
struct LeanTileKey {
    uint64_t epoch;
    const void* nodes;
    LeanTileView view;
    uint32_t width, height, n_words;
};
struct Lane {
    Stream stream;
    DevMem<PassDesc> d_desc;
    DevMem<uint32_t> d_ctr;
    HostMem<uint32_t> h_done;    // pinned, device-visible
    HostMem<PassDesc> h_desc;    // pinned copy of the pass descriptor (statistics read-back without a sync copy)
    Event ev0, ev1, ev_resolved, ev_traced;
    std::vector<Event> ev_pool;  // kernel-timing events (next_event)
    size_t ev_used = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_timed;  // kernel-event pairs to read at collection
    // workspace, allocated on first use and only ever grown
    DevMem<float4> d_slots;      // per-path result slots of a pass
    DevMem<float4> q_od[2], q_dt[2], q_tl[2];   // the wavefront pipeline's two global ray queues (QueueDev), shard_cap items per shard
    DevMem<uint2> q_ia[2];
    uint32_t shard_cap = 0;
    DevMem<float4> ring_mem, ot_ring_mem;
    WaveRings ring = {};         // wave-local pipeline: MPT_WL_LEVELS rings of MPT_WL_RING records per wave (in ring_mem)
    size_t ring_waves = 0;
    OtRings ot_ring = {};        // ... and its rings (MPT_OT_RINGS per wave, in ot_ring_mem)
    size_t ot_ring_waves = 0;
    uint32_t announced_id = 0;   // launch id of the lane's last trace kernel that announces its residency (0: none)
    // the lean ALL_LDS kernels' per-tile class words (mpt_lean_tiles.h), built on this lane's stream when `tile_key` changes: each lane has its own,
    // so a launch in flight on the other lane never sees its table change
    DevMem<uint32_t> d_tile_classes;
    LeanTileKey tile_key = {};
    bool in_flight = false;      // enqueued by mpt_render_async, not yet collected
    bool timed = false;
};

// mpt_render_async's submit thread (one per context, started by the first asynchronous render).  What a submission may have to wait
// for — the render lane it is going to use (two renders are in flight), the residency announcement of the trace kernel before it (the
// gate of run_pass, up to 200 ms when a foreign kernel holds the chip) — it waits for HERE, not on the caller's thread: mpt_render_async
// checks its arguments, queues the parameters and returns (round 4's version spun on the caller's thread: VERDICT r4 item 7).  The reference's
// per-frame submit is unfenced in the same way (R/Renderer/Renderer.cpp:253-266,307: commit() and return).  Every other entry point of the
// context first drains the queue (drain_submit), so the context stays single-threaded from the caller's point of view; the first
// failure of a queued render is reported by the call that drains it (mpt_wait, or whatever comes next).
struct Submitter {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv_work, cv_idle;
    std::deque<mpt_render_params> q;
    bool busy = false, stop = false;
    int rc = 0;            // first failure of a queued render since the last drain
    std::string err;
};
#define MPT_ASYNC_QUEUE_MAX 64   // queued renders beyond this make mpt_render_async wait for room (back pressure, not an error)

// One scene on the device, made whole by mpt_upload_scene or mpt_build_and_upload and put in place of the one before by install_scene.
// The arrays of a built scene are views into ONE device allocation (scene_block: nine hipMallocs on the build's critical path were
// ~0.3 ms of a 4.3 ms build); those of an uploaded scene own their allocations one by one (scene_bufs).
struct SceneState {
    DevMem<> scene_block;
    std::vector<DevMem<>> scene_bufs;
    float4* d_nodes = nullptr;
    float4* d_prims = nullptr;
    float4* d_mats = nullptr;
    uint32_t n_nodes = 0, n_prims = 0, n_mats = 0, n_lds_nodes = 0, n_lds_prims = 0;
    // the product's own tree (mpt_accel.h) for the closest-first pipeline; it shares d_prims with the threaded tree
    float4* d_acc_nodes = nullptr;
    float4* d_refleaf = nullptr;
    float4* d_refbox = nullptr;       // the box of its reference leaf PER PRIMITIVE, 2 float4 each: the final check of the closest-first walk needs no look-up through the primitive
    float4* d_always = nullptr;
    uint32_t n_acc_nodes = 0, n_always = 0, n_ref_leaves = 0, acc_depth = 0;
    // mpt_build_and_upload keeps its tree in the reference's buffer format on the device too (mpt_download_bvh)
    float4* d_ref_bvh = nullptr;
    int* d_ref_idx = nullptr;
    uint32_t n_ref_nodes = 0;
    uint32_t built_leaf_max = 0;     // leaf limit of that tree (mpt_build_info)
    float tri_extent = 0.0f, acc_eps_abs = 0.0f;
    bool acc_ok = false;             // the closest-first pipeline may be used for this scene
    std::string acc_why;
    hipError_t own(float4** p, size_t bytes) {   // an array of an uploaded scene
        scene_bufs.emplace_back();
        const hipError_t e = scene_bufs.back().alloc(bytes);
        *p = (float4*)scene_bufs.back().get();
        return e;
    }
};

// mpt_render_adaptive's tile buffers, for `tiles` tiles (allocated by its first call after a resize; mpt_resize drops them)
struct AdaptiveTiles {
    DevMem<uint32_t> tile_count;   // samples per tile, row-major
    DevMem<uint32_t> alist[2];     // ping-pong active tile lists (x | y << 16)
    DevMem<uint8_t> aflag;         // per list entry: the tile stays active
    DevMem<uint32_t> nsel;         // entries DeviceSelect::Flagged kept
    DevMem<> sel_tmp;              // its temporary storage ...
    size_t sel_tmp_bytes = 0;      // ... of the size it asked for
    uint32_t tiles = 0;
};

// The state of the post-processing stages (mpt_post.h drives them).  Each is valid while its `epoch` is the context's guide_epoch
// (every scene call and mpt_resize bump that one) and its W x H the context's size; mpt_resize lets go of all of them.
//
// The first-hit guide buffers of the current frame (k_dn_guide, mpt_denoise.h), traced again when stale; every stage reads them.
// Allocated, with DenoiseState, by the first stage call after a resize.
struct GuideState {
    DevMem<float4> ad;             // (albedo rgb, t)
    DevMem<float4> nc;             // (normal rgb, class)
    DevMem<int> prim;              // caller's primitive id, -1 = miss
    DevMem<float4> packed;         // packed per-tap guide (normal, t or MPT_DN_SKIP)
    uint32_t W = 0, H = 0;         // size of those buffers and of DenoiseState's
    uint64_t built = 0;            // the guide_epoch the guides were traced in (0 = never)
    float cam[14] = {};            // guide_key of the uniforms they were traced with
};
// The denoiser's own buffers (mpt_denoise.h)
struct DenoiseState {
    DevMem<float4> x[2];           // ping-pong (x rgb, luminance) of the levels
    DevMem<float4> out;
    bool valid = false;            // `out` holds the result of an mpt_denoise at the current size
};

// A reprojected history: the accumulated frame, the guide of the frame it belongs to and that frame's camera, ping-pong.  Temporal
// accumulation (mpt_temporal.h) keeps exactly this.  Allocated by the first accumulate call; mpt_temporal_reset / mpt_svgf_reset let go of it.
struct History {
    DevMem<float4> hist[2];        // (accumulated rgb, history length n)
    DevMem<float4> guide[2];       // (normal facing the ray, t; SVGF: t / -t by class; +inf for a miss)
    DevMem<unsigned long long> n_reset;
    uint32_t W = 0, H = 0;         // size of those buffers
    int cur = 0;                   // which of the two holds the history
    uint64_t epoch = 0;            // the guide_epoch the history was written in (0 = no history)
    float cam[14] = {};            // guide_key of the history's frame
};
using TemporalState = History;

// SVGF (mpt_svgf.h): the demodulated illumination history with its luminance moments, independent of TemporalState.  The a-trous
// buffers are this owner's too (not DenoiseState's): an mpt_denoise result survives an mpt_svgf_accumulate and the other way round.
struct SvgfState : History {
    DevMem<float2> mom[2];         // (M1, M2) of the luminance
    DevMem<float4> xv[3];          // (x, V): [0] = (X, V_0), kept for mpt_read_svgf_state; [1], [2] the ping-pong of the levels
    DevMem<float4> out;            // the filtered frame
};

// The display stage (mpt_display.h): the RGBA8 frame, the luminance histogram of the last call with auto_exposure, the result block
// (DpState: the mpt_display_info of the last call and the auto scale kept for the next one) and the three threshold tables.
// Allocated by the first mpt_display.
struct DisplayState {
    DevMem<uint32_t> out;          // W * H words: r | g << 8 | b << 16 | 255 << 24
    DevMem<uint32_t> hist;         // MPT_DP_BINS counts
    DevMem<DpState> st;
    DevMem<float> tables;          // MPT_DISPLAY_TABLE
    uint32_t W = 0, H = 0;
    uint64_t epoch = 0;            // the guide_epoch the buffers were made in (0 = none)
    bool shown = false;            // `out` holds a frame
};

// Ambient occlusion (mpt_ao.h): the result of the last mpt_ambient_occlusion and the two totals of its info.  Allocated by the first
// pass; the scene calls let go of it too.
struct AoState {
    DevMem<float> out;             // AoPass::out: W * H floats of ao, W * H counts, the two totals
    uint32_t W = 0, H = 0;
    uint64_t epoch = 0;            // the guide_epoch the result was written in (0 = none)
};

// The light table (mpt_direct.h): every primitive whose material has emissionPower > 0 and a usable weight, in ascending caller id.
// Built by the first call that needs it after a scene call (ensure_lights, mpt_post.h) from the arrays already on the device; the
// scene calls only let go of it.
struct LightState {
    DevMem<float4> rec;            // MPT_LIGHT_F4 float4 per light
    DevMem<float> cdf;
    DevMem<int32_t> d_ids;         // the lights' caller ids on the device (k_nee looks an emitter up in them)
    std::vector<int32_t> ids;      // host copies for mpt_read_lights
    std::vector<float> h_rec, h_cdf;
    uint64_t seen = 0, n_tri = 0, n_sph = 0;   // emissive primitives of the scene; lights of either type
    bool built = false;
    uint32_t n() const { return (uint32_t)ids.size(); }
};
// Direct lighting (mpt_direct.h): the result of the last mpt_direct_lighting.  Allocated by the first pass; mpt_resize and the scene
// calls let go of it.
struct DirectState {
    DevMem<float4> out;            // DirectPass::out: W * H rgba, W * H traced, W * H unoccluded, the three totals
    uint32_t W = 0, H = 0;
    uint64_t epoch = 0;            // the guide_epoch the result was written in (0 = none)
};

// Spatial reservoir reuse (mpt_restir.h): the result of the last mpt_direct_restir and what its rounds pass on, with the direct
// result's lifetime.  Allocated by the first call; mpt_resize and the scene calls let go of it.
struct RestirState {
    DevMem<float4> out;            // RestirPass::out: W * H rgba, W * H traced, W * H unoccluded, the MPT_RS_TOTAL_WORDS words of totals
    DevMem<float4> S;              // a pixel's sum across the rounds
    DevMem<uint4> res[2];          // two uint4 per pixel: the last round's reservoirs after step A, its picks after step B
    uint32_t W = 0, H = 0;
    uint64_t epoch = 0;            // the guide_epoch the result was written in (0 = none)
};

// Temporal reservoir reuse (mpt_restir_temporal.h): the last frame's result block and, ping-pong as a History, every pixel's reservoir
// with the guide and the camera of the frame it belongs to.  Not a History: that keeps 16 bytes per pixel and no result block; the
// validity rule (stage_valid) and the camera key are the same.  Allocated by the first mpt_direct_restir_temporal; mpt_resize, the scene
// calls and mpt_restir_temporal_reset let go of it.
struct RestirTemporalState {
    DevMem<float4> out;            // RestirPass::out of the last frame: W * H rgba, W * H traced, W * H unoccluded, the totals
    DevMem<uint4> initial;         // the frame's reservoirs after step A
    DevMem<uint4> res[2];          // two uint4 per pixel: (k, ua, ub, wsum) (fac, flags, Mh, 0)
    DevMem<float4> guide[2];       // (normal facing the ray, t; +inf for a miss)
    uint32_t W = 0, H = 0;
    int cur = 0;                   // which of the two holds the history
    uint64_t epoch = 0;            // the guide_epoch the history was written in (0 = no history)
    float cam[14] = {};            // guide_key of the history's frame
};

// Next-event estimation (mpt_nee.h): what every mpt_render_nee call needs besides the sum — the four totals of mpt_nee_info on the device
// and the pair of timing events.  Made by the first call, kept for the context's life (an allocation per call would cost a device
// synchronisation each time).
struct NeeState {
    DevMem<unsigned long long> totals;
    Event e0, e1;
};

struct mpt_ctx : SceneState {
    int device = 0;
    std::unique_ptr<Submitter> sub;      // mpt_render_async's submit thread (none until the first asynchronous render)
    uint64_t async_jobs = 0;             // renders submitted by that thread
    uint64_t gate_resident = 0;          // residency gate: the trace kernel before was resident (or finished) when asked
    uint64_t gate_timeout = 0;           // ... it was not within 200 ms: the event chain instead (a foreign kernel holds the chip)
    uint64_t async_call_us_max = 0;      // longest mpt_render_async call so far, microseconds of host time
    hipStream_t stream = nullptr;   // == lane[0].stream: uploads, clears, read-backs, mpt_draw
    Lane lane[2];
    int next_lane = 0;
    hipEvent_t last_resolved = nullptr;  // last operation on the HDR sum (resolve or clear): the next resolve waits for it
    hipEvent_t last_traced = nullptr;    // behind the last trace kernel enqueued (either lane): the next trace kernel waits for it (lane_order)
    int resolve_wgs_per_cu = 2;          // MPT_RESOLVE_WGS: workgroups of 256 per CU of a resolve that runs beside a trace kernel (0 = as many as pixels / 256)
    bool sync_render = false;            // inside mpt_render / mpt_draw: nothing else is in flight, the resolve may take the whole chip
    uint32_t launch_seq = 0;             // launch ids of the trace kernels (never 0)
    Lane* last_trace_lane = nullptr;     // lane of the last trace kernel enqueued
    int lane_order = 5;                  // MPT_LANE_ORDER: bit 0 = the event chain between trace kernels, bit 2 = the residency gate for overlapping k_wavelocal renders (run_pass), bit 1 = lane 0's stream has the higher priority (no effect measured)
    Event ev_sum_op;                     // recorded behind mpt_clear_sum
    hipDeviceProp_t prop;
    std::string err;
    std::mutex err_mu;                   // writers of `err`: the caller's thread and the submit thread (set_err)
    // scene (struct SceneState)
    bool have_scene = false;
    // the two operating points of the closest-first kernel (mpt_ordered.h: k_ordered<.., 5> = 5 x 256 threads per CU, k_ordered<.., 6> = 2 x 768) and
    // what each stages in LDS for the scene at hand (size_lds_images)
    struct OtPoint {
        uint32_t threads, wgs_per_cu, lds_nodes, lds_prims;
    } ot_pt[2] = {{MPT_OT_THREADS, MPT_OT_WGS_PER_CU, 0, 0}, {MPT_OT6_THREADS, (MPT_OT6_WAVES * 256) / MPT_OT6_THREADS, 0, 0}};
    int ot_occ = 0;                  // MPT_OT_OCC: 5 / 6 forces an operating point, 0 = by scene size (ordered_point)
    bool tile_order_forced = false;  // MPT_TILE_ORDER was given
    uint32_t ot_stack_depth = 8;     // LDS stack entries per lane (MPT_OT_STACK); deeper entries spill to global memory
    mpt_build::ScratchPool build_pool;  // scratch chunks of the GPU builders, kept between builds (<= 2 GiB)
    // the block of the built scene before is kept as the next build's (install_scene), so a rebuild allocates nothing
    DevMem<> spare_block;
    DevMem<> in_block;                 // device staging of mpt_build_and_upload's input arrays, kept between builds
    OtBudgets ot_budgets = default_ot_budgets();
    float acc_cull_rel = 9.765625e-4f;
    // uniforms / size
    mpt_uniforms u;
    bool have_uniforms = false;
    uint32_t W = 0, H = 0;
    DevMem<float4> d_accum[2];
    int cur_target = 0;
    DevMem<float4> d_sum_own;
    float4* d_sum = nullptr;             // d_sum_own, or the caller's buffer (mpt_set_sum_buffer)
    // this rank's tile processing order (x | y << 16), rebuilt when size or sharding changes
    DevMem<uint32_t> d_tile_xy;
    uint32_t tile_W = 0, tile_H = 0, tile_rank = 0, tile_nranks = 0, tile_count = 0;
    int tile_mode_built = -1;   // tile order the table was built for (tile_order_of)
    int tile_order_mode = 0;  // 0 row-major top-down (measured best with guided claims: the cheap sky tiles take the
                              // large early claims, the expensive tiles the small late ones), 1 strided, 2 bottom-up
    // literal RNG seeds
    DevMem<uint32_t> d_pixel_seed;
    float seed_rs[3] = {NAN, NAN, NAN};
    uint32_t seed_W = 0, seed_H = 0;
    // launch geometry
    int wg_size = 0;                // 0 = the kernel's own choice (MPT_WG_SIZE overrides, clamped to the kernel's bound)
    const void* occ_fun = nullptr;  // cached occupancy query
    size_t occ_lds = 0;
    int occ_per_cu = 0;
    bool time_kernels = true;
    WaveBudgets budgets = default_budgets();  // box-test loop trips per step of ring 0..3 (measured best
                                                        // ladder; an unlimited ring-3 budget leaves ring 4 unused)
    // guided path-id claims: max(wl_min, remaining / (wl_div * waves)).  wl_div, measured again after the kernels got faster
    // (serial 256-spp render of scene.xml, two runs): 16 -> 23.4-23.8 ms, 24 22.5, 32 22.3-22.4, 48 22.3-22.5, 64 22.3-22.4,
    // 128 22.5, 256 22.8; glass.xml, bunny x20, 32-spp and 640x360 renders move by +-1 % between 16 and 64
    // wl_min = 0: by the size of the pass (run_pass) — the smallest claim is 64 path ids (one step) when a wave's share of the pass is
    // small (a 1/8 shard: 11 k paths per wave) and up to 256 when it is large (a full 1080p x 256 spp pass: 86 k): scene.xml with 64 /
    // 128 / 256 / 512 / 1024 -> 16.79-16.86 / 16.70 / 16.62-16.65 / 16.65 / 17.87 ms, the 1/8 shard's serial step 2.54 / - / 2.71 / 3.36
    uint32_t wl_min = 0, wl_div = 32;
    bool wl_lean = true;               // MPT_WL_LEAN=0: every wave-local pass runs the generic kernels (development knob)
    bool ring_knobs_set = false;       // MPT_BUDGETS / MPT_MIN_ACTIVE / MPT_LIGHT_BUDGET given: the generic kernels too, whose ring steps read `budgets`
                                       // (the lean kernels' are constants, mpt_lds_cfg.h)
    bool lean_tiles = true;            // MPT_LEAN_TILES=0: the lean kernels get no class table, every tile is "general" (mpt_lean_tiles.h; development knob)
    bool lean_sky_resolve = true;      // MPT_LEAN_SKY_RESOLVE=0: the lean kernels trace the sky tiles and the resolve reads their slots (development knob)
    LeanCdivCache lean_cdiv;           // is the lean kernels' division by W and H exact at this context's size (mpt_lean_cdiv.h)
    DevMem<uint32_t> d_cdiv_bad;       // the mismatch count of k_lean_cdiv_check
    uint32_t wl_block = MPT_WL_BLOCK;  // path ids a wave claims per atomic (multiple of 64)
    int wgs_per_cu = 0;  // 0 = as many as the occupancy query admits
    size_t lds_budget = 78 * 1024;  // per workgroup; two workgroups per CU share the 160 KiB
    mpt_stats stats = {};
    uint64_t guide_epoch = 1;       // bumped by every scene upload / build and every mpt_resize
    uint64_t tile_class_builds = 0; // launches of k_lean_tile_classes (ensure_tile_classes)
    GuideState gd;
    DenoiseState dn;
    // adaptive sampling (mpt_adaptive.h): the moments buffer (W x H, allocated by the first render with MPT_FLAG_MOMENTS) and the
    // tile buffers of mpt_render_adaptive; mpt_resize drops both
    DevMem<float4> d_m2;
    AdaptiveTiles ad;
    TemporalState tp;
    SvgfState sv;
    DisplayState dp;
    AoState ao;
    LightState lights;
    DirectState di;
    RestirState rs;
    RestirTemporalState rt;
    NeeState nee;
    int32_t light_sampling = MPT_LIGHT_SAMPLING_AREA;   // mpt_set_light_sampling: host state, read at the start of the three calls that sample lights
    uint32_t light_candidates = 1u;                     // mpt_set_light_candidates: host state with the same life, read at the same three places
    int dp_px = 4;                  // MPT_DISPLAY_PX: pixels per thread of k_dp_present, 1 or 4 (the same bytes)
    bool dp_hist_agg = true;        // MPT_DISPLAY_HIST=plain: k_dp_histogram without the aggregation within the wave
};

// The trace kernels: every instantiation the four pipelines launch, ONCE.  trace_kernel picks a pass's row, create_impl raises the
// dynamic-LDS limit of every row, MPT_DEBUG_LAUNCH prints the row's name: a new variant is one more row and its term in trace_kernel.
struct TraceKernel {
    const void* fn;
    const char* name;   // as MPT_DEBUG_LAUNCH prints it
    int wg_max;         // the kernel's launch bound = its workgroup size (mpt_kernels.h: 768 for the wave-local kernels; mpt_ordered.h: 256 or 768 by operating point)
};
// variant of a row: plain, or (wave-local, never counted) the kernel that leaves room for a resolve beside it and / or the lean one
// (wl_lean_ok, mpt_wl_lean.h), or (closest-first, never counted) the six-wave operating point
enum { TK_PLAIN = 0, TK_CORUN = 1, TK_LEAN = 2, TK_SIX = 4 };
static const struct TraceKernelRow {
    int pipeline;
    bool count, all_lds;   // COUNT (work counters) x ALL_LDS (the whole tree fits the LDS budget)
    int variant;
    TraceKernel k;
} g_trace_kernels[] = {
    {MPT_PIPE_WAVEFRONT, true, true, TK_PLAIN, {(const void*)k_step<true, true>, "k_step", 1024}},
    {MPT_PIPE_WAVEFRONT, true, false, TK_PLAIN, {(const void*)k_step<true, false>, "k_step", 1024}},
    {MPT_PIPE_WAVEFRONT, false, true, TK_PLAIN, {(const void*)k_step<false, true>, "k_step", 1024}},
    {MPT_PIPE_WAVEFRONT, false, false, TK_PLAIN, {(const void*)k_step<false, false>, "k_step", 1024}},
    {MPT_PIPE_MEGAKERNEL, true, true, TK_PLAIN, {(const void*)k_megakernel<true, true>, "k_megakernel", 1024}},
    {MPT_PIPE_MEGAKERNEL, true, false, TK_PLAIN, {(const void*)k_megakernel<true, false>, "k_megakernel", 1024}},
    {MPT_PIPE_MEGAKERNEL, false, true, TK_PLAIN, {(const void*)k_megakernel<false, true>, "k_megakernel", 1024}},
    {MPT_PIPE_MEGAKERNEL, false, false, TK_PLAIN, {(const void*)k_megakernel<false, false>, "k_megakernel", 1024}},
    {MPT_PIPE_ORDERED, false, true, TK_SIX, {(const void*)k_ordered<false, true, MPT_OT6_WAVES>, "k_ordered", MPT_OT6_THREADS}},
    {MPT_PIPE_ORDERED, false, false, TK_SIX, {(const void*)k_ordered<false, false, MPT_OT6_WAVES>, "k_ordered", MPT_OT6_THREADS}},
    {MPT_PIPE_ORDERED, true, true, TK_PLAIN, {(const void*)k_ordered<true, true>, "k_ordered", MPT_OT_THREADS}},
    {MPT_PIPE_ORDERED, true, false, TK_PLAIN, {(const void*)k_ordered<true, false>, "k_ordered", MPT_OT_THREADS}},
    {MPT_PIPE_ORDERED, false, true, TK_PLAIN, {(const void*)k_ordered<false, true>, "k_ordered", MPT_OT_THREADS}},
    {MPT_PIPE_ORDERED, false, false, TK_PLAIN, {(const void*)k_ordered<false, false>, "k_ordered", MPT_OT_THREADS}},
    {MPT_PIPE_WAVELOCAL, false, true, TK_LEAN | TK_CORUN, {(const void*)k_wavelocal_lean_corun<true>, "k_wavelocal_lean_corun", MPT_WL_THREADS(true)}},
    {MPT_PIPE_WAVELOCAL, false, false, TK_LEAN | TK_CORUN, {(const void*)k_wavelocal_lean_corun<false>, "k_wavelocal_lean_corun", MPT_WL_THREADS(false)}},
    {MPT_PIPE_WAVELOCAL, false, true, TK_LEAN, {(const void*)k_wavelocal_lean<true>, "k_wavelocal_lean", MPT_WL_THREADS(true)}},
    {MPT_PIPE_WAVELOCAL, false, false, TK_LEAN, {(const void*)k_wavelocal_lean<false>, "k_wavelocal_lean", MPT_WL_THREADS(false)}},
    {MPT_PIPE_WAVELOCAL, false, true, TK_CORUN, {(const void*)k_wavelocal_corun<true>, "k_wavelocal_corun", MPT_WL_THREADS(true)}},
    {MPT_PIPE_WAVELOCAL, false, false, TK_CORUN, {(const void*)k_wavelocal_corun<false>, "k_wavelocal_corun", MPT_WL_THREADS(false)}},
    {MPT_PIPE_WAVELOCAL, true, true, TK_PLAIN, {(const void*)k_wavelocal<true, true>, "k_wavelocal", MPT_WL_THREADS(true)}},
    {MPT_PIPE_WAVELOCAL, true, false, TK_PLAIN, {(const void*)k_wavelocal<true, false>, "k_wavelocal", MPT_WL_THREADS(false)}},
    {MPT_PIPE_WAVELOCAL, false, true, TK_PLAIN, {(const void*)k_wavelocal<false, true>, "k_wavelocal", MPT_WL_THREADS(true)}},
    {MPT_PIPE_WAVELOCAL, false, false, TK_PLAIN, {(const void*)k_wavelocal<false, false>, "k_wavelocal", MPT_WL_THREADS(false)}},
};
// The row of a pass (pipeline: resolved).  A counted pass runs the plain kernel of its pipeline; a combination without a row is a null
// pointer, which run_pass reports: there is no other kernel to fall back to.
static const TraceKernel* trace_kernel(int pipeline, bool count, bool all_lds, int variant) {
    if (count) variant = TK_PLAIN;
    for (const TraceKernelRow& r : g_trace_kernels)
        if (r.pipeline == pipeline && r.count == count && r.all_lds == all_lds && r.variant == variant) return &r.k;
    return nullptr;
}

// The device check behind lean_cdiv_ok (mpt_lean_cdiv.h): all 2^24 numerators of gen_primary<true> over W and over H, on `st`, waited for.
// Runs when a context's size has changed since its last lean pass, never inside a render.
static bool lean_cdiv_device_check(mpt_ctx* ctx, hipStream_t st, float W, float H, uint32_t* mismatches) {
    if (!ctx->d_cdiv_bad && ctx->d_cdiv_bad.alloc(sizeof(uint32_t)) != hipSuccess) return false;
    if (hipMemsetAsync(ctx->d_cdiv_bad.get(), 0, sizeof(uint32_t), st) != hipSuccess) return false;
    hipLaunchKernelGGL(k_lean_cdiv_check, dim3(256), dim3(256), 0, st, W, H, ctx->d_cdiv_bad.get());
    if (hipGetLastError() != hipSuccess) return false;
    if (hipMemcpyAsync(mismatches, ctx->d_cdiv_bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    return hipStreamSynchronize(st) == hipSuccess;
}

#define MPT_LDS_MATS MPT_LDS_MATS_N               // materials staged in LDS (32 B each; mpt_kernels.h)
#define MPT_LDS_EXTRA (MPT_LDS_CFG_F4 * 16 + MPT_LDS_MATS * 32)  // material table + descriptor copy (k_step) / configuration block (k_wavelocal, k_ordered) behind the scene image

static void set_err(mpt_ctx* ctx, const std::string& msg);   // ctx->err = msg under ctx->err_mu (the submit thread may fail at the same moment)
#define HIPCHK(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_err(ctx, std::string(#call) + ": " + hipGetErrorString(e_));                \
            return MPT_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

static void set_err(mpt_ctx* ctx, const std::string& msg) {
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    ctx->err = msg;
}
static int fail(mpt_ctx* ctx, int code, const std::string& msg) {
    if (ctx) set_err(ctx, msg);
    return code;
}
static int wait_impl(mpt_ctx* ctx);  // collects the renders still in flight (defined with the render entry points)
static int drain_submit(mpt_ctx* ctx);   // waits until the renders queued by mpt_render_async have been submitted (struct Submitter)
static void stop_submit(mpt_ctx* ctx);

extern "C" const char* mpt_status_string(int s) {
    switch (s) {
        case MPT_OK: return "ok";
        case MPT_ERR_INVALID_ARG: return "invalid argument";
        case MPT_ERR_NO_DEVICE: return "no HIP device";
        case MPT_ERR_HIP: return "HIP runtime error";
        case MPT_ERR_BAD_SCENE: return "malformed scene arrays";
        case MPT_ERR_NOT_READY: return "scene, uniforms or size not set";
        case MPT_ERR_OVERFLOW: return "ray queue overflow";
    }
    return "unknown status";
}
extern "C" const char* mpt_last_error(const mpt_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

static int create_impl(int device_ordinal, mpt_ctx** out) {
    if (!out) return MPT_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MPT_ERR_NO_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return MPT_ERR_NO_DEVICE;
    std::unique_ptr<mpt_ctx> ctx(new mpt_ctx());   // (an early return frees what has been made so far)
    ctx->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess) return MPT_ERR_HIP;
    if (hipGetDeviceProperties(&ctx->prop, device_ordinal) != hipSuccess) return MPT_ERR_HIP;
    if (const char* lo = getenv("MPT_LANE_ORDER")) ctx->lane_order = atoi(lo);
    if (const char* rw = getenv("MPT_RESOLVE_WGS")) ctx->resolve_wgs_per_cu = std::max(0, atoi(rw));
    int prio_lo = 0, prio_hi = 0;   // (numerically lower = higher priority)
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_lo = prio_hi = 0;
    for (Lane& L : ctx->lane) {  // small per-lane state now; slots, rings and queues are allocated on first use
        const int prio = &L == &ctx->lane[0] ? prio_hi : prio_lo;
        if (((ctx->lane_order & 2) ? L.stream.create(hipStreamCreateWithPriority, hipStreamNonBlocking, prio)
                                   : L.stream.create(hipStreamCreateWithFlags, hipStreamNonBlocking)) != hipSuccess ||
            L.d_desc.alloc(sizeof(PassDesc)) != hipSuccess || hipMemset(L.d_desc.get(), 0, sizeof(PassDesc)) != hipSuccess ||
            L.d_ctr.alloc(MPT_CTR_WORDS * 4) != hipSuccess || hipMemset(L.d_ctr.get(), 0, MPT_CTR_WORDS * 4) != hipSuccess ||
            L.h_done.alloc(64, hipHostMallocMapped) != hipSuccess || L.h_desc.alloc(sizeof(PassDesc)) != hipSuccess ||
            L.ev0.create(hipEventCreate) != hipSuccess || L.ev1.create(hipEventCreate) != hipSuccess ||
            L.ev_resolved.create(hipEventCreate) != hipSuccess || L.ev_traced.create(hipEventCreateWithFlags, hipEventDisableTiming) != hipSuccess)
            return MPT_ERR_HIP;
        memset((void*)L.h_done.get(), 0, 64);   // (every word: the residency gate polls word MPT_HOST_RESIDENT against small launch ids — ADVICE r4)
    }
    ctx->stream = ctx->lane[0].stream.get();
    if (ctx->ev_sum_op.create(hipEventCreate) != hipSuccess) return MPT_ERR_HIP;
    const char* e;
    if ((e = getenv("MPT_WG_SIZE"))) ctx->wg_size = atoi(e);
    if ((e = getenv("MPT_WGS_PER_CU"))) ctx->wgs_per_cu = atoi(e);
    if ((e = getenv("MPT_LDS_BYTES"))) ctx->lds_budget = (size_t)atol(e);
    ctx->time_kernels = !((e = getenv("MPT_NO_KERNEL_EVENTS")) && atoi(e));
    if ((e = getenv("MPT_WL_BLOCK")) && atoi(e) >= 64) ctx->wl_block = (uint32_t)atoi(e) & ~63u;
    if ((e = getenv("MPT_DISPLAY_PX")) && (atoi(e) == 1 || atoi(e) == 4)) ctx->dp_px = atoi(e);
    if ((e = getenv("MPT_DISPLAY_HIST"))) ctx->dp_hist_agg = strcmp(e, "plain") != 0;
    if ((e = getenv("MPT_BUDGETS"))) fill_budgets(e, ctx->budgets.b, MPT_WL_LEVELS - 1u);   // (the last ring has none)
    if ((e = getenv("MPT_MIN_ACTIVE"))) fill_min_active(e, ctx->budgets.min_active, MPT_WL_LEVELS);
    if ((e = getenv("MPT_LIGHT_BUDGET")) && atoi(e) >= 1) {  // one number: geometric ladder b, 2b, 4b, 8b
        uint32_t b = (uint32_t)atoi(e);
        for (uint32_t k = 0; k + 1 < MPT_WL_LEVELS; ++k) ctx->budgets.b[k] = b > (1u << 28) ? b : std::min<uint64_t>((uint64_t)b << k, MPT_WL_NO_BUDGET);
    }
#if !defined(MPT_LEAN_RING_TESTING)   // (a test's build of the lean kernels reads the values as the generic ones do)
    ctx->ring_knobs_set = getenv("MPT_BUDGETS") || getenv("MPT_MIN_ACTIVE") || getenv("MPT_LIGHT_BUDGET");
#endif
    if ((e = getenv("MPT_WL_MIN")) && atoi(e) >= 64) ctx->wl_min = (uint32_t)atoi(e) & ~63u;
    if ((e = getenv("MPT_TILE_ORDER"))) {
        ctx->tile_order_mode = atoi(e);
        ctx->tile_order_forced = true;
    }
    if ((e = getenv("MPT_OT_OCC")) && (atoi(e) == 5 || atoi(e) == 6)) ctx->ot_occ = atoi(e);
    if ((e = getenv("MPT_WL_DIV")) && atoi(e) >= 1) ctx->wl_div = (uint32_t)atoi(e);
    if ((e = getenv("MPT_WL_LEAN"))) ctx->wl_lean = atoi(e) != 0;
    if ((e = getenv("MPT_LEAN_TILES"))) ctx->lean_tiles = atoi(e) != 0;
    if ((e = getenv("MPT_LEAN_SKY_RESOLVE"))) ctx->lean_sky_resolve = atoi(e) != 0;
    if ((e = getenv("MPT_OT_STACK")) && atoi(e) >= 2 && atoi(e) <= (int)MPT_OT_PARK) ctx->ot_stack_depth = (uint32_t)atoi(e);
    unsigned ot[MPT_OT_MLEVELS];   // "a,b,c": one number per tree-walk ring; the rings a list leaves out keep their defaults
    if ((e = getenv("MPT_OT_BUDGETS")))
        for (unsigned k = 0, n = parse_uint_list(e, ot, MPT_OT_MLEVELS); k < n && k + 1 < MPT_OT_MLEVELS; ++k) ctx->ot_budgets.trips[k] = ot[k] < 1 ? 1 : ot[k];
    if ((e = getenv("MPT_OT_MIN_ACTIVE")))
        for (unsigned k = 0, n = parse_uint_list(e, ot, MPT_OT_MLEVELS); k < n; ++k) ctx->ot_budgets.min_active[k] = ot[k] > 64 ? 64 : ot[k];
    if ((e = getenv("MPT_OT_INPLACE")) && atoi(e) >= 1) ctx->ot_budgets.inplace_min = (uint32_t)atoi(e);
    if ((e = getenv("MPT_OT_CULL_REL")) && atof(e) > 0.0) ctx->acc_cull_rel = (float)atof(e);
    if (ctx->wg_size < 64 || ctx->wg_size > 1024 || (ctx->wg_size & 63)) ctx->wg_size = 0;
    if (ctx->lds_budget > 160 * 1024) ctx->lds_budget = 160 * 1024;
    // allow the full 160 KiB of dynamic LDS
    for (const TraceKernelRow& r : g_trace_kernels) hipFuncSetAttribute(r.k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)k_trace_rays_ordered, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)k_trace_rays, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)k_dn_guide, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);   // (the image of k_trace_rays)
    for (const void* k : {(const void*)k_occluded_ref<false>, (const void*)k_occluded_ref<true>, (const void*)k_occluded_own, (const void*)k_ao<MPT_AO_REF>,
                          (const void*)k_ao<MPT_AO_REF_ALL_LDS>, (const void*)k_ao<MPT_AO_OWN>, (const void*)k_direct<MPT_AO_REF>,
                          (const void*)k_direct<MPT_AO_REF_ALL_LDS>, (const void*)k_direct<MPT_AO_OWN>, (const void*)k_nee<MPT_AO_REF>,
                          (const void*)k_nee<MPT_AO_REF_ALL_LDS>, (const void*)k_nee<MPT_AO_OWN>, (const void*)k_direct_cone<MPT_AO_REF>,
                          (const void*)k_direct_cone<MPT_AO_REF_ALL_LDS>, (const void*)k_direct_cone<MPT_AO_OWN>, (const void*)k_nee_cone<MPT_AO_REF>,
                          (const void*)k_nee_cone<MPT_AO_REF_ALL_LDS>, (const void*)k_nee_cone<MPT_AO_OWN>, (const void*)k_nee_adaptive<MPT_AO_REF>,
                          (const void*)k_nee_adaptive<MPT_AO_REF_ALL_LDS>, (const void*)k_nee_adaptive<MPT_AO_OWN>,
                          (const void*)k_nee_adaptive_cone<MPT_AO_REF>, (const void*)k_nee_adaptive_cone<MPT_AO_REF_ALL_LDS>,
                          (const void*)k_nee_adaptive_cone<MPT_AO_OWN>, (const void*)k_restir_initial<MPT_AO_REF>,
                          (const void*)k_restir_initial<MPT_AO_REF_ALL_LDS>, (const void*)k_restir_initial<MPT_AO_OWN>,
                          (const void*)k_restir_merge<MPT_AO_REF, true>, (const void*)k_restir_merge<MPT_AO_REF_ALL_LDS, true>,
                          (const void*)k_restir_merge<MPT_AO_OWN, true>, (const void*)k_restir_merge<MPT_AO_REF, false>,
                          (const void*)k_restir_merge<MPT_AO_REF_ALL_LDS, false>, (const void*)k_restir_merge<MPT_AO_OWN, false>})
        hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    *out = ctx.release();
    return MPT_OK;
}

extern "C" int mpt_destroy(mpt_ctx* ctx) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    stop_submit(ctx);   // (renders still queued are submitted, then the thread ends)
    hipSetDevice(ctx->device);
    for (Lane& L : ctx->lane)   // (nothing is freed while a kernel may still read it)
        if (L.stream) hipStreamSynchronize(L.stream.get());
    delete ctx;   // (and with it every resource it owns)
    return MPT_OK;
}

// ---- scene upload: reference arrays -> threaded, breadth-first, leaf-ordered device layout ----------------
// What each kernel stages in LDS, from the sizes of the uploaded scene.
static void size_lds_images(mpt_ctx* ctx) {
    // LDS image of the reference-order kernels = top of the tree + primitives of the shallowest leaves.  When the whole
    // tree fits, the rest of the budget goes to primitives; otherwise 6 KiB are reserved for them (the leaves next to the
    // root are visited by almost every ray: on scene.xml the three spheres take 65 % of all primitive tests).
    {
        const size_t budget = ctx->lds_budget > MPT_LDS_EXTRA ? ctx->lds_budget - MPT_LDS_EXTRA : 0;
        const size_t all_nodes = (size_t)ctx->n_nodes * 32, all_prims = (size_t)ctx->n_prims * 48;
        size_t prim_bytes = all_nodes <= budget ? std::min(all_prims, budget - all_nodes)
                                                : std::min<size_t>(all_prims, std::min<size_t>(6 * 1024, budget / 4));
        prim_bytes -= prim_bytes % 48;
        ctx->n_lds_prims = (uint32_t)(prim_bytes / 48);
        ctx->n_lds_nodes = (uint32_t)std::min<size_t>(ctx->n_nodes, (budget - prim_bytes) / 32);
    }
    // LDS image of the closest-first kernel at each of its operating points (wgs_per_cu workgroups of `threads` share a CU's 160 KiB):
    // the stacks, then as many own nodes as fit (breadth-first prefix), the always list, and primitives with what is left.
    for (mpt_ctx::OtPoint& pt : ctx->ot_pt) {
        const size_t stacks = (size_t)pt.threads * ctx->ot_stack_depth * 8;
        // (two workgroups per CU get 78 KiB each, not 80: the allocation granule must leave both room)
        const size_t avail = pt.wgs_per_cu == 1 ? 160 * 1024 : 156 * 1024 / pt.wgs_per_cu, fixed = MPT_LDS_EXTRA + stacks + (size_t)ctx->n_always * 80;
        const size_t total = avail > fixed + 112 ? avail - fixed : 112;
        const size_t all_nodes = (size_t)ctx->n_acc_nodes * 112, all_prims = (size_t)ctx->n_prims * 48;
        size_t prim_bytes = all_nodes <= total ? std::min(all_prims, total - all_nodes)
                                               : std::min<size_t>(all_prims, std::min<size_t>(4 * 1024, total / 4));
        if (const char* e = getenv("MPT_OT_LDS_PRIMS")) prim_bytes = std::min<size_t>(prim_bytes, (size_t)atoi(e) * 48);
        prim_bytes -= prim_bytes % 48;
        pt.lds_prims = (uint32_t)(prim_bytes / 48);
        pt.lds_nodes = (uint32_t)std::min<size_t>(ctx->n_acc_nodes, (total - prim_bytes) / 112);
    }
}
// Which operating point of the closest-first kernel renders this scene: the six-wave one up to MPT_OT6_MAX_PRIMS primitives (the
// sixth wave pays while a compute die's L2 can mostly hold the tree: 40 k / 99 k / 397 k / 596 k / 795 k primitives -4.4 / -4.0 / -2.7 /
// -1.5 / -0.7 % with the striped tile order, 994 k +1.7 %, the 1 M-triangle height fields of configs[4] +1.5 .. +7 % — mpt_ordered.h,
// gpurun_out/r05/s7, s9, s12), the five-wave one beyond and for counted renders.
#define MPT_OT6_MAX_PRIMS 800000u
static int ordered_point(const mpt_ctx* ctx, bool count) {
    if (count) return 0;
    if (ctx->ot_occ == 5) return 0;
    if (ctx->ot_occ == 6) return 1;
    return ctx->n_prims <= MPT_OT6_MAX_PRIMS ? 1 : 0;
}

// Puts a scene in place of the one before.  The block of a built scene it replaces becomes the next build's spare if it is not larger
// than 1 GiB and larger than the spare there is (the larger of the two is the one worth keeping: a spare that is too small for the
// scenes being built is never taken).
static void install_scene(mpt_ctx* ctx, SceneState&& s) {
    const DevMem<>& old = ctx->scene_block;
    if (old && old.bytes() <= ((size_t)1 << 30) && (!ctx->spare_block || old.bytes() > ctx->spare_block.bytes()))
        ctx->spare_block = std::move(ctx->scene_block);
    static_cast<SceneState&>(*ctx) = std::move(s);
    ctx->acc_eps_abs = ctx->tri_extent * 3.814697265625e-06f;  // 2^-18 of the largest triangle coordinate
    size_lds_images(ctx);
    ctx->have_scene = true;
    ctx->guide_epoch++;
    ctx->ao = AoState{};   // (an AO result belongs to the scene it was traced in)
    ctx->di = DirectState{};
    ctx->rs = RestirState{};
    ctx->rt = RestirTemporalState{};
    ctx->lights = LightState{};   // (built again by the first call that needs it)
}

// the per-primitive reference-leaf boxes of an uploaded scene (k_prim_refbox, mpt_devbuild.h)
static int make_prim_refbox(mpt_ctx* ctx, SceneState& s) {
    if (s.n_prims == 0 || s.d_refleaf == nullptr || s.n_ref_leaves == 0) return MPT_OK;
    HIPCHK(s.own(&s.d_refbox, (size_t)s.n_prims * 32));
    hipLaunchKernelGGL(mpt_devbuild::k_prim_refbox, dim3((s.n_prims + 255u) / 256u), dim3(256), 0, ctx->stream, (const float4*)s.d_prims,
                       (const float4*)s.d_refleaf, s.n_prims, s.d_refbox);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int upload_scene_impl(mpt_ctx* ctx, const float* bvh, uint64_t n_nodes, const float* prims,
                                const float* mats, const int32_t* prim_idx, uint64_t n_prims) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    if (!bvh || !prims || !mats || !prim_idx || n_nodes == 0 || n_prims == 0)
        return fail(ctx, MPT_ERR_INVALID_ARG, "null or empty scene array");
    if (n_nodes >= (1ull << 30) || n_prims >= (1ull << 27))
        return fail(ctx, MPT_ERR_BAD_SCENE, "scene too large for the 27-bit leaf encoding");
    {
        int wrc = wait_impl(ctx);  // renders in flight still read the old scene
        if (wrc) return wrc;
    }
    mpt_layout::SceneLayout lay;
    {
        std::string why;
        const int lrc = mpt_layout::layout_scene(bvh, n_nodes, prims, mats, prim_idx, n_prims, lay, why);
        if (lrc) return fail(ctx, lrc, why);
    }
    SceneState s;   // (the scene before stays in place until this one is complete)
    const struct {
        float4** dst;
        uint32_t* count;
        const std::vector<float>& v;
        size_t rec_floats;   // floats per record; an empty array still gets an allocation of one record
    } arrays[6] = {{&s.d_nodes, &s.n_nodes, lay.nodes, 8},
                   {&s.d_prims, &s.n_prims, lay.prims, 12},
                   {&s.d_mats, &s.n_mats, lay.mats, 8},
                   {&s.d_acc_nodes, &s.n_acc_nodes, lay.acc_nodes, MPT_ACCEL_NODE_FLOATS},
                   {&s.d_refleaf, &s.n_ref_leaves, lay.refleaf, 8},
                   {&s.d_always, &s.n_always, lay.always, 20}};
    for (const auto& a : arrays) {
        HIPCHK(s.own(a.dst, std::max(a.v.size(), a.rec_floats) * 4));
        if (!a.v.empty()) HIPCHK(hipMemcpy(*a.dst, a.v.data(), a.v.size() * 4, hipMemcpyHostToDevice));
        *a.count = (uint32_t)(a.v.size() / a.rec_floats);
    }
    {
        int rrc = make_prim_refbox(ctx, s);
        if (rrc) return rrc;
    }
    s.acc_depth = lay.acc_depth;
    s.tri_extent = lay.tri_extent;
    s.acc_ok = lay.acc_ok();
    s.acc_why = lay.acc_why();
    install_scene(ctx, std::move(s));
    return MPT_OK;
}

static int set_uniforms_impl(mpt_ctx* ctx, const mpt_uniforms* u) {
    if (!ctx || !u) return MPT_ERR_INVALID_ARG;
    ctx->u = *u;
    ctx->have_uniforms = true;
    return MPT_OK;
}

static int resize_impl(mpt_ctx* ctx, uint32_t width, uint32_t height) {
    if (!ctx || width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 31))
        return fail(ctx, MPT_ERR_INVALID_ARG, "bad size");
    {
        int wrc = wait_impl(ctx);
        if (wrc) return wrc;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // the buffers of the new size are made whole before they replace the old ones: a failure leaves the context as it was
    const size_t bytes = (size_t)width * height * 16;
    DevMem<float4> accum[2], sum;
    for (DevMem<float4>* b : {&accum[0], &accum[1], &sum}) {
        HIPCHK(b->alloc(bytes));
        HIPCHK(hipMemset(b->get(), 0, bytes));
    }
    ctx->d_accum[0] = std::move(accum[0]);
    ctx->d_accum[1] = std::move(accum[1]);
    ctx->d_sum_own = std::move(sum);
    ctx->d_sum = ctx->d_sum_own.get();
    ctx->d_m2.reset();   // (moments and tile counts of the old size: zero from here on)
    ctx->ad = AdaptiveTiles{};
    ctx->tp = TemporalState{};
    ctx->sv = SvgfState{};
    ctx->dp = DisplayState{};
    ctx->ao = AoState{};
    ctx->di = DirectState{};
    ctx->rs = RestirState{};
    ctx->rt = RestirTemporalState{};
    ctx->W = width;
    ctx->H = height;
    ctx->cur_target = 0;
    ctx->guide_epoch++;
    ctx->dn.valid = false;
    return MPT_OK;
}

extern "C" int mpt_sum_buffer(mpt_ctx* ctx, void** p, uint64_t* bytes) {
    if (!ctx || !p) return MPT_ERR_INVALID_ARG;
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    *p = ctx->d_sum;
    if (bytes) *bytes = (uint64_t)ctx->W * ctx->H * 16;
    return MPT_OK;
}
extern "C" int mpt_set_sum_buffer(mpt_ctx* ctx, void* p) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    int wrc = drain_submit(ctx);
    if (wrc) return wrc;
    wrc = wait_impl(ctx);
    if (wrc) return wrc;
    ctx->d_sum = p ? (float4*)p : ctx->d_sum_own.get();
    return MPT_OK;
}
static int clear_sum_impl(mpt_ctx* ctx) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    int wrc = wait_impl(ctx);
    if (wrc) return wrc;
    HIPCHK(hipMemsetAsync(ctx->d_sum, 0, (size_t)ctx->W * ctx->H * 16, ctx->stream));
    if (ctx->d_m2) HIPCHK(hipMemsetAsync(ctx->d_m2.get(), 0, (size_t)ctx->W * ctx->H * 16, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev_sum_op.get(), ctx->stream));  // the next resolve (on either lane) is ordered behind the clear
    ctx->last_resolved = ctx->ev_sum_op.get();
    return MPT_OK;
}
extern "C" void* mpt_stream(mpt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
extern "C" int mpt_synchronize(mpt_ctx* ctx) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    int wrc = drain_submit(ctx);
    if (wrc) return wrc;
    wrc = wait_impl(ctx);
    if (wrc) return wrc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int read_frame_impl(mpt_ctx* ctx, float* out) {
    if (!ctx || !out) return MPT_ERR_INVALID_ARG;
    if (!ctx->d_accum[0]) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    int wrc = wait_impl(ctx);
    if (wrc) return wrc;
    HIPCHK(hipMemcpyAsync(out, ctx->d_accum[ctx->cur_target].get(), (size_t)ctx->W * ctx->H * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int read_sum_impl(mpt_ctx* ctx, float* out) {
    if (!ctx || !out) return MPT_ERR_INVALID_ARG;
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    int wrc = wait_impl(ctx);
    if (wrc) return wrc;
    HIPCHK(hipMemcpyAsync(out, ctx->d_sum, (size_t)ctx->W * ctx->H * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
extern "C" int mpt_get_stats(mpt_ctx* ctx, mpt_stats* out) {
    if (!ctx || !out) return MPT_ERR_INVALID_ARG;
    drain_submit(ctx);   // (a failure of a queued render stays for the next call that can report it: this one returns numbers)
    *out = ctx->stats;
    return MPT_OK;
}
extern "C" int mpt_reset_stats(mpt_ctx* ctx) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    drain_submit(ctx);
    ctx->stats = mpt_stats{};
    return MPT_OK;
}

// ---- pass machinery -------------------------------------------------------------------------------------------
static SceneDev scene_dev(const mpt_ctx* ctx) {
    SceneDev s;
    s.nodes = ctx->d_nodes;
    s.prims = ctx->d_prims;
    s.mats = ctx->d_mats;
    s.n_nodes = ctx->n_nodes;
    s.n_lds_nodes = ctx->n_lds_nodes;
    s.n_lds_prims = ctx->n_lds_prims;
    s.n_lds_mats = std::min<uint32_t>(ctx->n_mats, MPT_LDS_MATS);
    s.n_prims = ctx->n_prims;
    s.n_mats = ctx->n_mats;
    s.lds_prim_off = 2u * s.n_lds_nodes;
    s.lds_mat_off = s.lds_prim_off + 3u * s.n_lds_prims;
    return s;
}

// The closest-first kernel's view: own nodes / always list / primitives / materials / stacks in LDS; the threaded
// reference-order nodes stay in global memory (ring E and the test hook walk them from there).
static size_t ordered_views(const mpt_ctx* ctx, int point, SceneDev& s, AccelDev& a) {
    const mpt_ctx::OtPoint& pt = ctx->ot_pt[point];
    const uint32_t threads = pt.threads;
    s = scene_dev(ctx);
    s.n_lds_nodes = 0;
    s.n_lds_prims = pt.lds_prims;
    a.nodes = ctx->d_acc_nodes;
    a.refleaf = ctx->d_refleaf;
    a.refbox = ctx->d_refbox;
    a.always = ctx->d_always;
    a.n_nodes = ctx->n_acc_nodes;
    a.n_lds_nodes = pt.lds_nodes;
    a.n_always = ctx->n_always;
    a.lds_always_off = 7u * a.n_lds_nodes;
    s.lds_prim_off = a.lds_always_off + 5u * a.n_always;
    s.lds_mat_off = s.lds_prim_off + 3u * s.n_lds_prims;
    const uint32_t image4 = mpt_lds_image_end_f4(s.lds_mat_off);   // (material table + the kernel's configuration block: the one definition of mpt_kernels.h)
    a.lds_stack_off = image4 * 16u;
    a.stack_depth = ctx->ot_stack_depth;
    a.eps_abs = ctx->acc_eps_abs;
    a.cull_rel = ctx->acc_cull_rel;
    a.o_limit = ctx->tri_extent > 0.0f ? 64.0f * ctx->tri_extent : INFINITY;  // no triangles: no tree, nothing to bound
    return (size_t)a.lds_stack_off + (size_t)threads * a.stack_depth * 8u;
}
// The regions of k_ordered's LDS image in the order the kernel addresses them: nodes, always list, primitives, materials, configuration
// block, per-lane stacks.  None may overlap the next and the last must end inside the launch's allocation (the check that would have
// caught round 4's fault at the first launch instead of on the GPU: see mpt_lds_cfg_off_f4).
static bool ordered_layout_ok(const SceneDev& s, const AccelDev& a, uint32_t threads, size_t lds_bytes) {
    const uint64_t nodes_end = 7ull * a.n_lds_nodes, always_end = (uint64_t)a.lds_always_off + 5ull * a.n_always,
                   prims_end = (uint64_t)s.lds_prim_off + 3ull * s.n_lds_prims, mats_end = (uint64_t)s.lds_mat_off + 2ull * s.n_lds_mats,
                   cfg_begin = mpt_lds_cfg_off_f4(s.lds_mat_off), cfg_end = mpt_lds_image_end_f4(s.lds_mat_off),
                   stack_end = (uint64_t)a.lds_stack_off + (uint64_t)threads * a.stack_depth * 8u;
    return nodes_end <= a.lds_always_off && always_end <= s.lds_prim_off && prims_end <= s.lds_mat_off && mats_end <= cfg_begin &&
           cfg_end * 16u <= a.lds_stack_off && (a.lds_stack_off & 7u) == 0u && stack_end <= lds_bytes && a.stack_depth >= 2u && a.stack_depth <= MPT_OT_PARK &&
           (uint64_t)a.n_nodes < (1ull << 24) /* MPT_OT_SIGNSEL: node offsets by a 24-bit multiply */;
}

// the closest-first pipeline needs nested boxes and few spheres (mpt_upload_scene); otherwise the reference-order
// wave-local pipeline renders the same image
// MPT_PIPE_AUTO never picks the closest-first pipeline for the literal RNG: that mode exists to reproduce the reference's
// frames, arithmetic artefacts included, and only the reference's own visit order does that for every ray (include/mpt.h).
static int resolve_pipeline(const mpt_ctx* ctx, int pipeline, int rng_mode = MPT_RNG_PHILOX) {
    if (pipeline == MPT_PIPE_AUTO)
        pipeline = ctx->n_prims >= MPT_AUTO_ORDERED_PRIMS && rng_mode != MPT_RNG_LITERAL ? MPT_PIPE_ORDERED : MPT_PIPE_WAVELOCAL;
    if (pipeline == MPT_PIPE_ORDERED && !ctx->acc_ok) pipeline = MPT_PIPE_WAVELOCAL;
    return pipeline;
}
// MPT_WALK_* -> does the own tree answer?  (-1: a bad value)
static int resolve_walk(const mpt_ctx* ctx, int32_t walk) {
    if (walk == MPT_WALK_REFERENCE) return 0;
    if (walk == MPT_WALK_OWN) return ctx->acc_ok ? 1 : 0;
    if (walk == MPT_WALK_AUTO) return resolve_pipeline(ctx, MPT_PIPE_AUTO) == MPT_PIPE_ORDERED ? 1 : 0;
    return -1;
}
static bool walk_valid(int32_t walk) { return walk == MPT_WALK_REFERENCE || walk == MPT_WALK_OWN || walk == MPT_WALK_AUTO; }
// the reference-order kernels' LDS image (size_lds_images), and whether it holds the whole tree (the ALL_LDS instantiations)
static size_t ref_lds_bytes(const mpt_ctx* ctx) { return (size_t)ctx->n_lds_nodes * 32 + (size_t)ctx->n_lds_prims * 48 + MPT_LDS_EXTRA; }
static bool ref_all_lds(const mpt_ctx* ctx) { return ctx->n_lds_nodes == ctx->n_nodes; }

// A walk choice made launchable: the views of the scene the kernel takes, the dynamic LDS bytes of a workgroup and which of the
// three instantiations (MPT_AO_*, mpt_ao.h) walks it.  Every launch that lets a tree answer a ray gets these from walk_views: the
// trace kernels of a pass (launch_geometry), the per-tile shadow-ray kernels (tile_walk_launch, mpt_post.h), the ray queries (mpt_query.h).
struct WalkViews {
    SceneDev sc;
    AccelDev ac;   // the own tree only
    size_t lds;
    int which;
};
// own: the closest-first kernel's image at operating point `point`, checked for workgroups of `threads` (the one-ray-per-lane and per-tile
// kernels take point 0, the five-wave one's: workgroups of 256); else the reference-order tree, wholly or partly in LDS.
static int walk_views(mpt_ctx* ctx, bool own, int point, uint32_t threads, WalkViews& v) {
    if (!own) {
        v = WalkViews{scene_dev(ctx), AccelDev{}, ref_lds_bytes(ctx), ref_all_lds(ctx) ? MPT_AO_REF_ALL_LDS : MPT_AO_REF};
        return MPT_OK;
    }
    v.ac = AccelDev{};
    v.lds = ordered_views(ctx, point, v.sc, v.ac);
    v.which = MPT_AO_OWN;
    if (!ordered_layout_ok(v.sc, v.ac, threads, v.lds)) return fail(ctx, MPT_ERR_INVALID_ARG, "LDS layout of the closest-first kernel overlaps (internal)");
    return MPT_OK;
}
// Fragment.metal:29 + Random.h:32-35: per-pixel u32 seed of the literal RNG.  The float sin-hash is
// chaotic in the last ulp of sin(), so it is evaluated once on the host with the
// C library's sinf and uploaded; everything downstream is integer hashing on the device.
static int ensure_pixel_seeds(mpt_ctx* ctx) {
    const float* rs = ctx->u.randomSeed;
    if (ctx->d_pixel_seed && ctx->seed_W == ctx->W && ctx->seed_H == ctx->H &&
        memcmp(ctx->seed_rs, rs, 12) == 0)
        return MPT_OK;
    std::vector<uint32_t> seeds((size_t)ctx->W * ctx->H);
    const float W = ctx->u.screenSize[0], H = ctx->u.screenSize[1];
    for (uint32_t y = 0; y < ctx->H; ++y)
        for (uint32_t x = 0; x < ctx->W; ++x) {
            float uvx = ((float)x + 0.5f) / W, uvy = ((float)y + 0.5f) / H;
            float v = sinf(uvx * rs[0] + uvy * rs[1]) * rs[2];
            v = v - floorf(v);
            seeds[(size_t)y * ctx->W + x] = (uint32_t)(v * 4294967296.0f);
        }
    HIPCHK(ctx->d_pixel_seed.alloc(seeds.size() * 4));
    HIPCHK(hipMemcpy(ctx->d_pixel_seed.get(), seeds.data(), seeds.size() * 4, hipMemcpyHostToDevice));
    memcpy(ctx->seed_rs, rs, 12);
    ctx->seed_W = ctx->W;
    ctx->seed_H = ctx->H;
    return MPT_OK;
}

// Tiles t with t % nranks == rank, in the order the pass walks them.  Strided order: local index k -> local tile
// (k * P) mod n with P ~ 0.618 n coprime to n, which spreads consecutive path-id windows over the whole image.
static int ensure_tile_order(mpt_ctx* ctx, uint32_t rank, uint32_t nranks, int mode, uint32_t& n_local) {
    const uint32_t tiles_x = (ctx->W + 7) / 8, tiles_y = (ctx->H + 7) / 8, tiles = tiles_x * tiles_y;
    n_local = tiles > rank ? (tiles - rank + nranks - 1) / nranks : 0;
    if (ctx->d_tile_xy && ctx->tile_W == ctx->W && ctx->tile_H == ctx->H && ctx->tile_rank == rank &&
        ctx->tile_nranks == nranks && ctx->tile_mode_built == mode)
        return MPT_OK;
    std::vector<uint32_t> xy(std::max<uint32_t>(n_local, 1));
    uint64_t P = 1;
    if (mode == 1 && n_local > 2) {
        P = (uint64_t)(0.6180339887 * n_local) | 1ull;
        auto gcd = [](uint64_t a, uint64_t b) {
            while (b) {
                uint64_t t = a % b;
                a = b;
                b = t;
            }
            return a;
        };
        while (gcd(P, n_local) != 1) P += 2;
    }
    for (uint32_t k = 0; k < n_local; ++k) {
        uint32_t tl = (uint32_t)(((uint64_t)k * P) % n_local);
        if (mode == 2) tl = n_local - 1u - k;  // bottom-up row-major
        const uint32_t T = tl * nranks + rank;
        xy[k] = (T % tiles_x) | ((T / tiles_x) << 16);
    }
    if (mode == 3 && n_local >= MPT_NGROUP) {
        // XCD stripes (round 5): claim range g — the workgroups with blockIdx % 8 == g, one XCD under round-robin placement, with an L2
        // of its own — owns the tiles at positions k % 8 == g of this table (range_chunk_to_path_chunk).  Row-major order gives every
        // range every 8th tile of every row: all eight L2s see the whole scene.  Here the rank's tiles are cut into eight vertical
        // stripes of equal tile count (sky, ground and geometry in each: balanced) and range g gets stripe g, top-down: the rays of one
        // XCD start in one part of the scene and its L2 holds that part of the tree.  Ranges that run dry steal from the next, as ever.
        std::vector<uint32_t> col(xy);   // the rank's tiles, column-major
        std::sort(col.begin(), col.end(), [](uint32_t a, uint32_t b) {
            const uint32_t ax = a & 0xFFFFu, bx = b & 0xFFFFu;
            return ax != bx ? ax < bx : (a >> 16) < (b >> 16);
        });
        size_t at = 0;
        for (uint32_t g = 0; g < MPT_NGROUP; ++g) {
            const uint32_t n_g = (n_local - g + MPT_NGROUP - 1u) / MPT_NGROUP;   // = range_paths' tile count of range g
            std::vector<uint32_t> stripe(col.begin() + at, col.begin() + at + n_g);
            at += n_g;
            std::sort(stripe.begin(), stripe.end(), [](uint32_t a, uint32_t b) {   // top-down, left to right inside the stripe
                const uint32_t ay = a >> 16, by = b >> 16;
                return ay != by ? ay < by : (a & 0xFFFFu) < (b & 0xFFFFu);
            });
            for (uint32_t j = 0; j < n_g; ++j) xy[(size_t)j * MPT_NGROUP + g] = stripe[j];
        }
    }
    HIPCHK(ctx->d_tile_xy.alloc(xy.size() * 4));
    HIPCHK(hipMemcpy(ctx->d_tile_xy.get(), xy.data(), xy.size() * 4, hipMemcpyHostToDevice));
    ctx->tile_W = ctx->W;
    ctx->tile_H = ctx->H;
    ctx->tile_rank = rank;
    ctx->tile_nranks = nranks;
    ctx->tile_mode_built = mode;
    ctx->tile_count = n_local;
    return MPT_OK;
}

// The global ray queues exist only for the wavefront pipeline; the other two never touch them.
static int ensure_workspace(mpt_ctx* ctx, Lane& L, uint32_t slots_items, uint64_t pass_paths, bool need_queues) {
    uint32_t cap = ((slots_items + MPT_NSHARD - 1) / MPT_NSHARD + 2) * 64u;
    if (need_queues && cap > L.shard_cap) {
        L.shard_cap = 0;
        size_t n = (size_t)cap * MPT_NSHARD;
        for (int i = 0; i < 2; ++i) {
            HIPCHK(L.q_od[i].alloc(n * 16));
            HIPCHK(L.q_dt[i].alloc(n * 16));
            HIPCHK(L.q_tl[i].alloc(n * 16));
            HIPCHK(L.q_ia[i].alloc(n * 8));
        }
        L.shard_cap = cap;
    }
    if (pass_paths * 16 > L.d_slots.bytes()) HIPCHK(L.d_slots.alloc(pass_paths * 16));
    return MPT_OK;
}

static int check_ready(mpt_ctx* ctx, const mpt_render_params* p) {
    if (!ctx || !p) return MPT_ERR_INVALID_ARG;
    if (!ctx->have_scene || !ctx->have_uniforms || !ctx->W) return fail(ctx, MPT_ERR_NOT_READY, "scene, uniforms or size not set");
    if ((uint32_t)ctx->u.screenSize[0] != ctx->W || (uint32_t)ctx->u.screenSize[1] != ctx->H)
        return fail(ctx, MPT_ERR_INVALID_ARG, "uniforms.screenSize does not match mpt_resize");
    if (p->rng_mode < 0 || p->rng_mode > 1 || p->bsdf_mode < 0 || p->bsdf_mode > 2 || p->max_depth < 1 ||
        p->max_depth > 31 + 1 || p->pipeline < 0 || p->pipeline > 4 || p->shard_count < 1 || p->shard_rank < 0 ||
        p->shard_rank >= p->shard_count || (uint64_t)p->sample_begin + p->sample_count > (1ull << 27))
        return fail(ctx, MPT_ERR_INVALID_ARG, "bad render params");
    return MPT_OK;
}

// Paths one pass may hold.  The global-wavefront queue packs path | bounce << 27 into one word; the wave-local
// rings and the megakernel carry full 32-bit path ids.  Per-path result slots cost 16 B each: cap a pass at 2^30
// paths (16 GiB of slots) — a whole 1920x1080x256spp render (531 M paths, 8.5 GB) is ONE pass and ONE launch.
static inline uint64_t pass_path_limit(int pipeline) {
    return pipeline == MPT_PIPE_WAVEFRONT ? (1ull << 27) : (1ull << 30);
}

static inline bool count_flag(const mpt_render_params* p) { return (p->flags & MPT_FLAG_COUNT_WORK) != 0; }

// The order in which a pass walks the rank's tiles: what MPT_TILE_ORDER says, else row-major — or, for the six-wave operating point of
// the closest-first kernel, one vertical stripe of the image per claim range = per XCD (ensure_tile_order, mode 3: measured together).
static int tile_order_of(const mpt_ctx* ctx, const mpt_render_params* p) {
    if (ctx->tile_order_forced) return ctx->tile_order_mode;
    return resolve_pipeline(ctx, p->pipeline, p->rng_mode) == MPT_PIPE_ORDERED && ordered_point(ctx, count_flag(p)) == 1 ? 3 : 0;
}

// A device list of tiles (x | y << 16) that a pass walks instead of the rank's table: mpt_render_adaptive's active tiles.
struct TileOverride {
    const uint32_t* tiles;
    uint32_t n;
};

// The next of the lane's kernel-timing events (the pool grows as a render needs them; collect_lane hands them all back).
static hipError_t next_event(Lane& L, hipEvent_t* e) {
    if (L.ev_used == L.ev_pool.size()) {
        Event ev;
        const hipError_t r = ev.create(hipEventCreate);
        if (r != hipSuccess) return r;
        L.ev_pool.push_back(std::move(ev));
    }
    *e = L.ev_pool[L.ev_used++].get();
    return hipSuccess;
}

// ---- one pass, step by step (run_pass below drives them in this order) ---------------------------------------------------------------
// What a pass launches: decided by select_trace_kernel and launch_geometry, used by the two launch functions.
struct PassLaunch {
    int pipeline = 0;                 // resolved (resolve_pipeline)
    const TraceKernel* k = nullptr;
    bool corun = false;               // the variant of the wave-local kernel that leaves room for a resolve: the pass may overlap the one before
    int ot_point = 0;                 // closest-first pipeline: its operating point (ordered_point)
    int wg = 0, grid = 0;
    size_t lds = 0;
    AccelDev accel = {};              // closest-first pipeline only
    WlLean lean_args = {0u, 0u, 0u};  // lean kernels only
    bool lean_all_lds = false;        // a lean kernel with the whole tree in LDS: the ones that read the class table
    const uint32_t* tile_classes = nullptr;   // ... and the table (ensure_tile_classes; null: every tile is general)
    uint32_t sky_resolve = 0u;        // ... and whether its sky tiles are left to the pass's resolve (run_pass)
};

// The result slots one iteration of the wavefront pipeline retires, in items of 64 (the other pipelines size k_begin_pass's cursors by it)
static uint32_t pass_slots(const mpt_render_params* p, uint64_t pass_paths) {
    uint32_t slots = p->slots_per_iter ? p->slots_per_iter : (16u << 20);
    uint32_t slots_items = std::max<uint32_t>(64, (slots + 63) / 64);
    if ((uint64_t)slots_items * 64 > pass_paths + 64) slots_items = (uint32_t)((pass_paths + 63) / 64);
    if (slots_items < 8) slots_items = 8;
    return slots_items;
}

// The kernels' view of the pass: scene, the lane's buffers, camera, tile walk, sample range and shading parameters.
static int fill_pass_params(mpt_ctx* ctx, Lane& L, const mpt_render_params* p, uint32_t sample_begin, uint32_t S, int tile_mode,
                            const TileOverride* ovr, PassParams& pp) {
    const uint32_t tiles_x = (ctx->W + 7) / 8;
    pp.scene = scene_dev(ctx);
    for (int i = 0; i < 2; ++i) pp.q[i] = QueueDev{L.q_od[i].get(), L.q_dt[i].get(), L.q_tl[i].get(), L.q_ia[i].get()};
    pp.shard_cap = L.shard_cap;
    pp.desc = L.d_desc.get();
    pp.ctr = L.d_ctr.get();
    pp.slots = L.d_slots.get();
    pp.pixel_seed = ctx->d_pixel_seed.get();
    const mpt_uniforms& u = ctx->u;
    pp.cam = F3{u.cameraPosition[0], u.cameraPosition[1], u.cameraPosition[2]};
    pp.first = F3{u.firstPixelPosition[0], u.firstPixelPosition[1], u.firstPixelPosition[2]};
    pp.vu = F3{u.viewportU[0], u.viewportU[1], u.viewportU[2]};
    pp.vv = F3{u.viewportV[0], u.viewportV[1], u.viewportV[2]};
    pp.W = u.screenSize[0];
    pp.H = u.screenSize[1];
    pp.width = ctx->W;
    pp.height = ctx->H;
    pp.tiles_x = tiles_x;
    pp.S = S;
    pp.s_shift = (S & (S - 1)) == 0 ? (uint32_t)__builtin_ctz(S) : 0xFFu;
    pp.tile_xy = ovr ? ovr->tiles : ctx->d_tile_xy.get();
    pp.sample_begin = sample_begin;
    pp.rank = (uint32_t)p->shard_rank;
    pp.nranks = (uint32_t)p->shard_count;
    {   // path -> pixel by arithmetic when the tiles are walked in row-major order: T / tiles_x = umulhi(T, ceil(2^32 / tiles_x)) is exact
        // while T * tiles_x < 2^32 (error term T * (tiles_x - 1) / (tiles_x * 2^32) < 1 / tiles_x); otherwise the table
        const uint64_t tiles = (uint64_t)tiles_x * ((ctx->H + 7) / 8);
        pp.tile_magic = 0u;
        if (!ovr && tile_mode == 0 && tiles_x >= 2u && tiles * tiles_x < (1ull << 32) && getenv("MPT_TILE_TABLE") == nullptr)
            pp.tile_magic = (uint32_t)(((1ull << 32) + tiles_x - 1u) / tiles_x);
    }
    pp.sp.rng_mode = p->rng_mode;
    pp.sp.bsdf_mode = p->bsdf_mode;
    pp.sp.max_depth = p->max_depth;
    pp.sp.seed_lo = p->seed_lo;
    pp.sp.seed_hi = p->seed_hi;
    pp.sp.primitive_count = (uint32_t)std::min<uint64_t>(u.primitiveCount, 0xFFFFFFFFull);
    uint32_t* dev_done = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&dev_done, L.h_done.get(), 0));
    pp.host_done = dev_done;
    return MPT_OK;
}

// Which kernel of the table runs the pass, and at what workgroup size.
static int select_trace_kernel(mpt_ctx* ctx, Lane& L, const mpt_render_params* p, uint32_t n_local_tiles, const PassParams& pp, PassLaunch& g) {
    const bool count = count_flag(p);
    bool all_lds = ref_all_lds(ctx);
    int variant = TK_PLAIN;
    if (g.pipeline == MPT_PIPE_WAVELOCAL) {
        // a render that overlaps others (mpt_render_async) runs the variant of the wave-local kernel that leaves room on the CU for the
        // resolve of the render before it (k_wavelocal_corun); only then may the end of one pass overlap the start of the next (order_behind_previous_trace)
        g.corun = (ctx->lane_order & 4) && !ctx->sync_render && !count;
        // Philox + Lambert without counters, inside the ranges of the lean kernels' 24-bit index arithmetic: the lean variant of the same kernel
        // ... and with the ring knobs untouched (the lean kernels' ring budgets are their own constants)
        const bool lean = ctx->wl_lean && !ctx->ring_knobs_set &&
                          wl_lean_ok(ctx->n_prims, n_local_tiles, pp.tiles_x, ctx->W, ctx->H, pp.nranks, pp.S, pp.tile_magic, p->rng_mode, p->bsdf_mode, count, &g.lean_args) &&
                          lean_cdiv_ok(ctx->lean_cdiv, pp.W, pp.H, [&](float W, float H, uint32_t* bad) { return lean_cdiv_device_check(ctx, L.stream.get(), W, H, bad); });
        variant = (g.corun ? TK_CORUN : 0) | (lean ? TK_LEAN : 0);
        g.lean_all_lds = lean && all_lds;
    } else if (g.pipeline == MPT_PIPE_ORDERED) {
        g.ot_point = ordered_point(ctx, count);
        all_lds = ctx->ot_pt[g.ot_point].lds_nodes == ctx->n_acc_nodes;
        variant = g.ot_point == 1 ? TK_SIX : TK_PLAIN;
    }
    g.k = trace_kernel(g.pipeline, count, all_lds, variant);
    if (!g.k) return fail(ctx, MPT_ERR_INVALID_ARG, "no trace kernel for this pass (internal)");
    g.wg = g.pipeline != MPT_PIPE_ORDERED && ctx->wg_size > 0 && ctx->wg_size <= g.k->wg_max ? ctx->wg_size : g.k->wg_max;
    return MPT_OK;
}

// LDS bytes per workgroup, workgroups per CU (the occupancy query is cached by kernel and LDS size) and the grid.  For the closest-first
// kernel this also makes its views of the scene (pp.scene, g.accel), checked by walk_views.
static int launch_geometry(mpt_ctx* ctx, PassParams& pp, PassLaunch& g) {
    WalkViews v;
    const int vrc = walk_views(ctx, g.pipeline == MPT_PIPE_ORDERED, g.ot_point, (uint32_t)g.wg, v);
    if (vrc) return vrc;
    pp.scene = v.sc;   // (the reference-order pipelines: scene_dev(ctx), as fill_pass_params left it)
    g.accel = v.ac;
    g.lds = v.lds;
    int per_cu = 0;
    if (ctx->occ_fun == g.k->fn && ctx->occ_lds == g.lds) {
        per_cu = ctx->occ_per_cu;
    } else {
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, g.k->fn, g.wg, g.lds));
        ctx->occ_fun = g.k->fn;
        ctx->occ_lds = g.lds;
        ctx->occ_per_cu = per_cu;
    }
    if (per_cu < 1) return fail(ctx, MPT_ERR_HIP, "kernel does not fit on a CU");
    if (getenv("MPT_DEBUG_LAUNCH"))
        fprintf(stderr, "[mpt] pipeline %d: %d workgroups of %d per CU, %zu B of LDS each, kernel %s\n", g.pipeline, per_cu, g.wg, g.lds, g.k->name);
    if (ctx->wgs_per_cu > 0 && per_cu > ctx->wgs_per_cu) per_cu = ctx->wgs_per_cu;
    g.grid = ctx->prop.multiProcessorCount * per_cu;
    return MPT_OK;
}

// Trace kernels are persistent and sized for the whole chip: two of them must never be DISPATCHED side by side (each would hold
// half of the workgroup slots for its whole life — measured: 21.7 ms per 256-spp step instead of 16.8), and which of two pending
// launches the hardware starts is not ours to choose.  Two ways to keep them apart:
//  * the chain: a trace kernel waits for the event behind the one enqueued before it, on whichever lane — strictly one after the
//    other; what the second lane overlaps is the resolve of the render before, the statistics copy, the host;
//  * the gate (renders of k_wavelocal_corun): this launch is SUBMITTED only once the trace kernel before it has announced that
//    all its workgroups are resident (announce_resident; the host waits here, at most for the render that is running) — from then
//    on this kernel's workgroups can only take the places the others give up as they finish: the end of one pass overlaps the
//    start of the next, and the resolve runs in the room the variant leaves.  Without the announcement within 200 ms (a kernel
//    that does not announce, a foreign kernel holding the chip): the chain.
static int order_behind_previous_trace(mpt_ctx* ctx, Lane& L, bool corun) {
    bool need_chain = (ctx->lane_order & 1) != 0;
    if (corun && ctx->last_trace_lane && ctx->last_trace_lane != &L) {
        Lane& O = *ctx->last_trace_lane;
        bool resident = false;
        if (O.announced_id != 0u) {
            const volatile uint32_t* flag = (const volatile uint32_t*)O.h_done.get() + MPT_HOST_RESIDENT;
            const auto t0 = std::chrono::steady_clock::now();
            for (;;) {
                if (*flag == O.announced_id || hipEventQuery(O.ev_traced.get()) == hipSuccess) {   // resident (or even finished)
                    resident = true;
                    break;
                }
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
                std::this_thread::yield();
            }
            (resident ? ctx->gate_resident : ctx->gate_timeout)++;
        }
        need_chain = !resident;
    }
    if (need_chain && ctx->last_traced && ctx->last_traced != L.ev_traced.get()) HIPCHK(hipStreamWaitEvent(L.stream.get(), ctx->last_traced, 0));
    return MPT_OK;
}

// The class table of a pass of the lean ALL_LDS kernels: built by k_lean_tile_classes on the lane's stream, ahead of the trace kernel, when
// the lane has none for this scene, camera and image (a batch render: once).  Without the item (MPT_LEAN_TILES=0 in the environment) the
// kernels get a null pointer.
static int ensure_tile_classes(mpt_ctx* ctx, Lane& L, const PassParams& pp, PassLaunch& g) {
    g.tile_classes = nullptr;
    if (!g.lean_all_lds || !ctx->lean_tiles) {   // (the lane's pass runs without a table: what mpt_read_lean_tile_classes reports for it)
        memset(&L.tile_key, 0, sizeof L.tile_key);
        return MPT_OK;
    }
    const uint32_t tiles_x = pp.tiles_x, tiles_y = (ctx->H + 7) / 8;
    LeanTileKey key;
    memset(&key, 0, sizeof key);
    key.epoch = ctx->guide_epoch;
    key.nodes = pp.scene.nodes;
    const F3 v3[4] = {pp.cam, pp.first, pp.vu, pp.vv};
    float* dst[4] = {key.view.cam, key.view.first, key.view.vu, key.view.vv};
    for (int k = 0; k < 4; ++k) {
        dst[k][0] = v3[k].x;
        dst[k][1] = v3[k].y;
        dst[k][2] = v3[k].z;
    }
    key.view.W = pp.W;
    key.view.H = pp.H;
    key.view.tiles_x = tiles_x;
    key.view.tiles_y = tiles_y;
    key.width = ctx->W;
    key.height = ctx->H;
    key.n_words = tiles_x * tiles_y + pp.nranks;   // (both below 2^24: wl_lean_ok)
    if (!L.d_tile_classes || memcmp(&key, &L.tile_key, sizeof key) != 0) {
        if (L.d_tile_classes.bytes() < (size_t)key.n_words * 4) {
            memset(&L.tile_key, 0, sizeof L.tile_key);
            HIPCHK(L.d_tile_classes.alloc((size_t)key.n_words * 4));
        }
        hipLaunchKernelGGL(k_lean_tile_classes, dim3((key.n_words + 63u) / 64u), dim3(64), 0, L.stream.get(), pp.scene.nodes, pp.scene.n_nodes, pp.scene.prims,
                           pp.scene.n_prims, key.view, L.d_tile_classes.get(), key.n_words);
        HIPCHK(hipGetLastError());
        L.tile_key = key;
        ctx->tile_class_builds++;
    }
    g.tile_classes = L.d_tile_classes.get();
    return MPT_OK;
}

// A lane's ring allocation, grown to `waves` waves (never shrunk): waves * per_wave records of 16 bytes in each of `arrays` arrays, and
// `extra` bytes behind them.  The records are indexed with 31 bits.
template <class Rings>
static int grow_rings(mpt_ctx* ctx, DevMem<float4>& mem, Rings& ring, size_t& ring_waves, size_t waves, size_t per_wave, size_t arrays, size_t extra) {
    if (waves <= ring_waves) return MPT_OK;
    ring = Rings{};
    ring_waves = 0;
    const size_t n = waves * per_wave;
    if (n >= (1ull << 31)) return fail(ctx, MPT_ERR_INVALID_ARG, "too many waves for the ring index (internal)");
    HIPCHK(mem.alloc(arrays * n * 16 + extra));
    ring = Rings{mem.get(), (uint32_t)n};
    ring_waves = waves;
    return MPT_OK;
}
// The rings of the pass's pipeline: the wave-local kernels' five arrays + room for the MPT_DEBUG_WAVE_TIMES records, or the closest-first kernel's
static int ensure_rings(mpt_ctx* ctx, Lane& L, int pipeline, size_t waves) {
    if (pipeline == MPT_PIPE_WAVELOCAL)
        return grow_rings(ctx, L.ring_mem, L.ring, L.ring_waves, waves, (size_t)MPT_WL_LEVELS * MPT_WL_RING, 5, waves * 128 + 1024);
    return grow_rings(ctx, L.ot_ring_mem, L.ot_ring, L.ot_ring_waves, waves, (size_t)MPT_OT_RINGS * MPT_WL_RING, MPT_OT_RING_ARRAYS, 0);
}

// One launch of the pass's kernel — when kernels are timed, between two events of the lane's pool, which go to `timed` (they are read
// after the ONE sync of mpt_render / mpt_draw).
static int launch_timed(mpt_ctx* ctx, Lane& L, const PassLaunch& g, void** args, bool time_kernels, std::vector<std::pair<hipEvent_t, hipEvent_t>>& timed) {
    hipStream_t st = L.stream.get();
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (time_kernels) {
        HIPCHK(next_event(L, &e0));
        HIPCHK(next_event(L, &e1));
        HIPCHK(hipEventRecord(e0, st));
    }
    HIPCHK(hipLaunchKernel(g.k->fn, dim3(g.grid), dim3(g.wg), args, g.lds, st));
    if (time_kernels) {
        HIPCHK(hipEventRecord(e1, st));
        timed.emplace_back(e0, e1);
    }
    return MPT_OK;
}

// Megakernel, wave-local and closest-first pipelines: ONE launch for the whole pass; nothing is waited for.
static int launch_persistent(mpt_ctx* ctx, Lane& L, PassLaunch& g, PassParams& pp, uint64_t pass_paths, bool time_kernels) {
    int rc;
    if (g.pipeline == MPT_PIPE_MEGAKERNEL) {
        void* args[] = {(void*)&pp};
        if ((rc = launch_timed(ctx, L, g, args, time_kernels, L.pending_timed))) return rc;
    } else {
        const size_t waves = (size_t)g.grid * (g.wg / 64);
        if ((rc = ensure_rings(ctx, L, g.pipeline, waves))) return rc;
        uint32_t wl_block = ctx->wl_block, wl_min = ctx->wl_min, wl_div = ctx->wl_div;
        if (wl_min == 0u) {   // (a wave's share of the pass / 16 Ki path ids, in steps of 64, between 64 and 256)
            const uint64_t share = pass_paths / std::max<size_t>(1, waves);
            wl_min = 64u * (uint32_t)std::min<uint64_t>(4, std::max<uint64_t>(1, share >> 14));
        }
        void* ordered_args[] = {(void*)&pp, (void*)&g.accel, (void*)&L.ot_ring, (void*)&ctx->ot_budgets, (void*)&wl_block, (void*)&wl_min, (void*)&wl_div};
        void* wavelocal_args[] = {(void*)&pp, (void*)&L.ring, (void*)&ctx->budgets, (void*)&wl_block, (void*)&wl_min, (void*)&wl_div, (void*)&g.lean_args, (void*)&g.tile_classes, (void*)&g.sky_resolve};   // (the last three: lean kernels only)
        if ((rc = launch_timed(ctx, L, g, g.pipeline == MPT_PIPE_ORDERED ? ordered_args : wavelocal_args, time_kernels, L.pending_timed))) return rc;
    }
    if (ctx->lane_order & 5) {   // (always, unless MPT_LANE_ORDER=0)
        HIPCHK(hipEventRecord(L.ev_traced.get(), L.stream.get()));
        ctx->last_traced = L.ev_traced.get();
        ctx->last_trace_lane = &L;
    }
    ctx->stats.iterations += 1;
    return MPT_OK;
}

// Wavefront pipeline: k_step + k_advance per bounce generation, enqueued in batches; the device publishes `done` to pinned host memory.
// Waits for the pass and reads its statistics back.
static int launch_wavefront(mpt_ctx* ctx, Lane& L, const PassLaunch& g, PassParams& pp, int max_depth, uint64_t pass_paths, uint32_t slots_items, bool time_kernels) {
    hipStream_t st = L.stream.get();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timed;
    uint32_t parity = 0;
    uint64_t launched = 0;
    // Expected number of iterations: every slot of an iteration retires one ray; a pass traces about
    // 1.7 rays per path here, and the queue drains over at most max_depth further iterations.  All of them
    // are enqueued without a host round trip (an iteration that finds no work exits at once); the device
    // publishes `done` to pinned host memory and the host only tops up if the estimate was short.
    const uint64_t est = (pass_paths * 7 / 4) / ((uint64_t)slots_items * 64) + (uint64_t)max_depth + 2;
    const uint64_t hard_cap = est * 8 + 64;
    uint64_t batch = est;
    for (;;) {
        for (uint64_t b = 0; b < batch; ++b) {
            void* args[] = {(void*)&pp, (void*)&parity};
            const int rc = launch_timed(ctx, L, g, args, time_kernels, timed);
            if (rc) return rc;
            hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, L.d_desc.get(), L.d_ctr.get(), pp.host_done);
            parity ^= 1u;
            launched++;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        uint32_t flag = *(volatile uint32_t*)L.h_done.get();
        if (flag & 2u) return fail(ctx, MPT_ERR_OVERFLOW, "ray queue overflow");
        if (flag & 1u) break;
        if (launched > hard_cap) return fail(ctx, MPT_ERR_HIP, "pass did not drain (internal)");
        batch = 4;
    }
    PassDesc hd;
    HIPCHK(hipMemcpy(&hd, L.d_desc.get(), sizeof hd, hipMemcpyDeviceToHost));
    // only the iterations that had work count as launches of the dominant kernel
    const uint64_t real = hd.iterations;
    for (size_t i = 0; i < timed.size() && i < real; ++i) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, timed[i].first, timed[i].second));
        ctx->stats.trace_kernel_ms += ms;
        if (getenv("MPT_DEBUG_ITERS")) fprintf(stderr, "[mpt] iter %zu: %.3f ms\n", i, ms);
    }
    if (time_kernels) ctx->stats.trace_launches += real;
    ctx->stats.iterations += real;
    return MPT_OK;
}

// Runs one pass of S samples/pixel over this rank's tiles (or the override's); leaves the per-path results in d_slots.
// `sky_classes` (null: the caller's resolve reads every slot, as k_resolve_frame does): the caller ends the pass in k_resolve_sum or
// k_resolve_sum_moments and hands them what this leaves there — the pass's class table when its trace kernel elided the sky tiles, which
// then have NO slot values (a lean kernel with a table, unless MPT_LEAN_SKY_RESOLVE=0), else null.
static int run_pass(mpt_ctx* ctx, Lane& L, const mpt_render_params* p, uint32_t sample_begin, uint32_t S, PassParams& pp,
                    uint32_t& n_local_tiles, bool time_kernels, const TileOverride* ovr = nullptr, const uint32_t** sky_classes = nullptr) {
    const int tile_mode = tile_order_of(ctx, p);
    int rc = ensure_tile_order(ctx, (uint32_t)p->shard_rank, (uint32_t)p->shard_count, tile_mode, n_local_tiles);
    if (rc) return rc;
    if (ovr) n_local_tiles = ovr->n;
    const uint64_t pass_paths = (uint64_t)n_local_tiles * S * 64ull;
    if (pass_paths >= pass_path_limit(p->pipeline)) return fail(ctx, MPT_ERR_INVALID_ARG, "pass too large (internal)");
    const uint32_t slots_items = pass_slots(p, pass_paths);
    if ((rc = ensure_workspace(ctx, L, slots_items, std::max<uint64_t>(pass_paths, 64), p->pipeline == MPT_PIPE_WAVEFRONT))) return rc;
    if (p->rng_mode == MPT_RNG_LITERAL && (rc = ensure_pixel_seeds(ctx))) return rc;
    if ((rc = fill_pass_params(ctx, L, p, sample_begin, S, tile_mode, ovr, pp))) return rc;
    if (pass_paths == 0) return MPT_OK;
    // test mode: poison the per-path result slots so that a path that is lost shows up as NaN in the image
    if (count_flag(p)) HIPCHK(hipMemsetAsync(L.d_slots.get(), 0xFF, pass_paths * 16, L.stream.get()));

    PassLaunch g;
    g.pipeline = resolve_pipeline(ctx, p->pipeline, p->rng_mode);
    if ((rc = select_trace_kernel(ctx, L, p, n_local_tiles, pp, g))) return rc;
    if ((rc = launch_geometry(ctx, pp, g))) return rc;
    if ((rc = ensure_tile_classes(ctx, L, pp, g))) return rc;
    g.sky_resolve = sky_classes && g.tile_classes && ctx->lean_sky_resolve ? 1u : 0u;
    if (sky_classes) *sky_classes = g.sky_resolve ? g.tile_classes : nullptr;
    if (getenv("MPT_DEBUG_LAUNCH") && g.sky_resolve) fprintf(stderr, "[mpt] sky tiles: summed by the resolve\n");

    *L.h_done.get() = 0;
    if ((rc = order_behind_previous_trace(ctx, L, g.corun))) return rc;
    pp.launch_id = 0u;
    if (g.pipeline == MPT_PIPE_WAVELOCAL || g.pipeline == MPT_PIPE_ORDERED) {
        if (++ctx->launch_seq == 0u) ctx->launch_seq = 1u;
        pp.launch_id = ctx->launch_seq;
    }
    L.announced_id = pp.launch_id;
    hipLaunchKernelGGL(k_begin_pass, dim3(1), dim3(64), 0, L.stream.get(), L.d_desc.get(), L.d_ctr.get(), (uint32_t)pass_paths, slots_items, pp.host_done,
                       g.pipeline == MPT_PIPE_WAVEFRONT ? 0 : 1);
    if (g.pipeline == MPT_PIPE_WAVEFRONT) return launch_wavefront(ctx, L, g, pp, p->max_depth, pass_paths, slots_items, time_kernels);
    return launch_persistent(ctx, L, g, pp, pass_paths, time_kernels);
}

// Statistics: the pass descriptor of a lane is copied to pinned memory behind the lane's last kernel
// (enqueue_stats_copy); collect_lane waits for the lane ONCE and reads the copy and the kernel-event pairs.
static int enqueue_stats_copy(mpt_ctx* ctx, Lane& L) {
    HIPCHK(hipMemcpyAsync(L.h_desc.get(), L.d_desc.get(), sizeof(PassDesc), hipMemcpyDeviceToHost, L.stream.get()));
    HIPCHK(hipMemsetAsync(&L.d_desc.get()->paths, 0, MPT_DESC_COUNTERS * sizeof(unsigned long long), L.stream.get()));
    HIPCHK(hipMemsetAsync(&L.d_desc.get()->overflow, 0, 4, L.stream.get()));
    return MPT_OK;
}

static int collect_lane(mpt_ctx* ctx, Lane& L) {
    HIPCHK(hipStreamSynchronize(L.stream.get()));
    L.in_flight = false;
    const PassDesc& hd = *L.h_desc.get();
    // duration of the trace kernels: what the persistent kernels stamped themselves (first workgroup's start to last wave's end on the
    // 100 MHz clock, note_wave_exit) — the event pairs of overlapping renders include the time a launch waits behind the running kernel
    float ev_ms = 0;
    for (auto& pr : L.pending_timed) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
        ev_ms += ms;
        ctx->stats.trace_launches += 1;
    }
    ctx->stats.trace_kernel_ms += hd.trace_ticks != 0 && !L.pending_timed.empty() ? (double)hd.trace_ticks * 1e-5 : (double)ev_ms;
    L.pending_timed.clear();
    L.ev_used = 0;
    if (L.timed) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, L.ev0.get(), L.ev1.get()));
        ctx->stats.total_ms += ms;
        L.timed = false;
    }
    if (hd.overflow) return fail(ctx, MPT_ERR_OVERFLOW, "ray ring overflow");
    ctx->stats.paths += hd.paths;
    ctx->stats.rays += hd.rays;
    ctx->stats.node_visits += hd.node_visits;
    ctx->stats.aabb_hits += hd.aabb_hits;
    ctx->stats.prim_tests += hd.prim_tests;
    ctx->stats.wave_node_iters += hd.node_iters;
    ctx->stats.wave_prim_iters += hd.prim_iters;
    ctx->stats.wave_leaf_phases += hd.leaf_phases;
    ctx->stats.exact_retraces += hd.flagged;
    ctx->stats.tree_parked += hd.parked;
    return MPT_OK;
}

// Waits for every render still in flight (oldest first) and folds its statistics into ctx->stats.
static int wait_impl(mpt_ctx* ctx) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    int first_rc = MPT_OK;
    for (int k = 0; k < 2; ++k) {
        Lane& L = ctx->lane[(ctx->next_lane + k) & 1];  // next_lane is the older of the two
        if (!L.in_flight) continue;
        int rc = collect_lane(ctx, L);
        if (rc && !first_rc) first_rc = rc;
    }
    return first_rc;
}

// Enqueues one render (all its passes, each followed by its resolve into the HDR sum) on the next lane and returns.
// At most two renders are in flight: the lane is collected first if it is still busy.
static int render_async_impl(mpt_ctx* ctx, const mpt_render_params* p, const TileOverride* ovr = nullptr) {
    int rc = check_ready(ctx, p);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    // a render with another size / sharding rebuilds the shared tile table: nothing may be in flight then
    if (ctx->d_tile_xy && (ctx->tile_W != ctx->W || ctx->tile_H != ctx->H || ctx->tile_rank != (uint32_t)p->shard_rank ||
                           ctx->tile_nranks != (uint32_t)p->shard_count || ctx->tile_mode_built != tile_order_of(ctx, p)) &&
        (rc = wait_impl(ctx)))
        return rc;
    Lane& L = ctx->lane[ctx->next_lane];
    if (L.in_flight && (rc = collect_lane(ctx, L))) return rc;
    if ((p->flags & MPT_FLAG_MOMENTS) && !ctx->d_m2) {   // (first render with moments since the resize: zeroed in stream order)
        const size_t bytes = (size_t)ctx->W * ctx->H * 16;
        HIPCHK(ctx->d_m2.alloc(bytes));
        HIPCHK(hipMemsetAsync(ctx->d_m2.get(), 0, bytes, L.stream.get()));
    }
    HIPCHK(hipEventRecord(L.ev0.get(), L.stream.get()));
    ctx->next_lane ^= 1;
    // from here on, a render that does not get enqueued whole (a HIP error, or a host exception that guarded() turns into a status):
    // drain what it has enqueued, forget its event pairs and give the lane back, so that the next render starts from a clean lane
    // (the HDR sum may hold some of this render's passes: the caller clears it)
    struct Abandon {
        mpt_ctx* ctx;
        Lane& L;
        bool enqueued = false;
        ~Abandon() {
            if (enqueued) return;
            // (the statistics copy that normally clears them never runs for an abandoned render)
            hipMemsetAsync(&L.d_desc.get()->paths, 0, MPT_DESC_COUNTERS * sizeof(unsigned long long), L.stream.get());
            hipMemsetAsync(&L.d_desc.get()->overflow, 0, 4, L.stream.get());
            hipStreamSynchronize(L.stream.get());
            L.pending_timed.clear();
            L.ev_used = 0;
            L.timed = false;
            L.in_flight = false;
            ctx->next_lane ^= 1;
        }
    } abandon{ctx, L};
    const uint32_t tiles = ((ctx->W + 7) / 8) * ((ctx->H + 7) / 8);
    const uint32_t local_tiles = ovr ? ovr->n : (tiles + p->shard_count - 1) / p->shard_count;
    uint32_t s_max = (uint32_t)std::max<uint64_t>(
        1, (pass_path_limit(p->pipeline) - 64) / ((uint64_t)std::max(1u, local_tiles) * 64ull));
    if (p->pipeline == MPT_PIPE_WAVEFRONT && s_max > 64) s_max = 64;
    if (s_max > 0x07FFFFFFu) s_max = 0x07FFFFFFu;
    {   // keep the samples per pass a power of two when possible (division-free path -> pixel)
        uint32_t pow2 = 1;
        while (pow2 * 2 <= s_max) pow2 *= 2;
        if (p->sample_count >= pow2) s_max = pow2;
    }
    const char* e = getenv("MPT_PASS_SPP");
    if (e && atoi(e) > 0) s_max = std::min<uint32_t>(s_max, (uint32_t)atoi(e));
    uint32_t done = 0;
    while (done < p->sample_count) {
        uint32_t S = std::min(s_max, p->sample_count - done);
        PassParams pp;
        uint32_t nlt = 0;
        const uint32_t* sky_classes = nullptr;
        rc = run_pass(ctx, L, p, p->sample_begin + done, S, pp, nlt, ctx->time_kernels, ovr, &sky_classes);
        if (rc) return rc;
        if (nlt) {
            // sum[p] += pass total must happen in submission order on both lanes (float addition does not commute
            // bit for bit): this resolve waits for the previous one, wherever it ran
            if (ctx->last_resolved) HIPCHK(hipStreamWaitEvent(L.stream.get(), ctx->last_resolved, 0));
            // beside the other lane's trace kernel: a footprint that fits next to it on every CU (k_resolve_sum); alone: the whole chip
            const uint32_t threads = nlt * 64u, wide = (threads + 255u) / 256u;
            const uint32_t narrow = (uint32_t)ctx->prop.multiProcessorCount * (uint32_t)ctx->resolve_wgs_per_cu;
            const uint32_t rgrid = !ctx->sync_render && ctx->resolve_wgs_per_cu > 0 ? std::min(wide, narrow) : wide;
            if (p->flags & MPT_FLAG_MOMENTS)
                hipLaunchKernelGGL(k_resolve_sum_moments, dim3(rgrid), dim3(256), 0, L.stream.get(), pp, ctx->d_sum, ctx->d_m2.get(), nlt, sky_classes);
            else
                hipLaunchKernelGGL(k_resolve_sum, dim3(rgrid), dim3(256), 0, L.stream.get(), pp, ctx->d_sum, nlt, sky_classes);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(L.ev_resolved.get(), L.stream.get()));
            ctx->last_resolved = L.ev_resolved.get();
        }
        done += S;
        // the next pass reuses the lane's slot buffer and descriptor: in-stream order is enough, no host sync here
    }
    HIPCHK(hipEventRecord(L.ev1.get(), L.stream.get()));
    L.timed = true;
    if ((rc = enqueue_stats_copy(ctx, L))) return rc;
    L.in_flight = true;
    abandon.enqueued = true;
    return MPT_OK;
}

// "Nothing else is in flight and nothing will be submitted behind this render": the trace kernel may be the variant that fills the
// scalar register file and the resolve may take the whole chip.  Set for the duration of mpt_render / mpt_draw; a guard, so that no
// exit path (an exception turned into a status by guarded()) leaves it set.
namespace {
struct SyncRenderScope {
    mpt_ctx* ctx;
    explicit SyncRenderScope(mpt_ctx* c) : ctx(c) { ctx->sync_render = true; }
    ~SyncRenderScope() { ctx->sync_render = false; }
    SyncRenderScope(const SyncRenderScope&) = delete;
    SyncRenderScope& operator=(const SyncRenderScope&) = delete;
};
}  // namespace
static int render_impl(mpt_ctx* ctx, const mpt_render_params* p) {
    int rc = wait_impl(ctx);
    if (rc) return rc;
    ctx->stats.trace_kernel_ms = 0;   // the synchronous call reports its own timings
    ctx->stats.trace_launches = 0;
    ctx->stats.total_ms = 0;
    ctx->next_lane = 0;  // nothing is in flight: serial renders stay on lane 0 (the second lane allocates only if used)
    {
        SyncRenderScope sync(ctx);
        rc = render_async_impl(ctx, p);
    }
    if (rc) return rc;
    return wait_impl(ctx);
}

static int draw_impl(mpt_ctx* ctx, const mpt_render_params* p) {
    int rc = check_ready(ctx, p);
    if (rc) return rc;
    if ((rc = wait_impl(ctx))) return rc;
    SyncRenderScope sync(ctx);   // (the frame protocol is synchronous: one frame at a time, collected before the call returns)
    Lane& L = ctx->lane[0];
    ctx->cur_target ^= 1;  // std::swap(_accumulationTargets[0], [1]) — Renderer.cpp:278
    PassParams pp;
    uint32_t nlt = 0;
    rc = run_pass(ctx, L, p, p->sample_begin, 1, pp, nlt, false);
    if (rc) return rc;
    if (nlt) {
        uint32_t threads = nlt * 64u;
        hipLaunchKernelGGL(k_resolve_frame, dim3((threads + 255) / 256), dim3(256), 0, L.stream.get(), pp,
                           (const float4*)ctx->d_accum[ctx->cur_target ^ 1].get(), ctx->d_accum[ctx->cur_target].get(), nlt,
                           (unsigned long long)ctx->u.frameCount);
        HIPCHK(hipGetLastError());
    }
    if ((rc = enqueue_stats_copy(ctx, L))) return rc;
    return collect_lane(ctx, L);
}

// ---- adaptive sampling (mpt_adaptive.h; the contract is in include/mpt.h) ----------------------------------------------------
static int read_moments_impl(mpt_ctx* ctx, float* out) {
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    int rc = wait_impl(ctx);
    if (rc) return rc;
    const size_t bytes = (size_t)ctx->W * ctx->H * 16;
    if (!ctx->d_m2) {   // (no render with moments since the resize)
        memset(out, 0, bytes);
        return MPT_OK;
    }
    HIPCHK(hipMemcpyAsync(out, ctx->d_m2.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int read_tile_samples_impl(mpt_ctx* ctx, uint32_t* out) {
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    int rc = wait_impl(ctx);
    if (rc) return rc;
    const size_t n = (size_t)((ctx->W + 7) / 8) * ((ctx->H + 7) / 8);
    if (!ctx->ad.tile_count) {   // (no adaptive render since the resize)
        memset(out, 0, n * 4);
        return MPT_OK;
    }
    HIPCHK(hipMemcpyAsync(out, ctx->ad.tile_count.get(), n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MPT_OK;
}
static int ensure_adaptive_buffers(mpt_ctx* ctx, uint32_t tiles) {
    AdaptiveTiles& a = ctx->ad;
    if (a.tile_count && a.tiles == tiles) return MPT_OK;
    a = AdaptiveTiles{};
    HIPCHK(a.tile_count.alloc((size_t)tiles * 4));
    HIPCHK(a.alist[0].alloc((size_t)tiles * 4));
    HIPCHK(a.alist[1].alloc((size_t)tiles * 4));
    HIPCHK(a.aflag.alloc(tiles));
    HIPCHK(a.nsel.alloc(4));
    size_t tmp = 0;
    HIPCHK(hipcub::DeviceSelect::Flagged(nullptr, tmp, a.alist[0].get(), a.aflag.get(), a.alist[1].get(), a.nsel.get(), (int)tiles,
                                         ctx->stream));
    HIPCHK(a.sel_tmp.alloc(std::max<size_t>(tmp, 16)));
    a.sel_tmp_bytes = tmp;
    a.tiles = tiles;
    return MPT_OK;
}
static int render_adaptive_impl(mpt_ctx* ctx, const mpt_render_params* p, const mpt_adaptive_params* a, mpt_adaptive_info* out) {
    const uint32_t N = p->sample_count;
    if (p->rng_mode == MPT_RNG_LITERAL) return fail(ctx, MPT_ERR_INVALID_ARG, "adaptive render with the literal RNG (no per-sample variance)");
    if (p->shard_count != 1) return fail(ctx, MPT_ERR_INVALID_ARG, "adaptive render with shard_count != 1");
    if (a->min_samples == 1u || !(a->threshold >= 0.0f) || N < 2u)
        return fail(ctx, MPT_ERR_INVALID_ARG, "bad adaptive params (min_samples 1, threshold < 0 or NaN, or sample_count < 2)");
    int rc = check_ready(ctx, p);
    if (rc) return rc;
    if ((rc = wait_impl(ctx))) return rc;   // (reports a failed mpt_render_async)
    const uint32_t min_s = a->min_samples ? a->min_samples : MPT_ADAPTIVE_DEFAULT_MIN_SAMPLES;
    const uint32_t batch = a->batch_samples ? a->batch_samples : MPT_ADAPTIVE_DEFAULT_BATCH;
    const float floor_l = a->luminance_floor > 0.0f ? a->luminance_floor : MPT_ADAPTIVE_DEFAULT_LUMINANCE_FLOOR;
    const uint32_t tiles_x = (ctx->W + 7) / 8, tiles_y = (ctx->H + 7) / 8, tiles = tiles_x * tiles_y;
    if ((rc = ensure_adaptive_buffers(ctx, tiles))) return rc;
    if ((rc = clear_sum_impl(ctx))) return rc;   // (the sum, and the moments if they exist yet: ordered before the first resolve)
    HIPCHK(hipMemsetAsync(ctx->ad.tile_count.get(), 0, (size_t)tiles * 4, ctx->stream));
    ctx->stats.trace_kernel_ms = 0;   // (totals over the passes, as one mpt_render reports its own)
    ctx->stats.trace_launches = 0;
    ctx->stats.total_ms = 0;
    mpt_render_params q = *p;
    q.flags |= MPT_FLAG_MOMENTS;
    uint32_t n = 0, passes = 0, n_active = 0, cur = 0;
    const uint32_t* list = nullptr;   // pass 0: the full tile table itself
    for (;;) {
        const uint32_t n_next = passes == 0 ? std::min(min_s, N) : (uint32_t)std::min<uint64_t>((uint64_t)n + batch, N);
        q.sample_begin = p->sample_begin + n;
        q.sample_count = n_next - n;
        ctx->next_lane = 0;   // every pass on lane 0, whose stream is ctx->stream: the evaluation below follows its resolve in stream order
        {
            SyncRenderScope sync(ctx);
            const TileOverride ovr{list, n_active};
            rc = render_async_impl(ctx, &q, list ? &ovr : nullptr);
        }
        if (rc) return rc;
        if ((rc = wait_impl(ctx))) return rc;
        passes++;
        n = n_next;
        if (!list) {
            list = ctx->d_tile_xy.get();   // (built by pass 0; one rank: every tile, in the table's order)
            n_active = ctx->tile_count;
        }
        AdaptiveEval ev;
        ev.list = list;
        ev.n_list = n_active;
        ev.sum = ctx->d_sum;
        ev.m2 = ctx->d_m2.get();
        ev.width = ctx->W;
        ev.height = ctx->H;
        ev.tiles_x = tiles_x;
        ev.n = n;
        ev.n_max = N;
        ev.threshold = (double)a->threshold;
        ev.luminance_floor = (double)floor_l;
        ev.tile_count = ctx->ad.tile_count.get();
        ev.flag = ctx->ad.aflag.get();
        hipLaunchKernelGGL(k_adaptive_eval, dim3((n_active + 3u) / 4u), dim3(256), 0, ctx->stream, ev);
        HIPCHK(hipGetLastError());
        uint32_t* next = ctx->ad.alist[cur].get();
        size_t tmp = ctx->ad.sel_tmp_bytes;
        HIPCHK(hipcub::DeviceSelect::Flagged(ctx->ad.sel_tmp.get(), tmp, list, ctx->ad.aflag.get(), next, ctx->ad.nsel.get(), (int)n_active, ctx->stream));
        uint32_t kept = 0;
        HIPCHK(hipMemcpyAsync(&kept, ctx->ad.nsel.get(), 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (kept == 0u) break;   // (every tile stopped: a tile at N is never flagged)
        if (kept > n_active) return fail(ctx, MPT_ERR_HIP, "adaptive compaction kept more tiles than it was given (internal)");
        list = next;
        n_active = kept;
        cur ^= 1u;
    }
    std::vector<uint32_t> counts(tiles);
    HIPCHK(hipMemcpy(counts.data(), ctx->ad.tile_count.get(), (size_t)tiles * 4, hipMemcpyDeviceToHost));
    mpt_adaptive_info info = {};
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t tx = t % tiles_x, ty = t / tiles_x;
        const uint64_t px = (uint64_t)std::min<uint32_t>(8u, ctx->W - tx * 8u) * std::min<uint32_t>(8u, ctx->H - ty * 8u);
        info.samples += px * counts[t];
        (counts[t] == N ? info.tiles_at_max : info.tiles_converged)++;
    }
    info.passes = passes;
    *out = info;
    return MPT_OK;
}

// The binary tree of the GPU builders (mpt_lbvh.h).  Default: top-down binned SAH over the primitives (as good a tree as the host's
// binned builder).  MPT_GPU_BUILD = ploc: the clustering pass (25 % faster to build, renders 1-7 % slower); lbvh: the plain Karras tree.
static int gpu_builder() {
    const char* e = getenv("MPT_GPU_BUILD");
    if (e && strcmp(e, "lbvh") == 0) return mpt_lbvh::BUILDER_KARRAS;
    if (e && strcmp(e, "ploc") == 0) return mpt_lbvh::BUILDER_PLOC;
    return mpt_lbvh::BUILDER_SAH;
}

// Primitives per leaf of the GPU builders (MPT_LBVH_LEAF = 1..8 overrides).  Scenes that MPT_PIPE_AUTO renders with the
// reference-order kernel (fewer than MPT_AUTO_ORDERED_PRIMS primitives: the tree and a prefix of the primitives live in LDS
// there) get leaves of <= 6 — scene.xml, ms per 256 spp with 2 / 4 / 5 / 6 / 7 / 8: 20.8 / 19.3 / 19.2 / 18.6 / 18.9 / 19.1,
// against 21.3 on the reference's own tree; the closest-first kernel tests every primitive of a leaf it enters and wants them
// small (bunny x20: 12.5 Grays/s with 4, 13.2 with 2).
static int gpu_leaf_max(uint64_t n_prims) {
    if (const char* lm = getenv("MPT_LBVH_LEAF")) return std::min(std::max(atoi(lm), 1), (int)MPT_LBVH_LEAF_MAX);
    return n_prims < MPT_AUTO_ORDERED_PRIMS ? 6 : 2;
}

// ---- build -> render without the host (mpt_devbuild.h) -------------------------------------------------------------------------
static int build_and_upload_impl(mpt_ctx* ctx, const float* prims, const float* mats, uint64_t n_prims, double* device_ms_out) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    if (!prims || !mats || n_prims == 0) return fail(ctx, MPT_ERR_INVALID_ARG, "null or empty primitive / material array");
    if (n_prims >= (1ull << 27)) return fail(ctx, MPT_ERR_BAD_SCENE, "scene too large for the 27-bit leaf encoding");
    {
        int wrc = wait_impl(ctx);  // renders in flight still read the old scene
        if (wrc) return wrc;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t)n_prims;
    // (whether the always list can be used decides the own boxes of the leaves that hold spheres.  The default builder counts the spheres on
    //  the device, in a kernel it runs anyway; a pass of the host over the 48 MB of 1 M primitives was 0.4 ms of the call)
    const int builder = gpu_builder();
    uint32_t n_spheres = 0xFFFFFFFFu;
    if (!(builder == mpt_lbvh::BUILDER_SAH && n > 2)) {
        n_spheres = 0;
        for (uint32_t i = 0; i < n; ++i) n_spheres += (int)prims[12 * (size_t)i + 3] != 1 ? 1u : 0u;
    }
    // the staging buffer of the inputs is kept between builds (<= 1 GiB; a larger one goes when the call ends): allocating and freeing
    // two buffers of 80 MB per build was 0.3 ms of the call
    const size_t in_bytes = (size_t)n * 80;
    DevMem<> too_large;
    DevMem<>& in = in_bytes <= ((size_t)1 << 30) ? ctx->in_block : too_large;
    if (in.bytes() < in_bytes) HIPCHK(in.alloc(in_bytes));
    float4* const d_p = (float4*)in.get();
    float4* const d_m = (float4*)((char*)in.get() + (size_t)n * 48);
    HIPCHK(hipMemcpyAsync(d_p, prims, (size_t)n * 48, hipMemcpyHostToDevice, ctx->stream));
    const int leaf_max = gpu_leaf_max(n);
    Event e0, e1;
    HIPCHK(e0.create(hipEventCreate));
    HIPCHK(e1.create(hipEventCreate));
    hipEventRecord(e0.get(), ctx->stream);
    mpt_devbuild::Built b;
    // (the materials are copied by the build itself, on its second stream, beside the tree build: mpt_devbuild.h build_pass)
    hipError_t e = mpt_devbuild::build(ctx->stream, d_p, d_m, mats, n, leaf_max, builder, n_spheres, b, ctx->build_pool, &ctx->spare_block);
    if (e == hipSuccess) e = hipEventRecord(e1.get(), ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1.get());
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0.get(), e1.get());
    if (e != hipSuccess) return fail(ctx, MPT_ERR_HIP, std::string("GPU BVH build: ") + hipGetErrorString(e));
    if (n_spheres == 0xFFFFFFFFu) n_spheres = b.n_spheres;
    if (b.n_spheres != n_spheres) return fail(ctx, MPT_ERR_HIP, "GPU BVH build: sphere count mismatch (internal)");
    SceneState s;
    s.scene_block = std::move(b.block);
    s.d_nodes = b.nodes;
    s.d_prims = b.prims;
    s.d_mats = b.mats;
    s.d_acc_nodes = b.acc_nodes;
    s.d_refleaf = b.refleaf;
    s.d_refbox = b.refbox;
    s.d_always = b.always;
    s.d_ref_bvh = b.ref_bvh;
    s.d_ref_idx = b.ref_idx;
    s.n_ref_nodes = b.n_nodes;
    s.built_leaf_max = (uint32_t)leaf_max;
    s.n_nodes = b.n_nodes;
    s.n_prims = b.n_prims;
    s.n_mats = b.n_mats;
    s.n_acc_nodes = b.n_acc_nodes;
    s.n_always = b.n_always;
    s.n_ref_leaves = b.n_ref_leaves;
    s.acc_depth = b.acc_depth;
    s.tri_extent = b.tri_extent;
    s.acc_ok = n_spheres <= MPT_ACCEL_MAX_ALWAYS;        // (parent boxes are unions of child boxes: nested by construction)
    s.acc_why = s.acc_ok ? "" : "more than 16 spheres";
    install_scene(ctx, std::move(s));   // (the old scene's block becomes the next build's)
    if (device_ms_out) *device_ms_out = ms;
    return MPT_OK;
}

static int download_bvh_impl(mpt_ctx* ctx, float* bvh_out, uint64_t cap_nodes, uint64_t* n_nodes_out, int32_t* prim_idx_out) {
    if (!ctx || !bvh_out || !n_nodes_out || !prim_idx_out) return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
    if (!ctx->have_scene || !ctx->d_ref_bvh) return fail(ctx, MPT_ERR_NOT_READY, "the scene was not built by mpt_build_and_upload");
    if (cap_nodes < ctx->n_ref_nodes) return fail(ctx, MPT_ERR_INVALID_ARG, "bvh_out too small");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy(bvh_out, ctx->d_ref_bvh, (size_t)ctx->n_ref_nodes * 32, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(prim_idx_out, ctx->d_ref_idx, (size_t)ctx->n_prims * 4, hipMemcpyDeviceToHost));
    *n_nodes_out = ctx->n_ref_nodes;
    return MPT_OK;
}

// ---- mpt_render_async's submit thread (struct Submitter) -------------------------------------------------------------------------
static void submit_thread_main(mpt_ctx* ctx) {
    Submitter& S = *ctx->sub;
    std::unique_lock<std::mutex> lk(S.mu);
    for (;;) {
        S.cv_work.wait(lk, [&] { return S.stop || !S.q.empty(); });
        if (S.q.empty()) return;   // (stop, and nothing left to submit)
        const mpt_render_params p = S.q.front();
        S.q.pop_front();
        S.busy = true;
        lk.unlock();
        int rc = MPT_ERR_HIP;
        try {
            rc = render_async_impl(ctx, &p);
            ctx->async_jobs++;
        } catch (const std::exception& e) {
            try {
                set_err(ctx, std::string("host exception: ") + e.what());
            } catch (...) {
            }
        } catch (...) {
        }
        lk.lock();
        if (rc != MPT_OK && S.rc == MPT_OK) {
            S.rc = rc;
            S.err = ctx->err;
        }
        S.busy = false;
        S.cv_idle.notify_all();
    }
}
// Everything queued has been submitted (and the thread is idle): the context is the caller's alone again.  Returns the first failure of
// a queued render, once.  Called by every entry point except mpt_render_async.
static int drain_submit(mpt_ctx* ctx) {
    if (!ctx || !ctx->sub) return MPT_OK;
    Submitter& S = *ctx->sub;
    if (std::this_thread::get_id() == S.th.get_id()) return MPT_OK;   // (the submit thread itself, inside render_async_impl)
    std::unique_lock<std::mutex> lk(S.mu);
    S.cv_idle.wait(lk, [&] { return S.q.empty() && !S.busy; });
    const int rc = S.rc;
    if (rc != MPT_OK) {
        set_err(ctx, S.err);
        S.rc = MPT_OK;
        S.err.clear();
    }
    return rc;
}
static void stop_submit(mpt_ctx* ctx) {
    if (!ctx || !ctx->sub) return;
    {
        std::lock_guard<std::mutex> lk(ctx->sub->mu);
        ctx->sub->stop = true;
    }
    ctx->sub->cv_work.notify_all();
    if (ctx->sub->th.joinable()) ctx->sub->th.join();   // (queued renders are submitted first: the thread leaves on an empty queue)
    ctx->sub.reset();
}
static int enqueue_render(mpt_ctx* ctx, const mpt_render_params* p) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = check_ready(ctx, p);   // argument and state errors are the caller's, at once (the state they depend on only changes in calls that drain)
    if (rc) return rc;
    if (!ctx->sub) {
        ctx->sub.reset(new Submitter());
        ctx->sub->th = std::thread(submit_thread_main, ctx);
    }
    Submitter& S = *ctx->sub;
    {
        std::unique_lock<std::mutex> lk(S.mu);
        S.cv_idle.wait(lk, [&] { return S.q.size() < MPT_ASYNC_QUEUE_MAX; });
        S.q.push_back(*p);
    }
    S.cv_work.notify_one();
    const uint64_t us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    ctx->async_call_us_max = std::max(ctx->async_call_us_max, us);
    return MPT_OK;
}

// ---- exception barrier: nothing thrown by the host-side containers may cross the C ABI (include/mpt.h) --------
// (and the join point of the submit thread: every guarded entry point first waits until the renders queued by mpt_render_async have
//  been submitted — DRAIN = false for mpt_render_async itself)
template <bool DRAIN = true, class F>
static int guarded(mpt_ctx* ctx, F&& body) noexcept {
    try {
        if (DRAIN) {
            const int d = drain_submit(ctx);
            if (d) return d;
        }
        return body();
    } catch (const std::exception& e) {
        if (ctx) {
            try {
                set_err(ctx, std::string("host exception: ") + e.what());
            } catch (...) {
            }
        }
        return MPT_ERR_HIP;
    } catch (...) {
        return MPT_ERR_HIP;
    }
}

extern "C" int mpt_create(int device_ordinal, mpt_ctx** out) {
    return guarded(nullptr, [&] { return create_impl(device_ordinal, out); });
}

extern "C" int mpt_upload_scene(mpt_ctx* ctx, const float* bvh, uint64_t n_nodes, const float* prims, const float* mats, const int32_t* prim_idx, uint64_t n_prims) {
    return guarded(ctx, [&] { return upload_scene_impl(ctx, bvh, n_nodes, prims, mats, prim_idx, n_prims); });
}

extern "C" int mpt_set_uniforms(mpt_ctx* ctx, const mpt_uniforms* u) {
    return guarded(ctx, [&] { return set_uniforms_impl(ctx, u); });
}

extern "C" int mpt_resize(mpt_ctx* ctx, uint32_t width, uint32_t height) {
    return guarded(ctx, [&] { return resize_impl(ctx, width, height); });
}

extern "C" int mpt_clear_sum(mpt_ctx* ctx) {
    return guarded(ctx, [&] { return clear_sum_impl(ctx); });
}

extern "C" int mpt_read_frame(mpt_ctx* ctx, float* out) {
    return guarded(ctx, [&] { return read_frame_impl(ctx, out); });
}

extern "C" int mpt_read_sum(mpt_ctx* ctx, float* out) {
    return guarded(ctx, [&] { return read_sum_impl(ctx, out); });
}

// The inverse: the HDR sum of an earlier run goes back in (checkpoint / resume of the accumulation: with the sample index the
// caller continues from, the resumed render is bit-identical to an uninterrupted one — sum[p] += sample_s in sample order either way).
static int write_sum_impl(mpt_ctx* ctx, const float* in) {
    if (!ctx || !in) return MPT_ERR_INVALID_ARG;
    if (!ctx->d_sum) return fail(ctx, MPT_ERR_NOT_READY, "mpt_resize not called");
    int wrc = wait_impl(ctx);
    if (wrc) return wrc;
    HIPCHK(hipMemcpyAsync(ctx->d_sum, in, (size_t)ctx->W * ctx->H * 16, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev_sum_op.get(), ctx->stream));   // the next resolve (on either lane) is ordered behind the upload
    ctx->last_resolved = ctx->ev_sum_op.get();
    HIPCHK(hipStreamSynchronize(ctx->stream));             // (the host array may be freed on return)
    return MPT_OK;
}
extern "C" int mpt_write_sum(mpt_ctx* ctx, const float* rgba_host) {
    return guarded(ctx, [&] { return write_sum_impl(ctx, rgba_host); });
}

extern "C" int mpt_render(mpt_ctx* ctx, const mpt_render_params* p) {
    return guarded(ctx, [&] { return render_impl(ctx, p); });
}
extern "C" int mpt_render_async(mpt_ctx* ctx, const mpt_render_params* p) {
    return guarded<false>(ctx, [&] { return enqueue_render(ctx, p); });
}
extern "C" int mpt_render_adaptive(mpt_ctx* ctx, const mpt_render_params* p, const mpt_adaptive_params* a, mpt_adaptive_info* out) {
    if (!ctx || !p || !a || !out) return MPT_ERR_INVALID_ARG;   // (before anything touches the context or a device)
    return guarded(ctx, [&] { return render_adaptive_impl(ctx, p, a, out); });
}
extern "C" int mpt_read_moments(mpt_ctx* ctx, float* rgba_host) {
    if (!ctx || !rgba_host) return MPT_ERR_INVALID_ARG;
    return guarded(ctx, [&] { return read_moments_impl(ctx, rgba_host); });
}
extern "C" int mpt_read_tile_samples(mpt_ctx* ctx, uint32_t* counts) {
    if (!ctx || !counts) return MPT_ERR_INVALID_ARG;
    return guarded(ctx, [&] { return read_tile_samples_impl(ctx, counts); });
}
extern "C" int mpt_async_info(mpt_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return MPT_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        const uint64_t v[4] = {ctx->async_jobs, ctx->gate_resident, ctx->gate_timeout, ctx->async_call_us_max};
        memcpy(out, v, sizeof v);
        return (int)MPT_OK;
    });
}
extern "C" int mpt_wait(mpt_ctx* ctx) {
    return guarded(ctx, [&] { return wait_impl(ctx); });
}

extern "C" int mpt_draw(mpt_ctx* ctx, const mpt_render_params* p) {
    return guarded(ctx, [&] { return draw_impl(ctx, p); });
}

extern "C" int mpt_accel_info(mpt_ctx* ctx, uint64_t out[8]) {
    if (!ctx || !out) return MPT_ERR_INVALID_ARG;
    if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
    const uint64_t v[8] = {ctx->acc_ok ? 1u : 0u, ctx->n_acc_nodes, ctx->acc_depth, ctx->ot_pt[ordered_point(ctx, false)].lds_nodes, ctx->n_always, ctx->n_ref_leaves, ctx->ot_pt[ordered_point(ctx, false)].lds_prims,
                           (uint64_t)resolve_pipeline(ctx, MPT_PIPE_AUTO)};
    memcpy(out, v, sizeof v);
    return MPT_OK;
}

extern "C" int mpt_gpu_leaf_max(uint64_t n_prims) { return gpu_leaf_max(n_prims); }

// ---- the post-processing stages: guide pass and denoiser, ambient occlusion, temporal accumulation, SVGF, display ----------------------
#include "mpt_post.h"

// ---- the ray queries: closest hit and any hit for caller rays, their timing hook, the known-answer kernels --------------------------
#include "mpt_query.h"

// ---- next-event estimation (mpt_nee.h; the estimator is specified in include/mpt.h) -------------------------------------------------
// One launch of k_nee<WALK> over the whole image on ctx->stream, synchronous like mpt_render: the renders in flight are collected first,
// the light table is built if stale, the kernel adds its samples onto the HDR sum in place.
// The two NEE renders (mpt_render_nee and mpt_render_nee_adaptive, mpt_nee_adaptive.h) share their host steps:
//   nee_check_params  what both refuse in p and n, before anything is waited for or touched
//   nee_ready         the renders in flight collected, the context ready, the light table built, the four totals zeroed on the stream
//   nee_fill_pass     the NeePass of p and n
//   nee_launch        the kernel of the walk and of `cone` between the two timing events
//   nee_collect       the totals read back (this synchronises), the statistics and the info
static int nee_check_params(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n) {
    if (!ctx) return MPT_ERR_INVALID_ARG;
    if (!p || !n) return fail(ctx, MPT_ERR_INVALID_ARG, "null render or NEE params");
    if (p->rng_mode != MPT_RNG_PHILOX) return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: rng_mode must be MPT_RNG_PHILOX");
    if (p->bsdf_mode != MPT_BSDF_LAMBERT && p->bsdf_mode != MPT_BSDF_SCATTER)
        return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: bsdf_mode must be MPT_BSDF_LAMBERT or MPT_BSDF_SCATTER");
    if (p->shard_count != 1 || p->shard_rank != 0) return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: no shards");
    if (p->flags != 0u) return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: flags must be 0");
    if (p->sample_count == 0u || (uint64_t)p->sample_begin + p->sample_count > (1ull << 27))
        return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: sample_count 0 or samples beyond 2^27");
    if (p->max_depth < 1 || p->max_depth > 32) return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: max_depth outside 1..32");
    if (!walk_valid(n->walk)) return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: bad walk");
    if (n->clamp != n->clamp) return fail(ctx, MPT_ERR_INVALID_ARG, "NEE render: NaN clamp");
    return MPT_OK;
}
static int nee_ready(mpt_ctx* ctx) {
    int rc = wait_impl(ctx);
    if (rc) return rc;
    if (!ctx->have_scene || !ctx->have_uniforms || !ctx->W) return fail(ctx, MPT_ERR_NOT_READY, "scene, uniforms or size not set");
    if ((uint32_t)ctx->u.screenSize[0] != ctx->W || (uint32_t)ctx->u.screenSize[1] != ctx->H)
        return fail(ctx, MPT_ERR_INVALID_ARG, "uniforms.screenSize does not match mpt_resize");
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = ensure_lights(ctx))) return rc;
    NeeState& ns = ctx->nee;
    if (!ns.totals) {
        HIPCHK(ns.totals.alloc(32));
        HIPCHK(ns.e0.create(hipEventCreate));
        HIPCHK(ns.e1.create(hipEventCreate));
    }
    HIPCHK(hipMemsetAsync(ns.totals.get(), 0, 32, ctx->stream));
    return MPT_OK;
}
static void nee_fill_pass(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, NeePass& P) {
    P.sum = ctx->d_sum;
    P.totals = ctx->nee.totals.get();
    P.lights = ctx->lights.rec.get();
    P.cdf = ctx->lights.cdf.get();
    P.ids = ctx->lights.d_ids.get();
    P.n_lights = ctx->lights.n();
    float key[14];
    guide_key(ctx->u, key);
    pass_frame(P, key, ctx->W, ctx->H, *p);
    P.fW = key[12];   // uniforms.screenSize itself, as gen_primary divides by it (nee_ready compares it with (W, H) as integers)
    P.fH = key[13];
    P.bsdf_mode = p->bsdf_mode;
    P.max_depth = p->max_depth;
    P.primitive_count = (uint32_t)std::min<uint64_t>(ctx->u.primitiveCount, 0xFFFFFFFFull);
    P.clamp = n->clamp > 0.0f ? n->clamp : INFINITY;
}
template <class Pass>
static int nee_launch(mpt_ctx* ctx, int32_t walk, bool cone, const WalkKernel<Pass> k_area[3], const WalkKernel<Pass> k_cone[3], const Pass& P) {
    HIPCHK(hipEventRecord(ctx->nee.e0.get(), ctx->stream));
    const int rc = tile_walk_launch(ctx, ctx->W, ctx->H, walk, cone ? k_cone : k_area, P);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ctx->nee.e1.get(), ctx->stream));
    return MPT_OK;
}
static int nee_collect(mpt_ctx* ctx, mpt_nee_info* out) {
    NeeState& ns = ctx->nee;
    unsigned long long totals[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(totals, ns.totals.get(), 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ns.e0.get(), ns.e1.get()));
    ctx->stats.paths += totals[0];
    ctx->stats.rays += totals[1];
    ctx->stats.trace_kernel_ms = (double)ms;
    ctx->stats.total_ms = (double)ms;
    ctx->stats.trace_launches = 1;
    if (out) {
        out->paths = totals[0];
        out->rays = totals[1];
        out->shadow_rays = totals[2];
        out->shadow_rays_occluded = totals[3];
        out->lights = ctx->lights.n();
        out->device_ms = (double)ms;
    }
    return MPT_OK;
}
static int render_nee_impl(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, mpt_nee_info* out) {
    int rc = nee_check_params(ctx, p, n);
    if (rc) return rc;
    const uint32_t m = ctx->light_candidates;   // (read at the start)
    if ((rc = nee_ready(ctx))) return rc;
    NeePass P = {};
    nee_fill_pass(ctx, p, n, P);
    static const WalkKernel<NeePass> area[3] = {k_nee<MPT_AO_REF>, k_nee<MPT_AO_REF_ALL_LDS>, k_nee<MPT_AO_OWN>},
                                     cone[3] = {k_nee_cone<MPT_AO_REF>, k_nee_cone<MPT_AO_REF_ALL_LDS>, k_nee_cone<MPT_AO_OWN>};
    const bool use_cone = ctx->light_sampling == MPT_LIGHT_SAMPLING_CONE;
    if (m == 1u) {   // today's kernels, bit for bit
        if ((rc = nee_launch(ctx, n->walk, use_cone, area, cone, P))) return rc;
    } else {         // the same render with the vertex's light sample resampled from m candidates (mpt_ris.h)
        static const WalkKernel<NeeRisPass> ris_area[3] = {k_nee_ris<MPT_AO_REF>, k_nee_ris<MPT_AO_REF_ALL_LDS>, k_nee_ris<MPT_AO_OWN>},
                                            ris_cone[3] = {k_nee_ris_cone<MPT_AO_REF>, k_nee_ris_cone<MPT_AO_REF_ALL_LDS>, k_nee_ris_cone<MPT_AO_OWN>};
        NeeRisPass R = {P, m};
        if ((rc = nee_launch(ctx, n->walk, use_cone, ris_area, ris_cone, R))) return rc;
    }
    return nee_collect(ctx, out);
}
extern "C" int mpt_render_nee(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, mpt_nee_info* out) {
    return guarded(ctx, [&] { return render_nee_impl(ctx, p, n, out); });
}

// mpt_render_nee_adaptive: ONE launch of k_nee_adaptive<WALK> over the whole image.  Every wave renders its tile up to the quota of
// mpt_render_adaptive's schedule, applies the stopping rule itself and goes on or stops (mpt_nee_adaptive.h); the host clears the three
// buffers before the launch and derives the info from the tile counts after it.
static int render_nee_adaptive_impl(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, const mpt_adaptive_params* a,
                                    mpt_adaptive_info* out, mpt_nee_info* nee_out) {
    int rc = nee_check_params(ctx, p, n);
    if (rc) return rc;
    if (!a) return fail(ctx, MPT_ERR_INVALID_ARG, "null adaptive params");
    if (ctx->light_candidates != 1u)   // (the adaptive loop draws k_nee's one sample: a loop with ris_pick in it is not written yet)
        return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_render_nee_adaptive: light candidates must be 1 (mpt_set_light_candidates)");
    const uint32_t N = p->sample_count;
    if (a->min_samples == 1u || !(a->threshold >= 0.0f) || N < 2u)
        return fail(ctx, MPT_ERR_INVALID_ARG, "bad adaptive params (min_samples 1, threshold < 0 or NaN, or sample_count < 2)");
    const bool cone = ctx->light_sampling == MPT_LIGHT_SAMPLING_CONE;   // (read at the start, as mpt_render_nee reads it)
    if ((rc = nee_ready(ctx))) return rc;
    const uint32_t tiles_x = (ctx->W + 7) / 8, tiles_y = (ctx->H + 7) / 8, tiles = tiles_x * tiles_y;
    if ((rc = ensure_adaptive_buffers(ctx, tiles))) return rc;
    if (!ctx->d_m2) HIPCHK(ctx->d_m2.alloc((size_t)ctx->W * ctx->H * 16));   // (cleared with the sum, next)
    if ((rc = clear_sum_impl(ctx))) return rc;
    HIPCHK(hipMemsetAsync(ctx->ad.tile_count.get(), 0, (size_t)tiles * 4, ctx->stream));
    NeeAdaptivePass A = {};
    nee_fill_pass(ctx, p, n, A.nee);
    A.m2 = ctx->d_m2.get();
    A.tile_count = ctx->ad.tile_count.get();
    A.tiles_x = tiles_x;
    A.min_samples = a->min_samples ? a->min_samples : MPT_ADAPTIVE_DEFAULT_MIN_SAMPLES;
    A.batch = a->batch_samples ? a->batch_samples : MPT_ADAPTIVE_DEFAULT_BATCH;
    A.threshold = a->threshold;
    A.floor = a->luminance_floor > 0.0f ? a->luminance_floor : MPT_ADAPTIVE_DEFAULT_LUMINANCE_FLOOR;
    static const WalkKernel<NeeAdaptivePass> k_area[3] = {k_nee_adaptive<MPT_AO_REF>, k_nee_adaptive<MPT_AO_REF_ALL_LDS>,
                                                          k_nee_adaptive<MPT_AO_OWN>},
                                             k_cone[3] = {k_nee_adaptive_cone<MPT_AO_REF>, k_nee_adaptive_cone<MPT_AO_REF_ALL_LDS>,
                                                          k_nee_adaptive_cone<MPT_AO_OWN>};
    if ((rc = nee_launch(ctx, n->walk, cone, k_area, k_cone, A))) return rc;
    if ((rc = nee_collect(ctx, nee_out))) return rc;
    std::vector<uint32_t> counts(tiles);
    HIPCHK(hipMemcpy(counts.data(), ctx->ad.tile_count.get(), (size_t)tiles * 4, hipMemcpyDeviceToHost));
    const uint32_t n0 = std::min(A.min_samples, N);
    mpt_adaptive_info info = {};
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t tx = t % tiles_x, ty = t / tiles_x, c = counts[t];
        const uint64_t px = (uint64_t)std::min<uint32_t>(8u, ctx->W - tx * 8u) * std::min<uint32_t>(8u, ctx->H - ty * 8u);
        info.samples += px * c;
        (c == N ? info.tiles_at_max : info.tiles_converged)++;
        // the schedule steps this tile took, the first included: n_0, then batches up to its count
        const uint32_t steps = c <= n0 ? 1u : 1u + (uint32_t)(((uint64_t)(c - n0) + A.batch - 1u) / A.batch);
        info.passes = std::max(info.passes, steps);
    }
    if (out) *out = info;
    return MPT_OK;
}
extern "C" int mpt_render_nee_adaptive(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, const mpt_adaptive_params* a,
                                       mpt_adaptive_info* out, mpt_nee_info* nee_out) {
    return guarded(ctx, [&] { return render_nee_adaptive_impl(ctx, p, n, a, out, nee_out); });
}
// How mpt_direct_lighting, mpt_direct_image and mpt_render_nee sample a sphere light: host state of the context alone — no scene call,
// mpt_resize or mpt_clear_sum touches it, and the light table does not depend on it.
extern "C" int mpt_set_light_sampling(mpt_ctx* ctx, int32_t mode) {
    return guarded(ctx, [&]() -> int {
        if (!ctx) return MPT_ERR_INVALID_ARG;
        if (mode != MPT_LIGHT_SAMPLING_AREA && mode != MPT_LIGHT_SAMPLING_CONE)
            return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_set_light_sampling: mode must be MPT_LIGHT_SAMPLING_AREA or MPT_LIGHT_SAMPLING_CONE");
        ctx->light_sampling = mode;
        return MPT_OK;
    });
}
extern "C" int mpt_get_light_sampling(mpt_ctx* ctx, int32_t* mode) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !mode) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
        *mode = ctx->light_sampling;
        return MPT_OK;
    });
}
// How many candidates a light sample of those three calls is resampled from: host state with the life of the light-sampling mode.
extern "C" int mpt_set_light_candidates(mpt_ctx* ctx, uint32_t m) {
    return guarded(ctx, [&]() -> int {
        if (!ctx) return MPT_ERR_INVALID_ARG;
        if (m == 0u || m > MPT_LIGHT_CANDIDATES_MAX)
            return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_set_light_candidates: m must be in 1..MPT_LIGHT_CANDIDATES_MAX (32)");
        ctx->light_candidates = m;
        return MPT_OK;
    });
}
extern "C" int mpt_get_light_candidates(mpt_ctx* ctx, uint32_t* m) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !m) return fail(ctx, MPT_ERR_INVALID_ARG, "null argument");
        *m = ctx->light_candidates;
        return MPT_OK;
    });
}

// Position-sensitive 64-bit digest of a device array of 32-bit words: sum over i of splitmix64(i << 32 | word[i]) (a commutative sum, so
// the order in which the waves add is free).  What the tests compare two builds of a scene by, array by array (mpt_scene_digest).
__global__ void k_digest(const uint32_t* w, uint64_t n_words, unsigned long long* out) {
    unsigned long long acc = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long z = (i << 32 | w[i]) + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        acc += z ^ (z >> 31);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63u) == 0) atomicAdd(out, acc);
}
// The nine device arrays of the scene as 32-bit words, in the order of mpt_scene_digest's first nine words (and of mpt_read_scene_array's `which`)
struct SceneArray {
    const void* p;
    uint64_t words;
};
static void scene_arrays(const mpt_ctx* ctx, SceneArray a[9]) {
    const bool built = ctx->d_ref_bvh != nullptr;
    const SceneArray v[9] = {
        {ctx->d_nodes, (uint64_t)ctx->n_nodes * 8}, {ctx->d_prims, (uint64_t)ctx->n_prims * 12}, {ctx->d_mats, (uint64_t)ctx->n_mats * 8},
        {ctx->d_acc_nodes, (uint64_t)ctx->n_acc_nodes * MPT_OT_NODE_STRIDE * 4}, {ctx->d_refleaf, (uint64_t)ctx->n_ref_leaves * 8},
        {ctx->d_refbox, ctx->d_refbox ? (uint64_t)ctx->n_prims * 8 : 0u}, {ctx->d_always, (uint64_t)ctx->n_always * 20},
        {ctx->d_ref_bvh, built ? (uint64_t)ctx->n_ref_nodes * 8 : 0u}, {ctx->d_ref_idx, built ? (uint64_t)ctx->n_prims : 0u}};
    for (int k = 0; k < 9; ++k) a[k] = v[k];
}
extern "C" int mpt_read_scene_array(mpt_ctx* ctx, int which, uint32_t* out, uint64_t capacity_words, uint64_t* n_words_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx) return MPT_ERR_INVALID_ARG;
        if (n_words_out) *n_words_out = 0;
        if (!n_words_out || which < 0 || which > 8) return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_read_scene_array: bad array number or null n_words_out");
        if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
        SceneArray a[9];
        scene_arrays(ctx, a);
        const uint64_t words = a[which].p ? a[which].words : 0u;
        *n_words_out = words;
        if (!out && capacity_words == 0) return MPT_OK;   // the size query
        if (!out || capacity_words < words) return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_read_scene_array: out is null or too small");
        if (words == 0) return MPT_OK;
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemcpyAsync(out, a[which].p, words * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return MPT_OK;
    });
}
// Test hook: the class table of render lane `lane` (0 or 1; -1: the lane of the last trace kernel) as the lane's last pass of a lean ALL_LDS kernel left it, its tiles only (row-major,
// tiles_x * tiles_y words); *builds_out: launches of k_lean_tile_classes in this context so far.  No table: *n_words_out = 0.
extern "C" int mpt_read_lean_tile_classes(mpt_ctx* ctx, int lane, uint32_t* out, uint64_t capacity_words, uint64_t* n_words_out, uint64_t* builds_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx) return MPT_ERR_INVALID_ARG;
        if (n_words_out) *n_words_out = 0;
        if (!n_words_out || lane < -1 || lane > 1) return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_read_lean_tile_classes: bad lane or null n_words_out");
        int rc = drain_submit(ctx);
        if (rc) return rc;
        if ((rc = wait_impl(ctx))) return rc;
        Lane& L = lane >= 0 ? ctx->lane[lane] : ctx->last_trace_lane ? *ctx->last_trace_lane : ctx->lane[0];
        if (builds_out) *builds_out = ctx->tile_class_builds;
        const uint64_t words = L.d_tile_classes && L.tile_key.n_words ? (uint64_t)L.tile_key.view.tiles_x * L.tile_key.view.tiles_y : 0u;
        *n_words_out = words;
        if (!out && capacity_words == 0) return MPT_OK;   // the size query
        if (!out || capacity_words < words) return fail(ctx, MPT_ERR_INVALID_ARG, "mpt_read_lean_tile_classes: out is null or too small");
        if (words == 0) return MPT_OK;
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemcpyAsync(out, L.d_tile_classes.get(), words * 4, hipMemcpyDeviceToHost, L.stream.get()));
        HIPCHK(hipStreamSynchronize(L.stream.get()));
        return MPT_OK;
    });
}
extern "C" int mpt_scene_digest(mpt_ctx* ctx, uint64_t out[16]) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !out) return MPT_ERR_INVALID_ARG;
        if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
        HIPCHK(hipSetDevice(ctx->device));
        SceneArray a[9];
        scene_arrays(ctx, a);
        DevMem<> d;
        HIPCHK(d.alloc(16 * 8));
        HIPCHK(hipMemsetAsync(d.get(), 0, 16 * 8, ctx->stream));
        for (int k = 0; k < 9; ++k)
            if (a[k].p && a[k].words) {
                const uint32_t g = (uint32_t)std::min<uint64_t>((a[k].words + 255) / 256, 2048);
                hipLaunchKernelGGL(k_digest, dim3(g), dim3(256), 0, ctx->stream, (const uint32_t*)a[k].p, a[k].words, (unsigned long long*)d.get() + k);
            }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, d.get(), 16 * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const uint64_t counts[7] = {ctx->n_nodes, ctx->n_prims, ctx->n_mats, ctx->n_acc_nodes, ctx->n_ref_leaves, ctx->n_always, ctx->acc_depth};
        for (int k = 0; k < 7; ++k) out[9 + k] = counts[k];
        return MPT_OK;
    });
}

extern "C" int mpt_build_info(mpt_ctx* ctx, uint64_t out[8]) {
    if (!ctx || !out) return MPT_ERR_INVALID_ARG;
    if (!ctx->have_scene) return fail(ctx, MPT_ERR_NOT_READY, "no scene");
    const bool built = ctx->d_ref_bvh != nullptr;
    const uint64_t v[8] = {built ? ctx->n_prims : 0u, built ? ctx->n_ref_nodes : 0u, built ? ctx->built_leaf_max : 0u, MPT_AUTO_ORDERED_PRIMS,
                           ctx->n_prims, ctx->n_nodes, ctx->n_mats, 0u /* (was: nodes left unquantised by round 4's 64-byte node experiment) */};
    memcpy(out, v, sizeof v);
    return MPT_OK;
}

extern "C" int mpt_build_bvh(mpt_ctx* ctx, const float* prims, uint64_t n_prims, float* bvh_out, uint64_t bvh_capacity_nodes,
                             uint64_t* n_nodes_out, int32_t* prim_idx_out, double* device_ms_out) {
    return guarded(ctx, [&]() -> int {
        if (!ctx || !prims || !bvh_out || !n_nodes_out || !prim_idx_out || n_prims == 0 || n_prims >= (1ull << 27))
            return fail(ctx, MPT_ERR_INVALID_ARG, "bad argument");
        if (bvh_capacity_nodes < 2 * n_prims - 1) return fail(ctx, MPT_ERR_INVALID_ARG, "bvh_out must hold 2 * n_prims - 1 nodes");
        HIPCHK(hipSetDevice(ctx->device));
        float ms = 0.0f;
        const int leaf_max = gpu_leaf_max(n_prims);
        hipError_t e = mpt_lbvh::build(ctx->stream, prims, (uint32_t)n_prims, leaf_max, gpu_builder(), bvh_out, n_nodes_out, prim_idx_out, &ms, ctx->build_pool);
        if (e != hipSuccess) return fail(ctx, MPT_ERR_HIP, std::string("GPU BVH build: ") + hipGetErrorString(e));
        if (device_ms_out) *device_ms_out = ms;
        return MPT_OK;
    });
}

extern "C" int mpt_build_and_upload(mpt_ctx* ctx, const float* prims, const float* mats, uint64_t n_prims, double* device_ms_out) {
    return guarded(ctx, [&] { return build_and_upload_impl(ctx, prims, mats, n_prims, device_ms_out); });
}

extern "C" int mpt_download_bvh(mpt_ctx* ctx, float* bvh_out, uint64_t bvh_capacity_nodes, uint64_t* n_nodes_out, int32_t* prim_idx_out) {
    return guarded(ctx, [&] { return download_bvh_impl(ctx, bvh_out, bvh_capacity_nodes, n_nodes_out, prim_idx_out); });
}

// ---- multi-GPU: RCCL reduce of the HDR sum (include/mpt.h) ----------------------------------------------------------
#include "mpt_comm.h"

// ---- diagnostics of the instrumented builds ------------------------------------------------------------------------------------------
#include "mpt_debug.h"
