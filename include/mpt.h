/* mpt.h — C ABI of the MI355X-native path-tracing hot path (libmpt_hip.so).
 *
 * The reference (omkhairate/MetalPathtracer) has no plugin/FFI layer: its seam is the
 * Renderer <-> fragment-shader binding contract (buffers 0..6 + two accumulation textures,
 * R/Renderer/Renderer.cpp:289-301 <-> R/Renderer/Shaders/Fragment.metal:10-18; byte layouts in
 * SURVEY.md App. D).  Every entry point below replaces one piece of that contract; the cited
 * file:line is the reference interface it stands in for.  R/ = "MetalCpp Path Tracer/".
 *
 * Conventions: plain pointers and sizes only; every call returns an mpt_status (0 = ok); no
 * exceptions, printf or assert cross the boundary (the reference printf+assert(false)s,
 * Renderer.cpp:87-91); a context is owned by one host thread and is not thread-safe (the
 * reference is single-threaded).  Host arrays passed in are copied during the
 * call and may be freed immediately (as Renderer.cpp:135,146,214-215 does).
 */
#ifndef MPT_H
#define MPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpt_ctx mpt_ctx;

typedef enum mpt_status {
    MPT_OK = 0,
    MPT_ERR_INVALID_ARG = 1,   /* null pointer, zero size, bad enum                                   */
    MPT_ERR_NO_DEVICE = 2,     /* no HIP device / ordinal out of range: the product never falls back   */
    MPT_ERR_HIP = 3,           /* a HIP runtime call failed (mpt_last_error has the text)              */
    MPT_ERR_BAD_SCENE = 4,     /* BVH/primitive arrays are not a well-formed tree (cycle, range, ...)  */
    MPT_ERR_NOT_READY = 5,     /* render before scene / uniforms / size were set                       */
    MPT_ERR_OVERFLOW = 6       /* internal ray-queue capacity exceeded (a bug; never expected)         */
} mpt_status;

/* UniformsData, 144 bytes — R/Renderer/Shaders/Structs.h:23-41 == R/Renderer/Renderer.cpp:12-28
 * (simd::float3 is 16-byte aligned; offsets in SURVEY.md App. D).                                  */
typedef struct mpt_uniforms {
    int32_t primitiveIndex;        /* off   0  unused by the shader                                  */
    int32_t _pad0[3];
    float cameraPosition[4];       /* off  16                                                        */
    float screenSize[2];           /* off  32                                                        */
    float _pad1[2];
    float viewportU[4];            /* off  48                                                        */
    float viewportV[4];            /* off  64                                                        */
    float firstPixelPosition[4];   /* off  80                                                        */
    float randomSeed[4];           /* off  96  literal RNG: sin-hash parameters (Random.h:32-35)     */
    uint64_t primitiveCount;       /* off 112  material-index guard (PathTracing.h:234-236)          */
    uint64_t triangleCount;        /* off 120  unused by the shader                                  */
    uint64_t frameCount;           /* off 128  running-mean weight (Fragment.metal:23,63)            */
    uint64_t totalPrimitiveCount;  /* off 136  never set by the reference                            */
} mpt_uniforms;

enum { MPT_RNG_LITERAL = 0,  /* bit-faithful to the reference's stuck PCG stream      */
       MPT_RNG_PHILOX = 1 }; /* Philox4x32-10, counter (pixel, sample, bounce, 0): the benchmark RNG  */
enum { MPT_BSDF_LAMBERT = 0, /* what rayColor executes (PathTracing.h:251-255)                        */
       MPT_BSDF_SCATTER = 1, /* + mirror (materialType < 0) / dielectric (> 0 = IOR) per Scatter.h:28-40, which is
                                  dead code in the reference; diffuse surfaces (materialType == 0) keep rayColor's own
                                  bounce (PathTracing.h:251-255).  Own choices, DESIGN.md "RNG / math specification":
                                  pow(x, 5) is a multiply chain and a transmitted ray starts at p - 1e-4 n (the
                                  reference's + n would re-hit the surface).  Two behaviours that follow from the
                                  reference's text and that tests/test_optics_cpu.py pins: (1) the sphere test takes the
                                  near root alone (PathTracing.h:120-142), so a ray that starts inside a sphere does
                                  not see it: a glass sphere refracts on entry only.  (2) a refraction whose
                                  discriminant 1 - ri^2 (1 - cos^2) rounds below zero while ri * sin > 1 is false (a
                                  few 1e-6 rad around the critical angle) returns the zero vector, whose normalize is
                                  a NaN direction; that ray hits nothing, the sample ends as a miss and contributes
                                  (0, 0, 0) with alpha 1 (clamp of a NaN colour is 0).                              */
       MPT_BSDF_SCATTER_ALL = 2 }; /* scatter() for every material: as MPT_BSDF_SCATTER, and diffuse surfaces take
                                  Scatter.h's own Lambert branch too (Scatter.h:24-27,42: normalize(normal +
                                  normalize(randomFloat3(seed))), a point of the cube [-1,1]^3 per Random.h:18-30 —
                                  literal RNG: three draws from a copy of the stuck seed; philox: words 0, 1, 2 of
                                  the bounce's block)                                                               */
enum { MPT_PIPE_WAVEFRONT = 0,  /* global SoA ray queues + wave64 ballot compaction, one kernel/bounce */
       MPT_PIPE_MEGAKERNEL = 1, /* one thread per path, whole bounce loop in registers                */
       MPT_PIPE_WAVELOCAL = 2,  /* persistent waves, wave-private ray rings + ballot compaction; pipelines 0-2 walk
                                   the BVH in the reference's own order (PathTracing.h:188-193)                      */
       MPT_PIPE_ORDERED = 3,    /* the same wave-local wavefront over the product's own 4-wide BVH, closest child
                                   first, with the reference-order walk for the rays whose answer could depend on the
                                   order (falls back to pipeline 2 when a scene's child boxes are not nested in their
                                   parents' or it has more than 16 spheres).  EXACTNESS: it returns the reference's closest
                                   hit for every ray EXCEPT where the reference's own answer is an artefact of its float
                                   arithmetic: a triangle accepted at a computed t that lies in FRONT of the triangle's
                                   bounding box by more than t * 2^-10 — possible only when the ray lies within about
                                   1e-5 / |e1 x e2| radians of the triangle's plane, so that |det| is just above the 1e-5
                                   of PathTracing.h:153 and t = f * dot(e2, q) has lost its digits.  The closest-first
                                   walk culls the box of such a triangle by distance and never computes that t; the
                                   reference does if it happens to visit the leaf first.  Measured: 0 such rays in 1.3e11
                                   rays of rendering (scene.xml, bunny x20, height fields, Cornell); 6e-6 of the rays
                                   AIMED along the planes of 1..30-unit slivers (tests/test_gpu_adversarial.py, which
                                   checks in exact arithmetic that every difference is of this kind).  No affordable
                                   rule closes the gap: pipelines 0-2 reproduce the artefacts too.        */
       MPT_PIPE_AUTO = 4 };     /* pipeline 3 for scenes of MPT_AUTO_ORDERED_PRIMS (8192) primitives or more — where it
                                   is 1.5-2.2x faster — and pipeline 2 below that (scene.xml: pipeline 2 leads by a few
                                   per cent since its box-test loop was rewritten for the scalar unit) and ALWAYS with
                                   MPT_RNG_LITERAL, the mode that exists to reproduce the reference's frames.
                                   mpt_accel_info out[7] tells which of the two AUTO stands for (philox) with the
                                   uploaded scene.                                                                     */
#define MPT_AUTO_ORDERED_PRIMS 8192u

typedef struct mpt_render_params {
    int32_t rng_mode;        /* MPT_RNG_*                                                             */
    int32_t bsdf_mode;       /* MPT_BSDF_*                                                            */
    int32_t max_depth;       /* reference: 32 (PathTracing.h:216)                                     */
    int32_t pipeline;        /* MPT_PIPE_*                                                            */
    uint32_t sample_begin;   /* first sample index of this call (philox counter word 1)               */
    uint32_t sample_count;   /* samples per pixel rendered by this call                               */
    uint32_t seed_lo, seed_hi; /* philox key                                                          */
    int32_t shard_rank;      /* this GPU renders 8x8 pixel tiles t with t % shard_count == shard_rank */
    int32_t shard_count;     /* 1 = whole image                                                       */
    uint32_t slots_per_iter; /* wavefront width (ray slots per iteration); 0 = default                */
    uint32_t flags;          /* MPT_FLAG_*                                                            */
} mpt_render_params;

enum { MPT_FLAG_COUNT_WORK = 1u,   /* also count node visits / primitive tests (slower; for tests)    */
       MPT_FLAG_MOMENTS = 2u };    /* mpt_render / mpt_render_async: also add the per-sample second moments to the
                                      context's moments buffer (mpt_read_moments); mpt_draw ignores it                    */

typedef struct mpt_stats {   /* cumulative since mpt_reset_stats                                      */
    uint64_t paths;          /* primary rays generated                                                */
    uint64_t rays;           /* closest-hit queries (primary + bounce)                                */
    uint64_t node_visits;    /* BVH nodes box-tested       (only with MPT_FLAG_COUNT_WORK)            */
    uint64_t aabb_hits;      /* box tests passed           (only with MPT_FLAG_COUNT_WORK)            */
    uint64_t prim_tests;     /* sphere + triangle tests    (only with MPT_FLAG_COUNT_WORK)            */
    uint64_t iterations;     /* wavefront iterations launched                                         */
    double trace_kernel_ms;  /* HIP-event time of the trace/shade kernels of the last mpt_render      */
    double total_ms;         /* HIP-event time of the whole last mpt_render (all kernels, its stream) */
    uint64_t trace_launches; /* trace/shade kernel launches in the last mpt_render                    */
    /* divergence diagnostics (only with MPT_FLAG_COUNT_WORK): loop trips per WAVE; 64 x trips = issued lane
     * slots, so node_visits / (64 * wave_node_iters) is the lane utilisation of the box-test loop            */
    uint64_t wave_node_iters;   /* box-test loop trips                                                        */
    uint64_t wave_prim_iters;   /* primitive-test loop trips                                                  */
    uint64_t wave_leaf_phases;  /* leaf phases entered                                                        */
    /* MPT_PIPE_ORDERED only */
    uint64_t exact_retraces;    /* rays handed to the reference-order walk (ties, inconsistent winners, ...)          */
    uint64_t tree_parked;       /* rays parked for a full-width tree step after the top test                          */
} mpt_stats;

/* Device selection / lifetime.  Replaces MTL::CreateSystemDefaultDevice + Renderer::Renderer /
 * ~Renderer resource ownership (R/Window/ApplicationDelegate.cpp:33, R/Renderer/Renderer.cpp:43-78). */
int mpt_create(int device_ordinal, mpt_ctx** out);
int mpt_destroy(mpt_ctx* ctx);
const char* mpt_last_error(const mpt_ctx* ctx);     /* text of the last failure on this context      */
const char* mpt_status_string(int status);

/* Fragment buffers 0 (bvhNodes), 1 (primitives), 2 (materials), 6 (primitiveIndices):
 * Renderer::updateVisibleScene / buildBuffers, R/Renderer/Renderer.cpp:127-146,199-215, fed with the
 * arrays Scene::createBVHBuffer / createTransformsBuffer / createMaterialsBuffer /
 * createPrimitiveIndexBuffer return (R/Scene/Scene.h:99-167).  bvh: 2 float4 per node; prims: 3
 * float4 per primitive; mats: 2 float4 per primitive; prim_idx: one int32 per primitive.            */
int mpt_upload_scene(mpt_ctx* ctx, const float* bvh, uint64_t n_nodes, const float* prims, const float* mats,
                     const int32_t* prim_idx, uint64_t n_prims);

/* Fragment buffer 3 (uniforms): Renderer::updateUniforms / recalculateViewport,
 * R/Renderer/Renderer.cpp:153-182,251-267.                                                          */
int mpt_set_uniforms(mpt_ctx* ctx, const mpt_uniforms* u);

/* Textures 0/1 (RGBA32F accumulation targets): Renderer::buildTextures / drawableSizeWillChange,
 * R/Renderer/Renderer.cpp:228-241,312-321.  Clears both targets and the HDR sum.                     */
int mpt_resize(mpt_ctx* ctx, uint32_t width, uint32_t height);

/* One reference frame: swap targets, run the hot path for 1 sample/pixel with the current
 * uniforms (frameCount as given), write the running mean into the current target —
 * Renderer::draw, R/Renderer/Renderer.cpp:269-310 + Fragment.metal:8-72.  Returns when the frame is complete
 * (its statistics are folded into mpt_get_stats); mpt_render_async is the commit()-style call.        */
int mpt_draw(mpt_ctx* ctx, const mpt_render_params* p);

/* Batch rendering (this project's extension of the same loop): adds, for every owned pixel, the
 * sum over [sample_begin, sample_begin+sample_count) of the per-sample clamped colour
 * (PathTracing.h:258) into the HDR sum buffer.  Synchronous; fills the timing fields of mpt_stats.  */
int mpt_render(mpt_ctx* ctx, const mpt_render_params* p);

/* The same, without waiting: checks the arguments, queues the render and RETURNS (microseconds: whatever a submission has to
 * wait for — a free render lane, the trace kernel before it becoming resident — is waited for on the context's own submit thread,
 * not on the caller's; at most 64 renders are queued, a 65th call waits for room).  Up to two renders are in flight on the device:
 * their trace kernels overlap — the next render fills the compute units that the previous one's tail and resolve leave idle —
 * while the updates of the HDR sum stay in submission order, so the result is bit-identical to consecutive mpt_render calls.
 * mpt_wait collects everything queued and in flight and reports the first failure of a queued render; statistics of
 * asynchronous renders appear in mpt_get_stats after they were collected (trace_kernel_ms / total_ms / trace_launches
 * then accumulate until mpt_reset_stats or the next mpt_render).  Every other call on the context first waits until the queue
 * has been submitted (and those that touch the scene, the size or the sum buffer until the renders are done): the context is
 * still driven by ONE caller thread.  This mirrors Metal's commit() without waitUntilCompleted (Renderer.cpp:253-266,307-308). */
int mpt_render_async(mpt_ctx* ctx, const mpt_render_params* p);
int mpt_wait(mpt_ctx* ctx);
/* Diagnostics of the asynchronous path: out4 = {renders submitted by the submit thread, submissions that found the trace kernel
 * before them resident (the residency gate), submissions that did not within 200 ms and fell back to the event chain (a foreign
 * kernel holds the chip), the longest mpt_render_async call so far in microseconds of host time}.                                */
int mpt_async_info(mpt_ctx* ctx, uint64_t out4[4]);

/* HDR sum buffer (RGBA32F, W*H*4 floats, row-major, top-left origin).  The pointer is device
 * memory on the context's device, e.g. for an RCCL reduce by the caller.  mpt_set_sum_buffer lets
 * the caller supply the storage (e.g. a torch tensor); pass NULL to return to the internal one.     */
int mpt_sum_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);
int mpt_set_sum_buffer(mpt_ctx* ctx, void* device_ptr);
int mpt_clear_sum(mpt_ctx* ctx);

/* Read-back (the reference never reads back).  read_frame: the current running-mean
 * target of mpt_draw.  read_sum: the raw HDR sum.  Both RGBA32F, W*H*4 floats.                        */
int mpt_read_frame(mpt_ctx* ctx, float* rgba_host);
int mpt_read_sum(mpt_ctx* ctx, float* rgba_host);
/* Checkpoint / resume of the accumulation (the reference keeps its running mean in a GPU-private texture and never reads it back,
 * R/Renderer/Renderer.cpp:236, Fragment.metal:62-69): mpt_read_sum is the checkpoint, mpt_write_sum puts it back.
 * Continuing with sample_begin = the number of samples the sum holds gives, bit for bit, the sum of an uninterrupted render.     */
int mpt_write_sum(mpt_ctx* ctx, const float* rgba_host);

int mpt_get_stats(mpt_ctx* ctx, mpt_stats* out);
int mpt_reset_stats(mpt_ctx* ctx);
void* mpt_stream(mpt_ctx* ctx);                      /* hipStream_t of uploads, clears, mpt_draw and serial mpt_render
                                                        (mpt_render_async alternates between this and a second stream) */
int mpt_synchronize(mpt_ctx* ctx);

/* Device-side closest-hit for a batch of rays (unit tests of firstHitBVH, PathTracing.h:75-204).
 * origins/directions: 3 floats per ray (host).  Outputs (host): t, primitive id (-1 = miss),
 * normal (3 floats, flipped to face the ray), front-face flag.                                       */
int mpt_trace_rays(mpt_ctx* ctx, const float* origins, const float* directions, uint64_t n_rays, float* t_out,
                   int32_t* prim_out, float* normal_out, int32_t* front_out);

/* The same through the closest-first walk of MPT_PIPE_ORDERED (must return exactly what mpt_trace_rays returns).
 * flags_out (host, one uint32 per ray): 0 = answered by the closest-first walk; otherwise the ray was re-traced in
 * reference order because of 1 a (nearly) zero / non-finite direction component or a far origin, 2 a tie between two
 * primitives, 4 a winner in front of its own reference leaf box, 8 stack overflow.                                   */
int mpt_trace_rays_ordered(mpt_ctx* ctx, const float* origins, const float* directions, uint64_t n_rays, float* t_out,
                           int32_t* prim_out, float* normal_out, int32_t* front_out, uint32_t* flags_out);

/* Shape of the product's own acceleration structure for the uploaded scene: out[0] = 1 if MPT_PIPE_ORDERED can be used,
 * [1] own 4-wide nodes, [2] its depth, [3] nodes staged in LDS, [4] spheres on the always list, [5] reference leaves,
 * [6] primitives staged in LDS, [7] the pipeline MPT_PIPE_AUTO resolves to for this scene (MPT_PIPE_WAVELOCAL or
 * MPT_PIPE_ORDERED).                                                                                                   */
int mpt_accel_info(mpt_ctx* ctx, uint64_t out[8]);

/* BVH construction on the GPU — stands where the reference has Scene::buildBVH / buildBVHRecursive (R/Scene/Scene.h:71-93,
 * 195-317: sequential full-sweep SAH, 8.2 s for 1 M primitives): a top-down binned SAH over the primitives, built level by
 * level on the device (16 bins over the box centres, cost = area * primitives: the tree of the host's binned builder), with
 * leaves of <= mpt_gpu_leaf_max(n_prims) primitives — 6 for scenes below MPT_AUTO_ORDERED_PRIMS primitives (the ones the
 * reference-order kernel renders: tree and hot primitives sit in LDS there), 2 from there on (the closest-first kernel tests
 * every primitive of a leaf it enters); MPT_LBVH_LEAF = 1..8 overrides — written in the REFERENCE's buffer format so that
 * mpt_upload_scene (and the reference's shader, and the oracle) can consume it: bvh_out = 2 float4 per node as
 * Scene::createBVHBuffer returns them (root = node 0), prim_idx_out = Scene::createPrimitiveIndexBuffer.  The same input
 * gives the same arrays on every call.  MPT_GPU_BUILD = ploc | lbvh selects the two earlier builders instead (63-bit
 * Morton codes + radix sort, then nearest-neighbour clustering or Karras' radix tree: slower to render by 1-16 %).
 * prims: the 3-float4-per-primitive array of Scene::createTransformsBuffer (host memory, already sorted spheres first as
 * Scene::buildBVH does, Scene.h:72-75).  bvh_capacity_nodes >= 2 * n_prims - 1 is always enough.  device_ms_out
 * (optional): HIP-event time of the build kernels.  Parent boxes are exact unions of child boxes.                      */
int mpt_build_bvh(mpt_ctx* ctx, const float* prims, uint64_t n_prims, float* bvh_out, uint64_t bvh_capacity_nodes,
                  uint64_t* n_nodes_out, int32_t* prim_idx_out, double* device_ms_out);

/* Build -> render without the host: the same tree, built on the device from the caller's primitive and material arrays
 * (prims: 3 float4 each as Scene::createTransformsBuffer returns them, mats: 2 float4 each as Scene::createMaterialsBuffer)
 * and turned ON THE DEVICE into everything mpt_upload_scene derives on the host — the threaded reference-order tree, the
 * leaf-ordered primitive records, the de-duplicated materials, the product's own 4-wide tree — so that the scene is ready
 * to render when the call returns (1 M primitives: 9 ms, 4 of them the upload; mpt_build_bvh + mpt_upload_scene: 0.55 s).  Stands
 * for Scene::buildBVH + the four packers + Renderer::updateVisibleScene / buildBuffers (R/Scene/Scene.h:71-93,99-167,195-317,
 * R/Renderer/Renderer.cpp:127-146,199-215).  mpt_download_bvh returns that tree in the REFERENCE's buffer format (as
 * mpt_build_bvh does): what the reference's shader — and the oracle — would walk to produce the same image.                 */
int mpt_build_and_upload(mpt_ctx* ctx, const float* prims, const float* mats, uint64_t n_prims, double* device_ms_out);
int mpt_download_bvh(mpt_ctx* ctx, float* bvh_out, uint64_t bvh_capacity_nodes, uint64_t* n_nodes_out, int32_t* prim_idx_out);

/* The leaf limit the GPU builders (mpt_build_bvh, mpt_build_and_upload) use for a scene of n_prims primitives: 6 below
 * MPT_AUTO_ORDERED_PRIMS, 2 from there on, or what MPT_LBVH_LEAF says.  A pure function (no context).                      */
int mpt_gpu_leaf_max(uint64_t n_prims);
/* What the last scene call left on the device: out[0] = primitives of the tree mpt_download_bvh would return (0 when the scene
 * came through mpt_upload_scene: MPT_ERR_NOT_READY there), [1] nodes of that tree, [2] the leaf limit it was built with,
 * [3] MPT_AUTO_ORDERED_PRIMS (the scene size from which MPT_PIPE_AUTO means the closest-first pipeline), [4] primitives of the
 * uploaded scene, [5] threaded reference-order nodes, [6] de-duplicated materials, [7] nodes of the own 4-wide tree that the
 * closest-first walk fetches in their float form because their boxes could not be quantised (degenerate input; normally 0).  */
int mpt_build_info(mpt_ctx* ctx, uint64_t out[8]);

/* Diagnostics: a position-sensitive 64-bit digest of every device array of the uploaded scene, computed on the device —
 * out[0..8] = threaded tree, primitive records, materials, own 4-wide tree, reference leaf boxes, per-primitive leaf boxes,
 * always list, reference-format tree, reference-format primitive indices (0 where the scene has none); out[9..15] = the
 * counts (nodes, primitives, materials, own nodes, reference leaves, always-list entries, own-tree depth).  Two builds of the
 * same input must give the same 16 words (the tests' "same arrays" check covers what mpt_download_bvh does not return).
 * No reference counterpart (the reference builds once, on the host: R/Scene/Scene.h:71-93).                                */
int mpt_scene_digest(mpt_ctx* ctx, uint64_t out[16]);
/* Diagnostics: one of those nine device arrays copied to the host as 32-bit words (a device-to-host copy on the context's stream,
 * synchronised; no kernel, the scene is untouched).  which = 0..8 in the order of out[0..8] above, with the same word counts: 8 per
 * threaded node, 12 per primitive record, 8 per material, 28 per own node, 8 per reference leaf, 8 per primitive (leaf boxes), 20 per
 * always-list entry, 8 per reference-format node, 1 per reference-format index.  *n_words_out is always written: the array's size, 0
 * for an array the scene does not have (the reference-format tree after mpt_upload_scene; MPT_OK) and 0 with the errors that know
 * no size.  out = NULL with capacity_words = 0 is a size query.  MPT_ERR_NOT_READY without a scene; MPT_ERR_INVALID_ARG, with out
 * untouched, for a bad which, a null n_words_out or a capacity below the array's size.  tests/scene_check.py checks every
 * invariant the arrays carry.                                                                                               */
int mpt_read_scene_array(mpt_ctx* ctx, int which, uint32_t* out, uint64_t capacity_words, uint64_t* n_words_out);

/* Diagnostics: the per-tile class words of the lean wave-local kernels (csrc/mpt_lean_tiles.h) that render lane `lane` (0 or 1; -1: the lane
 * of the last trace kernel) holds from its last pass, if that pass ran those kernels: tiles_x * tiles_y words in row-major tile order, bit 31 = skip, bits 0..15 = mask, 0 = general.
 * Waits for the renders in flight.  *n_words_out is always written (0: the lane has no table — another kernel ran, or
 * MPT_LEAN_TILES=0); out = NULL with capacity_words = 0 is a size query.  *builds_out (may be NULL): how often this context has
 * built a table so far.  MPT_ERR_INVALID_ARG for a bad lane, a null n_words_out or a capacity below the size.                  */
int mpt_read_lean_tile_classes(mpt_ctx* ctx, int lane, uint32_t* out, uint64_t capacity_words, uint64_t* n_words_out, uint64_t* builds_out);

/* ---- multi-GPU: tile shards + ONE RCCL reduce of the HDR sum over xGMI ---------------------------------
 * The reference is single-GPU (it presents straight to the drawable, R/Renderer/Renderer.cpp:303-307); this is the
 * product's extension.  Every GPU renders the 8x8 pixel tiles t % N == rank (mpt_render_params.shard_rank / shard_count)
 * at full spp into its own zero-initialised HDR sum; mpt_reduce_sum adds the N buffers onto the root's with
 * ncclReduce(sum, float32, 4*W*H) — each pixel has exactly one owner, so the result is bit-identical to one GPU's.
 * librccl.so is opened on first use (dlopen): nothing here needs it for N = 1, where the reduce is a no-op.
 *   one host thread, N contexts:   mpt_comm_create_all(ctxs, N, &comm)            (ncclCommInitAll)
 *   one process per GPU:           rank 0: mpt_comm_unique_id(id); every rank: mpt_comm_create_rank(ctx, r, N, id, &comm)
 * All contexts of a communicator must have the same size (mpt_resize).                                                  */
typedef struct mpt_comm mpt_comm;
#define MPT_COMM_ID_BYTES 128
int mpt_comm_unique_id(void* id_out /* MPT_COMM_ID_BYTES */);
int mpt_comm_create_all(mpt_ctx* const* ctxs, int n, mpt_comm** out);
int mpt_comm_create_rank(mpt_ctx* ctx, int rank, int nranks, const void* id /* MPT_COMM_ID_BYTES */, mpt_comm** out);
int mpt_reduce_sum(mpt_comm* comm, int root);   /* waits for the renders in flight, reduces, returns when the root holds the image */
int mpt_comm_destroy(mpt_comm* comm);
const char* mpt_comm_last_error(const mpt_comm* comm);

/* ---- denoiser: first-hit guide buffers + an edge-avoiding a-trous filter (Dammertz et al. 2010) --------------------------
 * No reference counterpart (the reference presents the raw running mean, Fragment.metal:62-69).  Guide buffers: one ray per pixel
 * through the pixel centre (mpt_draw's primary ray without jitter), traced on the device with the scene, uniforms and size of the
 * context; they are traced again when stale (after mpt_resize, mpt_upload_scene, mpt_build_and_upload, or new uniforms whose
 * cameraPosition, viewportU/V, firstPixelPosition or screenSize differ).  Per pixel: the first hit's albedo and distance t
 * along the normalised ray, the shading normal facing the ray, a class (0 surface, 1 emissive material: emissionPower > 0,
 * 2 miss) and the caller's primitive id (-1 on a miss; a miss has albedo 0, t = +inf, normal 0).  Neither the guide pass nor
 * the filter touches the HDR sum, the frame targets or mpt_stats.
 *
 * The filter (tests/denoise_ref.py restates it in numpy), colour c = sum / samples (SUM) or the current mpt_draw target
 * (FRAME); pixels of class 1 / 2 are returned bit for bit and are never taps; alpha is c's alpha.  x0 = c / max(albedo, 1e-3);
 * level i = 0..N-1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer), kernel h = {1, 4, 6, 4, 1} / 16:
 *   w(q) = max(0, n_p . n_q)^sigma_normal * exp(-|t_p - t_q| / (sigma_depth * t_p * s)) * exp(-|l_p - l_q| / (sigma_luminance * 2^-i))
 * (l = Rec. 709 luminance of level i's x; the centre's w is 1), taps outside the image or of class != 0 skipped,
 * x_{i+1}(p) = sum h[dx] h[dy] w x_q / sum h[dx] h[dy] w; output = x_N * max(albedo, 1e-3), unclamped.  N = 0: the input.
 * Defaults (a sigma <= 0 or iterations < 0 selects them): chosen by the sweep of profiles/r06_denoise_sweep.txt.          */
enum { MPT_DENOISE_SUM = 0,     /* the HDR sum divided by samples                                                          */
       MPT_DENOISE_FRAME = 1 }; /* the current mpt_draw target (the running mean)                                          */
#define MPT_DENOISE_DEFAULT_ITERATIONS 3
#define MPT_DENOISE_MAX_ITERATIONS 8
#define MPT_DENOISE_DEFAULT_SIGMA_LUMINANCE 8.0f
#define MPT_DENOISE_DEFAULT_SIGMA_NORMAL 32.0f
#define MPT_DENOISE_DEFAULT_SIGMA_DEPTH 0.25f
typedef struct mpt_denoise_params {
    int32_t source;           /* MPT_DENOISE_* (mpt_denoise; mpt_denoise_image filters the colour it is given)              */
    uint32_t samples;         /* SUM: samples per pixel the sum holds (> 0)                                                 */
    int32_t iterations;       /* levels N, 0..MPT_DENOISE_MAX_ITERATIONS; < 0 = MPT_DENOISE_DEFAULT_ITERATIONS               */
    float sigma_luminance;    /* <= 0: the defaults above                                                                   */
    float sigma_normal;
    float sigma_depth;
} mpt_denoise_params;

/* The guide buffers (traced first if stale), W*H*4 floats each: albedo_depth = (albedo rgb, t), normal_class = (normal, class);
 * prim (W*H int32, may be NULL) = primitive ids.                                                                             */
int mpt_read_aovs(mpt_ctx* ctx, float* albedo_depth, float* normal_class, int32_t* prim);
/* Waits for the renders queued and in flight (reporting a failed mpt_render_async), refreshes stale guides, filters; the
 * result stays on the device (ctx's stream) for mpt_read_denoised / mpt_denoised_buffer (RGBA32F, W*H*4 floats).            */
int mpt_denoise(mpt_ctx* ctx, const mpt_denoise_params* params);
int mpt_read_denoised(mpt_ctx* ctx, float* rgba_host);
int mpt_denoised_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);
/* The same filter kernels on caller arrays (host, W*H*4 floats each; the unit-test hook): color is c itself (source and
 * samples are ignored), albedo_depth / normal_class as mpt_read_aovs returns them; a surface's t must be > 0.  No scene needed. */
int mpt_denoise_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* color, const float* albedo_depth,
                      const float* normal_class, const mpt_denoise_params* params, float* rgba_out);

/* ---- adaptive sampling: per-pixel moments + per-tile early stopping -------------------------------------------------------
 * No reference counterpart (the reference spends one sample per pixel per frame everywhere, Fragment.metal:8-72).
 *
 * Moments (MPT_FLAG_MOMENTS): the resolve of a render with the flag also adds, per pixel and per sample v (the clamped per-sample
 * colour the HDR sum adds), in sample order, m2 += (v.x^2, v.y^2, v.z^2, l^2) with l = (0.2126 v.x + 0.7152 v.y) + 0.0722 v.z into
 * a context-owned RGBA32F buffer (W*H*4 floats).  The HDR sum is bit-identical with and without the flag.  The buffer is allocated
 * by the first render with the flag; mpt_resize and mpt_clear_sum zero it, a render without the flag leaves it as it is.
 * mpt_write_sum, checkpoints and mpt_reduce_sum do not carry it.  mpt_read_moments: MPT_ERR_NOT_READY before mpt_resize, zeros
 * when no render with the flag has run since the last clear.                                                                  */
int mpt_read_moments(mpt_ctx* ctx, float* rgba_host);

/* Adaptive render: renders p's 8x8 tiles in passes until each tile's noise meets a target, with b = p->sample_begin and
 * N = p->sample_count the most samples any tile gets.  Synchronous, like mpt_render: it first waits for the renders queued and in
 * flight (reporting a failed mpt_render_async), then clears the HDR sum (the caller's storage of mpt_set_sum_buffer included), the
 * moments and the tile counts, and renders with MPT_FLAG_MOMENTS.
 *   schedule: n_0 = min(min_samples, N), n_{k+1} = min(n_k + batch_samples, N); pass 0 renders samples [b, b+n_0) of every tile,
 *             pass k+1 renders [b+n_k, b+n_{k+1}) of the tiles still active (every active tile holds n_k samples).
 *   stopping: after each pass, in double precision from the float32 sum and moments, for every pixel inside the image of a tile
 *             holding n samples: s = lum(sum.rgb), mean = s / n, var = max(0, (m2.w - s * mean) / (n - 1)),
 *             err = sqrt(var / n) / max(mean, luminance_floor); lum uses the three float constants above.  The tile's error is the
 *             maximum over its pixels; the tile stays active iff error > threshold and n < N.  A stopped tile never resumes.
 * Afterwards mpt_read_tile_samples gives every tile's sample count; the per-pixel estimate is sum / count(tile).  Each tile holds,
 * bit for bit, the sum a plain mpt_render of [b, b+count) produces.  mpt_get_stats: paths grows by out->samples; trace_kernel_ms,
 * total_ms and trace_launches are the totals over the passes.  Every pipeline and BSDF mode works.
 * MPT_ERR_INVALID_ARG, with nothing rendered: a null argument, MPT_RNG_LITERAL (its stream repeats per pixel: no variance),
 * shard_count != 1, min_samples == 1, a negative or NaN threshold, N < 2.  MPT_ERR_NOT_READY before scene, uniforms and size.  */
#define MPT_ADAPTIVE_DEFAULT_MIN_SAMPLES 16u
#define MPT_ADAPTIVE_DEFAULT_BATCH 16u
#define MPT_ADAPTIVE_DEFAULT_LUMINANCE_FLOOR 0.05f
typedef struct mpt_adaptive_params {
    uint32_t min_samples;     /* first pass, every tile (>= 2); 0 = MPT_ADAPTIVE_DEFAULT_MIN_SAMPLES                            */
    uint32_t batch_samples;   /* samples per later pass (>= 1); 0 = MPT_ADAPTIVE_DEFAULT_BATCH                                  */
    float threshold;          /* target relative standard error of a pixel's mean (>= 0; 0 = every tile to N)                   */
    float luminance_floor;    /* <= 0: MPT_ADAPTIVE_DEFAULT_LUMINANCE_FLOOR                                                     */
} mpt_adaptive_params;
typedef struct mpt_adaptive_info {
    uint64_t samples;           /* pixel samples rendered (pixels inside the image only)                                        */
    uint32_t passes;            /* trace passes run (the first pass included)                                                   */
    uint32_t tiles_converged;   /* tiles stopped by the threshold below N                                                       */
    uint32_t tiles_at_max;      /* tiles that reached N = p->sample_count                                                       */
    uint32_t _pad;
} mpt_adaptive_info;
int mpt_render_adaptive(mpt_ctx* ctx, const mpt_render_params* p, const mpt_adaptive_params* a, mpt_adaptive_info* out);
/* Samples per tile of the last mpt_render_adaptive (or mpt_render_nee_adaptive): ceil(W/8) * ceil(H/8) uint32, row-major tiles (zeros before the first one;
 * MPT_ERR_NOT_READY before mpt_resize).                                                                                       */
int mpt_read_tile_samples(mpt_ctx* ctx, uint32_t* counts);

/* ---- temporal accumulation: the history follows the camera ----------------------------------------------------------------------
 * No reference counterpart (the reference restarts its running mean on every camera change, Renderer.cpp:255-257).
 *
 * State per context: a history image (RGBA32F; rgb = accumulated radiance, a = history length n, a float >= 1), the history guide
 * of the frame it belongs to (per pixel: the ray-facing normal and the hit distance t of mpt_read_aovs, t = +inf for a miss) and
 * that frame's camera (cameraPosition, viewportU/V, firstPixelPosition, screenSize: the fourteen floats that make guides stale).
 * Two of each, ping-pong.  Allocated by the first mpt_temporal_accumulate; dropped by mpt_resize, mpt_upload_scene,
 * mpt_build_and_upload and mpt_temporal_reset.  mpt_clear_sum does not touch it.
 *
 * mpt_temporal_accumulate waits for the renders queued and in flight (reporting a failed mpt_render_async), refreshes stale guides,
 * then for every pixel p of the current frame, c = sum / samples (SUM) or the current mpt_draw target (FRAME), (cam, first, vu, vv)
 * the current camera, primes marking the history's camera.  All arithmetic is float32, one IEEE operation at a time in the order
 * written; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; |r| = sqrt(dot(r, r)) (tests/temporal_ref.py restates it in numpy):
 *   1. d = the pixel-centre direction of the guide pass: dv = (first + ((px + 0.5) / W) vu + ((py + 0.5) / H) vv) - cam,
 *      d = dv * (1 / sqrt(dot(dv, dv))).  For a hit (class 0 or 1): r = (cam + t_p * d) - cam'.  For a miss: r = d (a miss
 *      reprojects by direction only).
 *   2. nn = cross(vu', vv'); fc = first' - cam'; s = dot(fc, nn) / dot(r, nn).  No history unless s > 0 and s is finite.
 *   3. q = s * r - fc; u = dot(q, vu') / dot(vu', vu'); v = dot(q, vv') / dot(vv', vv') (the viewport vectors are orthogonal);
 *      fx = u * W - 0.5, fy = v * H - 0.5.  No history unless -1 <= fx < W and -1 <= fy < H.  x0 = floor(fx), y0 = floor(fy),
 *      ax = fx - x0, ay = fy - y0.
 *   4. Four taps (x0 + i, y0 + j), j outer, i inner, weight (i ? ax : 1 - ax) * (j ? ay : 1 - ay).  A tap counts iff it is inside
 *      the image and, for a hit p: the tap is a hit, |t_q - |r|| <= depth_tolerance * |r|, and dot(n_p, n_q) >= normal_threshold;
 *      for a miss p: the tap is a miss.
 *   5. sw = sum of the counted weights, in tap order.  If !(sw >= min_weight): out = (c.rgb, 1) — c's bits — and the pixel counts as
 *      reset.  Otherwise h = (sum w * hist.rgb) / sw, m = (sum w * hist.a) / sw, n = min(m + 1, max_history),
 *      out = (h + (c.rgb - h) / n, n).
 *   6. Same camera: when the fourteen camera floats equal the history's bit for bit, the only tap is p itself with weight 1 and no
 *      test (a float reprojection of an unmoved camera lands up to 1e-4 pixel off the centre and would blur a little more every
 *      frame; with this rule a still camera gives the plain running mean).
 *   7. No history at all (first call, after a reset or a drop): every pixel is reset.
 * The new history guide is the current guide.  pixels_reprojected + pixels_reset = W * H.  The stage reads the HDR sum or the frame
 * target and writes neither; mpt_stats is untouched.
 * MPT_ERR_INVALID_ARG, with nothing changed: null params, a bad source, SUM with samples = 0, a NaN tolerance.  MPT_ERR_NOT_READY
 * before scene, uniforms and size, and from mpt_read_temporal / mpt_temporal_buffer / mpt_denoise_temporal while there is no history.
 * Defaults: chosen by the sweep of profiles/r07_temporal_sweep.txt.                                                               */
#define MPT_TEMPORAL_DEFAULT_MAX_HISTORY 32u
#define MPT_TEMPORAL_DEFAULT_DEPTH_TOLERANCE 0.05f
#define MPT_TEMPORAL_DEFAULT_NORMAL_THRESHOLD 0.5f
#define MPT_TEMPORAL_DEFAULT_MIN_WEIGHT 0.05f
typedef struct mpt_temporal_params {
    int32_t source;            /* MPT_DENOISE_SUM (sum / samples) or MPT_DENOISE_FRAME: this frame's colour c                        */
    uint32_t samples;          /* SUM: samples the sum holds (> 0)                                                                  */
    uint32_t max_history;      /* cap of n; 0 = MPT_TEMPORAL_DEFAULT_MAX_HISTORY                                                    */
    float depth_tolerance;     /* relative; <= 0 = default                                                                          */
    float normal_threshold;    /* least n_p . n_q of a tap; <= 0 = default                                                          */
    float min_weight;          /* least sum of valid tap weights; <= 0 = default                                                    */
} mpt_temporal_params;
typedef struct mpt_temporal_info {
    uint64_t pixels_reprojected, pixels_reset;
} mpt_temporal_info;

int mpt_temporal_accumulate(mpt_ctx* ctx, const mpt_temporal_params* params, mpt_temporal_info* out /* may be NULL */);
int mpt_read_temporal(mpt_ctx* ctx, float* rgba_host);                 /* rgb = accumulated colour, a = n (W*H*4 floats)             */
int mpt_temporal_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);
int mpt_temporal_reset(mpt_ctx* ctx);
/* The a-trous filter of mpt_denoise over the history's rgb with the current guides, into the denoised buffer (mpt_read_denoised);
 * source / samples of the params are ignored; alpha = n.                                                                          */
int mpt_denoise_temporal(mpt_ctx* ctx, const mpt_denoise_params* params);
/* The same kernels on caller arrays (host, W*H*4 floats each; the unit-test hook, no scene needed): color is c itself (source and
 * samples are ignored), the guides as mpt_read_aovs returns them, the cameras as uniforms (W, H stand for screenSize in the
 * arithmetic).  history_prev = NULL: no history (the three other *_prev arguments are ignored).                                   */
int mpt_temporal_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* color, const float* albedo_depth_cur,
                       const float* normal_class_cur, const mpt_uniforms* cam_cur, const float* history_prev,
                       const float* albedo_depth_prev, const float* normal_class_prev, const mpt_uniforms* cam_prev,
                       const mpt_temporal_params* params, float* history_out, mpt_temporal_info* out /* may be NULL */);

/* ---- SVGF: temporal luminance moments and a variance-guided a-trous filter -----------------------------------------------------
 * No reference counterpart.  After Schied et al. 2017, with the departures written below.
 *
 * State per context, two of each (ping-pong), with the lifetime of the temporal history — allocated by the first
 * mpt_svgf_accumulate; dropped by mpt_resize, mpt_upload_scene, mpt_build_and_upload and mpt_svgf_reset; untouched by mpt_clear_sum —
 * and independent of it: this stage neither reads nor writes the mpt_temporal_* history.
 *   illumination history (X.rgb, n), RGBA32F: for a surface pixel (class 0) X is demodulated (divided by the albedo), for an emitter
 *     or a miss it is the radiance itself; n = history length, a float >= 1;
 *   moments history (M1, M2): first and second moment of the luminance of the per-frame x below, two floats;
 *   history guide, 16 bytes: (ray-facing normal, t) with the pixel's class in t: t for a surface, -t for an emitter (a hit distance
 *     is > 0), +inf for a miss;
 *   the fourteen camera floats of the history's frame.
 *
 * mpt_svgf_accumulate waits for the renders queued and in flight (reporting a failed mpt_render_async), refreshes stale guides, then
 * runs three steps.  All arithmetic float32, one IEEE operation at a time in the order written; dot as in the temporal section;
 * lum(x) = (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b.  c = sum / samples (SUM) or the current mpt_draw target (FRAME);
 * a = max(albedo, 1e-3) per channel for a surface pixel, a = 1 for classes 1 / 2; x = c.rgb / a; l = lum(x).
 *
 * A. Temporal step (only + - * / sqrt floor and comparisons: tests/svgf_ref.py agrees bit for bit).  Every pixel is accumulated, sky
 *    and emitters too.  Reprojection as steps 1-4 and 6 of mpt_temporal_accumulate (hit rule for classes 0 and 1, miss rule for
 *    class 2; a history tap's distance is |t_q|) with one more condition on a tap of a hit: the history pixel has the class of p, so
 *    that demodulated and plain values never mix.  Sums over the counted taps, in tap order: sx (rgb), sm1, sm2, sn, sw.
 *    !(sw >= min_weight) or no history: reset — X = x, M1 = l, M2 = l * l, n = 1.  Otherwise h = sx / sw, m1 = sm1 / sw,
 *    m2 = sm2 / sw, m = sn / sw, n = min(m + 1, max_history), X = h + (x - h) / n, M1 = m1 + (l - m1) / n,
 *    M2 = m2 + (l * l - m2) / n.  pixels_reprojected + pixels_reset = W * H.
 * B. Variance of the accumulated mean, V_0; surface pixels only (0 for classes 1 / 2).  n >= 4: V = max(0, M2 - M1 * M1) / n.
 *    Otherwise a 7 x 7 window of this frame's (M1, M2): taps q = p + (dx, dy), dy outer, both from -3 to 3, the centre in its
 *    place; taps outside the image or of class != 0 skipped; w = wn * wz with wn = pow(max(0, dot(n_p, n_q)), sigma_normal),
 *    wz = exp(-|t_p - t_q| / (sigma_depth * t_p)), the centre's w = 1; S1 = sum w * M1_q, S2 = sum w * M2_q, Sw = sum w;
 *    e1 = S1 / Sw; V = max(0, S2 / Sw - e1 * e1) / n.  Dividing by n departs from the paper, which filters with the per-sample
 *    variance: with the variance of the MEAN the filter closes as the history grows, and a disoccluded pixel gets a wide one.
 * C. N a-trous levels over (x_i.rgb, V_i), x_0 = X, V_0 as above; level i, s = 2^i, the 5 x 5 taps and the kernel h of mpt_denoise
 *    (dy outer; taps outside the image or of class != 0 skipped).  g_p = the 3 x 3 binomial mean of V_i over the ADJACENT pixels
 *    (not +-s): k = k3[dx] * k3[dy], k3 = {1/4, 1/2, 1/4}, dy outer, g_p = (sum k * V_q) / (sum k) over the taps not skipped.
 *    wl = exp(-|lum(x_p) - lum(x_q)| / (sigma_luminance * sqrt(g_p) + MPT_SVGF_EPSILON));
 *    wz = exp(-|t_p - t_q| / ((sigma_depth * t_p) * s)); w = (h[dx] * h[dy]) * ((wn * wz) * wl), the centre's w = h[0]^2 exactly.
 *    x_{i+1} = (sum w * x_q) / (sum w); V_{i+1} = (sum (w * w) * V_q) / ((sum w) * (sum w)).
 * Output (mpt_read_svgf, mpt_svgf_buffer): (x_N * a, n) for a surface pixel; (X, n) — the accumulated radiance, unfiltered, never a
 * tap — for classes 1 / 2; N = 0 gives X * a.  Feedback (feedback != 0 and N >= 1): the illumination history kept for the next
 * frame is x_1.rgb for surface pixels (n unchanged); the moments are never filtered.
 * mpt_read_svgf_state: the illumination history as kept for the next frame, and (M1, M2, V_0, 0).
 * The stage reads the HDR sum or the frame target and writes neither; mpt_stats is untouched; the a-trous buffers are its own, so
 * an mpt_denoise result stays readable.
 * MPT_ERR_INVALID_ARG, with nothing changed: null params, a bad source, SUM with samples = 0, a NaN tolerance or sigma, iterations
 * above MPT_DENOISE_MAX_ITERATIONS.  MPT_ERR_NOT_READY before scene, uniforms and size, and from mpt_read_svgf / mpt_svgf_buffer /
 * mpt_read_svgf_state while there is no state.  Defaults: chosen from the sweep of profiles/r08_svgf_sweep.txt; step A's are the
 * MPT_TEMPORAL_DEFAULT_*.                                                                                                         */
#define MPT_SVGF_EPSILON 1e-4f
#define MPT_SVGF_DEFAULT_ITERATIONS 2
#define MPT_SVGF_DEFAULT_SIGMA_LUMINANCE 2.0f
#define MPT_SVGF_DEFAULT_SIGMA_NORMAL 32.0f
#define MPT_SVGF_DEFAULT_SIGMA_DEPTH 0.25f
#define MPT_SVGF_DEFAULT_FEEDBACK 0
typedef struct mpt_svgf_params {
    int32_t source;            /* MPT_DENOISE_SUM (sum / samples) or MPT_DENOISE_FRAME: this frame's colour c                        */
    uint32_t samples;          /* SUM: samples the sum holds (> 0)                                                                  */
    uint32_t max_history;      /* step A, as mpt_temporal_params: 0 = MPT_TEMPORAL_DEFAULT_MAX_HISTORY                              */
    float depth_tolerance;     /* <= 0 = MPT_TEMPORAL_DEFAULT_DEPTH_TOLERANCE                                                       */
    float normal_threshold;    /* <= 0 = MPT_TEMPORAL_DEFAULT_NORMAL_THRESHOLD                                                      */
    float min_weight;          /* <= 0 = MPT_TEMPORAL_DEFAULT_MIN_WEIGHT                                                            */
    int32_t iterations;        /* levels N, 0..MPT_DENOISE_MAX_ITERATIONS; < 0 = MPT_SVGF_DEFAULT_ITERATIONS                        */
    float sigma_luminance;     /* in standard deviations of the accumulated mean; <= 0 = MPT_SVGF_DEFAULT_SIGMA_LUMINANCE           */
    float sigma_normal;        /* <= 0 = MPT_SVGF_DEFAULT_SIGMA_NORMAL                                                              */
    float sigma_depth;         /* <= 0 = MPT_SVGF_DEFAULT_SIGMA_DEPTH                                                               */
    int32_t feedback;          /* != 0: x_1 becomes the illumination history; < 0 = MPT_SVGF_DEFAULT_FEEDBACK                       */
} mpt_svgf_params;
typedef struct mpt_svgf_info {
    uint64_t pixels_reprojected, pixels_reset;
} mpt_svgf_info;

int mpt_svgf_accumulate(mpt_ctx* ctx, const mpt_svgf_params* params, mpt_svgf_info* out /* may be NULL */);
int mpt_read_svgf(mpt_ctx* ctx, float* rgba_host);                     /* the filtered frame: rgb, a = n (W*H*4 floats)             */
int mpt_svgf_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);
int mpt_read_svgf_state(mpt_ctx* ctx, float* history /* W*H*4 */, float* moments_variance /* W*H*4: M1, M2, V_0, 0 */);
int mpt_svgf_reset(mpt_ctx* ctx);
/* The same kernels on caller arrays (host; the unit-test hook, no scene needed): color is c itself (source and samples are ignored),
 * the guides as mpt_read_aovs returns them, the cameras as uniforms, W*H*4 floats each except moments_prev (W*H*2: M1, M2).
 * history_prev = NULL: no history (the other *_prev arguments are ignored).  The three outputs may each be NULL.                  */
int mpt_svgf_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* color, const float* albedo_depth_cur,
                   const float* normal_class_cur, const mpt_uniforms* cam_cur, const float* history_prev, const float* moments_prev,
                   const float* albedo_depth_prev, const float* normal_class_prev, const mpt_uniforms* cam_prev,
                   const mpt_svgf_params* params, float* history_out, float* moments_variance_out, float* filtered_out,
                   mpt_svgf_info* out /* may be NULL */);

/* ---- display: auto-exposure, tone curve, exact 8-bit encoding --------------------------------------------------------------------
 * No reference counterpart (the reference hands its float target to the drawable, Renderer.cpp:303-307).  The last step between a
 * rendered frame and a picture, on the device: W*H RGBA8 words instead of W*H*4 floats come back to the host.
 *
 * State per context: the display buffer (one word per pixel), the 256-bin histogram of the last call with auto_exposure, and the auto
 * scale kept for the next call.  Allocated by the first mpt_display; dropped by mpt_resize, mpt_upload_scene and mpt_build_and_upload;
 * mpt_display_reset forgets only the kept auto scale.  mpt_clear_sum does not touch it.
 *
 * mpt_display waits for the renders queued and in flight (reporting a failed mpt_render_async), then for every pixel with c the source's
 * colour (MPT_DISPLAY_*).  All arithmetic is float32, one IEEE operation at a time in the order written;
 * lum(c) = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b; no pow, exp or log runs on the device (tests/display_ref.py restates it in numpy and
 * agrees bit for bit):
 *   A. Histogram (only with auto_exposure).  l = lum(c.rgb), before any exposure.  A pixel is counted iff l > 0 and l < +inf.  With
 *      e = float_bits(l) >> 21 its bin is b = min(max(e, 380), 635) - 380: 256 bins, four per octave, from 2^-32 to 2^32; smaller
 *      values fall in bin 0, larger ones in bin 255.  The lower edge of bin b is E_b = bits_to_float((b + 380) << 21).  Counts are
 *      uint32; pixels_counted = N, their sum.
 *   B. Exposure.  N = 0: auto_scale = 1, key_bin = 0xFFFFFFFF.  Otherwise key_bin = the smallest b with cum(b) * 100 >= N * percentile
 *      in 64-bit integers (cum = the inclusive prefix sum); target = key / E_key_bin; if the context keeps a previous auto scale p and
 *      0 < adaptation < 1: auto_scale = p + (target - p) * adaptation, otherwise auto_scale = target.  The new auto scale is kept for
 *      the next call.  Without auto_exposure: auto_scale = 1, key_bin = 0xFFFFFFFF, pixels_counted = 0 and the kept state is untouched.
 *      scale = exposure * auto_scale.
 *   C. Tone curve, per channel: x = c_ch * scale; v = x > 0 ? x : 0 (a NaN becomes 0); v = min(v, 65504).
 *      CLAMP: y = v.  REINHARD: y = (v * (1 + v / (white * white))) / (1 + v).
 *      ACES (Narkowicz's fit): y = (v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f).
 *      A pixel is clipped iff any of its three y is >= 1 (pixels_clipped counts them).  Then y = min(y, 1).
 *   D. Encoding: code = |{k in 1..255 : T[k] <= y}|, T[k] = the float32 nearest to f^-1((k - 0.5) / 255) — the correctly rounded
 *      round(255 f(y)) without a transcendental.  SRGB: f^-1(s) = s <= 0.04045 ? s / 12.92 : ((s + 0.055) / 1.055)^2.4; GAMMA22:
 *      f^-1(s) = s^2.2 (what mpt_write_ppm's pow(v, 1 / 2.2) * 255 + 0.5, truncated, means); LINEAR: f^-1(s) = s.  The three tables are
 *      computed once in float64 by tools/make_display_table.py and committed (mpt_display_table.h); mpt_display_table returns them,
 *      out[k - 1] = T[k].  Output word: r | g << 8 | b << 16 | 255 << 24.
 * The stage reads its source and writes none of: the HDR sum, the frame targets, the moments, the denoised buffer, the temporal and
 * SVGF state, mpt_stats.  It needs a size but no scene.
 * MPT_ERR_INVALID_ARG, with nothing changed: null params, a bad source, tone or transfer, SUM with samples = 0, percentile > 100, a NaN
 * in any float field.  MPT_ERR_NOT_READY before mpt_resize and for a source that does not exist yet (no denoised result, no temporal or
 * SVGF history, no adaptive render), and from mpt_read_display / mpt_display_buffer / mpt_read_display_histogram before the first
 * mpt_display.  Defaults: conventional values, not swept.                                                                            */
enum { MPT_DISPLAY_SUM = 0,       /* HDR sum / samples (IEEE division by (float)samples per channel, as the denoiser's c)              */
       MPT_DISPLAY_FRAME = 1,     /* the current mpt_draw target                                                                      */
       MPT_DISPLAY_DENOISED = 2,  /* what mpt_read_denoised returns (mpt_denoise / mpt_denoise_temporal)                              */
       MPT_DISPLAY_TEMPORAL = 3,  /* rgb of the mpt_temporal_* history                                                                */
       MPT_DISPLAY_SVGF = 4,      /* rgb of mpt_read_svgf                                                                             */
       MPT_DISPLAY_ADAPTIVE = 5 };/* HDR sum / (float)count(tile) of the last mpt_render_adaptive or mpt_render_nee_adaptive, the tile
                                     of pixel (x, y) being (y / 8) * ceil(W / 8) + x / 8; a count of 0 gives 0                        */
enum { MPT_TONE_CLAMP = 0, MPT_TONE_REINHARD = 1, MPT_TONE_ACES = 2 };
enum { MPT_TRANSFER_SRGB = 0, MPT_TRANSFER_GAMMA22 = 1, MPT_TRANSFER_LINEAR = 2 };
#define MPT_DISPLAY_DEFAULT_WHITE 4.0f
#define MPT_DISPLAY_DEFAULT_PERCENTILE 50u
#define MPT_DISPLAY_DEFAULT_KEY 0.18f
typedef struct mpt_display_params {
    int32_t source;            /* MPT_DISPLAY_* (mpt_display; mpt_display_image presents the colour it is given)                     */
    uint32_t samples;          /* SUM: samples per pixel the sum holds (> 0)                                                         */
    int32_t tone;              /* MPT_TONE_*                                                                                         */
    int32_t transfer;          /* MPT_TRANSFER_*                                                                                     */
    float exposure;            /* linear multiplier; <= 0 selects 1                                                                  */
    float white;               /* REINHARD's white point; <= 0 selects MPT_DISPLAY_DEFAULT_WHITE                                     */
    int32_t auto_exposure;     /* != 0: multiply by the histogram's scale (steps A, B)                                               */
    uint32_t percentile;       /* 1..100; 0 selects MPT_DISPLAY_DEFAULT_PERCENTILE                                                   */
    float key;                 /* the value the key bin's lower edge is mapped to; <= 0 selects MPT_DISPLAY_DEFAULT_KEY              */
    float adaptation;          /* (0, 1): share of the way to the target taken per call; <= 0 or >= 1: no smoothing                  */
} mpt_display_params;
typedef struct mpt_display_info {
    float scale, auto_scale;   /* scale = exposure * auto_scale, as used                                                             */
    uint32_t key_bin, _pad;    /* 0xFFFFFFFF when nothing was counted or auto_exposure is off                                        */
    uint64_t pixels_counted, pixels_clipped;
} mpt_display_info;

int mpt_display(mpt_ctx* ctx, const mpt_display_params* params, mpt_display_info* out /* may be NULL */);
int mpt_read_display(mpt_ctx* ctx, uint8_t* rgba8_host);               /* W*H*4 bytes (r, g, b, 255), row-major, top-left origin     */
int mpt_display_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);
int mpt_read_display_histogram(mpt_ctx* ctx, uint32_t out[256]);       /* of the last call with auto_exposure (zeros before one)     */
int mpt_display_reset(mpt_ctx* ctx);                                   /* forgets the kept auto scale: the next call is unsmoothed   */
int mpt_display_table(int transfer, float out[255]);                   /* a pure function (no context)                               */
/* The same kernels on a caller array (host, W*H*4 floats; the unit-test hook, no scene and no size needed): color is c itself (source
 * and samples are ignored); prev_auto_scale = NULL: no kept auto scale; the context's own display state is neither read nor written.
 * histogram_out (256 uint32, may be NULL): this call's histogram, zeros without auto_exposure.  out may be NULL.                     */
int mpt_display_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* color, const mpt_display_params* params,
                      const float* prev_auto_scale, uint8_t* rgba8_out, uint32_t* histogram_out, mpt_display_info* out);

/* ---- shadow rays: occlusion queries and ambient occlusion ---------------------------------------------------------------------------
 * No reference counterpart (every ray of the reference is a closest-hit ray, PathTracing.h:75-204).
 *
 * Any hit.  A ray (o, d) with the limit tmax is OCCLUDED iff the reference's walk, started with best t = tmax instead of +inf, accepts
 * any primitive: the same slab test (tMin = 1e-4, tMax = best t), the same sphere and triangle tests, acceptance t > 1e-4 && t < best t.
 * !(tmax > 1e-4) (a NaN included) and a direction with a NaN component are "not occluded"; tmax = +inf asks for any hit at all.
 * With the same tree, "occluded" implies that mpt_trace_rays returns t < tmax, exactly.  The converse fails only for the reference's
 * known artefact — a hit whose computed t lies in front of its own leaf's slab entry — when tmax falls between the two, and, with
 * tmax within a rounding of t (one ulp above it, say), for a leaf whose slab entry rounds to >= tmax: hi > lo fails, the hit is not seen.
 * MPT_WALK_REFERENCE walks the threaded reference-order tree, MPT_WALK_OWN the product's own 4-wide tree (children culled beyond
 * tmax * (1 + 2^-10) + eps_abs, primitives tested with the reference's exact tests, no final check: for that artefact it answers by
 * the primitive test alone); rays the closest-first walk hands to the reference-order walk for their direction or origin (flag 1), or
 * whose stack overflows (flag 8), are answered by the reference-order walk.  OWN on a scene whose mpt_accel_info out[0] is 0 is
 * REFERENCE; MPT_WALK_AUTO is OWN where mpt_accel_info out[7] is MPT_PIPE_ORDERED and REFERENCE elsewhere.
 * mpt_trace_occluded is the sibling of mpt_trace_rays: host arrays, at most 2^22 rays per call, tmax per ray (NULL = +inf for all),
 * occluded_out one byte per ray (0 / 1), flags_out (may be NULL) as mpt_trace_rays_ordered's (0 for every ray of the REFERENCE walk).
 * MPT_ERR_INVALID_ARG for a null pointer, n_rays = 0 or a bad walk; MPT_ERR_NOT_READY without a scene.  Touches neither mpt_stats nor
 * the sum.                                                                                                                          */
enum { MPT_WALK_REFERENCE = 0, MPT_WALK_OWN = 1, MPT_WALK_AUTO = 2 };
int mpt_trace_occluded(mpt_ctx* ctx, const float* origins, const float* directions, const float* tmax, uint64_t n_rays, int32_t walk,
                       uint8_t* occluded_out, uint32_t* flags_out);

/* Measurement hook: the closest-hit and the any-hit kernel of either tree on the SAME rays (uploaded once; at most 2^22), launched in
 * turn — warmup untimed rounds, then reps (1..1000) rounds — with a pair of HIP events around every launch.  ms_out[4 * r + k], k = 0
 * closest hit in reference order (what mpt_trace_rays launches), 1 any hit in reference order, 2 closest hit through the own tree (what
 * mpt_trace_rays_ordered launches), 3 any hit through the own tree; 2 and 3 are 0 where mpt_accel_info out[0] is 0.  No result is returned. */
int mpt_time_trace(mpt_ctx* ctx, const float* origins, const float* directions, const float* tmax, uint64_t n_rays, uint32_t warmup,
                   uint32_t reps, double* ms_out);

/* Ambient occlusion over the first-hit guide buffers (float32, one IEEE operation at a time, dot and normalize as the guide pass:
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, normalize(v) = v * (1 / sqrt(dot(v, v))); tests/ao_ref.py restates it in numpy).
 * Every pixel of the (refreshed) guide buffers has a class, a ray-facing normal n and a hit distance t; dc is the pixel-centre direction
 * of step 1 of mpt_temporal_accumulate.  Class 1 and 2: ao = 1, occluded = 0, no ray is traced.  Class 0:
 *   P = cam + t * dc,  o = P + 0.0001f * n   (the origin the bounce ray leaves from)
 *   for sample s in [sample_begin, sample_begin + sample_count):
 *     r = philox4x32_10(counter = (py * W + px, s, 0xFFFFFFFE, 0), key = (seed_lo, seed_hi))   — word 2 = 0xFFFFFFFE is taken by no
 *         bounce and not by the pixel jitter (0xFFFFFFFF)
 *     uz = u01(r.x), uphi = u01(r.y), z = 2 uz - 1, (sn, cs) = sincos_2pi(uphi), rr = sqrt(1 - z * z)
 *     dir = normalize(n + (rr * cs, rr * sn, z))       (the Lambert direction of PathTracing.h:252-254 as mpt_render draws it)
 *     the sample is occluded iff any-hit(o, dir, radius > 0 ? radius : +inf)
 *   occluded = the count, ao = (float)(N - count) / (float)N.
 * One lane per (pixel, sample); a pixel's count is a ballot and a popcount over its lanes (no atomics), so the result does not depend on
 * how lanes are mapped.  The pass waits for queued renders, refreshes the guides if stale and writes none of: the HDR sum, the frame
 * targets, the moments, the denoised buffer, the temporal, SVGF and display state, mpt_stats.  Its result is dropped by mpt_resize,
 * mpt_upload_scene and mpt_build_and_upload.
 * MPT_ERR_INVALID_ARG, with nothing changed: null params, sample_count 0 or > MPT_AO_MAX_SAMPLES, a NaN radius, a bad walk.
 * MPT_ERR_NOT_READY before scene, uniforms and size, and from mpt_read_ao / mpt_ao_buffer before the first pass.                      */
#define MPT_AO_MAX_SAMPLES 1024u
typedef struct mpt_ao_params {
    uint32_t sample_begin, sample_count;   /* sample_count: 1..MPT_AO_MAX_SAMPLES                                                      */
    float radius;                          /* <= 0: +inf                                                                               */
    uint32_t seed_lo, seed_hi;
    int32_t walk;                          /* MPT_WALK_*                                                                               */
} mpt_ao_params;
typedef struct mpt_ao_info {
    uint64_t pixels_surface, rays, rays_occluded;
    double device_ms;                      /* HIP-event time of the pass (a guide refresh not included)                                */
} mpt_ao_info;
int mpt_ambient_occlusion(mpt_ctx* ctx, const mpt_ao_params* params, mpt_ao_info* out /* may be NULL */);
int mpt_read_ao(mpt_ctx* ctx, float* ao_host /* W*H */, uint32_t* occluded_host /* W*H, may be NULL */);
int mpt_ao_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);    /* the W*H floats of ao                                        */
/* The same kernel on caller guides (host arrays as mpt_read_aovs returns them; the unit-test hook: it needs a scene but no size and
 * neither reads nor writes context state).  Of cam_uniforms only cameraPosition, viewportU, viewportV and firstPixelPosition are read.
 * occluded_out may be NULL.                                                                                                          */
int mpt_ao_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* albedo_depth, const float* normal_class,
                 const mpt_uniforms* cam_uniforms, const mpt_ao_params* params, float* ao_out, uint32_t* occluded_out);

/* ---- direct lighting: the light table and one shadow ray per sample -------------------------------------------------------------------
 * No reference counterpart (the reference finds its lights by bounces alone).  tests/direct_ref.py restates both parts in numpy.
 *
 * The light table.  A primitive is a LIGHT iff its material has emissionPower > 0 (the guide pass's class 1).  Its radiance is
 * Le = emission.rgb * power (one float32 multiply per channel).  A triangle emits from both sides, as the path tracer adds emission
 * whichever side is hit; a sphere emits OUTWARD only for this pass — a shading point inside an emissive sphere gets nothing from it (a
 * departure from the path tracer, which adds emission for a hit from inside too).  Geometry as the device holds it: triangle v0,
 * e1 = v1 - v0, e2 = v2 - v0 (float32); sphere centre c and radius r.  Weights in float64 from those float32 values:
 *   A = 0.5 * |cross(e1, e2)| (cross as below, |v| = sqrt((v.x v.x + v.y v.y) + v.z v.z)),  or ((4 pi) r) r
 *   l = (0.2126 Le.r + 0.7152 Le.g) + 0.0722 Le.b,   W = A * l
 * A light whose W is zero or not finite is left out (a degenerate triangle, black emission).  The others stand in ascending caller
 * primitive id (the id mpt_trace_rays and mpt_read_aovs report); C_k is the running sum of W in that order and C the last one:
 *   cdf[k] = (float)(C_k / C), cdf[last] = 1.0f exactly;   inv_pdf[k] = (float)(C / l_k)   (= A_k / p_k, the reciprocal of the area
 *   pdf when a light is drawn in proportion to its power)
 * The table is built by the first call that needs it after mpt_upload_scene / mpt_build_and_upload, from the arrays on the device, and
 * is the same for the same scene through either call and any tree.  More than MPT_LIGHTS_MAX emissive primitives: MPT_ERR_BAD_SCENE
 * from the call that needed the table, nothing kept.  A scene without lights is not an error (n = 0).
 * mpt_light_info: out = {lights, emissive primitives seen, triangle lights, sphere lights}.  mpt_read_lights: the first
 * min(n, capacity) lights — prim_id, 16 floats each (v0 | c, type: 1 triangle, 0 sphere) (e1 | r 0 0, 0) (e2 | 0, 0) (Le, inv_pdf), cdf —
 * and n itself in n_out; any of the three arrays may be NULL.  Both: MPT_ERR_NOT_READY without a scene.                               */
#define MPT_LIGHTS_MAX 65536u
int mpt_light_info(mpt_ctx* ctx, uint64_t out[4]);
int mpt_read_lights(mpt_ctx* ctx, uint32_t capacity, int32_t* prim_id, float* records, float* cdf, uint32_t* n_out);

/* Direct lighting over the first-hit guide buffers (float32, one IEEE operation at a time in the order given; dot and normalize as the
 * AO pass, cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), u01 and sincos_2pi as mpt_kat_philox / mpt_kat_sincos
 * pin them).  EVERY surface pixel is shaded as a Lambert surface (MPT_BSDF_LAMBERT: the guides carry no material type).
 * Class 1 and 2: rgba = (0, 0, 0, 1), traced = unoccluded = 0, no ray — EMITTERS SHOW BLACK in this pass.  Class 0:
 *   o = (cam + t * dc) + 0.0001f * n          (dc: the pixel-centre direction, as in the AO pass)
 *   for sample s in [sample_begin, sample_begin + N), ascending:
 *     r = philox4x32_10(counter = (py * W + px, s, 0xFFFFFFFD, 0), key = (seed_lo, seed_hi))   — word 2 = 0xFFFFFFFD is taken by no
 *         bounce, not by the pixel jitter (0xFFFFFFFF) and not by AO (0xFFFFFFFE)
 *     u = u01(r.x); the light k = the smallest index with u < cdf[k]
 *     triangle: a = u01(r.y), b = u01(r.z); if (a + b > 1) { a = 1 - a; b = 1 - b; }   P = (v0 + a * e1) + b * e2,
 *               nl = normalize(cross(e1, e2))
 *     sphere:   z = 2 * u01(r.y) - 1, (sn, cs) = sincos_2pi(u01(r.z)), rr = sqrt(1 - z * z), nl = (rr * cs, rr * sn, z), P = c + r * nl
 *     v = P - o, d2 = dot(v, v), dist = sqrt(d2), wi = v * (1 / dist)
 *     cos_s = dot(n, wi);  cos_l = |dot(nl, wi)| (triangle), -dot(nl, wi) (sphere)
 *     the sample is SKIPPED unless d2 > 0 && cos_s > 0 && cos_l > 0 (a NaN skips): no ray, counted neither as traced nor as unoccluded
 *     traced += 1; the shadow ray is any-hit(o, wi, tmax = dist * 0.9990234375f) (1 - 2^-10: the sampled light itself is outside)
 *     not occluded: unoccluded += 1, g = (cos_s * cos_l) / d2, w = g * inv_pdf[k], S += (Le.r * w, Le.g * w, Le.b * w)
 *   rgba = ((albedo.r * 0.31830987f) * (S.r / (float)N), likewise g and b, 1)
 * With no light in the table every class 0 pixel is (0, 0, 0, 1) with zero counts.  One lane per pixel: S runs in sample order.
 * The pass waits for queued renders, refreshes the guides if stale, builds the light table if stale and writes none of: the HDR sum,
 * the frame targets, the moments, the denoised buffer, the temporal, SVGF, display and AO state, mpt_stats.  Its result is dropped by
 * mpt_resize, mpt_upload_scene and mpt_build_and_upload.
 * MPT_ERR_INVALID_ARG, with nothing changed: null params, sample_count 0 or > MPT_DIRECT_MAX_SAMPLES, a bad walk.
 * MPT_ERR_NOT_READY before scene, uniforms and size, and from mpt_read_direct / mpt_direct_buffer before the first pass.              */
#define MPT_DIRECT_MAX_SAMPLES 1024u
typedef struct mpt_direct_params {
    uint32_t sample_begin, sample_count;   /* sample_count: 1..MPT_DIRECT_MAX_SAMPLES                                                  */
    uint32_t seed_lo, seed_hi;
    int32_t walk;                          /* MPT_WALK_*                                                                               */
} mpt_direct_params;
typedef struct mpt_direct_info {
    uint64_t pixels_surface, rays /* traced */, rays_occluded, lights;
    double device_ms;                      /* HIP-event time of the pass (guide refresh and table build not included)                  */
} mpt_direct_info;
int mpt_direct_lighting(mpt_ctx* ctx, const mpt_direct_params* params, mpt_direct_info* out /* may be NULL */);
int mpt_read_direct(mpt_ctx* ctx, float* rgba /* W*H*4 */, uint32_t* traced /* W*H, may be NULL */, uint32_t* unoccluded /* may be NULL */);
int mpt_direct_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);   /* the RGBA32F image, laid out as the HDR sum                */
/* The same kernel on caller guides (host arrays as mpt_read_aovs returns them; the unit-test hook: it needs a scene but no size and
 * touches no state of the context except a stale light table).  Of cam_uniforms only cameraPosition, viewportU, viewportV and
 * firstPixelPosition are read.  traced_out and unoccluded_out may be NULL.                                                            */
int mpt_direct_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* albedo_depth, const float* normal_class,
                     const mpt_uniforms* cam_uniforms, const mpt_direct_params* params, float* rgba_out, uint32_t* traced_out,
                     uint32_t* unoccluded_out);

/* ---- next-event estimation: a light sample with MIS at every Lambert vertex of a path render -------------------------------------------
 * No reference counterpart.  mpt_render_nee renders what mpt_render renders — same primary rays, same bounces, same HDR sum — with one
 * more estimate of the direct light at every diffuse vertex: a point on a light of the table above, one shadow ray, combined with the
 * light the bounce finds by the power heuristic.  tests/nee_ref.py restates the estimator in numpy.
 *
 * The call is synchronous, like mpt_render: it waits for the renders queued and in flight (reporting a failed mpt_render_async), builds
 * the light table if stale and, for every pixel, adds the per-sample values v_s of samples [sample_begin, sample_begin + sample_count)
 * to the HDR sum IN SAMPLE ORDER, sum = ((sum + v_b) + v_{b+1}) + ..., all four channels — the caller's storage of mpt_set_sum_buffer
 * included.  Denoiser, temporal, SVGF, display, checkpoint and mpt_read_sum work on the result unchanged.  From p it reads rng_mode
 * (must be MPT_RNG_PHILOX), bsdf_mode (MPT_BSDF_LAMBERT or MPT_BSDF_SCATTER), max_depth, sample_begin, sample_count, seed_lo, seed_hi;
 * pipeline and slots_per_iter are ignored.  It writes none of: the frame targets, the moments, the denoised buffer, the temporal, SVGF,
 * display, AO and direct state.  mpt_get_stats: paths and rays grow by the info's, trace_kernel_ms and total_ms are set as after an
 * mpt_render, trace_launches = 1.
 * OUT OF SCOPE: moments (MPT_FLAG_MOMENTS), shards, the asynchronous lane and adaptive rendering over this estimator (that is a call of
 * its own with its own kernel: mpt_render_nee_adaptive, below).
 * MPT_ERR_INVALID_ARG, with nothing rendered: a null p or n, MPT_RNG_LITERAL, MPT_BSDF_SCATTER_ALL (its direction pdf is not the cosine
 * pdf), shard_count != 1 or shard_rank != 0, flags != 0, sample_count == 0, max_depth < 1, a bad walk, a NaN clamp, and mpt_render's
 * upper limits: max_depth > 32, sample_begin + sample_count > 2^27.  MPT_ERR_NOT_READY before scene, uniforms and size.  MPT_ERR_BAD_SCENE from the light table, as mpt_direct_lighting.
 *
 * The estimator.  float32, one IEEE operation at a time in the order written; dot, cross and normalize as in the direct-lighting section;
 * philox(a, b, c, e) = philox4x32_10(counter = (a, b, c, e), key = (seed_lo, seed_hi)).  Sample s of pixel p = py * W + px:
 *   primary ray: mpt_render's for philox (jitter block (p, s, 0xFFFFFFFF, 0)).  thr = (1, 1, 1), L = (0, 0, 0), La = 0, b = 0,
 *   sampled = false, pb = 0.  Loop: (t, prim) = closest hit of (o, d).
 *   miss: L += thr * sky(d), La += 1, exactly as mpt_render; the path ends.  The sky is never sampled as a light and counts in full.
 *   hit: point P_h = o + t * d, n = the geometric normal facing the ray, front = whether the ray met the outside.  A primitive whose
 *     caller id is >= uniforms.primitiveCount ends the path (the material guard of PathTracing.h:234-236).
 *   emission, if power > 0 || materialType == 2 (mpt_render's condition):
 *     w = 1, unless all of: sampled; the primitive is light k of the table (a binary search of the ascending ids); for a sphere, front.
 *     Then cos_l = -dot(n, d), pl = (t * t) / (cos_l * inv_pdf[k]), q = pl / pb, w = 1 / (1 + q * q)  (the power heuristic, written so
 *     that no inf / inf arises).   L.c += ((thr.c * emission.c) * power) * w  (with w = 1: mpt_render's bits);  La += power.
 *   Lambert vertex (MPT_BSDF_LAMBERT, or materialType == 0):
 *     nd = normalize(n + ruv), ruv from block (p, s, b, 0) as mpt_render draws it;  o' = P_h + 0.0001f * n.
 *     light sample, only if the table has a light and b + 1 < max_depth (the ray that could find the light by a bounce is traced):
 *       r = philox(p, s, b, 1) — word 3 = 1 is used by nothing else: every other block has word 3 = 0.
 *       light k, the point P, nl, v, d2, dist, wi, cos_s, cos_l, the skip rule and the shadow ray any-hit(o', wi, dist * 0.9990234375f)
 *       are EXACTLY the direct-lighting pass's, with its n = n and its o = o'.  Not skipped and not occluded:
 *         g = (cos_s * cos_l) / d2,  pl = d2 / (cos_l * inv_pdf[k]),  pbs = cos_s * 0.31830987f,  q = pbs / pl,  wl = 1 / (1 + q * q),
 *         m = (g * inv_pdf[k]) * wl,   L.c += ((thr.c * albedo.c) * 0.31830987f) * (Le_k.c * m)
 *     sampled = whether a light sample was attempted at this vertex (skipped samples included);  pb = dot(n, nd) * 0.31830987f.
 *   specular vertex (MPT_BSDF_SCATTER and materialType != 0): mpt_render's mirror / dielectric bounce unchanged, no light sample,
 *     sampled = false.
 *   thr *= albedo;  (o, d) = (o' or the transmitted origin, nd);  b += 1;  the path continues iff b < max_depth.
 *   per-sample value: v.c = L.c > 0 ? min(L.c, clamp) : 0 (a NaN gives 0);  v.a = min(max(La, 0), 1).
 * Hence: with an empty light table, or with max_depth = 1, and with clamp = 1, the call adds bit for bit what mpt_render adds; with
 * clamp = +inf its expectation is that of the unclamped path tracer at the same max_depth.  Sphere lights are sampled uniformly over
 * their whole surface, as in the direct pass, unless mpt_set_light_sampling (below) selects the cone they subtend.
 * walk: the tree BOTH the closest hits and the shadow rays walk; MPT_WALK_OWN / MPT_WALK_AUTO fall back as in mpt_direct_lighting.  With
 * the own tree the closest hits are those of MPT_PIPE_ORDERED (its exactness note above applies) and the shadow rays those of
 * mpt_trace_occluded(MPT_WALK_OWN).                                                                                                   */
typedef struct mpt_nee_params {
    int32_t walk;        /* MPT_WALK_*                                                                                                   */
    float clamp;         /* per-sample, per-channel upper clamp; <= 0 selects +inf (none); a NaN is MPT_ERR_INVALID_ARG                  */
} mpt_nee_params;
typedef struct mpt_nee_info {
    uint64_t paths, rays /* closest-hit queries */, shadow_rays, shadow_rays_occluded, lights;
    double device_ms;    /* HIP-event time of the trace kernel (table build not included)                                               */
} mpt_nee_info;
int mpt_render_nee(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, mpt_nee_info* out /* may be NULL */);

/* ---- adaptive sampling over the NEE estimator: every 8x8 tile decides on the device ---------------------------------------------------
 * No reference counterpart.  mpt_render_nee_adaptive spends mpt_render_nee's samples the way mpt_render_adaptive allocates them: with
 * b = p->sample_begin and N = p->sample_count the most samples any tile gets, every tile renders samples [b, b + count(tile)) of the
 * estimator above, count(tile) being where the stopping rule of the adaptive section first holds along its schedule
 *   n_0 = min(min_samples, N),  n_{k+1} = min(n_k + batch_samples, N)   (the tile goes on iff error > threshold and n_k < N),
 * with the rule's arithmetic unchanged: double precision from the float32 sum and the float32 moments of the n_k samples the tile holds
 * (so, as there, a tile without any variance — error exactly 0 — stops at n_0 even under threshold 0).
 * The moments are those of MPT_FLAG_MOMENTS, m2 += (v.x^2, v.y^2, v.z^2, l^2) per sample value v in sample order, one IEEE operation at a
 * time.  The wave that renders a tile keeps both in registers and applies the rule itself: ONE kernel launch, no host passes.
 *
 * The call is synchronous.  It waits for the renders queued and in flight (reporting a failed mpt_render_async), builds the light table
 * if stale, clears the HDR sum (the caller's storage of mpt_set_sum_buffer included), the moments buffer (allocated if absent) and the
 * tile counts, and launches the kernel.  The light-sampling mode is read at the start, as mpt_render_nee reads it.  From p and n it reads
 * what mpt_render_nee reads; a's zeros select the defaults of mpt_adaptive_params.
 * Afterwards each tile holds, bit for bit, the sum that mpt_render_nee of [b, b + count(tile)) adds to a cleared sum (same walk, clamp,
 * BSDF mode and light sampling); mpt_read_tile_samples gives the counts and mpt_read_moments the moments of exactly those samples.
 * MPT_DISPLAY_ADAPTIVE, mpt_denoise with the adaptive mean and mpt_read_sum read the same buffers and work unchanged.  Like
 * mpt_render_nee it writes none of: the frame targets, the denoised buffer, the temporal, SVGF, display, AO and direct state.
 * out (may be NULL): samples = pixel samples inside the image; passes = the schedule steps the farthest tile took, the first included;
 * tiles_converged / tiles_at_max as after mpt_render_adaptive — all derived from the tile counts after the kernel.
 * nee_out (may be NULL) and mpt_get_stats: as after mpt_render_nee (paths and rays grow, the timing fields are set, trace_launches = 1).
 * OUT OF SCOPE: shards and more than one GPU, the asynchronous lane, checkpoints of an adaptive render, camera paths.
 * MPT_ERR_INVALID_ARG, with nothing rendered and nothing cleared: every refusal of mpt_render_nee (a null p or n, MPT_RNG_LITERAL,
 * MPT_BSDF_SCATTER_ALL, shards, flags != 0, max_depth < 1 or > 32, a bad walk, a NaN clamp, sample_begin + sample_count > 2^27) and every
 * refusal of mpt_render_adaptive (a null a, min_samples == 1, a negative or NaN threshold, N < 2).  MPT_ERR_NOT_READY before scene,
 * uniforms and size; MPT_ERR_BAD_SCENE from the light table, as mpt_direct_lighting.                                                   */
int mpt_render_nee_adaptive(mpt_ctx* ctx, const mpt_render_params* p, const mpt_nee_params* n, const mpt_adaptive_params* a,
                            mpt_adaptive_info* out /* may be NULL */, mpt_nee_info* nee_out /* may be NULL */);

/* ---- light sampling: a sphere light by the solid angle it subtends ---------------------------------------------------------------------
 * A property of the context, host state only: how mpt_direct_lighting, mpt_direct_image and mpt_render_nee sample a SPHERE light.  It is
 * read at the start of each of the three calls.  MPT_LIGHT_SAMPLING_AREA (the default) is the rule of the two sections above, bit for bit.
 * The setting survives mpt_resize, mpt_upload_scene, mpt_build_and_upload and mpt_clear_sum and does not make the light table stale; the
 * table, mpt_read_lights and the selection of light k (by power, from u01(r.x)) are the same in both modes, and a TRIANGLE light is
 * sampled exactly as above in both.  A bad mode: MPT_ERR_INVALID_ARG, nothing changed.  tests/cone_ref.py restates the rule in numpy.
 *
 * MPT_LIGHT_SAMPLING_CONE.  Uniform over a sphere's whole surface, half of the points face away and the rest carry the full cos_l / d2
 * spread; uniform in the cone of directions the sphere subtends, every direction meets the sphere and the factor is cos_s times a
 * constant of the shading point.  float32, one IEEE operation at a time in the order written; dot, normalize, u01 and sincos_2pi as above.
 * For a sphere light (c, r) drawn as light k, from the origin o and normal n of the area rule, with u1 = u01(r.y), u2 = u01(r.z) of the
 * same Philox block (direct pass: word 2 = 0xFFFFFFFD; NEE: word 3 = 1):
 *   w = c - o,  dc2 = dot(w, w),  r2 = r * r
 *   the sample is SKIPPED unless dc2 > r2 (a NaN skips): a point inside or on the sphere gets nothing, as under AREA
 *   s2 = r2 / dc2,  cm = sqrt(1 - s2),  omc = s2 / (1 + cm)              (1 - cos(theta_max), without the cancellation)
 *   k = u1 * omc,  ct = 1 - k,  st = sqrt(k * (2 - k)),  (sn, cs) = sincos_2pi(u2)
 *   dc = sqrt(dc2),  wc = w * (1 / dc);  the frame (t1, t2, wc) of Duff et al. 2017 ("Building an Orthonormal Basis, Revisited"):
 *     sg = wc.z >= 0 ? 1 : -1,  a = -1 / (sg + wc.z),  b = (wc.x * wc.y) * a
 *     t1 = (1 + ((sg * wc.x) * wc.x) * a,  sg * b,  -(sg * wc.x)),   t2 = (b,  sg + (wc.y * wc.y) * a,  -wc.y)
 *   wi = normalize(((st * cs) * t1 + (st * sn) * t2) + ct * wc)          (scalar * vector, vector + vector: per component)
 *   dist = dc * ct - sqrt(dc2 * ((omc * (1 - u1)) * ((2 - omc) - k)))    (the near intersection of the sphere.  The root's argument is
 *     r2 - dc2 st^2 = dc2 (sin^2(theta_max) - st^2) = dc2 (omc - k) (2 - omc - k) with omc - k = omc (1 - u1) and 1 - u1 exact: a product
 *     of factors, where the difference written out loses every digit at the cone's edge)
 *   cos_s = dot(n, wi);  the sample is also SKIPPED unless cos_s > 0 && dist > 0
 *   the shadow ray is any-hit(o, wi, tmax = dist * 0.9990234375f), the margin of the area rule
 *   J = omc * (inv_pdf[k] / ((2 * r) * r))     (the reciprocal of the solid-angle pdf 1 / (2 pi omc), selection included: inv_pdf = A / p_k,
 *                                               A = 4 pi r^2)
 * Direct pass, not occluded: w = cos_s * J, S += (Le.r * w, Le.g * w, Le.b * w) — where the area rule has w = g * inv_pdf[k].  The
 *   counts and rgba = ((albedo.c * 0.31830987f) * (S.c / (float)N), 1) are unchanged.
 * mpt_render_nee, the light sample, not occluded:  pbs = cos_s * 0.31830987f,  q = pbs * J,  wl = 1 / (1 + q * q),  m = (cos_s * J) * wl,
 *   L.c += ((thr.c * albedo.c) * 0.31830987f) * (Le_k.c * m).
 * mpt_render_nee, the emission of sphere light k of the table that a bounce found (sampled, front), with o the origin of the ray that
 *   found it: dc2, r2, omc and J as above from the table's c, r and inv_pdf[k].  !(dc2 > r2): w = 1.  Otherwise q = 1 / (J * pb),
 *   w = 1 / (1 + q * q).  Neither t nor cos_l enters.
 * Everything else — sampled, pb, the attempt rule b + 1 < max_depth, specular vertices, the sky, the clamp, the sample order, the
 * counts — is the area contract's.
 * KNOWN LIMIT.  Where dist exceeds the distance at which the walk itself meets the sphere by more than the 2^-10 margin of tmax, the
 * sample is counted as occluded (by its own light).  Two places: within about 1e-4 * r of the sphere's surface, where dc * ct and the root
 * cancel, and a direction within a few ulp of the cone's edge, where the near intersection of the ROUNDED direction moves by the square
 * root of that rounding.  Measured in float32 on the CPU, 2 * 10^6 samples per band, |dist - exact near root| / root along the rounded wi:
 *   1e-4 r .. 1e-3 r from the surface: 99.99 % within 1.3e-3, the largest 1.2e-2
 *   1e-3 r .. 1e-2 r:                  99.99 % within 1.5e-4, the largest 1.8e-3
 *   1e-2 r .. 100 r:                   99.99 % within 1.5e-5, the largest 1.6e-4
 * tests/test_cone_cpu.py holds dist to 2^-11 of that root over 2 * 10^5 points spread evenly in log distance from 1e-3 r to 100 r.       */
enum { MPT_LIGHT_SAMPLING_AREA = 0, MPT_LIGHT_SAMPLING_CONE = 1 };
int mpt_set_light_sampling(mpt_ctx* ctx, int32_t mode);
int mpt_get_light_sampling(mpt_ctx* ctx, int32_t* mode);

/* ---- light candidates: resampled light sampling (RIS) ---------------------------------------------------------------------------------
 * A property of the context, host state only, with the life of mpt_set_light_sampling: from how many CANDIDATES m a light sample of
 * mpt_direct_lighting, mpt_direct_image and mpt_render_nee is resampled.  It is read at the start of each of the three calls, survives
 * mpt_resize, mpt_upload_scene, mpt_build_and_upload and mpt_clear_sum and does not make the light table stale.  m = 1 (the default)
 * is the contract of the sections above and launches their kernels: every result is theirs bit for bit.  m = 0, m >
 * MPT_LIGHT_CANDIDATES_MAX or a null pointer: MPT_ERR_INVALID_ARG, nothing changed.  mpt_render_nee_adaptive with m > 1 returns
 * MPT_ERR_INVALID_ARG with nothing rendered and nothing cleared (OUT OF SCOPE: the adaptive loop draws one sample per vertex).
 * tests/ris_ref.py restates the rule in numpy.
 *
 * m >= 2.  A light sample is drawn blind — a light by power, a point uniformly on it — and a full any-hit walk is paid for whatever
 * comes out.  Here m candidates are drawn that way, each is weighted by the light it would deliver unshadowed, one is kept in
 * proportion to that weight in a streaming reservoir of one, and ONE shadow ray is traced.  float32, one IEEE operation at a time in the
 * order written.  Everything not named below is the m = 1 contract under the light-sampling mode in effect: the selection by cdf, the
 * sample geometry of a triangle and of a sphere (area or cone), the skip rule, tmax = dist * 0.9990234375f, sampled, pb, the weight of
 * an emitter a bounce finds, the clamp, the sample order, the sky.
 *
 * Direct pass.  Per surface pixel and sample s: wsum = 0, nothing taken.  For j = 0 .. m-1, ascending:
 *   r_j = philox4x32_10(counter = (py*W+px, s, 0xFFFFFFFD, j), key)       (j = 0 is the m = 1 block; word 2 = 0xFFFFFFFD is nobody else's)
 *   candidate j: light k_j from u01(r_j.x), its point or direction from (u01(r_j.y), u01(r_j.z)), formed from o and n exactly as the
 *     m = 1 sample: ok_j (the sample would not be skipped), wi_j, dist_j and its factor
 *       fac_j = ((cos_s * cos_l) / d2) * inv_pdf[k_j]      a triangle; a sphere under AREA
 *       fac_j = cos_s * J                                  a sphere under CONE
 *   l_j = (0.2126f * Le.r + 0.7152f * Le.g) + 0.0722f * Le.b               (Le of light k_j, from the table)
 *   w_j = l_j * fac_j;  the candidate COUNTS iff ok_j && w_j > 0 && w_j < +inf (a NaN does not); one that does not changes nothing
 *   a candidate that counts: wsum = wsum + w_j; it is TAKEN iff nothing has been taken yet or u01(r_j.w) * wsum < w_j (r.w is the one
 *     word the m = 1 sample leaves unused); taking it keeps wi_j, dist_j, Le_j and l_j as (wi_y, dist_y, Le_y, l_y)
 * The sample is SKIPPED (no ray, not counted) unless a candidate was taken.  Otherwise traced += 1 and the shadow ray is
 * any-hit(o, wi_y, dist_y * 0.9990234375f); not occluded: unoccluded += 1, Fy = (wsum / (float)m) / l_y,
 * S += (Le_y.r * Fy, Le_y.g * Fy, Le_y.b * Fy).  rgba, the counts, the totals and the result's lifetime are unchanged.
 *
 * mpt_render_nee.  At a Lambert vertex where a light sample is attempted, the same loop over the blocks philox(p, s, b, 1 + j) (every
 * other block has word 3 = 0; j = 0 is the m = 1 block), from the origin o' and the normal n.  The candidate's factor is the m_j of the
 * m = 1 rule — the factor times its power-heuristic weight wl against pbs, in the area or the cone form — and w_j = l_j * m_j; counting,
 * taking and skipping as above.  shadow_rays grows by one per vertex that took a candidate.  Not occluded:
 *   Fy = (wsum / (float)m) / l_y,   L.c += ((thr.c * albedo.c) * 0.31830987f) * (Le_y.c * Fy)
 * added where the m = 1 contribution is added.  sampled = attempt and pb are unchanged, and the emitter branch is the m = 1 branch.
 *
 * UNBIASED.  The target is p^ = l * fac (l * fac * wl in the render), the source pdf p is the m = 1 pdf, w_j = p^ / p, and the estimate
 * is f(y) / p^(y) * (1/m) sum w_j with f = Le * fac * V: resampled importance sampling (Talbot et al. 2005), unbiased as p^ > 0
 * wherever f != 0.  In the render the two MIS weights stay functions of the sampled point alone and still sum to 1.                   */
#define MPT_LIGHT_CANDIDATES_MAX 32u
int mpt_set_light_candidates(mpt_ctx* ctx, uint32_t m);   /* 1..MPT_LIGHT_CANDIDATES_MAX; default 1 */
int mpt_get_light_candidates(mpt_ctx* ctx, uint32_t* m);

/* ---- spatial reservoir reuse (ReSTIR) in the direct pass -------------------------------------------------------------------------------
 * mpt_direct_restir is the direct pass with m candidates per sample (m: the context's mpt_set_light_candidates setting, read at the
 * start of the call; m = 1 runs the same candidate loop) in which a pixel does not forget its candidates: in every round it merges its
 * one-sample reservoir with those of K nearby pixels that see the same surface (Bitterli et al. 2020, "Spatiotemporal reservoir
 * resampling", the spatial part).  Only a reservoir whose sample was found visible carries weight.  A new call with state of its own: no
 * other call, result or kernel changes.  tests/restir_ref.py restates the section in numpy.  float32, one IEEE operation at a time in the
 * order written; dot, normalize, u01, sincos_2pi, philox and the origin o as in the direct-lighting section.
 * OUT OF SCOPE: mpt_render_nee, cone sampling, the adaptive calls.  Temporal reuse over a camera path is a call of its own,
 * mpt_direct_restir_temporal (the "temporal reservoir reuse" section below).  The pass samples lights by AREA only: under MPT_LIGHT_SAMPLING_CONE the call returns
 * MPT_ERR_INVALID_ARG, because a direction drawn in one point's cone is not a sample for another point.
 *
 * Surface pixels, emitters, misses, o, n and the final rgba = ((albedo.c * 0.31830987f) * (S.c / (float)N), 1) are the direct pass's.
 * A RESERVOIR of pixel q in round s is EMPTY or HOLDS (k, ua, ub, wsum_q, fac_q): the light, the two uniforms u01(r.y), u01(r.z) the kept
 * candidate was formed from, the running weight, and the kept candidate's factor ((cos_s * cos_l) / d2) * inv_pdf[k] at q.  The uniforms
 * are stored, not the point, so "sample y seen from another pixel" is the candidate's geometry with another (o, n).
 *
 * Per round s in [sample_begin, sample_begin + N), ascending:
 * Step A (every surface pixel p, before any pixel's step B of the round).  The candidate loop of the light-candidates section for the
 *   direct pass — blocks (pixel, s, 0xFFFFFFFD, j), j < m, area geometry — remembering k, ua, ub and fac of the kept candidate.  Nothing
 *   taken: EMPTY, no ray.  Otherwise traced += 1, the ray is any-hit(o_p, wi_y, dist_y * 0.9990234375f); occluded: EMPTY; not occluded:
 *   unoccluded += 1 and the reservoir HOLDS.
 * Step B.  held = the own reservoir holds; if so y = its sample, Wp = wsum_p, own = true; else Wp = 0.  For i = 0 .. K-1, ascending:
 *   r_i = philox4x32_10(counter = (py*W+px, s, 0xFFFFFFFC, i), key)          (word 2 = 0xFFFFFFFC is nobody else's)
 *   dx = min((int)(u01(r_i.x) * (float)(2R+1)), 2R) - R, dy likewise from r_i.y;  q = (px + dx, py + dy)
 *   neighbour i is ACCEPTED iff (dx, dy) != (0, 0), q lies inside the image, q is class 0, dot(n_p, n_q) >= normal_threshold and
 *     |t_q - t_p| <= depth_tolerance * t_p
 *   ACCEPTED and q HOLDS: the light sample of (k_q, ua_q, ub_q) is formed from (o_p, n_p) exactly as a candidate is; fac its factor;
 *     w = wsum_q * (fac / fac_q); it COUNTS iff ok && w > 0 && w < +inf
 *   it counts: Wp = Wp + w; it is TAKEN iff !held || u01(r_i.z) * Wp < w; taking sets y = q's sample, own = false; then held = true
 *   Not held: the round adds nothing and traces nothing more.
 * Step C.  own: y's visibility is known, no ray.  Otherwise traced += 1, the ray is any-hit(o_p, wi_y, dist_y * 0.9990234375f) with y
 *   formed from (o_p, n_p); occluded: the round ends; not occluded: unoccluded += 1.
 * Step D.  c = 1 (the pixel itself).  For every ACCEPTED neighbour i, ascending, holding or not: y formed from (o_q, n_q); if
 *   ok && fac > 0 && fac < +inf:   MPT_RESTIR_BIASED: c += 1.   MPT_RESTIR_UNBIASED: traced += 1, the ray is
 *   any-hit(o_q, wi, dist * 0.9990234375f); not occluded: unoccluded += 1, c += 1.
 * Step E.  Fy = (Wp / (float)(m * c)) / l_y,  S += (Le_y.r * Fy, Le_y.g * Fy, Le_y.b * Fy)    (l_y as in the light-candidates section;
 *   the geometry factor cancels between the target and the integrand, hence the RIS pass's shape)
 *
 * With K = 0, or when no neighbour is accepted, rgba, traced and unoccluded are bit for bit mpt_direct_lighting's for m >= 2.
 * UNBIASED is the 1/Z weighting of Bitterli et al., Alg. 6: the visibility test is inside the count because step A discarded occluded
 * samples, and the pixel's own candidates cover every y with f_p(y) != 0.  BIASED omits the K correction rays: it counts a neighbour that
 * could not have seen y, so it is wrong exactly there and DARKENS the image at visibility edges (penumbrae, contact shadows).
 *
 * Parameters: neighbours K in 0..MPT_RESTIR_MAX_NEIGHBOURS (0: no reuse), radius R in 1..MPT_RESTIR_MAX_RADIUS pixels (0: the default),
 * normal_threshold and depth_tolerance (<= 0: the defaults, the temporal stage's).
 * The call waits for queued renders, refreshes stale guides and the stale light table, and writes no other stage's state — not the
 * direct pass's, not mpt_stats.  Its result has the direct result's lifetime: dropped by mpt_resize, mpt_upload_scene and
 * mpt_build_and_upload.  MPT_ERR_INVALID_ARG with nothing changed: null params, sample_count outside 1..MPT_DIRECT_MAX_SAMPLES, a bad
 * walk or mode, K > 16, R > 64, a NaN threshold or tolerance, cone sampling in effect.  MPT_ERR_NOT_READY and MPT_ERR_BAD_SCENE as the
 * direct pass.
 * mpt_restir_info: traced summed over the image = rays_initial + rays_final + rays_correction; rays_occluded of all three kinds;
 * neighbours_accepted counts step B's accepted neighbours over surface pixels and rounds, samples_from_neighbours the pixel-rounds whose
 * step B ended with a neighbour's sample.
 * Test hooks.  mpt_restir_image: the same kernels on caller guides, as mpt_direct_image (needs a scene and no size).
 * mpt_read_restir_reservoirs: the LAST round's reservoirs, six words per pixel — k, the bits of ua, ub, wsum, fac, and flags (bit 0 =
 * holds, bit 1 = own).  which = 0: after step A (bit 1 never set).  which = 1: the pick after step B — wsum is Wp, fac the sample's
 * factor at this pixel.  A reservoir that does not hold is six zero words.                                                            */
#define MPT_RESTIR_MAX_NEIGHBOURS 16u
#define MPT_RESTIR_MAX_RADIUS 64u
#define MPT_RESTIR_DEFAULT_RADIUS 4u   /* the smallest radius measured was the best at every K */
#define MPT_RESTIR_DEFAULT_NORMAL_THRESHOLD 0.5f
#define MPT_RESTIR_DEFAULT_DEPTH_TOLERANCE 0.05f
enum { MPT_RESTIR_UNBIASED = 0, MPT_RESTIR_BIASED = 1 };
typedef struct mpt_restir_params {
    uint32_t sample_begin, sample_count;   /* rounds N: 1..MPT_DIRECT_MAX_SAMPLES                                                      */
    uint32_t seed_lo, seed_hi;
    int32_t walk;                          /* MPT_WALK_*                                                                               */
    uint32_t neighbours;                   /* K: 0..MPT_RESTIR_MAX_NEIGHBOURS                                                          */
    uint32_t radius;                       /* R: 1..MPT_RESTIR_MAX_RADIUS, 0 = MPT_RESTIR_DEFAULT_RADIUS                               */
    int32_t mode;                          /* MPT_RESTIR_UNBIASED or MPT_RESTIR_BIASED                                                 */
    float normal_threshold, depth_tolerance;   /* <= 0: the defaults                                                                   */
} mpt_restir_params;
typedef struct mpt_restir_info {
    uint64_t pixels_surface, rays_initial, rays_final, rays_correction, rays_occluded, neighbours_accepted, samples_from_neighbours, lights;
    double device_ms;                      /* HIP-event time of the rounds (guide refresh and table build not included)                */
} mpt_restir_info;
int mpt_direct_restir(mpt_ctx* ctx, const mpt_restir_params* params, mpt_restir_info* out /* may be NULL */);
int mpt_read_restir(mpt_ctx* ctx, float* rgba /* W*H*4 */, uint32_t* traced /* W*H, may be NULL */, uint32_t* unoccluded /* may be NULL */);
int mpt_restir_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);   /* the RGBA32F image, laid out as the HDR sum                */
int mpt_restir_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* albedo_depth, const float* normal_class,
                     const mpt_uniforms* cam_uniforms, const mpt_restir_params* params, float* rgba_out, uint32_t* traced_out,
                     uint32_t* unoccluded_out);
int mpt_read_restir_reservoirs(mpt_ctx* ctx, int32_t which, uint32_t* out /* W*H*6 */);

/* ---- temporal reservoir reuse in the direct pass over a camera path ---------------------------------------------------------------
 * mpt_direct_restir_temporal is one FRAME of the direct pass in which a pixel does not forget last frame's candidates: one round, m
 * candidates (the context's mpt_set_light_candidates setting, read at the start of the call; it may differ from frame to frame), the
 * pixel's one-sample reservoir merged with the reservoir of the ONE nearest pixel of the previous frame that the pixel's surface point
 * reprojects to (Bitterli et al. 2020, the temporal part).  The candidates of the frames before cost one reprojection and, UNBIASED, one
 * ray.  A new call with state of its own: no other call, result or kernel changes; there is no spatial step in the same frame.
 * tests/restir_temporal_ref.py restates the section in numpy.  float32, one IEEE operation at a time in the order written; dot, u01,
 * philox, the light sample of (k, ua, ub) from any (o, n), its factor fac, l_y, Le and the origin o as in the direct-lighting,
 * light-candidates and spatial sections.  Lights are sampled by AREA only, as there.
 *
 * State per context, two of each, ping-pong, with the lifetime of the mpt_temporal_* history: a reservoir per pixel — two uint4,
 * (k, ua, ub, wsum) (fac, flags, Mh, 0); flags bit 0 = the reservoir HOLDS, bit 1 = the pick was the pixel's own sample; Mh = the count
 * (uint32) of the candidates the reservoir stands for, 0 exactly at pixels that were no surface — the history guide of its frame ((normal
 * facing the ray, t), t = +inf for a miss) and that frame's fourteen camera floats.  Allocated by the first call; dropped by mpt_resize,
 * mpt_upload_scene, mpt_build_and_upload and mpt_restir_temporal_reset.  The scene is static while a history lives: that is why a ray
 * from last frame's surface point may be traced in the current scene.
 *
 * C = max_history, primes mark the history's camera.  For every surface pixel p (class 0) of the frame:
 * Step A.  The spatial step A with s = frame, for every pixel before any pixel's step T: the own reservoir HOLDS
 *   (k, ua, ub, wsum_p, fac_p) iff something was taken and its shadow ray arrives.
 * Step T, the tap.  No valid history: no tap.  The camera's fourteen floats equal the history's bit for bit: the tap is q = p and no
 *   test applies (step 6 of the temporal section).  Otherwise steps 1-3 of mpt_temporal_accumulate with the hit rule give r, s, fx, fy
 *   under the same conditions (s > 0, s finite, -1 <= fx < W, -1 <= fy < H; a NaN fails them); qx = (int)floor(fx + 0.5f), qy
 *   likewise; the tap COUNTS iff q is inside the image (tested on the integers), the history guide at q is a hit,
 *   |t_q - |r|| <= depth_tolerance * |r| and dot(n_p, n_q) >= normal_threshold.  The tap is ACCEPTED iff it counts and Mh_q > 0.
 * Step B.  held = own = (the own reservoir holds); y = its sample; Wp = wsum_p if it holds, else 0.  ACCEPTED: Mc = min(Mh_q, C * m).
 *   ACCEPTED and q HOLDS: the light sample of (k_q, ua_q, ub_q) formed from (o_p, n_p), fac its factor,
 *     w = (wsum_q * (fac / fac_q)) * ((float)Mc / (float)Mh_q); it COUNTS iff ok && w > 0 && w < +inf
 *   it counts: Wp = Wp + w; it is TAKEN iff !held || u01(r.z) * Wp < w, r = philox4x32_10(counter = (py*W+px, frame, 0xFFFFFFFB, 0), key)
 *     (word 2 = 0xFFFFFFFB is nobody else's); taking sets y = q's sample, own = false, yfac = fac; then held = true
 *   Not held: the frame adds nothing and traces nothing more.
 * Step C.  The spatial step C: own: no ray.  Otherwise traced += 1, the ray is any-hit(o_p, wi_y, dist_y * 0.9990234375f) with y formed
 *   from (o_p, n_p); occluded: the frame adds nothing, traces nothing more and the new reservoir does not hold; else unoccluded += 1.
 * Step D.  Z = m.  ACCEPTED, q holding or not: y formed from (o_q', n_q'), last frame's point at q — the origin o evaluated with the
 *   HISTORY's camera at the integer pixel q with the history guide's t and n: the bits frame f-1 used.  If ok && fac > 0 && fac < +inf:
 *   MPT_RESTIR_BIASED: Z += Mc.  MPT_RESTIR_UNBIASED: traced += 1, the ray is any-hit(o_q', wi, dist * 0.9990234375f); not occluded:
 *   unoccluded += 1, Z += Mc.
 * Step E.  Fy = (Wp / (float)Z) / l_y, S = Le_y * Fy, rgba = ((albedo.c * 0.31830987f) * (S.c / 1.0f), 1).  Mnew = m + (ACCEPTED ? Mc : 0).
 *   The frame went through: the new reservoir HOLDS (yk, yua, yub, Wp * ((float)Mnew / (float)Z), yfac), flags = 1 | own << 1,
 *   Mh = Mnew.  Otherwise it is zeros with Mh = Mnew and S = 0.  A pixel that is no surface stores zeros and rgba = (0, 0, 0, 1).
 *   The new history guide is the current guide, written for every pixel.
 *
 * With no accepted tap, rgba, traced and unoccluded are bit for bit mpt_direct_restir's with K = 0, N = 1, sample_begin = frame.
 * UNBIASED is unbiased because a stored sample passed a shadow ray at its own pixel: the history's support is "visible from o_q' with a
 * positive factor", which is what step D tests — the 1/Z weight of Alg. 6 with the temporal neighbour counted Mc times.  BIASED omits
 * the ray and darkens where last frame's point could not see y.  Frames share samples over time: their noise is correlated, and feeding
 * them to mpt_temporal_accumulate is out of scope, as are a spatial merge in the same frame, more than one round per frame,
 * mpt_render_nee and moving geometry.
 *
 * The call waits for queued renders, refreshes stale guides and the stale light table, and writes no other stage's state.
 * MPT_ERR_INVALID_ARG with nothing changed — the result and the history stay: null params, a bad walk or mode, a NaN threshold or
 * tolerance, max_history > MPT_RESTIR_TEMPORAL_MAX_HISTORY, cone sampling in effect.  MPT_ERR_NOT_READY and MPT_ERR_BAD_SCENE as the
 * direct pass.
 * mpt_restir_temporal_info: traced summed over the image = rays_initial + rays_final + rays_correction; rays_occluded of all three
 * kinds; history_accepted = surface pixels with an ACCEPTED tap, pixels_reset the other surface pixels; samples_from_history = the
 * pixels whose step B ended with the history's sample.
 * Read-backs and hooks.  mpt_read_restir_temporal_reservoirs: the frame's reservoirs, seven words per pixel — k, the bits of ua, ub,
 * wsum, fac, then flags and Mh.  mpt_restir_temporal_image: the same kernels on caller arrays (needs a scene and no size; never touches
 * the context's history): reservoirs_prev = W*H*7 words in that format, or NULL = no history (the three other *_prev arguments are
 * ignored); a holding reservoir whose k is no light of the table is MPT_ERR_INVALID_ARG.                                              */
#define MPT_RESTIR_TEMPORAL_DEFAULT_HISTORY 20u   /* Bitterli et al.'s cap */
#define MPT_RESTIR_TEMPORAL_MAX_HISTORY 1024u
typedef struct mpt_restir_temporal_params {
    uint32_t frame;                        /* Philox counter word 1, where the spatial pass has s                                      */
    uint32_t seed_lo, seed_hi;
    int32_t walk;                          /* MPT_WALK_*                                                                               */
    int32_t mode;                          /* MPT_RESTIR_UNBIASED or MPT_RESTIR_BIASED                                                 */
    uint32_t max_history;                  /* C: 1..MPT_RESTIR_TEMPORAL_MAX_HISTORY, 0 = MPT_RESTIR_TEMPORAL_DEFAULT_HISTORY           */
    float normal_threshold, depth_tolerance;   /* <= 0: MPT_RESTIR_DEFAULT_*                                                           */
} mpt_restir_temporal_params;
typedef struct mpt_restir_temporal_info {
    uint64_t pixels_surface, rays_initial, rays_final, rays_correction, rays_occluded, history_accepted, samples_from_history, pixels_reset,
        lights;
    double device_ms;                      /* HIP-event time of the two launches (guide refresh and table build not included)          */
} mpt_restir_temporal_info;
int mpt_direct_restir_temporal(mpt_ctx* ctx, const mpt_restir_temporal_params* params, mpt_restir_temporal_info* out /* may be NULL */);
int mpt_read_restir_temporal(mpt_ctx* ctx, float* rgba /* W*H*4 */, uint32_t* traced /* W*H, may be NULL */, uint32_t* unoccluded /* may be NULL */);
int mpt_restir_temporal_buffer(mpt_ctx* ctx, void** device_ptr, uint64_t* bytes);   /* the RGBA32F image, laid out as the HDR sum      */
int mpt_read_restir_temporal_reservoirs(mpt_ctx* ctx, uint32_t* out /* W*H*7 */);
int mpt_restir_temporal_reset(mpt_ctx* ctx);
int mpt_restir_temporal_image(mpt_ctx* ctx, uint32_t width, uint32_t height, const float* albedo_depth_cur, const float* normal_class_cur,
                              const mpt_uniforms* cam_cur, const float* albedo_depth_prev, const float* normal_class_prev,
                              const mpt_uniforms* cam_prev, const uint32_t* reservoirs_prev /* W*H*7, or NULL */,
                              const mpt_restir_temporal_params* params, float* rgba_out, uint32_t* traced_out /* may be NULL */,
                              uint32_t* unoccluded_out /* may be NULL */, uint32_t* reservoirs_out /* W*H*7, may be NULL */,
                              mpt_restir_temporal_info* out /* may be NULL */);

/* RNG known-answer hooks evaluated ON THE DEVICE (Random.h:6-16 and the philox / sincos spec).      */
int mpt_kat_pcg(mpt_ctx* ctx, const uint32_t* seeds, uint64_t n, uint32_t* hash_out, float* float_out);
int mpt_kat_philox(mpt_ctx* ctx, const uint32_t* ctr4, const uint32_t* key2, uint64_t n, uint32_t* out4);
int mpt_kat_sincos(mpt_ctx* ctx, const float* u, uint64_t n, float* sin_out, float* cos_out);
/* The reciprocal of the hot path (1.0 / r.direction[i], PathTracing.h:61; 1 / a of the triangle test, :153-165): the kernels' short
 * form (v_rcp_f32 + the compiler's own fma chain, without v_div_scale / v_div_fixup) against the correctly rounded division, over ALL
 * 2^32 operands, on the device.  out4 = {mismatches inside the range the kernels use the short form in, operands in that range,
 * mismatches outside it, operands outside it}; out4[0] must be 0.                                                                   */
int mpt_kat_rcp(mpt_ctx* ctx, uint64_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* MPT_H */
