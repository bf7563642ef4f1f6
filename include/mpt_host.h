/* mpt_host.h — C ABI of the HOST layer (libmpt_host.so): scene ingest, BVH build, buffer packing,
 * camera/viewport maths, the Renderer frame protocol and image output.  Pure host C++ underneath
 * (metalpathtracer_amd/csrc/host/); the Renderer entry points drive the GPU through include/mpt.h.
 *
 * Reference interfaces replaced (R/ = "MetalCpp Path Tracer/"):
 *   mpt_scene_*        class Scene                      R/Scene/Scene.h:34-188
 *   mpt_scene_load_xml SceneLoader::LoadSceneFromXML    R/Scene/SceneLoader.h:11, SceneLoader.cpp:75-133
 *   mpt_camera_*       namespace Camera + recalculateViewport   R/Renderer/Camera.h:24-32, Renderer.cpp:153-182
 *   mpt_renderer_*     class Renderer                   R/Renderer/Renderer.h:16-29
 */
#ifndef MPT_HOST_H
#define MPT_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "mpt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpt_scene mpt_scene;
typedef struct mpt_renderer mpt_renderer;

enum { MPT_BVH_REFERENCE_SWEEP = 0, MPT_BVH_BINNED_CENTROID = 1,
       MPT_BVH_GPU_LBVH = 2 /* built on the GPU by mpt_build_bvh (include/mpt.h); needs a device */ };
enum { MPT_PRIM_SPHERE = 0, MPT_PRIM_TRIANGLE = 1 };

/* Scene (R/Scene/Scene.h) */
int mpt_scene_create(mpt_scene** out);
int mpt_scene_destroy(mpt_scene* s);
int mpt_scene_clear(mpt_scene* s);
/* returns SceneLoader::Status (0 ok, 1 xml unreadable, 2 no <Scene>, 3 malformed, 4 mesh unreadable);
 * what the reference would printf is copied (NUL-terminated, truncated) into log when log_cap > 0 */
int mpt_scene_load_xml(mpt_scene* s, const char* xml_path, const char* asset_root, char* log, size_t log_cap);
/* type: MPT_PRIM_*; sphere: d0 centre, d1[0] radius; triangle: three vertices; mat: albedo rgb, materialType,
 * emission rgb, emissionPower */
int mpt_scene_add_primitive(mpt_scene* s, int type, const float d0[3], const float d1[3], const float d2[3],
                            const float mat[8]);
int mpt_scene_build_bvh(mpt_scene* s, int mode);
/* Scene::sortPrimitives: spheres before triangles, stable — the first thing Scene::buildBVH does (R/Scene/Scene.h:72-75),
 * and all that mpt_build_and_upload needs of it (primitive ids are the positions after this sort).  Drops a host tree. */
int mpt_scene_sort_primitives(mpt_scene* s);
int mpt_scene_counts(const mpt_scene* s, uint64_t* prims, uint64_t* triangles, uint64_t* nodes, int32_t* depth);
/* copies the four flat buffers: bvh 8 floats/node, prims 12 floats/prim, mats 8 floats/prim,
 * prim_idx 1 int/prim; any pointer may be NULL to skip */
int mpt_scene_copy_buffers(const mpt_scene* s, float* bvh, float* prims, float* mats, int32_t* prim_idx);

/* Camera (R/Renderer/Camera.h:24-32) + viewport (R/Renderer/Renderer.cpp:153-182).  Writes cameraPosition,
 * viewportU/V, firstPixelPosition and screenSize of *u; other fields untouched. */
int mpt_camera_reset_values(float pos[3], float fwd[3], float up[3], float* vfov_deg);
int mpt_camera_viewport(const float pos[3], const float fwd[3], const float up[3], float vfov_deg, float width,
                        float height, mpt_uniforms* u);
/* host PCG stream behind Renderer::updateUniforms' randomSeed (R/Renderer/Renderer.cpp:30-41) */
float mpt_host_random_float(uint32_t* state);

/* Renderer (R/Renderer/Renderer.h:16-29) — constructor order of Renderer.cpp:43-57 */
int mpt_renderer_create(int device, const char* xml_path, const char* asset_root, mpt_renderer** out, char* err,
                        size_t err_cap);
int mpt_renderer_destroy(mpt_renderer* r);
int mpt_renderer_drawable_size_will_change(mpt_renderer* r, uint32_t width, uint32_t height);
int mpt_renderer_set_params(mpt_renderer* r, const mpt_render_params* p);
int mpt_renderer_draw(mpt_renderer* r);                       /* updateUniforms + one frame              */
/* InputSystem state consumed by the next draw (R/Window/InputSystem.h:11-21, R/Renderer/Camera.h:75-89): any
 * non-zero input moves the camera, which resets frameCount and draws a new randomSeed (Renderer.cpp:255-257)   */
int mpt_renderer_input(mpt_renderer* r, const float move[3], const float rotate[2], float zoom, int reset);
int mpt_renderer_read_frame(mpt_renderer* r, float* rgba);    /* W*H*4 floats                            */
int mpt_renderer_render_batch(mpt_renderer* r, uint32_t sample_begin, uint32_t sample_count);
int mpt_renderer_read_sum(mpt_renderer* r, float* rgba);
int mpt_renderer_clear_sum(mpt_renderer* r);
int mpt_renderer_uniforms(mpt_renderer* r, mpt_uniforms* out);
int mpt_renderer_stats(mpt_renderer* r, mpt_stats* out);
/* mpt_denoise + mpt_read_denoised of what was rendered last: the FRAME source after mpt_renderer_draw, the SUM after
 * mpt_renderer_render_batch (params->source is ignored; params->samples = 0 means the samples rendered since the sum was
 * last cleared).  rgba: W*H*4 floats.                                                                                  */
int mpt_renderer_denoise(mpt_renderer* r, const mpt_denoise_params* params, float* rgba);
/* mpt_render_adaptive with the renderer's params and uniforms: samples [sample_begin, sample_begin + max_samples) at most per tile,
 * the counts per tile through mpt_read_tile_samples(mpt_renderer_context(r), ...).  out may not be NULL.                         */
int mpt_renderer_render_adaptive(mpt_renderer* r, uint32_t sample_begin, uint32_t max_samples, const mpt_adaptive_params* params,
                                 mpt_adaptive_info* out);
/* One frame of temporal accumulation (mpt_temporal_accumulate, include/mpt.h): consumes the pending input as mpt_renderer_draw does,
 * clears the sum, renders samples_per_frame philox samples starting at frame * samples_per_frame — the frame counter is never reset
 * by camera motion, so no two frames share samples — and blends them into the history reprojected from the previous frame's camera.
 * params (may be NULL: keep the renderer's, initially the defaults): max_history and the tolerances; source / samples are ignored.
 * out may be NULL.  mpt_renderer_read_temporal: the history (rgb, a = its length); mpt_renderer_denoise_temporal:
 * mpt_denoise_temporal + mpt_read_denoised.  rgba: W*H*4 floats.                                                                  */
int mpt_renderer_draw_temporal(mpt_renderer* r, uint32_t samples_per_frame, const mpt_temporal_params* params, mpt_temporal_info* out);
int mpt_renderer_read_temporal(mpt_renderer* r, float* rgba);
int mpt_renderer_denoise_temporal(mpt_renderer* r, const mpt_denoise_params* params, float* rgba);
/* One frame of SVGF (mpt_svgf_accumulate, include/mpt.h), with the frame numbering of mpt_renderer_draw_temporal (the two share the
 * counter: samples frame * samples_per_frame onwards, never reset by camera motion).  params (may be NULL: keep the renderer's,
 * initially the defaults): everything but source / samples, which are ignored.  out may be NULL.  mpt_renderer_read_svgf: the
 * filtered frame (rgb, a = the history length), W*H*4 floats.                                                                    */
int mpt_renderer_draw_svgf(mpt_renderer* r, uint32_t samples_per_frame, const mpt_svgf_params* params, mpt_svgf_info* out);
int mpt_renderer_read_svgf(mpt_renderer* r, float* rgba);
/* mpt_display + mpt_read_display (include/mpt.h) of params->source as given; for MPT_DISPLAY_SUM, params->samples = 0 means the
 * samples rendered since the sum was last cleared.  rgba8: W*H*4 bytes.  out may be NULL.                                        */
int mpt_renderer_display(mpt_renderer* r, const mpt_display_params* params, uint8_t* rgba8, mpt_display_info* out);
/* mpt_ambient_occlusion + mpt_read_ao (include/mpt.h) for the renderer's camera: `samples` shadow rays per surface pixel numbered from
 * 0, keyed by the render parameters' seed, radius <= 0 = no limit, MPT_WALK_AUTO.  ao: W*H floats (1 = open).  out may be NULL.     */
int mpt_renderer_ambient_occlusion(mpt_renderer* r, uint32_t samples, float radius, float* ao, mpt_ao_info* out);
/* mpt_direct_lighting + mpt_read_direct (include/mpt.h) for the renderer's camera: `samples` light samples per surface pixel numbered
 * from 0, keyed by the render parameters' seed, `walk` one of MPT_WALK_*.  rgba: W*H*4 floats.  out may be NULL.                     */
int mpt_renderer_direct_lighting(mpt_renderer* r, uint32_t samples, int32_t walk, float* rgba, mpt_direct_info* out);
/* mpt_direct_restir + mpt_read_restir (include/mpt.h) for the renderer's camera: mpt_renderer_direct_lighting with spatial reservoir
 * reuse — `neighbours` 0..16 per round from within `radius` pixels (0 = the default), `mode` MPT_RESTIR_UNBIASED or MPT_RESTIR_BIASED,
 * the default thresholds.  rgba: W*H*4 floats.  out may be NULL.                                                                       */
int mpt_renderer_direct_restir(mpt_renderer* r, uint32_t samples, uint32_t neighbours, uint32_t radius, int32_t mode, int32_t walk, float* rgba,
                               mpt_restir_info* out);
/* mpt_direct_restir_temporal + mpt_read_restir_temporal (include/mpt.h) for the renderer's camera: frame number `frame` of a camera
 * path with the pending mpt_renderer_input applied, its reservoirs merged with the previous frame's — `max_history` 1..1024 (0 = the
 * default), `mode` MPT_RESTIR_UNBIASED or MPT_RESTIR_BIASED, the default thresholds, the context's light candidates.  rgba: W*H*4
 * floats.  out may be NULL.                                                                                                           */
int mpt_renderer_direct_restir_temporal(mpt_renderer* r, uint32_t frame, uint32_t max_history, int32_t mode, int32_t walk, float* rgba,
                                        mpt_restir_temporal_info* out);
/* mpt_render_nee (include/mpt.h) for the renderer's camera and render parameters: samples [0, spp) onto the HDR sum (read it with
 * mpt_renderer_read_sum) at max_depth `depth`, `walk` one of MPT_WALK_*, clamp <= 0 = no per-sample clamp.  out may be NULL.          */
int mpt_renderer_render_nee(mpt_renderer* r, uint32_t spp, int32_t depth, int32_t walk, float clamp, mpt_nee_info* out);
/* mpt_set_light_sampling (include/mpt.h) on the renderer's context: MPT_LIGHT_SAMPLING_AREA (the default) or MPT_LIGHT_SAMPLING_CONE for
 * the two calls above.  A bad mode: MPT_ERR_INVALID_ARG, nothing changed.                                                             */
int mpt_renderer_set_light_sampling(mpt_renderer* r, int32_t mode);
/* mpt_set_light_candidates / mpt_get_light_candidates (include/mpt.h) on the renderer's context: from how many candidates, 1 (the
 * default) to MPT_LIGHT_CANDIDATES_MAX, a light sample of the same two calls is resampled.  m outside that range or a null pointer:
 * MPT_ERR_INVALID_ARG, nothing changed.  mpt_renderer_render_nee_adaptive refuses m > 1.                                              */
int mpt_renderer_set_light_candidates(mpt_renderer* r, uint32_t m);
int mpt_renderer_get_light_candidates(mpt_renderer* r, uint32_t* m);
/* mpt_render_nee_adaptive (include/mpt.h) for the renderer's camera and render parameters: samples [0, max_samples) at most per 8x8 tile
 * at max_depth `depth`, stopped per tile on the device by the rule of p.  The sum is cleared first; the counts per tile are
 * mpt_read_tile_samples' on mpt_renderer_context.  out and nee_out may be NULL.                                                       */
int mpt_renderer_render_nee_adaptive(mpt_renderer* r, uint32_t max_samples, int32_t depth, int32_t walk, float clamp,
                                     const mpt_adaptive_params* p, mpt_adaptive_info* out, mpt_nee_info* nee_out);
mpt_ctx* mpt_renderer_context(mpt_renderer* r);
mpt_scene* mpt_renderer_scene(mpt_renderer* r);               /* borrowed                                */

/* Image output (the reference has none).  rgba: W*H*4 floats, top-left origin; value = rgba * scale. */
int mpt_write_pfm(const char* path, const float* rgba, uint32_t width, uint32_t height, float scale);
int mpt_write_ppm(const char* path, const float* rgba, uint32_t width, uint32_t height, float scale, float gamma);
/* The same file from finished bytes (mpt_read_display: W*H*4, r g b 255): writes r, g, b and does no arithmetic. */
int mpt_write_ppm8(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);

#ifdef __cplusplus
}
#endif
#endif /* MPT_HOST_H */
