// Renderer.h — host renderer over the HIP C ABI (include/mpt.h).
//
// Public method names and call order are the reference's class Renderer (R/Renderer/Renderer.h:16-29):
//   Renderer(device) -> updateVisibleScene, buildShaders, buildBuffers, buildTextures, recalculateViewport;
//   per frame draw(view) -> updateUniforms -> (swap targets, bind, launch).
// MTL::Device* becomes a HIP device ordinal; MTK::View* becomes an OffscreenView (the reference renders into
// an MTKView drawable and never reads back).  Everything device-side goes through libmpt_hip.so;
// this class contains no tracing code and there is no CPU fallback: construction throws if no GPU is found.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "Scene.h"
#include "mpt.h"

namespace MetalCppPathTracer {

struct OffscreenView {  // stands in for MTK::View: the size of the drawable + where a frame lands
    uint32_t width = 1280, height = 720;
    std::vector<float> rgba;  // filled by Renderer::readFrame (RGBA32F, top-left origin)
};
struct DrawableSize {
    double width, height;
};

class Renderer {
public:
    // tree builder used by updateVisibleScene: the reference's own (the drop-in default), or one of the product's
    enum { BUILD_REFERENCE = 0, BUILD_BINNED = 1, BUILD_GPU = 2, BUILD_AUTO = 3 };
    explicit Renderer(int deviceOrdinal = 0, const std::string& scenePath = std::string(),
                      const std::string& assetRoot = std::string(), int buildMode = BUILD_REFERENCE);
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void updateVisibleScene();   // load XML, build BVH, upload BVH + index buffers, then buildBuffers()
    void buildShaders();         // the kernels are precompiled in libmpt_hip.so: verifies the context only
    void buildBuffers();         // upload primitive + material buffers; uniforms start zero-filled
    void buildTextures();        // two RGBA32F accumulation targets at Camera::screenSize
    void recalculateViewport();  // R/Renderer/Renderer.cpp:153-182
    bool updateCamera();
    void updateUniforms();       // R/Renderer/Renderer.cpp:251-267 (frameCount / randomSeed protocol)
    void draw(OffscreenView* view);
    void drawableSizeWillChange(OffscreenView* view, DrawableSize size);

    // ---- extensions (not in the reference) ----
    void setScenePath(const std::string& xml, const std::string& assetRoot = std::string());
    void setRenderParams(const mpt_render_params& p) { params_ = p; }
    void setBuildMode(int mode) { buildMode_ = mode; }   // takes effect at the next updateVisibleScene()
    mpt_render_params& renderParams() { return params_; }
    Scene* scene() { return scene_; }
    mpt_ctx* context() { return ctx_; }
    const mpt_uniforms& uniforms() const { return uniforms_; }
    void readFrame(OffscreenView* view);                       // running-mean target of draw()
    int renderBatch(uint32_t sampleBegin, uint32_t sampleCount); // HDR sum accumulation (mpt_render)
    void readSum(std::vector<float>& rgba);
    void writeSum(const std::vector<float>& rgba);   // checkpoint / resume: the inverse of readSum (mpt_write_sum)
    void clearSum();
    mpt_stats stats();
    // mpt_denoise of what was rendered last: the draw() target after draw(), the sum after renderBatch() (samples = p.samples, or
    // when 0 the samples added since the sum was last cleared); rgba = the W*H*4 denoised floats
    void denoise(const mpt_denoise_params& p, std::vector<float>& rgba);
    // mpt_render_adaptive of [sampleBegin, sampleBegin + maxSamples) at most per tile; readAdaptiveMean = the sum / the tile's count
    mpt_adaptive_info renderAdaptive(uint32_t sampleBegin, uint32_t maxSamples, const mpt_adaptive_params& a);
    void readAdaptiveMean(std::vector<float>& rgba);
    // Temporal accumulation (mpt_temporal_accumulate, include/mpt.h): updateCamera(), then the sum is cleared, samplesPerFrame philox
    // samples starting at frame * samplesPerFrame are rendered — the frame counter is never reset by camera motion, so no two frames
    // share samples — and blended into the history reprojected from the previous frame's camera.  draw() is unchanged.
    mpt_temporal_info drawTemporal(OffscreenView* view, uint32_t samplesPerFrame);
    void setTemporalParams(const mpt_temporal_params& p) { temporal_ = p; }
    void readTemporal(std::vector<float>& rgba);                                        // the history: rgb, a = its length
    void denoiseTemporal(const mpt_denoise_params& p, std::vector<float>& rgba);        // mpt_denoise_temporal + mpt_read_denoised
    // SVGF (mpt_svgf_accumulate, include/mpt.h): drawTemporal's frame protocol and frame counter; the frame is readSvgf()'s.
    mpt_svgf_info drawSvgf(OffscreenView* view, uint32_t samplesPerFrame);
    void setSvgfParams(const mpt_svgf_params& p) { svgf_ = p; }
    void readSvgf(std::vector<float>& rgba);                                            // the filtered frame: rgb, a = the history length
    // mpt_display + mpt_read_display of p.source as given (MPT_DISPLAY_SUM with samples = 0: the samples added since the sum was last
    // cleared); rgba8 = the W*H*4 finished bytes
    mpt_display_info display(const mpt_display_params& p, std::vector<uint8_t>& rgba8);
    // mpt_ambient_occlusion over the first-hit guides of the current camera: `samples` shadow rays per surface pixel, numbered from 0,
    // keyed by the render parameters' seed, no farther than `radius` (<= 0: no limit), through MPT_WALK_AUTO; readAmbientOcclusion =
    // the W*H floats of ao (1 = open)
    mpt_ao_info renderAmbientOcclusion(uint32_t samples, float radius);
    void readAmbientOcclusion(std::vector<float>& ao);
    // mpt_direct_lighting over the same guides: `samples` light samples per surface pixel, numbered from 0, keyed by the render
    // parameters' seed, one shadow ray each through `walk` (MPT_WALK_*); readDirectLighting = the W*H*4 floats of the pass's rgba
    mpt_direct_info renderDirectLighting(uint32_t samples, int32_t walk = MPT_WALK_AUTO);
    void readDirectLighting(std::vector<float>& rgba);
    // mpt_direct_restir over the same guides: renderDirectLighting with spatial reservoir reuse — every round merges a pixel's
    // reservoir with `neighbours` from within `radius` pixels (0: the default), `mode` MPT_RESTIR_UNBIASED or MPT_RESTIR_BIASED, the
    // default thresholds; readDirectRestir = the W*H*4 floats of its rgba
    mpt_restir_info renderDirectRestir(uint32_t samples, uint32_t neighbours, uint32_t radius = 0, int32_t mode = MPT_RESTIR_UNBIASED,
                                       int32_t walk = MPT_WALK_AUTO);
    void readDirectRestir(std::vector<float>& rgba);
    // mpt_direct_restir_temporal: frame number `frame` of a camera path — the frame's inputs applied as drawTemporal applies them, then
    // one round of the direct pass whose reservoirs are merged with the previous frame's, which count for at most `maxHistory` frames'
    // candidates (0: the default); readDirectRestirTemporal = the W*H*4 floats of its rgba
    mpt_restir_temporal_info drawDirectRestirTemporal(OffscreenView* view, uint32_t frame, uint32_t maxHistory = 0, int32_t mode = MPT_RESTIR_UNBIASED,
                                                      int32_t walk = MPT_WALK_AUTO);
    void readDirectRestirTemporal(std::vector<float>& rgba);
    // mpt_render_nee: renderBatch's samples [sampleBegin, sampleBegin + spp) onto the HDR sum with a light sample and MIS at every Lambert
    // vertex, at max_depth `depth`, both kinds of ray through `walk` (MPT_WALK_*), per-sample clamp `clamp` (<= 0: none)
    mpt_nee_info renderNee(uint32_t spp, int32_t depth, int32_t walk = MPT_WALK_AUTO, float clamp = 0.0f, uint32_t sampleBegin = 0);
    // mpt_render_nee_adaptive: renderNee's estimator, [sampleBegin, sampleBegin + maxSamples) at most per tile, every tile stopped on the
    // device by renderAdaptive's rule (a); the sum is cleared first, readAdaptiveMean gives the image; neeInfo, if given, gets the NEE counts
    mpt_adaptive_info renderNeeAdaptive(uint32_t maxSamples, int32_t depth, const mpt_adaptive_params& a, int32_t walk = MPT_WALK_AUTO,
                                        float clamp = 0.0f, uint32_t sampleBegin = 0, mpt_nee_info* neeInfo = nullptr);
    // mpt_set_light_sampling: how renderDirectLighting and renderNee sample a sphere light (MPT_LIGHT_SAMPLING_AREA, the default, or
    // MPT_LIGHT_SAMPLING_CONE); a bad mode throws and changes nothing
    void setLightSampling(int mode);
    // mpt_set_light_candidates: from how many candidates (1, the default, to MPT_LIGHT_CANDIDATES_MAX) a light sample of the same two
    // calls is resampled; a bad count throws and changes nothing.  renderNeeAdaptive refuses more than 1.
    void setLightCandidates(uint32_t m);
    uint32_t lightCandidates();

private:
    void check(int status, const char* where);
    float hostRandomFloat();

    int device_ = 0;
    mpt_ctx* ctx_ = nullptr;
    Scene* scene_ = nullptr;
    std::string scenePath_, assetRoot_;
    mpt_uniforms uniforms_;
    mpt_render_params params_;
    uint32_t hostSeed_ = 92407235u;  // R/Renderer/Renderer.cpp:32
    bool sceneUploaded_ = false;
    int buildMode_ = BUILD_REFERENCE;
    bool deviceBuild_ = false, deviceDirty_ = false;
    mpt_temporal_params temporal_ = {};  // zeros: the defaults of include/mpt.h
    uint32_t temporalFrame_ = 0;         // frames drawTemporal() and drawSvgf() have drawn
    mpt_svgf_params svgf_ = {0, 0, 0, 0.0f, 0.0f, 0.0f, -1, 0.0f, 0.0f, 0.0f, -1};   // the defaults of include/mpt.h
    int lastSource_ = MPT_DENOISE_SUM;   // what denoise() filters: the source of the last draw() / renderBatch()
    uint32_t sumSamples_ = 0;            // samples renderBatch() added since the sum was cleared   // BUILD_GPU: mpt_build_and_upload, no tree on the host
};

}  // namespace MetalCppPathTracer
