// Renderer.cpp — see Renderer.h.  Host-side frame protocol of the reference renderer
// (R/Renderer/Renderer.cpp) expressed over the C ABI.
#include "Renderer.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "Camera.h"
#include "SceneLoader.h"

namespace MetalCppPathTracer {

void Renderer::check(int status, const char* where) {
    if (status == MPT_OK) return;
    std::string msg = std::string(where) + ": " + mpt_status_string(status);
    if (ctx_) msg += std::string(" (") + mpt_last_error(ctx_) + ")";
    throw std::runtime_error(msg);
}

// host PCG stream of the reference (R/Renderer/Renderer.cpp:30-41)
float Renderer::hostRandomFloat() {
    const uint32_t state = hostSeed_ * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state);
    hostSeed_ = (word >> 22u) ^ word;
    return static_cast<float>(hostSeed_) / static_cast<float>(std::numeric_limits<uint32_t>::max());
}

Renderer::Renderer(int deviceOrdinal, const std::string& scenePath, const std::string& assetRoot, int buildMode)
    : device_(deviceOrdinal), scene_(new Scene()), scenePath_(scenePath), assetRoot_(assetRoot), buildMode_(buildMode) {
    std::memset(&uniforms_, 0, sizeof uniforms_);
    std::memset(&params_, 0, sizeof params_);
    params_.rng_mode = MPT_RNG_LITERAL;  // what the reference's shader does
    params_.bsdf_mode = MPT_BSDF_LAMBERT;
    params_.max_depth = 32;              // R/Renderer/Shaders/PathTracing.h:216
    params_.pipeline = MPT_PIPE_AUTO;
    params_.sample_count = 1;
    params_.seed_lo = 1;
    params_.shard_count = 1;
    int rc = mpt_create(deviceOrdinal, &ctx_);
    if (rc != MPT_OK) {
        delete scene_;
        scene_ = nullptr;
        throw std::runtime_error(std::string("mpt_create: ") + mpt_status_string(rc) +
                                 " — a MI355X GPU is required, there is no CPU fallback");
    }
    Camera::reset();
    Camera::screenSize = mpt::float2{1280.0f, 720.0f};  // R/Renderer/Renderer.cpp:48-49
    if (!scenePath_.empty()) {
        try {
            updateVisibleScene();
            buildShaders();
            buildBuffers();
            buildTextures();
            recalculateViewport();
        } catch (...) {  // the destructor does not run for a constructor that throws
            mpt_destroy(ctx_);
            ctx_ = nullptr;
            delete scene_;
            scene_ = nullptr;
            throw;
        }
    }
}

Renderer::~Renderer() {
    if (ctx_) mpt_destroy(ctx_);
    delete scene_;
}

void Renderer::setScenePath(const std::string& xml, const std::string& assetRoot) {
    scenePath_ = xml;
    assetRoot_ = assetRoot;
}

void Renderer::updateVisibleScene() {
    std::string log;
    SceneLoader::Load(scenePath_, scene_, assetRoot_, &log);
    std::fputs(log.c_str(), stdout);
    std::printf("Scene loaded: %zu total primitives (%zu spheres, %zu triangles)\n", scene_->getPrimitiveCount(),
                scene_->getPrimitiveCount() - scene_->getTriangleCount(), scene_->getTriangleCount());
    // The drop-in default is the reference's own sweep builder (R/Scene/Scene.h:195-317, the very same tree): with the
    // literal RNG and the frame protocol the reference's answer on ties and inconsistent hits depends on the visit order,
    // so the tree is part of the behaviour.  A caller that wants throughput asks for it (setBuildMode / MPT_BVH_MODE):
    // "auto" / "gpu" = mpt_build_and_upload, build -> render on the device with the host binned builder's algorithm: scene.xml
    // renders 10 % faster than on the reference's tree (leaves of <= 8 for the reference-order kernel), bunny x20 is ready in
    // 5 ms instead of 105 (host binned SAH + upload), 1 M primitives in 9 ms instead of 890, at 99-100 % of the host tree's
    // rays per second; "binned" = the host's 16-bin SAH builder.
    int want = buildMode_;
    if (const char* e = std::getenv("MPT_BVH_MODE")) {
        if (std::strcmp(e, "reference") == 0) want = BUILD_REFERENCE;
        else if (std::strcmp(e, "binned") == 0) want = BUILD_BINNED;
        else if (std::strcmp(e, "gpu") == 0) want = BUILD_GPU;
        else if (std::strcmp(e, "auto") == 0) want = BUILD_AUTO;
    }
    if (want == BUILD_AUTO) want = BUILD_GPU;
    const Scene::BuildMode mode = want == BUILD_BINNED ? Scene::BuildMode::BinnedCentroid
                                  : want == BUILD_GPU  ? Scene::BuildMode::GpuLbvh
                                                       : Scene::BuildMode::ReferenceSweep;
    std::printf("BVH builder: %s\n", want == BUILD_BINNED ? "binned SAH (host)" : want == BUILD_GPU ? "binned SAH on the device (build -> render without the host)" : "reference sweep SAH");
    deviceBuild_ = want == BUILD_GPU;
    if (deviceBuild_) {   // mpt_build_and_upload in buildBuffers(): the tree never exists on the host
        scene_->sortPrimitives();
        scene_->dropBVH();   // a tree left by an earlier host build (setBuildMode) is not what the device renders: getBVHNodeCount = 0
        deviceDirty_ = true;
        buildBuffers();
        return;
    }
    scene_->buildBVH(mode);
    std::printf("BVH node count: %zu\n", scene_->getBVHNodeCount());
    buildBuffers();
}

void Renderer::buildShaders() {
    if (!ctx_) throw std::runtime_error("buildShaders: no device context");
}

void Renderer::buildBuffers() {
    // The reference uploads BVH/index buffers in updateVisibleScene and primitive/material buffers here
    // (R/Renderer/Renderer.cpp:127-146,199-215); the device layout needs all four at once, so one upload.
    const size_t P = scene_->getPrimitiveCount();
    sceneUploaded_ = false;
    if (deviceBuild_) {
        if (!deviceDirty_) {   // (the constructor calls buildBuffers() once more after updateVisibleScene(), as the reference's does)
            sceneUploaded_ = P != 0;
            return;
        }
        deviceDirty_ = false;
        if (P == 0) return;
        mpt::float4* prims = scene_->createTransformsBuffer();
        mpt::float4* mats = scene_->createMaterialsBuffer();
        double ms = 0.0;
        int rc = mpt_build_and_upload(ctx_, reinterpret_cast<const float*>(prims), reinterpret_cast<const float*>(mats), P, &ms);
        delete[] prims;
        delete[] mats;
        check(rc, "mpt_build_and_upload");
        std::printf("BVH built on the device in %.2f ms\n", ms);
        sceneUploaded_ = true;
        std::memset(&uniforms_, 0, sizeof uniforms_);
        return;
    }
    if (P == 0 || scene_->getBVHNodeCount() == 0) return;
    mpt::float4* bvh = scene_->createBVHBuffer();
    mpt::float4* prims = scene_->createTransformsBuffer();
    mpt::float4* mats = scene_->createMaterialsBuffer();
    int* idx = scene_->createPrimitiveIndexBuffer();
    int rc = mpt_upload_scene(ctx_, reinterpret_cast<const float*>(bvh), scene_->getBVHNodeCount(),
                              reinterpret_cast<const float*>(prims), reinterpret_cast<const float*>(mats), idx, P);
    delete[] bvh;
    delete[] prims;
    delete[] mats;
    delete[] idx;
    check(rc, "mpt_upload_scene");
    sceneUploaded_ = true;
    // a fresh uniforms buffer is zero-filled (Metal zero-fills new buffers)
    std::memset(&uniforms_, 0, sizeof uniforms_);
}

void Renderer::buildTextures() {
    check(mpt_resize(ctx_, static_cast<uint32_t>(Camera::screenSize.x), static_cast<uint32_t>(Camera::screenSize.y)),
          "mpt_resize");
    sumSamples_ = 0;
}

void Renderer::recalculateViewport() {
    const float aspect = Camera::screenSize.x / Camera::screenSize.y;
    const float fovRad = Camera::verticalFov * (M_PI / 180.0f);
    const float halfH = tanf(fovRad * 0.5f);
    const float halfW = aspect * halfH;
    const mpt::float3 w = mpt::normalize(-Camera::forward);
    const mpt::float3 u = mpt::normalize(mpt::cross(Camera::up, w));
    const mpt::float3 v = mpt::cross(w, u);
    const mpt::float3 vu = u * (2.0f * halfW);
    const mpt::float3 vv = (-v) * (2.0f * halfH);
    const mpt::float3 first = Camera::position - w - (vu * 0.5f) - (vv * 0.5f);
    auto put = [](float* dst, const mpt::float3& s) {
        dst[0] = s.x;
        dst[1] = s.y;
        dst[2] = s.z;
        dst[3] = 0.0f;
    };
    put(uniforms_.cameraPosition, Camera::position);
    put(uniforms_.viewportU, vu);
    put(uniforms_.viewportV, vv);
    put(uniforms_.firstPixelPosition, first);
    uniforms_.screenSize[0] = Camera::screenSize.x;
    uniforms_.screenSize[1] = Camera::screenSize.y;
    std::printf("viewportU: (%f, %f, %f)\n", vu.x, vu.y, vu.z);
    std::printf("viewportV: (%f, %f, %f)\n", vv.x, vv.y, vv.z);
    std::printf("firstPixel: (%f, %f, %f)\n", first.x, first.y, first.z);
}

bool Renderer::updateCamera() {
    const bool changed = Camera::transformWithInputs();
    if (changed) recalculateViewport();
    return changed;
}

void Renderer::updateUniforms() {
    if (updateCamera()) {
        uniforms_.frameCount = 0;
        uniforms_.randomSeed[0] = hostRandomFloat();
        uniforms_.randomSeed[1] = hostRandomFloat();
        uniforms_.randomSeed[2] = hostRandomFloat();
    } else {
        uniforms_.frameCount++;
    }
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
}

void Renderer::draw(OffscreenView* /*view*/) {
    updateUniforms();
    mpt_render_params p = params_;
    p.sample_count = 1;
    if (p.rng_mode == MPT_RNG_PHILOX) p.sample_begin = static_cast<uint32_t>(uniforms_.frameCount);
    check(mpt_draw(ctx_, &p), "mpt_draw");  // swaps the accumulation targets, then launches
    lastSource_ = MPT_DENOISE_FRAME;
}

void Renderer::drawableSizeWillChange(OffscreenView* view, DrawableSize size) {
    Camera::screenSize = mpt::float2{static_cast<float>(size.width), static_cast<float>(size.height)};
    if (view) {
        view->width = static_cast<uint32_t>(size.width);
        view->height = static_cast<uint32_t>(size.height);
    }
    buildTextures();
    recalculateViewport();
}

void Renderer::readFrame(OffscreenView* view) {
    const uint32_t W = static_cast<uint32_t>(Camera::screenSize.x), H = static_cast<uint32_t>(Camera::screenSize.y);
    view->width = W;
    view->height = H;
    view->rgba.resize(static_cast<size_t>(W) * H * 4);
    check(mpt_read_frame(ctx_, view->rgba.data()), "mpt_read_frame");
}

int Renderer::renderBatch(uint32_t sampleBegin, uint32_t sampleCount) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    mpt_render_params p = params_;
    p.sample_begin = sampleBegin;
    p.sample_count = sampleCount;
    int rc = mpt_render(ctx_, &p);
    check(rc, "mpt_render");
    lastSource_ = MPT_DENOISE_SUM;
    sumSamples_ += sampleCount;
    return rc;
}

mpt_adaptive_info Renderer::renderAdaptive(uint32_t sampleBegin, uint32_t maxSamples, const mpt_adaptive_params& a) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    mpt_render_params p = params_;
    p.sample_begin = sampleBegin;
    p.sample_count = maxSamples;
    mpt_adaptive_info info;
    check(mpt_render_adaptive(ctx_, &p, &a, &info), "mpt_render_adaptive");
    lastSource_ = MPT_DENOISE_SUM;
    sumSamples_ = 0;   // (the tiles hold different counts: denoise() needs an explicit sample count)
    return info;
}

void Renderer::readAdaptiveMean(std::vector<float>& rgba) {
    const uint32_t W = static_cast<uint32_t>(Camera::screenSize.x), H = static_cast<uint32_t>(Camera::screenSize.y);
    const uint32_t tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    std::vector<uint32_t> counts(static_cast<size_t>(tilesX) * tilesY);
    readSum(rgba);
    check(mpt_read_tile_samples(ctx_, counts.data()), "mpt_read_tile_samples");
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const float n = static_cast<float>(counts[static_cast<size_t>(y / 8) * tilesX + x / 8]);
            float* v = &rgba[(static_cast<size_t>(y) * W + x) * 4];
            for (int c = 0; c < 4; ++c) v[c] = v[c] / n;
        }
}

mpt_temporal_info Renderer::drawTemporal(OffscreenView* /*view*/, uint32_t samplesPerFrame) {
    if (samplesPerFrame == 0) throw std::runtime_error("drawTemporal: samplesPerFrame = 0");
    if (params_.rng_mode != MPT_RNG_PHILOX) throw std::runtime_error("drawTemporal: needs MPT_RNG_PHILOX (the literal stream repeats per pixel)");
    updateCamera();
    clearSum();
    renderBatch(temporalFrame_ * samplesPerFrame, samplesPerFrame);
    ++temporalFrame_;
    mpt_temporal_params p = temporal_;
    p.source = MPT_DENOISE_SUM;
    p.samples = samplesPerFrame;
    mpt_temporal_info info;
    check(mpt_temporal_accumulate(ctx_, &p, &info), "mpt_temporal_accumulate");
    return info;
}

void Renderer::readTemporal(std::vector<float>& rgba) {
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_temporal(ctx_, rgba.data()), "mpt_read_temporal");
}

void Renderer::denoiseTemporal(const mpt_denoise_params& p, std::vector<float>& rgba) {
    check(mpt_denoise_temporal(ctx_, &p), "mpt_denoise_temporal");
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_denoised(ctx_, rgba.data()), "mpt_read_denoised");
}

mpt_svgf_info Renderer::drawSvgf(OffscreenView* /*view*/, uint32_t samplesPerFrame) {
    if (samplesPerFrame == 0) throw std::runtime_error("drawSvgf: samplesPerFrame = 0");
    if (params_.rng_mode != MPT_RNG_PHILOX) throw std::runtime_error("drawSvgf: needs MPT_RNG_PHILOX (the literal stream repeats per pixel)");
    updateCamera();
    clearSum();
    renderBatch(temporalFrame_ * samplesPerFrame, samplesPerFrame);
    ++temporalFrame_;
    mpt_svgf_params p = svgf_;
    p.source = MPT_DENOISE_SUM;
    p.samples = samplesPerFrame;
    mpt_svgf_info info;
    check(mpt_svgf_accumulate(ctx_, &p, &info), "mpt_svgf_accumulate");
    return info;
}

void Renderer::readSvgf(std::vector<float>& rgba) {
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_svgf(ctx_, rgba.data()), "mpt_read_svgf");
}

void Renderer::readSum(std::vector<float>& rgba) {
    const size_t n = static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4;
    rgba.resize(n);
    check(mpt_read_sum(ctx_, rgba.data()), "mpt_read_sum");
}

void Renderer::clearSum() {
    check(mpt_clear_sum(ctx_), "mpt_clear_sum");
    sumSamples_ = 0;
}

void Renderer::denoise(const mpt_denoise_params& p, std::vector<float>& rgba) {
    mpt_denoise_params q = p;
    q.source = lastSource_;
    if (q.source == MPT_DENOISE_SUM && q.samples == 0) q.samples = sumSamples_;
    check(mpt_denoise(ctx_, &q), "mpt_denoise");
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_denoised(ctx_, rgba.data()), "mpt_read_denoised");
}
mpt_display_info Renderer::display(const mpt_display_params& p, std::vector<uint8_t>& rgba8) {
    mpt_display_params q = p;
    if (q.source == MPT_DISPLAY_SUM && q.samples == 0) q.samples = sumSamples_;
    mpt_display_info info;
    check(mpt_display(ctx_, &q, &info), "mpt_display");
    rgba8.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_display(ctx_, rgba8.data()), "mpt_read_display");
    return info;
}
mpt_ao_info Renderer::renderAmbientOcclusion(uint32_t samples, float radius) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    const mpt_ao_params p = {0u, samples, radius, params_.seed_lo, params_.seed_hi, MPT_WALK_AUTO};
    mpt_ao_info info;
    check(mpt_ambient_occlusion(ctx_, &p, &info), "mpt_ambient_occlusion");
    return info;
}
void Renderer::readAmbientOcclusion(std::vector<float>& ao) {
    ao.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y));
    check(mpt_read_ao(ctx_, ao.data(), nullptr), "mpt_read_ao");
}
mpt_direct_info Renderer::renderDirectLighting(uint32_t samples, int32_t walk) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    const mpt_direct_params p = {0u, samples, params_.seed_lo, params_.seed_hi, walk};
    mpt_direct_info info;
    check(mpt_direct_lighting(ctx_, &p, &info), "mpt_direct_lighting");
    return info;
}
void Renderer::readDirectLighting(std::vector<float>& rgba) {
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_direct(ctx_, rgba.data(), nullptr, nullptr), "mpt_read_direct");
}
mpt_restir_info Renderer::renderDirectRestir(uint32_t samples, uint32_t neighbours, uint32_t radius, int32_t mode, int32_t walk) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    const mpt_restir_params p = {0u, samples, params_.seed_lo, params_.seed_hi, walk, neighbours, radius, mode, 0.0f, 0.0f};
    mpt_restir_info info;
    check(mpt_direct_restir(ctx_, &p, &info), "mpt_direct_restir");
    return info;
}
void Renderer::readDirectRestir(std::vector<float>& rgba) {
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_restir(ctx_, rgba.data(), nullptr, nullptr), "mpt_read_restir");
}
mpt_restir_temporal_info Renderer::drawDirectRestirTemporal(OffscreenView* /*view*/, uint32_t frame, uint32_t maxHistory, int32_t mode, int32_t walk) {
    updateCamera();   // (the frame's inputs; the frame counter and the seed protocol of draw() are not this pass's)
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    const mpt_restir_temporal_params p = {frame, params_.seed_lo, params_.seed_hi, walk, mode, maxHistory, 0.0f, 0.0f};
    mpt_restir_temporal_info info;
    check(mpt_direct_restir_temporal(ctx_, &p, &info), "mpt_direct_restir_temporal");
    return info;
}
void Renderer::readDirectRestirTemporal(std::vector<float>& rgba) {
    rgba.resize(static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4);
    check(mpt_read_restir_temporal(ctx_, rgba.data(), nullptr, nullptr), "mpt_read_restir_temporal");
}
mpt_nee_info Renderer::renderNee(uint32_t spp, int32_t depth, int32_t walk, float clamp, uint32_t sampleBegin) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    mpt_render_params p = params_;
    p.max_depth = depth;
    p.sample_begin = sampleBegin;
    p.sample_count = spp;
    const mpt_nee_params n = {walk, clamp};
    mpt_nee_info info;
    check(mpt_render_nee(ctx_, &p, &n, &info), "mpt_render_nee");
    lastSource_ = MPT_DENOISE_SUM;
    sumSamples_ += spp;
    return info;
}
mpt_adaptive_info Renderer::renderNeeAdaptive(uint32_t maxSamples, int32_t depth, const mpt_adaptive_params& a, int32_t walk, float clamp,
                                              uint32_t sampleBegin, mpt_nee_info* neeInfo) {
    uniforms_.primitiveCount = scene_->getPrimitiveCount();
    uniforms_.triangleCount = scene_->getTriangleCount();
    check(mpt_set_uniforms(ctx_, &uniforms_), "mpt_set_uniforms");
    mpt_render_params p = params_;
    p.max_depth = depth;
    p.sample_begin = sampleBegin;
    p.sample_count = maxSamples;
    const mpt_nee_params n = {walk, clamp};
    mpt_adaptive_info info;
    check(mpt_render_nee_adaptive(ctx_, &p, &n, &a, &info, neeInfo), "mpt_render_nee_adaptive");
    lastSource_ = MPT_DENOISE_SUM;
    sumSamples_ = 0;   // (the tiles hold different counts, as after renderAdaptive)
    return info;
}
void Renderer::setLightSampling(int mode) { check(mpt_set_light_sampling(ctx_, static_cast<int32_t>(mode)), "mpt_set_light_sampling"); }
void Renderer::setLightCandidates(uint32_t m) { check(mpt_set_light_candidates(ctx_, m), "mpt_set_light_candidates"); }
uint32_t Renderer::lightCandidates() {
    uint32_t m = 0;
    check(mpt_get_light_candidates(ctx_, &m), "mpt_get_light_candidates");
    return m;
}
void Renderer::writeSum(const std::vector<float>& rgba) {
    const size_t n = static_cast<size_t>(Camera::screenSize.x) * static_cast<size_t>(Camera::screenSize.y) * 4;
    if (rgba.size() != n) throw std::runtime_error("writeSum: the array does not have the size of the frame");
    check(mpt_write_sum(ctx_, rgba.data()), "mpt_write_sum");
}

mpt_stats Renderer::stats() {
    mpt_stats s;
    check(mpt_get_stats(ctx_, &s), "mpt_get_stats");
    return s;
}

}  // namespace MetalCppPathTracer
