// main.cpp — mpt_render: headless command-line front end of the host Renderer.
// (The reference's main.cpp starts an NSApplication + MTKView, R/main.cpp:15-28; that shell is out of scope.)
// What the command line says and refuses is cli_options.h, the checkpoint file is cli_checkpoint.h; here are the run modes, one function
// each, and main(), which picks one.
#include <cctype>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Camera.h"
#include "Renderer.h"
#include "cli_checkpoint.h"
#include "cli_options.h"
#include "mpt_host.h"

using namespace MetalCppPathTracer;

// what a checkpoint was accumulated FROM: FNV-1a over the packed primitive and material arrays (Scene::create*Buffer, spheres first)
static unsigned long long sceneFingerprint(const Scene& sc) {
    unsigned long long h = 0xcbf29ce484222325ull;
    auto eat = [&](const void* p, size_t bytes) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    };
    const size_t n = sc.getPrimitiveCount();
    mpt::float4* prims = sc.createTransformsBuffer();
    mpt::float4* mats = sc.createMaterialsBuffer();
    eat(&n, sizeof n);
    if (prims) eat(prims, n * 3 * sizeof(mpt::float4));
    if (mats) eat(mats, n * 2 * sizeof(mpt::float4));
    delete[] prims;
    delete[] mats;
    return h;
}
// the header of the checkpoint this run reads (--resume) or writes (--checkpoint): the estimator picks the kind
static CheckpointHeader checkpointHeader(const Options& o, unsigned long long sceneHash, uint32_t samples) {
    CheckpointHeader h;
    h.kind = o.neeRis() ? CheckpointHeader::NEE_RIS : o.neeCone() ? CheckpointHeader::NEE_CONE : o.nee ? CheckpointHeader::NEE : CheckpointHeader::PLAIN;
    h.width = o.width;
    h.height = o.height;
    h.samples = samples;
    h.seed = o.prm.seed_lo;
    h.rng = o.prm.rng_mode;
    h.depth = o.prm.max_depth;
    h.bsdf = o.prm.bsdf_mode;
    h.sceneHash = sceneHash;
    if (o.nee && o.neeClamp > 0.0f) std::memcpy(&h.clampBits, &o.neeClamp, sizeof h.clampBits);
    h.sampling = o.lightSampling;
    h.candidates = o.lightCandidates;
    return h;
}

// One frame of input in the reference's vocabulary (R/Window/ControllerView.mm:41-73): held keys set the movement
// vector to +-1 per axis (keyDown), `r` requests a reset, a mouse drag gives the rotation deltas, the scroll wheel the
// zoom (negated, :70-72).  Camera::transformWithInputs() consumes and clears them inside the next draw().
static bool applyInputLine(const std::string& line, int* repeat) {
    std::vector<std::string> tok;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && std::isspace((unsigned char)line[i])) ++i;
        size_t j = i;
        while (j < line.size() && !std::isspace((unsigned char)line[j])) ++j;
        if (j > i) tok.push_back(line.substr(i, j - i));
        i = j;
    }
    *repeat = 1;
    size_t k = 0;
    if (!tok.empty() && std::isdigit((unsigned char)tok[0][0]) && tok[0].find_first_not_of("0123456789") == std::string::npos) {
        *repeat = std::atoi(tok[0].c_str());
        k = 1;
    }
    InputSystem::clearInputs();
    for (; k < tok.size(); ++k) {
        const std::string& t = tok[k];
        if (t[0] == '#') break;
        if (t == "d") InputSystem::movementInput.x = 1.0f;        // keyCode 2
        else if (t == "a") InputSystem::movementInput.x = -1.0f;  // keyCode 0
        else if (t == "space") InputSystem::movementInput.y = 1.0f;   // keyCode 49
        else if (t == "c") InputSystem::movementInput.y = -1.0f;      // keyCode 8
        else if (t == "w") InputSystem::movementInput.z = 1.0f;   // keyCode 13
        else if (t == "s") InputSystem::movementInput.z = -1.0f;  // keyCode 1
        else if (t == "r") InputSystem::resetInput = true;        // keyCode 15
        else if (t == "mouse" && k + 2 < tok.size()) {
            InputSystem::rotationInput.x = (float)std::atof(tok[k + 1].c_str());
            InputSystem::rotationInput.y = (float)std::atof(tok[k + 2].c_str());
            k += 2;
        } else if (t == "scroll" && k + 1 < tok.size()) {
            InputSystem::zoomInput = -(float)std::atof(tok[k + 1].c_str());
            k += 1;
        } else {
            std::fprintf(stderr, "camera path: unknown token '%s'\n", t.c_str());
            return false;
        }
    }
    return true;
}

// The display flags (--tonemap ...): a .ppm is written from mpt_display's bytes instead of the float read-back.
struct DisplayOut {
    mpt_display_params params;      // tone, transfer, exposure ...: source and samples are set per call
    std::vector<uint8_t> rgba8;     // the last frame presented
    mpt_display_info info = {};
};
static void present(Renderer& r, DisplayOut& d, int source, uint32_t samples = 0) {
    mpt_display_params q = d.params;
    q.source = source;
    q.samples = samples;
    d.info = r.display(q, d.rgba8);
}
// mpt_denoise / mpt_denoise_temporal without the read-back: the result stays on the device for MPT_DISPLAY_DENOISED
static void denoiseOnDevice(Renderer& r, const mpt_denoise_params& dn, int source, uint32_t samples, bool temporal = false) {
    mpt_denoise_params q = dn;
    q.source = source;
    q.samples = samples;
    const int rc = temporal ? mpt_denoise_temporal(r.context(), &q) : mpt_denoise(r.context(), &q);
    if (rc) throw std::runtime_error(std::string("denoise: ") + mpt_status_string(rc) + ": " + mpt_last_error(r.context()));
}
static double msSince(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the reference hard-codes Camera::reset(); the flags overwrite the same globals before the viewport is built
static void applyCameraFlags(const Options& o) {
    if (o.havePos) Camera::position = mpt::float3(o.camPos[0], o.camPos[1], o.camPos[2]);
    if (o.haveDir) Camera::forward = mpt::normalize(mpt::float3(o.camDir[0], o.camDir[1], o.camDir[2]));
    if (o.haveUp) Camera::up = mpt::normalize(mpt::float3(o.camUp[0], o.camUp[1], o.camUp[2]));
    if (o.vfov > 0.0f) Camera::verticalFov = o.vfov;
}
// the float image to --out, by its suffix: .ppm (gamma 2.2) or .pfm; the writers' status
static int writeImage(const Options& o, const std::vector<float>& img, float scale) {
    return o.outPpm() ? mpt_write_ppm(o.out.c_str(), img.data(), o.width, o.height, scale, 2.2f)
                      : mpt_write_pfm(o.out.c_str(), img.data(), o.width, o.height, scale);
}

// ---- what a mode adds to the JSON line -------------------------------------------------------------------------------------------------

__attribute__((format(printf, 1, 2))) static std::string format(const char* fmt, ...) {
    char buf[1024];
    va_list args;
    va_start(args, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, args);
    va_end(args);
    return buf;
}
using ull = unsigned long long;
// the tail of a "direct" / "restir" / "nee" object: it names the sampling and the candidates only when their flag was given (without
// it the line is what it was), and closes the object
static std::string samplingJson(const Options& o) {
    return std::string(!o.haveLightSampling ? "" : o.lightSampling == MPT_LIGHT_SAMPLING_CONE ? ", \"light_sampling\": \"cone\"" : ", \"light_sampling\": \"area\"") +
           (o.haveLightCandidates ? ", \"light_candidates\": " + std::to_string(o.lightCandidates) : std::string()) + "}";
}
static std::string aoJson(const mpt_ao_info& info, const Options& o) {
    return format(", \"ao\": {\"samples\": %d, \"radius\": %.9g, \"pixels_surface\": %llu, \"rays\": %llu, \"rays_occluded\": %llu, \"device_ms\": %.3f}", o.ao,
                  static_cast<double>(o.aoRadius), (ull)info.pixels_surface, (ull)info.rays, (ull)info.rays_occluded, info.device_ms);
}
static std::string directJson(const mpt_direct_info& info, const Options& o) {
    return format(", \"direct\": {\"samples\": %d, \"pixels_surface\": %llu, \"rays\": %llu, \"rays_occluded\": %llu, \"lights\": %llu, \"device_ms\": %.3f", o.direct,
                  (ull)info.pixels_surface, (ull)info.rays, (ull)info.rays_occluded, (ull)info.lights, info.device_ms) +
           samplingJson(o);
}
static std::string restirJson(const mpt_restir_info& info, const Options& o) {
    return format(", \"restir\": {\"samples\": %d, \"neighbours\": %d, \"radius\": %d, \"mode\": \"%s\", \"pixels_surface\": %llu, \"rays_initial\": %llu, "
                  "\"rays_final\": %llu, \"rays_correction\": %llu, \"rays_occluded\": %llu, \"neighbours_accepted\": %llu, "
                  "\"samples_from_neighbours\": %llu, \"lights\": %llu, \"device_ms\": %.3f",
                  o.direct, o.restirK, o.restirRadius ? o.restirRadius : static_cast<int>(MPT_RESTIR_DEFAULT_RADIUS), o.restirBiased ? "biased" : "unbiased",
                  (ull)info.pixels_surface, (ull)info.rays_initial, (ull)info.rays_final, (ull)info.rays_correction, (ull)info.rays_occluded,
                  (ull)info.neighbours_accepted, (ull)info.samples_from_neighbours, (ull)info.lights, info.device_ms) +
           samplingJson(o);
}
static std::string neeJson(const mpt_nee_info& info, const Options& o) {
    return format(", \"nee\": {\"paths\": %llu, \"rays\": %llu, \"shadow_rays\": %llu, \"shadow_rays_occluded\": %llu, \"lights\": %llu, \"device_ms\": %.3f",
                  (ull)info.paths, (ull)info.rays, (ull)info.shadow_rays, (ull)info.shadow_rays_occluded, (ull)info.lights, info.device_ms) +
           samplingJson(o);
}
static std::string adaptiveJson(const mpt_adaptive_info& info, const Options& o) {
    const double pixels = static_cast<double>(o.width) * o.height;
    return format(", \"adaptive\": {\"passes\": %u, \"samples\": %llu, \"tiles_converged\": %u, \"tiles_at_max\": %u, \"mean_spp\": %.4f}", info.passes,
                  (ull)info.samples, info.tiles_converged, info.tiles_at_max, pixels > 0 ? static_cast<double>(info.samples) / pixels : 0.0);
}

// ---- the run modes of one GPU ------------------------------------------------------------------------------------------------------------
// Each renders what its flags ask for and returns what main()'s tail needs.  With the display flags the bytes for a .ppm are in `shown`
// instead of `img`.

struct Rendered {
    std::vector<float> img;   // the float image for --out ...
    float scale = 1.0f;       // ... which the writer multiplies by this
    std::string extraJson;    // the mode's objects of the JSON line
    int frames = 0;           // a camera path: the frames played; < 0: it could not be, and has said why
};

// --ao N: grey (ao, ao, ao, 1) through the writer the radiance goes through
static Rendered runAo(Renderer& r, OffscreenView&, const Options& o, DisplayOut&) {
    Rendered res;
    const mpt_ao_info info = r.renderAmbientOcclusion(static_cast<uint32_t>(o.ao), o.aoRadius);
    std::vector<float> a;
    r.readAmbientOcclusion(a);
    res.img.resize(a.size() * 4);
    for (size_t k = 0; k < a.size(); ++k) {
        res.img[4 * k] = res.img[4 * k + 1] = res.img[4 * k + 2] = a[k];
        res.img[4 * k + 3] = 1.0f;
    }
    res.extraJson = aoJson(info, o);
    return res;
}

// --direct N: the pass's rgba through the writer the radiance goes through; with --restir K, after spatial reservoir reuse
static Rendered runDirect(Renderer& r, OffscreenView&, const Options& o, DisplayOut&) {
    Rendered res;
    if (o.haveRestir) {
        const mpt_restir_info info = r.renderDirectRestir(static_cast<uint32_t>(o.direct), static_cast<uint32_t>(o.restirK), static_cast<uint32_t>(o.restirRadius),
                                                          o.restirMode(), o.directWalk);
        r.readDirectRestir(res.img);
        res.extraJson = restirJson(info, o);
    } else {
        const mpt_direct_info info = r.renderDirectLighting(static_cast<uint32_t>(o.direct), o.directWalk);
        r.readDirectLighting(res.img);
        res.extraJson = directJson(info, o);
    }
    return res;
}

// --adaptive T, --nee-adaptive T: the per-pixel mean
static Rendered runAdaptive(Renderer& r, OffscreenView&, const Options& o, DisplayOut& shown) {
    Rendered res;
    mpt_nee_info neeInfo = {};
    const mpt_adaptive_info info = o.neeAdaptive ? r.renderNeeAdaptive(static_cast<uint32_t>(o.spp), o.prm.max_depth, o.adp, o.neeWalk, o.neeClamp, 0, &neeInfo)
                                                 : r.renderAdaptive(0, static_cast<uint32_t>(o.spp), o.adp);
    if (!o.display || o.denoise) r.readAdaptiveMean(res.img);
    if (o.display && !o.denoise) present(r, shown, MPT_DISPLAY_ADAPTIVE);
    if (o.denoise) {   // the mean through the filter kernels, with the context's guides (mpt_read_aovs + mpt_denoise_image)
        std::vector<float> ad(res.img.size()), nc(res.img.size()), dn(res.img.size());
        mpt_ctx* ctx = r.context();
        int rc = mpt_read_aovs(ctx, ad.data(), nc.data(), nullptr);
        if (!rc) rc = mpt_denoise_image(ctx, o.width, o.height, res.img.data(), ad.data(), nc.data(), &o.dnp, dn.data());
        if (rc) throw std::runtime_error(std::string("adaptive denoise: ") + mpt_status_string(rc) + ": " + mpt_last_error(ctx));
        res.img.swap(dn);
        if (o.display) {   // (that mean is on the host: the display kernels take it from there)
            shown.rgba8.resize(static_cast<size_t>(o.width) * o.height * 4);
            rc = mpt_display_image(ctx, o.width, o.height, res.img.data(), &shown.params, nullptr, shown.rgba8.data(), nullptr, &shown.info);
            if (rc) throw std::runtime_error(std::string("adaptive display: ") + mpt_status_string(rc) + ": " + mpt_last_error(ctx));
        }
    }
    res.extraJson = adaptiveJson(info, o);
    if (o.neeAdaptive) res.extraJson += neeJson(neeInfo, o);
    return res;
}

// One frame of a camera path, the inputs applied: drawn by the protocol in effect, read back into view.rgba (or, with the display flags,
// presented into `shown`), written to --out-dir, and its JSON line printed (camera, frameCount) for checking against the reference's
// protocol (a camera change resets the accumulation and reseeds, R/Renderer/Renderer.cpp:255-257).
static void playPathFrame(Renderer& r, OffscreenView& view, const Options& o, DisplayOut& shown, int frame) {
    const mpt_denoise_params* dn = o.denoise ? &o.dnp : nullptr;
    const uint32_t temporalSpp = o.temporal || o.svgf ? o.temporalSpp : 0u;
    DisplayOut* dp = o.display ? &shown : nullptr;
    const std::string& outDir = o.outDir;
    const char* ft = std::getenv("MPT_FRAME_TIMES");   // 1: the JSON line gains the host's milliseconds around render / read-back / file write
    const bool frameTimes = ft && std::atoi(ft);
    mpt_temporal_info ti = {};
    mpt_restir_temporal_info ri = {};
    auto t0 = std::chrono::steady_clock::now();
    double renderMs = 0.0;
    if (o.restirTemporal) {   // --direct 1 --restir-temporal: the frame is the direct pass's, its reservoirs merged with the frame's before
        ri = r.drawDirectRestirTemporal(&view, static_cast<uint32_t>(frame), static_cast<uint32_t>(o.restirHistory), o.restirMode(), o.directWalk);
        renderMs = msSince(t0);
        r.readDirectRestirTemporal(view.rgba);
    } else if (temporalSpp && o.svgf) {   // --svgf: the frame is the variance-filtered history
        const mpt_svgf_info si = r.drawSvgf(&view, temporalSpp);
        ti.pixels_reprojected = si.pixels_reprojected;
        ti.pixels_reset = si.pixels_reset;
        renderMs = msSince(t0);
        if (dp) present(r, *dp, MPT_DISPLAY_SVGF);
        else r.readSvgf(view.rgba);
    } else if (temporalSpp) {   // --temporal: the frame is the history (or the filtered history)
        ti = r.drawTemporal(&view, temporalSpp);
        if (dn && dp) denoiseOnDevice(r, *dn, MPT_DENOISE_SUM, 0, true);
        renderMs = msSince(t0);
        if (dp) present(r, *dp, dn ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_TEMPORAL);
        else if (dn) r.denoiseTemporal(*dn, view.rgba);
        else r.readTemporal(view.rgba);
    } else {
        r.draw(&view);
        if (dn && dp) denoiseOnDevice(r, *dn, MPT_DENOISE_FRAME, 0);
        renderMs = msSince(t0);
        if (dp) {
            present(r, *dp, dn ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_FRAME);
        } else {
            r.readFrame(&view);
            if (dn) r.denoise(*dn, view.rgba);
        }
    }
    const double readMs = msSince(t0) - renderMs;   // the float read-back, or mpt_display + its W*H*4 bytes
    const mpt_uniforms& u = r.uniforms();
    char name[64];
    std::snprintf(name, sizeof name, "/frame_%04d.ppm", frame);
    if (dp ? mpt_write_ppm8((outDir + name).c_str(), dp->rgba8.data(), view.width, view.height)
           : mpt_write_ppm((outDir + name).c_str(), view.rgba.data(), (int)view.width, (int)view.height, 1.0f, 2.2f))
        std::fprintf(stderr, "cannot write %s%s\n", outDir.c_str(), name);
    const double writeMs = msSince(t0) - renderMs - readMs;   // without the display flags: the conversion and the file
    char temporalJson[320] = "";
    size_t tj = 0;
    if (temporalSpp)
        tj += std::snprintf(temporalJson + tj, sizeof temporalJson - tj, ", \"reprojected\": %llu, \"reset\": %llu",
                            (unsigned long long)ti.pixels_reprojected, (unsigned long long)ti.pixels_reset);
    if (o.restirTemporal)
        tj += std::snprintf(temporalJson + tj, sizeof temporalJson - tj, ", \"accepted\": %llu, \"from_history\": %llu, \"reset\": %llu",
                            (unsigned long long)ri.history_accepted, (unsigned long long)ri.samples_from_history, (unsigned long long)ri.pixels_reset);
    if (dp)
        tj += std::snprintf(temporalJson + tj, sizeof temporalJson - tj, ", \"scale\": %.9g, \"key_bin\": %lld, \"clipped\": %llu",
                            dp->info.scale, dp->info.key_bin == 0xFFFFFFFFu ? -1ll : (long long)dp->info.key_bin,
                            (unsigned long long)dp->info.pixels_clipped);
    if (frameTimes)
        tj += std::snprintf(temporalJson + tj, sizeof temporalJson - tj, ", \"ms\": {\"render\": %.3f, \"read\": %.3f, \"write\": %.3f}",
                            renderMs, readMs, writeMs);
    std::printf("{\"frame\": %d, \"frameCount\": %llu, \"camera\": [%.9g, %.9g, %.9g], \"forward\": [%.9g, %.9g, %.9g], \"vfov\": %.9g%s}\n",
                frame, (unsigned long long)u.frameCount, u.cameraPosition[0], u.cameraPosition[1], u.cameraPosition[2],
                Camera::forward.x, Camera::forward.y, Camera::forward.z, Camera::verticalFov, temporalJson);
}

// Replays a camera path: one draw() per frame with that frame's inputs, every frame written to --out-dir.  Returns the
// number of frames, -1 on error.
static int playCameraPath(Renderer& r, OffscreenView& view, const Options& o, DisplayOut& shown) {
    FILE* f = std::fopen(o.cameraPath.c_str(), "r");
    if (!f) {
        std::fprintf(stderr, "cannot open camera path %s\n", o.cameraPath.c_str());
        return -1;
    }
    std::error_code ec;
    std::filesystem::create_directories(o.outDir, ec);
    if (ec) std::fprintf(stderr, "cannot create %s: %s\n", o.outDir.c_str(), ec.message().c_str());
    char buf[512];
    int frame = 0;
    while (std::fgets(buf, sizeof buf, f)) {
        std::string line(buf);
        size_t h = line.find('#');
        if (h != std::string::npos) line.erase(h);
        if (line.find_first_not_of(" \t\r\n") == std::string::npos) continue;
        int repeat = 1;
        for (int k = 0, n = 1; k < n; ++k) {
            if (!applyInputLine(line, &repeat)) {
                std::fclose(f);
                return -1;
            }
            n = repeat;
            playPathFrame(r, view, o, shown, frame++);
        }
    }
    std::fclose(f);
    return frame;
}

// --camera-path F: the frames go to --out-dir, and --out gets what the last frame got
static Rendered runCameraPath(Renderer& r, OffscreenView& view, const Options& o, DisplayOut& shown) {
    Rendered res;
    if (o.temporal) r.setTemporalParams(o.tpp);
    if (o.svgf) {
        mpt_svgf_params sp = {0, 0, o.tpp.max_history, 0.0f, 0.0f, 0.0f, o.haveSvgfIterations ? o.svgfIterations : -1, 0.0f, 0.0f, 0.0f, -1};
        r.setSvgfParams(sp);
    }
    res.frames = playCameraPath(r, view, o, shown);
    if (res.frames < 0 || o.display) return res;   // (with the display flags: the last frame's bytes, which `shown` still holds)
    if (o.restirTemporal) r.readDirectRestirTemporal(view.rgba);
    else if (o.svgf) r.readSvgf(view.rgba);
    else if (o.temporal && o.denoise) r.denoiseTemporal(o.dnp, view.rgba);   // the filtered history
    else if (o.temporal) r.readTemporal(view.rgba);
    else r.readFrame(&view);
    res.img = view.rgba;
    if (o.denoise && !o.temporal) r.denoise(o.dnp, res.img);   // (--svgf takes no --denoise)
    return res;
}

// --frames N: the reference's frame protocol, N draw() calls into the running mean
static Rendered runFrames(Renderer& r, OffscreenView& view, const Options& o, DisplayOut& shown) {
    Rendered res;
    for (int f = 0; f < o.frames; ++f) r.draw(&view);
    if (o.display) {
        if (o.denoise) denoiseOnDevice(r, o.dnp, MPT_DENOISE_FRAME, 0);
        present(r, shown, o.denoise ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_FRAME);
    } else {
        r.readFrame(&view);
        res.img = view.rgba;
        if (o.denoise) r.denoise(o.dnp, res.img);
    }
    return res;
}

// The batch render: --spp samples of the plain or the --nee estimator added to the HDR sum, which --resume starts from a checkpoint
// (its samples numbered from where that one stopped) and --checkpoint writes out, raw, before --denoise or the display flags see it.
static Rendered runBatch(Renderer& r, OffscreenView&, const Options& o, DisplayOut& shown) {
    Rendered res;
    r.clearSum();
    const unsigned long long sceneHash = sceneFingerprint(*r.scene());
    uint32_t have = 0;
    if (!o.resume.empty()) {
        std::vector<float> sum;
        have = readCheckpoint(o.resume, checkpointHeader(o, sceneHash, 0), sum);
        r.writeSum(sum);
    }
    if (o.nee) res.extraJson = neeJson(r.renderNee(static_cast<uint32_t>(o.spp), o.prm.max_depth, o.neeWalk, o.neeClamp, have), o);
    else r.renderBatch(have, static_cast<uint32_t>(o.spp));
    const uint32_t samples = have + static_cast<uint32_t>(o.spp);
    if (!o.display || !o.checkpoint.empty()) r.readSum(res.img);
    if (!o.checkpoint.empty()) writeCheckpoint(o.checkpoint, checkpointHeader(o, sceneHash, samples), res.img);
    res.scale = 1.0f / static_cast<float>(samples);
    if (o.display) {
        if (o.denoise) denoiseOnDevice(r, o.dnp, MPT_DENOISE_SUM, samples);
        present(r, shown, o.denoise ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_SUM, samples);
    } else if (o.denoise) {   // the image is the denoised sum / samples
        mpt_denoise_params q = o.dnp;
        q.samples = samples;
        r.denoise(q, res.img);
        res.scale = 1.0f;
    }
    return res;
}

// --out of a render on several GPUs: from the sum reduced onto the root, where --denoise (the guide pass and the filter) and the display
// flags (exposure, tone curve and encoding) run too
static void writeReducedSum(Renderer& root, const Options& o) {
    const uint32_t spp = static_cast<uint32_t>(o.spp);
    int rc;
    if (o.display) {
        DisplayOut shown;
        shown.params = o.shown;
        if (o.denoise) denoiseOnDevice(root, o.dnp, MPT_DENOISE_SUM, spp);
        present(root, shown, o.denoise ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_SUM, spp);
        rc = mpt_write_ppm8(o.out.c_str(), shown.rgba8.data(), o.width, o.height);
    } else if (o.denoise) {
        std::vector<float> img;
        mpt_denoise_params q = o.dnp;
        q.samples = spp;
        root.denoise(q, img);
        rc = writeImage(o, img, 1.0f);
    } else {
        std::vector<float> img;
        root.readSum(img);
        rc = writeImage(o, img, 1.0f / (float)o.spp);
    }
    if (rc) throw std::runtime_error("cannot write " + o.out);
}

// Batch render on N GPUs driven by this one host thread (SURVEY.md 8e / include/mpt.h "multi-GPU"): every GPU gets the
// scene, renders its interleaved tile shard asynchronously, and ONE ncclReduce(sum) lands the HDR sum on the first GPU.
static int renderOnSeveralGpus(const Options& o) {
    std::vector<std::unique_ptr<Renderer>> rs;
    mpt_comm* comm = nullptr;
    const std::vector<int> devices = o.devices();
    const int gpus = o.gpus();
    const uint32_t spp = static_cast<uint32_t>(o.spp);
    try {
        for (int g = 0; g < gpus; ++g) rs.emplace_back(new Renderer(devices[g], o.scene, o.assetRoot, o.bvh()));
        applyCameraFlags(o);
        std::vector<mpt_ctx*> ctxs;
        OffscreenView view;
        for (int g = 0; g < gpus; ++g) {
            rs[g]->drawableSizeWillChange(&view, DrawableSize{(double)o.width, (double)o.height});
            rs[g]->clearSum();
            ctxs.push_back(rs[g]->context());
        }
        int rc = mpt_comm_create_all(ctxs.data(), gpus, &comm);
        if (rc) throw std::runtime_error(std::string("mpt_comm_create_all: ") + mpt_last_error(ctxs[0]));
        auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gpus; ++g) {  // enqueue everywhere first: mpt_render_async returns at once
            mpt_render_params p = o.prm;
            p.sample_begin = 0;
            p.sample_count = spp;
            p.shard_rank = g;
            p.shard_count = gpus;
            mpt_uniforms u = rs[g]->uniforms();
            u.primitiveCount = rs[g]->scene()->getPrimitiveCount();
            u.triangleCount = rs[g]->scene()->getTriangleCount();
            if ((rc = mpt_set_uniforms(ctxs[g], &u)) || (rc = mpt_render_async(ctxs[g], &p)))
                throw std::runtime_error(std::string("render on GPU ") + std::to_string(devices[g]) + ": " + mpt_last_error(ctxs[g]));
        }
        if ((rc = mpt_reduce_sum(comm, 0))) throw std::runtime_error(std::string("mpt_reduce_sum: ") + mpt_comm_last_error(comm));
        double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        unsigned long long rays = 0, paths = 0;
        for (int g = 0; g < gpus; ++g) {
            mpt_stats st = rs[g]->stats();
            rays += st.rays;
            paths += st.paths;
        }
        std::printf("{\"gpus\": %d, \"paths\": %llu, \"rays\": %llu, \"seconds\": %.6f, \"mrays_per_s\": %.1f}\n", gpus, paths, rays, sec,
                    sec > 0 ? rays / sec / 1e6 : 0.0);
        if (!o.out.empty()) writeReducedSum(*rs[0], o);
        mpt_comm_destroy(comm);
        return 0;
    } catch (const std::exception& e) {
        if (comm) mpt_comm_destroy(comm);
        std::fprintf(stderr, "mpt_render: %s\n", e.what());
        return 1;
    }
}

int main(int argc, char** argv) {
    Options o;
    if (const int status = parseOptions(argc, argv, o); status != kParsed) return status;   // (--help: 0)
    if (const int status = validate(o)) return status;
    if (o.gpus() > 1) return renderOnSeveralGpus(o);
    try {
        Renderer r(o.devices().front(), o.scene, o.assetRoot, o.bvh());
        r.setRenderParams(o.prm);
        if (o.haveLightSampling) r.setLightSampling(o.lightSampling);
        if (o.haveLightCandidates) r.setLightCandidates(static_cast<uint32_t>(o.lightCandidates));
        applyCameraFlags(o);
        OffscreenView view;
        r.drawableSizeWillChange(&view, DrawableSize{(double)o.width, (double)o.height});
        DisplayOut shown;
        shown.params = o.shown;
        auto t0 = std::chrono::steady_clock::now();
        const auto run = o.ao > 0                            ? runAo
                         : o.restirTemporal                  ? runCameraPath
                         : o.direct > 0                      ? runDirect
                         : o.adaptive || o.neeAdaptive       ? runAdaptive
                         : !o.cameraPath.empty()             ? runCameraPath
                         : o.frames > 0                      ? runFrames
                                                             : runBatch;
        const Rendered res = run(r, view, o, shown);
        if (res.frames < 0) return 1;
        double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        mpt_stats st = r.stats();
        std::printf("{\"paths\": %llu, \"rays\": %llu, \"seconds\": %.6f, \"device_ms\": %.3f, \"mrays_per_s\": %.1f%s}\n",
                    (unsigned long long)st.paths, (unsigned long long)st.rays, sec, st.total_ms,
                    st.total_ms > 0 ? st.rays / st.total_ms / 1e3 : 0.0, res.extraJson.c_str());
        if (!o.out.empty()) {
            const int rc = !o.display           ? writeImage(o, res.img, res.scale)
                           : shown.rgba8.empty() ? MPT_ERR_NOT_READY   // (a camera path without a frame)
                                                 : mpt_write_ppm8(o.out.c_str(), shown.rgba8.data(), o.width, o.height);
            if (rc) {
                std::fprintf(stderr, "cannot write %s\n", o.out.c_str());
                return 1;
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mpt_render: %s\n", e.what());
        return 1;
    }
    return 0;
}
