// main.cpp — mpt_render: headless command-line front end of the host Renderer.
// (The reference's main.cpp starts an NSApplication + MTKView, R/main.cpp:15-28; that shell is out of scope.)
#include <cctype>
#include <cmath>
#include <chrono>
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
static void usage() {
    std::puts(
        "mpt_render --scene scene.xml [--asset-root DIR] [--width 1280] [--height 720]\n"
        "           [--spp 64] [--depth 32] [--seed 1] [--rng philox|literal] [--bsdf lambert|scatter|scatter-all]\n"
        "           [--pipeline auto|ordered|wavelocal|wavefront|megakernel] [--frames N] [--device 0] [--out image.pfm|image.ppm]\n"
        "           [--camera-pos x,y,z] [--camera-dir x,y,z] [--camera-up x,y,z] [--vfov degrees]\n"
        "           [--gpus N | --devices a,b,...] [--camera-path FILE [--out-dir runs]] [--bvh reference|binned|gpu|auto]\n"
        "           [--checkpoint FILE] [--resume FILE] [--denoise [--denoise-iterations N]] [--ao N [--ao-radius R]]\n"
        "           [--direct N [--direct-walk reference|own|auto] [--restir K [--restir-radius R] [--restir-biased]]]\n"
        "           [--nee [--nee-walk reference|own|auto] [--nee-clamp C]]\n"
        "           [--nee-adaptive THRESHOLD [--nee-walk ...] [--nee-clamp C] [--adaptive-min N] [--adaptive-batch N] [--adaptive-floor F]]\n"
        "           [--light-sampling area|cone]\n"
        "           [--adaptive THRESHOLD [--adaptive-min N] [--adaptive-batch N] [--adaptive-floor F]]\n"
        "           [--temporal [--temporal-history N] [--temporal-spp K]]\n"
        "           [--svgf [--svgf-iterations N] [--temporal-history N] [--temporal-spp K]]\n"
        "           [--tonemap clamp|reinhard|aces] [--transfer srgb|gamma22|linear] [--exposure EV] [--white W]\n"
        "           [--auto-exposure [--key K] [--percentile P] [--adaptation A]]\n"
        "  --tonemap, --transfer, --exposure, --white, --auto-exposure\n"
        "                    any of them: every .ppm written (--out and the frames of --camera-path) is made on the device by\n"
        "                    mpt_display (include/mpt.h) — exposure 2^EV (times the histogram's scale with --auto-exposure: the\n"
        "                    --percentile P luminance, default 50, goes to --key K, default 0.18, smoothed over the frames of a\n"
        "                    camera path by --adaptation A in (0, 1)), the tone curve (default clamp; reinhard with white point\n"
        "                    --white W, default 4; aces) and the transfer function (default srgb) — from what the mode in effect\n"
        "                    produces: the sum, the denoised, adaptive, temporal or SVGF result, the frame protocol's target, with\n"
        "                    --gpus N the root's reduced sum; only W*H*4 bytes come back.  The JSON line of a camera-path frame gains\n"
        "                    \"scale\", \"key_bin\" and \"clipped\".  Not with a .pfm --out.  Without them nothing changes\n"
        "  --svgf            with --camera-path: as --temporal, but what is accumulated is the illumination (the colour divided by the\n"
        "                    first hit's albedo) with the moments of its luminance, and every frame written is that history through\n"
        "                    --svgf-iterations a-trous levels (default 2) whose luminance stop is each pixel's own variance\n"
        "                    (mpt_svgf_accumulate, include/mpt.h): converged pixels keep their detail, disoccluded ones are filtered\n"
        "                    wide; the per-frame JSON line gains \"reprojected\" and \"reset\".  Not with --temporal, --denoise,\n"
        "                    --rng literal, --gpus > 1, --adaptive, --checkpoint or --resume\n"
        "  --temporal        with --camera-path: every frame renders --temporal-spp fresh philox samples (default 1) and blends them\n"
        "                    into the image accumulated so far, reprojected from the previous camera (mpt_temporal_accumulate,\n"
        "                    include/mpt.h; the history is at most --temporal-history frames long, default 32); the frame written is\n"
        "                    the history (with --denoise: mpt_denoise_temporal's); the per-frame JSON line gains \"reprojected\" and\n"
        "                    \"reset\".  Not with --rng literal, --gpus > 1, --adaptive, --checkpoint or --resume\n"
        "  --adaptive T      batch mode, adaptive sampling (mpt_render_adaptive, include/mpt.h): every 8x8 tile gets --adaptive-min\n"
        "                    samples (default 16), then --adaptive-batch more per pass (default 16) until the relative standard error\n"
        "                    of each of its pixels' mean luminance is <= T (luminance below --adaptive-floor, default 0.05, counts as\n"
        "                    the floor) or it holds --spp samples.  --out gets the per-pixel mean (the sum / its tile's count; with\n"
        "                    --denoise the denoised mean); the JSON line gains an \"adaptive\" object.  Not with --frames,\n"
        "                    --camera-path, --gpus > 1, --rng literal, --checkpoint or --resume\n"
        "  --ao N            write ambient occlusion instead of the radiance to --out (a .ppm): N shadow rays per surface pixel of the\n"
        "                    first hits (mpt_ambient_occlusion, include/mpt.h), no farther than --ao-radius R (default: no limit); grey,\n"
        "                    1 = open, through the same .ppm writer; the JSON line gains an \"ao\" object.  Nothing is path traced.\n"
        "                    Only with a plain run: not with --frames, --camera-path, --gpus > 1, --adaptive, --denoise, the display\n"
        "                    flags, --checkpoint or --resume\n"
        "  --direct N        write direct lighting instead of the radiance to --out (a .ppm): N points on the scene's lights per surface\n"
        "                    pixel of the first hits, drawn by power, one shadow ray each (mpt_direct_lighting, include/mpt.h) through\n"
        "                    the --direct-walk tree (default auto); every surface shaded as Lambert, emitters black, through the same\n"
        "                    .ppm writer; the JSON line gains a \"direct\" object.  Nothing is path traced.  Only with a plain run: not\n"
        "                    with --ao, --frames, --camera-path, --gpus > 1, --adaptive, --denoise, --temporal, --svgf, the display\n"
        "                    flags, --checkpoint or --resume\n"
        "  --nee             render the still image (--out, --spp, --depth) with next-event estimation (mpt_render_nee, include/mpt.h): a\n"
        "                    point on the scene's lights and a shadow ray at every diffuse vertex, weighted against the light the bounce\n"
        "                    finds; both kinds of ray through the --nee-walk tree (default auto); --nee-clamp C clamps every sample's\n"
        "                    channels at C (default: no clamp; 1 is the plain render's).  The JSON line gains a \"nee\" object.  --denoise,\n"
        "                    --checkpoint / --resume and the display flags work on the sum; a checkpoint of an --nee render records the\n"
        "                    estimator and its clamp (header MPTNEE1) and is resumed only by an --nee run with the same clamp, a plain one\n"
        "                    only by a plain run.  Not with --adaptive, --gpus > 1, --camera-path (hence --temporal, --svgf), --frames,\n"
        "                    --ao, --direct, --rng literal or --bsdf scatter-all\n"
        "  --nee-adaptive T  render the still image with the estimator of --nee and the allocation of --adaptive in ONE kernel launch\n"
        "                    (mpt_render_nee_adaptive, include/mpt.h): the wave that renders an 8x8 tile keeps its pixels' sums and second\n"
        "                    moments in registers and applies the stopping rule of --adaptive itself, after --adaptive-min samples and then\n"
        "                    every --adaptive-batch, up to --spp.  Takes --nee-walk, --nee-clamp and --light-sampling as --nee does,\n"
        "                    --adaptive-min, --adaptive-batch and --adaptive-floor as --adaptive does, --denoise and the display flags over\n"
        "                    the per-pixel mean, which --out gets; the JSON line gains the \"adaptive\" and the \"nee\" object.  A flag of\n"
        "                    its own because --nee --adaptive stays refused: those two calls keep their contracts (mpt_render_nee adds to\n"
        "                    the sum and writes no moments, mpt_render_adaptive drives the plain path loop in host passes).  Not with --nee,\n"
        "                    --adaptive, --gpus > 1, --camera-path, --frames, --checkpoint, --resume, --ao, --direct, --rng literal or\n"
        "                    --bsdf scatter-all\n"
        "  --light-sampling  with --direct, --nee or --nee-adaptive: how a sphere light is sampled (mpt_set_light_sampling, include/mpt.h) — area: uniformly\n"
        "                    over its whole surface (the default); cone: uniformly in the cone of directions it subtends from the\n"
        "                    shading point, so that every sample meets the light.  Triangle lights are sampled the same either way.  The\n"
        "                    \"direct\" / \"nee\" JSON object gains \"light_sampling\"; a checkpoint of an --nee render with cone sampling\n"
        "                    has the header MPTNEE2 and is resumed only by such a run, one with area sampling (MPTNEE1) only by such a run\n"
        "  --light-candidates M  with --direct or --nee: resample every light sample from M candidates, 1..32 (mpt_set_light_candidates,\n"
        "                    include/mpt.h) — M lights and points are drawn as the one sample is, each weighted by the light it would deliver\n"
        "                    unshadowed, one kept in proportion to that weight, and one shadow ray traced for it.  1 (the default) is no\n"
        "                    resampling: every file and every line is what it is without the flag.  The \"direct\" / \"nee\" JSON object gains\n"
        "                    \"light_candidates\"; a checkpoint of an --nee render with M > 1 has the header MPTNEE3 (its last fields the\n"
        "                    sampling and M) and is resumed only by a run with the same M and sampling.  With --nee-adaptive only M = 1\n"
        "  --restir K        with --direct: spatial reservoir reuse (mpt_direct_restir, include/mpt.h) — in every one of the N rounds a pixel\n"
        "                    keeps the sample its --light-candidates pick only if its shadow ray arrives, then merges that one-sample\n"
        "                    reservoir with those of K pixels (0..16; 4 is a fair start) drawn within --restir-radius R pixels (1..64, default 4) that\n"
        "                    see the same surface.  Unbiased by default: one more shadow ray per accepted neighbour; --restir-biased omits\n"
        "                    those rays and darkens the image at visibility edges.  The JSON line gains a \"restir\" object.  Lights are\n"
        "                    sampled by area: not with --light-sampling cone.  Without --restir every file and line is what it was\n"
        "  --denoise         write the denoised image (mpt_denoise: first-hit guides + a-trous filter, include/mpt.h) to --out\n"
        "                    and to every --camera-path frame; with --gpus N the root's reduced sum; N levels (default 3, 0..8)\n"
        "  --bvh             tree builder: the reference's sweep SAH (default with --rng literal, --frames and --camera-path:\n"
        "                    the drop-in behaviour) or auto (default for batch renders: the tree of every scene is built on the\n"
        "                    device, mpt_build_and_upload, with leaves of <= 6 primitives below 8192 primitives and <= 2 from there\n"
        "                    on; gpu = the same); binned = the host's 16-bin SAH builder\n"
        "  --checkpoint F    batch mode: after the render, write the HDR sum and the number of samples it holds to F\n"
        "  --resume F        batch mode: start from the checkpoint F (same scene, size, seed and RNG) and add --spp MORE samples, numbered\n"
        "                    from where it stopped: the result is bit-identical to one uninterrupted render of all the samples\n"
        "  --frames N        run the reference's frame protocol (N draw() calls, running mean) instead of batch spp\n"
        "  --gpus N          batch mode on GPUs device .. device+N-1: 8x8 pixel tiles interleaved over the GPUs, one RCCL\n"
        "                    reduce(sum) of the HDR framebuffer onto the first (mpt_comm_create_all / mpt_reduce_sum)\n"
        "  --devices a,b,..  the same on the listed device ordinals, one rank each (RCCL itself refuses an ordinal listed twice)\n"
        "  --camera-path F   headless replay of the reference's input handling (R/Window/ControllerView.mm:41-73): one\n"
        "                    line of F per frame, optionally prefixed by a repeat count, holding the keys\n"
        "                    w a s d space c (move), r (reset), `mouse dx dy`, `scroll dy`; every frame is one draw()\n"
        "                    and is written to <out-dir>/frame_NNNN.ppm (default out-dir: runs, as R/runs/)");
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

// Replays a camera path: one draw() per frame with that frame's inputs, every frame written to outDir.  Returns the
// number of frames, -1 on error.  Prints one JSON line per frame (camera, frameCount) for checking against the reference's
// protocol (a camera change resets the accumulation and reseeds, R/Renderer/Renderer.cpp:255-257).
static int playCameraPath(Renderer& r, OffscreenView& view, const std::string& path, const std::string& outDir,
                          const mpt_denoise_params* dn, uint32_t temporalSpp = 0, bool svgf = false, DisplayOut* dp = nullptr) {
    const char* ft = std::getenv("MPT_FRAME_TIMES");   // 1: the JSON line gains the host's milliseconds around render / read-back / file write
    const bool frameTimes = ft && std::atoi(ft);
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) {
        std::fprintf(stderr, "cannot open camera path %s\n", path.c_str());
        return -1;
    }
    std::error_code ec;
    std::filesystem::create_directories(outDir, ec);
    if (ec) std::fprintf(stderr, "cannot create %s: %s\n", outDir.c_str(), ec.message().c_str());
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
            mpt_temporal_info ti = {};
            auto t0 = std::chrono::steady_clock::now();
            double renderMs = 0.0;
            if (temporalSpp && svgf) {   // --svgf: the frame is the variance-filtered history
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
            ++frame;
        }
    }
    std::fclose(f);
    return frame;
}

// Batch render on N GPUs driven by this one host thread (SURVEY.md 8e / include/mpt.h "multi-GPU"): every GPU gets the
// scene, renders its interleaved tile shard asynchronously, and ONE ncclReduce(sum) lands the HDR sum on the first GPU.
static int renderOnSeveralGpus(const std::string& scene, const std::string& assetRoot, const std::string& out, int width, int height,
                               int spp, const std::vector<int>& devices, int bvh, mpt_render_params prm, const float* camPos, const float* camDir,
                               const float* camUp, float vfov, const mpt_denoise_params* dn, DisplayOut* dp) {
    std::vector<std::unique_ptr<Renderer>> rs;
    mpt_comm* comm = nullptr;
    const int gpus = static_cast<int>(devices.size());
    try {
        for (int g = 0; g < gpus; ++g) rs.emplace_back(new Renderer(devices[g], scene, assetRoot, bvh));
        if (camPos) Camera::position = mpt::float3(camPos[0], camPos[1], camPos[2]);
        if (camDir) Camera::forward = mpt::normalize(mpt::float3(camDir[0], camDir[1], camDir[2]));
        if (camUp) Camera::up = mpt::normalize(mpt::float3(camUp[0], camUp[1], camUp[2]));
        if (vfov > 0.0f) Camera::verticalFov = vfov;
        std::vector<mpt_ctx*> ctxs;
        OffscreenView view;
        for (int g = 0; g < gpus; ++g) {
            rs[g]->drawableSizeWillChange(&view, DrawableSize{(double)width, (double)height});
            rs[g]->clearSum();
            ctxs.push_back(rs[g]->context());
        }
        int rc = mpt_comm_create_all(ctxs.data(), gpus, &comm);
        if (rc) throw std::runtime_error(std::string("mpt_comm_create_all: ") + mpt_last_error(ctxs[0]));
        auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gpus; ++g) {  // enqueue everywhere first: mpt_render_async returns at once
            mpt_render_params p = prm;
            p.sample_begin = 0;
            p.sample_count = (uint32_t)spp;
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
        if (!out.empty() && dp) {   // exposure, tone curve and encoding on the root too, over the reduced sum (or its denoised mean)
            if (dn) denoiseOnDevice(*rs[0], *dn, MPT_DENOISE_SUM, (uint32_t)spp);
            present(*rs[0], *dp, dn ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_SUM, (uint32_t)spp);
            if (mpt_write_ppm8(out.c_str(), dp->rgba8.data(), width, height)) throw std::runtime_error("cannot write " + out);
        } else if (!out.empty()) {
            std::vector<float> img;
            float scale = 1.0f / (float)spp;
            if (dn) {   // the guide pass and the filter run on the root, over the reduced sum
                mpt_denoise_params q = *dn;
                q.samples = (uint32_t)spp;
                rs[0]->denoise(q, img);
                scale = 1.0f;
            } else {
                rs[0]->readSum(img);
            }
            bool ppm = out.size() > 4 && out.substr(out.size() - 4) == ".ppm";
            if (ppm ? mpt_write_ppm(out.c_str(), img.data(), width, height, scale, 2.2f) : mpt_write_pfm(out.c_str(), img.data(), width, height, scale))
                throw std::runtime_error("cannot write " + out);
        }
        mpt_comm_destroy(comm);
        return 0;
    } catch (const std::exception& e) {
        if (comm) mpt_comm_destroy(comm);
        std::fprintf(stderr, "mpt_render: %s\n", e.what());
        return 1;
    }
}

int main(int argc, char** argv) {
    std::string scene, assetRoot, out, cameraPath, outDir = "runs", checkpoint, resume;
    int width = 1280, height = 720, spp = 64, depth = 32, device = 0, frames = 0, gpus = 1;
    int bvh = -1;   // -1 = by mode: the reference's builder for the frame protocol / the literal RNG, auto for batch renders
    unsigned seed = 1;
    float camPos[3], camDir[3], camUp[3], vfov = 0.0f;
    bool havePos = false, haveDir = false, haveUp = false;
    std::vector<int> deviceList;   // --devices a,b,...: the ordinals of a multi-GPU render, one rank each (default: --device .. --device + gpus - 1)
    mpt_render_params prm;
    std::memset(&prm, 0, sizeof prm);
    prm.rng_mode = MPT_RNG_PHILOX;
    prm.shard_count = 1;
    prm.pipeline = MPT_PIPE_AUTO;
    bool denoise = false;
    mpt_denoise_params dnp;
    std::memset(&dnp, 0, sizeof dnp);
    dnp.iterations = -1;   // (defaults of include/mpt.h)
    bool temporal = false;
    mpt_temporal_params tpp = {};
    uint32_t temporalSpp = 1;
    bool svgf = false;
    int svgfIterations = -1;   // (the default of include/mpt.h)
    bool haveSvgfIterations = false;
    bool adaptive = false;
    mpt_adaptive_params adp;
    std::memset(&adp, 0, sizeof adp);   // (0 = the defaults of include/mpt.h)
    int ao = 0;             // --ao N: shadow rays per surface pixel (0 = none)
    bool haveAo = false;    // --ao was given (with whatever count: 0 is refused, not ignored)
    float aoRadius = 0.0f;
    bool haveAoRadius = false;
    int direct = 0;         // --direct N: light samples per surface pixel (0 = none)
    bool haveDirect = false, haveDirectWalk = false;
    int32_t directWalk = MPT_WALK_AUTO;
    bool nee = false, haveNeeOpt = false;   // --nee; --nee-walk / --nee-clamp were given
    int32_t neeWalk = MPT_WALK_AUTO;
    float neeClamp = 0.0f;
    bool neeAdaptive = false;   // --nee-adaptive T (the threshold goes into adp, as --adaptive's)
    bool haveLightSampling = false;   // --light-sampling was given
    int lightSampling = MPT_LIGHT_SAMPLING_AREA;
    bool haveLightCandidates = false;   // --light-candidates was given
    bool haveRestir = false, haveRestirRadius = false, haveRestirOpt = false;   // --restir K; --restir-radius; it or --restir-biased were given
    int restirK = 0, restirRadius = 0;
    int32_t restirMode = MPT_RESTIR_UNBIASED;
    int lightCandidates = 1;
    bool display = false;   // a display flag was given: .ppm files come from mpt_display
    DisplayOut shown;
    std::memset(&shown.params, 0, sizeof shown.params);   // (clamp, srgb, and 0 = the defaults of include/mpt.h)
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) {
                usage();
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--scene") scene = next();
        else if (a == "--asset-root") assetRoot = next();
        else if (a == "--width") width = std::atoi(next());
        else if (a == "--height") height = std::atoi(next());
        else if (a == "--spp") spp = std::atoi(next());
        else if (a == "--depth") depth = std::atoi(next());
        else if (a == "--seed") seed = static_cast<unsigned>(std::strtoul(next(), nullptr, 10));
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--devices") {
            for (const char* q = next(); *q;) {
                char* end = nullptr;
                const long v = std::strtol(q, &end, 10);
                if (end == q || v < 0) {
                    usage();
                    return 2;
                }
                deviceList.push_back(static_cast<int>(v));
                q = *end == ',' ? end + 1 : end;
            }
        }
        else if (a == "--camera-path") cameraPath = next();
        else if (a == "--out-dir") outDir = next();
        else if (a == "--out") out = next();
        else if (a == "--checkpoint") checkpoint = next();
        else if (a == "--resume") resume = next();
        else if (a == "--denoise") denoise = true;
        else if (a == "--ao") {
            ao = std::atoi(next());
            haveAo = true;
        }
        else if (a == "--ao-radius") {
            aoRadius = static_cast<float>(std::atof(next()));
            haveAoRadius = true;
        }
        else if (a == "--direct") {
            direct = std::atoi(next());
            haveDirect = true;
        }
        else if (a == "--direct-walk") {
            const char* v = next();
            directWalk = std::strcmp(v, "reference") == 0 ? MPT_WALK_REFERENCE : std::strcmp(v, "own") == 0 ? MPT_WALK_OWN : MPT_WALK_AUTO;
            haveDirectWalk = true;
        }
        else if (a == "--nee") nee = true;
        else if (a == "--nee-walk") {
            const char* v = next();
            neeWalk = std::strcmp(v, "reference") == 0 ? MPT_WALK_REFERENCE : std::strcmp(v, "own") == 0 ? MPT_WALK_OWN : MPT_WALK_AUTO;
            haveNeeOpt = true;
        }
        else if (a == "--nee-clamp") {
            neeClamp = static_cast<float>(std::atof(next()));
            haveNeeOpt = true;
        }
        else if (a == "--light-sampling") {
            const char* v = next();
            if (std::strcmp(v, "area") != 0 && std::strcmp(v, "cone") != 0) {
                std::fprintf(stderr, "mpt_render: --light-sampling takes area or cone\n");
                return 2;
            }
            lightSampling = std::strcmp(v, "cone") == 0 ? MPT_LIGHT_SAMPLING_CONE : MPT_LIGHT_SAMPLING_AREA;
            haveLightSampling = true;
        }
        else if (a == "--restir") {
            restirK = std::atoi(next());
            haveRestir = true;
        }
        else if (a == "--restir-radius") {
            restirRadius = std::atoi(next());
            haveRestirRadius = haveRestirOpt = true;
        }
        else if (a == "--restir-biased") {
            restirMode = MPT_RESTIR_BIASED;
            haveRestirOpt = true;
        }
        else if (a == "--light-candidates") {
            lightCandidates = std::atoi(next());
            if (lightCandidates < 1 || lightCandidates > static_cast<int>(MPT_LIGHT_CANDIDATES_MAX)) {
                std::fprintf(stderr, "mpt_render: --light-candidates takes a count in 1..32\n");
                return 2;
            }
            haveLightCandidates = true;
        }
        else if (a == "--denoise-iterations") dnp.iterations = std::atoi(next());
        else if (a == "--adaptive") {
            adaptive = true;
            adp.threshold = static_cast<float>(std::atof(next()));
        }
        else if (a == "--nee-adaptive") {
            neeAdaptive = true;
            adp.threshold = static_cast<float>(std::atof(next()));
        }
        else if (a == "--temporal") temporal = true;
        else if (a == "--svgf") svgf = true;
        else if (a == "--svgf-iterations") {
            svgfIterations = std::atoi(next());
            haveSvgfIterations = true;
        }
        else if (a == "--temporal-history") tpp.max_history = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--temporal-spp") temporalSpp = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--tonemap" || a == "--transfer") {
            static const char* const names[2][3] = {{"clamp", "reinhard", "aces"}, {"srgb", "gamma22", "linear"}};
            const int which = a == "--transfer";
            const char* v = next();
            int k = 0;
            while (k < 3 && std::strcmp(v, names[which][k]) != 0) ++k;
            if (k == 3) {
                usage();
                return 2;
            }
            (which ? shown.params.transfer : shown.params.tone) = k;
            display = true;
        }
        else if (a == "--exposure") {
            shown.params.exposure = exp2f(static_cast<float>(std::atof(next())));
            display = true;
        }
        else if (a == "--white") {
            shown.params.white = static_cast<float>(std::atof(next()));
            display = true;
        }
        else if (a == "--auto-exposure") {
            shown.params.auto_exposure = 1;
            display = true;
        }
        else if (a == "--key") shown.params.key = static_cast<float>(std::atof(next()));
        else if (a == "--percentile") shown.params.percentile = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--adaptation") shown.params.adaptation = static_cast<float>(std::atof(next()));
        else if (a == "--adaptive-min") adp.min_samples = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--adaptive-batch") adp.batch_samples = static_cast<uint32_t>(std::strtoul(next(), nullptr, 10));
        else if (a == "--adaptive-floor") adp.luminance_floor = static_cast<float>(std::atof(next()));
        else if (a == "--bvh") {
            const char* v = next();
            bvh = std::strcmp(v, "reference") == 0 ? Renderer::BUILD_REFERENCE
                  : std::strcmp(v, "binned") == 0  ? Renderer::BUILD_BINNED
                  : std::strcmp(v, "gpu") == 0     ? Renderer::BUILD_GPU : Renderer::BUILD_AUTO;
        }
        else if (a == "--camera-pos" || a == "--camera-dir" || a == "--camera-up") {
            float v[3] = {0, 0, 0};
            if (std::sscanf(next(), "%f,%f,%f", &v[0], &v[1], &v[2]) != 3) {
                usage();
                return 2;
            }
            float* dst = a == "--camera-pos" ? camPos : (a == "--camera-dir" ? camDir : camUp);
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
            (a == "--camera-pos" ? havePos : (a == "--camera-dir" ? haveDir : haveUp)) = true;
        }
        else if (a == "--vfov") vfov = static_cast<float>(std::atof(next()));
        else if (a == "--rng") prm.rng_mode = std::strcmp(next(), "literal") == 0 ? MPT_RNG_LITERAL : MPT_RNG_PHILOX;
        else if (a == "--bsdf") {
            const char* v = next();
            prm.bsdf_mode = std::strcmp(v, "scatter") == 0 ? MPT_BSDF_SCATTER : std::strcmp(v, "scatter-all") == 0 ? MPT_BSDF_SCATTER_ALL : MPT_BSDF_LAMBERT;
        }
        else if (a == "--pipeline") {
            const char* v = next();
            prm.pipeline = std::strcmp(v, "megakernel") == 0 ? MPT_PIPE_MEGAKERNEL
                           : std::strcmp(v, "wavefront") == 0 ? MPT_PIPE_WAVEFRONT
                           : std::strcmp(v, "wavelocal") == 0 ? MPT_PIPE_WAVELOCAL
                           : std::strcmp(v, "ordered") == 0 ? MPT_PIPE_ORDERED : MPT_PIPE_AUTO;
        }
        else {
            usage();
            return a == "--help" ? 0 : 2;
        }
    }
    if (scene.empty()) {
        usage();
        return 2;
    }
    prm.max_depth = depth;
    prm.seed_lo = seed;
    if (bvh < 0) bvh = prm.rng_mode == MPT_RNG_LITERAL || frames > 0 || !cameraPath.empty() ? Renderer::BUILD_REFERENCE : Renderer::BUILD_AUTO;
    if (!deviceList.empty()) gpus = static_cast<int>(deviceList.size());
    const bool outPpm = out.size() > 4 && out.substr(out.size() - 4) == ".ppm";
    if (display && !out.empty() && !outPpm) {
        std::fprintf(stderr, "mpt_render: the display flags (--tonemap, --transfer, --exposure, --white, --auto-exposure) need a .ppm --out\n");
        return 2;
    }
    if (!display && (shown.params.key != 0.0f || shown.params.percentile != 0u || shown.params.adaptation != 0.0f)) {
        std::fprintf(stderr, "mpt_render: --key, --percentile and --adaptation go with --auto-exposure\n");
        return 2;
    }
    if (neeAdaptive) {   // (first: whatever it meets, the message names this flag)
        const char* why = nee ? "--nee" : adaptive ? "--adaptive" : neeClamp != neeClamp ? "a --nee-clamp that is no number" : gpus > 1 ? "--gpus > 1"
                          : !cameraPath.empty() ? "--camera-path" : frames > 0 ? "--frames" : !checkpoint.empty() ? "--checkpoint"
                          : !resume.empty() ? "--resume" : haveAo || haveAoRadius ? "--ao" : haveDirect || haveDirectWalk ? "--direct"
                          : prm.rng_mode == MPT_RNG_LITERAL ? "--rng literal" : prm.bsdf_mode == MPT_BSDF_SCATTER_ALL ? "--bsdf scatter-all" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --nee-adaptive cannot be combined with %s\n", why);
            return 2;
        }
    }
    if (haveLightSampling && !nee && !haveDirect && !neeAdaptive) {
        std::fprintf(stderr, "mpt_render: --light-sampling goes with --direct, --nee or --nee-adaptive\n");
        return 2;
    }
    if (haveLightCandidates && (neeAdaptive ? lightCandidates > 1 : !nee && !haveDirect)) {
        std::fprintf(stderr, neeAdaptive ? "mpt_render: --light-candidates above 1 cannot be combined with --nee-adaptive\n"
                                         : "mpt_render: --light-candidates goes with --direct or --nee\n");
        return 2;
    }
    if (haveRestir || haveRestirOpt) {
        const char* why = !haveRestir ? "--restir-radius and --restir-biased go with --restir K" : !haveDirect ? "--restir goes with --direct"
                          : restirK < 0 || restirK > static_cast<int>(MPT_RESTIR_MAX_NEIGHBOURS) ? "--restir takes a count in 0..16"
                          : haveRestirRadius && (restirRadius < 1 || restirRadius > static_cast<int>(MPT_RESTIR_MAX_RADIUS)) ? "--restir-radius takes a radius in 1..64"
                          : lightSampling == MPT_LIGHT_SAMPLING_CONE ? "--restir cannot be combined with --light-sampling cone" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: %s\n", why);
            return 2;
        }
    }
    if (!neeAdaptive && (nee || haveNeeOpt)) {
        const char* why = !nee ? "a run without --nee" : neeClamp != neeClamp ? "a --nee-clamp that is no number" : adaptive ? "--adaptive" : gpus > 1 ? "--gpus > 1"
                          : !cameraPath.empty() ? "--camera-path" : frames > 0 ? "--frames" : haveAo || haveAoRadius ? "--ao"
                          : haveDirect || haveDirectWalk ? "--direct"
                          : prm.rng_mode == MPT_RNG_LITERAL ? "--rng literal" : prm.bsdf_mode == MPT_BSDF_SCATTER_ALL ? "--bsdf scatter-all" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --nee cannot be combined with %s\n", why);
            return 2;
        }
    }
    if (haveDirect || haveDirectWalk) {
        const char* why = direct < 1 || direct > static_cast<int>(MPT_DIRECT_MAX_SAMPLES) ? "a sample count outside 1..1024" : !outPpm ? "an --out that is no .ppm"
                          : haveAo || haveAoRadius ? "--ao" : frames > 0 ? "--frames" : !cameraPath.empty() ? "--camera-path" : gpus > 1 ? "--gpus > 1"
                          : adaptive ? "--adaptive" : denoise ? "--denoise" : display ? "the display flags" : temporal ? "--temporal" : svgf ? "--svgf"
                          : !checkpoint.empty() ? "--checkpoint" : !resume.empty() ? "--resume" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --direct cannot be combined with %s\n", why);
            return 2;
        }
    }
    if (haveAo || haveAoRadius) {
        const char* why = ao < 1 || ao > static_cast<int>(MPT_AO_MAX_SAMPLES) ? "a sample count outside 1..1024" : !outPpm ? "an --out that is no .ppm"
                          : frames > 0 ? "--frames" : !cameraPath.empty() ? "--camera-path" : gpus > 1 ? "--gpus > 1" : adaptive ? "--adaptive"
                          : denoise ? "--denoise" : display ? "the display flags" : temporal ? "--temporal" : svgf ? "--svgf"
                          : !checkpoint.empty() ? "--checkpoint" : !resume.empty() ? "--resume" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --ao cannot be combined with %s\n", why);
            return 2;
        }
    }
    if (adaptive) {
        const char* why = frames > 0 ? "--frames" : !cameraPath.empty() ? "--camera-path" : gpus > 1 ? "--gpus > 1"
                          : prm.rng_mode == MPT_RNG_LITERAL ? "--rng literal" : !checkpoint.empty() ? "--checkpoint"
                          : !resume.empty() ? "--resume" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --adaptive cannot be combined with %s\n", why);
            return 2;
        }
    }
    if (temporal) {
        const char* why = cameraPath.empty() ? "a run without --camera-path" : prm.rng_mode == MPT_RNG_LITERAL ? "--rng literal" : gpus > 1 ? "--gpus > 1"
                          : adaptive ? "--adaptive" : !checkpoint.empty() ? "--checkpoint" : !resume.empty() ? "--resume"
                          : temporalSpp == 0 ? "--temporal-spp 0" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --temporal cannot be combined with %s\n", why);
            return 2;
        }
    }
    if (svgf) {
        // (--adaptive first: it needs a run without --camera-path, which --svgf cannot be)
        const char* why = adaptive ? "--adaptive" : cameraPath.empty() ? "a run without --camera-path" : temporal ? "--temporal"
                          : denoise ? "--denoise" : prm.rng_mode == MPT_RNG_LITERAL ? "--rng literal" : gpus > 1 ? "--gpus > 1"
                          : !checkpoint.empty() ? "--checkpoint" : !resume.empty() ? "--resume" : temporalSpp == 0 ? "--temporal-spp 0" : nullptr;
        if (why) {
            std::fprintf(stderr, "mpt_render: --svgf cannot be combined with %s\n", why);
            return 2;
        }
        if (haveSvgfIterations && (svgfIterations < 0 || svgfIterations > MPT_DENOISE_MAX_ITERATIONS)) {
            std::fprintf(stderr, "mpt_render: --svgf-iterations must be between 0 and %d\n", MPT_DENOISE_MAX_ITERATIONS);
            return 2;
        }
    }
    if (gpus > 1) {
        if (deviceList.empty())
            for (int g = 0; g < gpus; ++g) deviceList.push_back(device + g);
        return renderOnSeveralGpus(scene, assetRoot, out, width, height, spp, deviceList, bvh, prm, havePos ? camPos : nullptr, haveDir ? camDir : nullptr,
                                   haveUp ? camUp : nullptr, vfov, denoise ? &dnp : nullptr, display ? &shown : nullptr);
    }
    if (deviceList.size() == 1) device = deviceList[0];
    try {
        Renderer r(device, scene, assetRoot, bvh);
        r.setRenderParams(prm);
        if (haveLightSampling) r.setLightSampling(lightSampling);
        if (haveLightCandidates) r.setLightCandidates(static_cast<uint32_t>(lightCandidates));
        // the reference hard-codes Camera::reset(); the flags overwrite the same globals before the viewport is built
        if (havePos) Camera::position = mpt::float3(camPos[0], camPos[1], camPos[2]);
        if (haveDir) Camera::forward = mpt::normalize(mpt::float3(camDir[0], camDir[1], camDir[2]));
        if (haveUp) Camera::up = mpt::normalize(mpt::float3(camUp[0], camUp[1], camUp[2]));
        if (vfov > 0.0f) Camera::verticalFov = vfov;
        OffscreenView view;
        r.drawableSizeWillChange(&view, DrawableSize{(double)width, (double)height});
        std::vector<float> img;
        float scale = 1.0f;
        std::string extraJson;
        // (the "direct" / "nee" object names the sampling only when the flag was given: without it the line is what it was)
        const std::string samplingJson = std::string(!haveLightSampling ? "" : lightSampling == MPT_LIGHT_SAMPLING_CONE ? ", \"light_sampling\": \"cone\"" : ", \"light_sampling\": \"area\"") +
                                         (haveLightCandidates ? ", \"light_candidates\": " + std::to_string(lightCandidates) : std::string());
        const bool neeRis = nee && lightCandidates > 1;   // (resampled: the header MPTNEE3 names the sampling and the candidates)
        const bool neeCone = nee && !neeRis && lightSampling == MPT_LIGHT_SAMPLING_CONE;
        auto t0 = std::chrono::steady_clock::now();
        if (ao > 0) {   // grey (ao, ao, ao, 1) through the writer the radiance goes through
            const mpt_ao_info info = r.renderAmbientOcclusion(static_cast<uint32_t>(ao), aoRadius);
            std::vector<float> a;
            r.readAmbientOcclusion(a);
            img.resize(a.size() * 4);
            for (size_t k = 0; k < a.size(); ++k) {
                img[4 * k] = img[4 * k + 1] = img[4 * k + 2] = a[k];
                img[4 * k + 3] = 1.0f;
            }
            char buf[256];
            std::snprintf(buf, sizeof buf, ", \"ao\": {\"samples\": %d, \"radius\": %.9g, \"pixels_surface\": %llu, \"rays\": %llu, \"rays_occluded\": %llu, \"device_ms\": %.3f}",
                          ao, static_cast<double>(aoRadius), (unsigned long long)info.pixels_surface, (unsigned long long)info.rays,
                          (unsigned long long)info.rays_occluded, info.device_ms);
            extraJson = buf;
        } else if (direct > 0 && haveRestir) {   // the same, with spatial reservoir reuse
            const mpt_restir_info info = r.renderDirectRestir(static_cast<uint32_t>(direct), static_cast<uint32_t>(restirK), static_cast<uint32_t>(restirRadius),
                                                              restirMode, directWalk);
            r.readDirectRestir(img);
            char buf[640];
            std::snprintf(buf, sizeof buf,
                          ", \"restir\": {\"samples\": %d, \"neighbours\": %d, \"radius\": %d, \"mode\": \"%s\", \"pixels_surface\": %llu, \"rays_initial\": %llu, "
                          "\"rays_final\": %llu, \"rays_correction\": %llu, \"rays_occluded\": %llu, \"neighbours_accepted\": %llu, "
                          "\"samples_from_neighbours\": %llu, \"lights\": %llu, \"device_ms\": %.3f",
                          direct, restirK, restirRadius ? restirRadius : static_cast<int>(MPT_RESTIR_DEFAULT_RADIUS),
                          restirMode == MPT_RESTIR_BIASED ? "biased" : "unbiased", (unsigned long long)info.pixels_surface,
                          (unsigned long long)info.rays_initial, (unsigned long long)info.rays_final, (unsigned long long)info.rays_correction,
                          (unsigned long long)info.rays_occluded, (unsigned long long)info.neighbours_accepted,
                          (unsigned long long)info.samples_from_neighbours, (unsigned long long)info.lights, info.device_ms);
            extraJson = buf + samplingJson + "}";
        } else if (direct > 0) {   // the pass's rgba through the writer the radiance goes through
            const mpt_direct_info info = r.renderDirectLighting(static_cast<uint32_t>(direct), directWalk);
            r.readDirectLighting(img);
            char buf[320];
            std::snprintf(buf, sizeof buf, ", \"direct\": {\"samples\": %d, \"pixels_surface\": %llu, \"rays\": %llu, \"rays_occluded\": %llu, \"lights\": %llu, \"device_ms\": %.3f",
                          direct, (unsigned long long)info.pixels_surface, (unsigned long long)info.rays, (unsigned long long)info.rays_occluded,
                          (unsigned long long)info.lights, info.device_ms);
            extraJson = buf + samplingJson + "}";
        } else if (adaptive || neeAdaptive) {
            mpt_nee_info neeInfo = {};
            const mpt_adaptive_info info = neeAdaptive ? r.renderNeeAdaptive(static_cast<uint32_t>(spp), depth, adp, neeWalk, neeClamp, 0, &neeInfo)
                                                       : r.renderAdaptive(0, static_cast<uint32_t>(spp), adp);
            if (!display || denoise) r.readAdaptiveMean(img);
            if (display && !denoise) present(r, shown, MPT_DISPLAY_ADAPTIVE);
            if (denoise) {   // the mean through the filter kernels, with the context's guides (mpt_read_aovs + mpt_denoise_image)
                std::vector<float> ad(img.size()), nc(img.size()), dn(img.size());
                mpt_ctx* ctx = r.context();
                int rc = mpt_read_aovs(ctx, ad.data(), nc.data(), nullptr);
                if (!rc) rc = mpt_denoise_image(ctx, width, height, img.data(), ad.data(), nc.data(), &dnp, dn.data());
                if (rc) throw std::runtime_error(std::string("adaptive denoise: ") + mpt_status_string(rc) + ": " + mpt_last_error(ctx));
                img.swap(dn);
                if (display) {   // (that mean is on the host: the display kernels take it from there)
                    shown.rgba8.resize(static_cast<size_t>(width) * height * 4);
                    rc = mpt_display_image(ctx, width, height, img.data(), &shown.params, nullptr, shown.rgba8.data(), nullptr, &shown.info);
                    if (rc) throw std::runtime_error(std::string("adaptive display: ") + mpt_status_string(rc) + ": " + mpt_last_error(ctx));
                }
            }
            const double pixels = static_cast<double>(width) * height;
            char buf[256];
            std::snprintf(buf, sizeof buf,
                          ", \"adaptive\": {\"passes\": %u, \"samples\": %llu, \"tiles_converged\": %u, \"tiles_at_max\": %u, \"mean_spp\": %.4f}",
                          info.passes, (unsigned long long)info.samples, info.tiles_converged, info.tiles_at_max,
                          pixels > 0 ? static_cast<double>(info.samples) / pixels : 0.0);
            extraJson = buf;
            if (neeAdaptive) {
                char nbuf[320];
                std::snprintf(nbuf, sizeof nbuf, ", \"nee\": {\"paths\": %llu, \"rays\": %llu, \"shadow_rays\": %llu, \"shadow_rays_occluded\": %llu, \"lights\": %llu, \"device_ms\": %.3f",
                              (unsigned long long)neeInfo.paths, (unsigned long long)neeInfo.rays, (unsigned long long)neeInfo.shadow_rays,
                              (unsigned long long)neeInfo.shadow_rays_occluded, (unsigned long long)neeInfo.lights, neeInfo.device_ms);
                extraJson += nbuf + samplingJson + "}";
            }
        } else if (!cameraPath.empty()) {
            if (temporal) r.setTemporalParams(tpp);
            if (svgf) {
                mpt_svgf_params sp = {0, 0, tpp.max_history, 0.0f, 0.0f, 0.0f, haveSvgfIterations ? svgfIterations : -1, 0.0f, 0.0f, 0.0f, -1};
                r.setSvgfParams(sp);
            }
            const int n = playCameraPath(r, view, cameraPath, outDir, denoise ? &dnp : nullptr, temporal || svgf ? temporalSpp : 0u, svgf,
                                         display ? &shown : nullptr);
            if (n < 0) return 1;
            frames = n;
            if (display) {
                // --out gets what the last frame got: its bytes, which `shown` still holds
            } else if (svgf) {   // --out gets what the last frame got
                r.readSvgf(view.rgba);
                img = view.rgba;
            } else if (temporal) {   // --out gets what the last frame got: the history, or the filtered history
                if (denoise) r.denoiseTemporal(dnp, view.rgba);
                else r.readTemporal(view.rgba);
                img = view.rgba;
            } else {
                r.readFrame(&view);
                img = view.rgba;
                if (denoise) r.denoise(dnp, img);
            }
        } else if (frames > 0) {
            for (int f = 0; f < frames; ++f) r.draw(&view);
            if (display) {
                if (denoise) denoiseOnDevice(r, dnp, MPT_DENOISE_FRAME, 0);
                present(r, shown, denoise ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_FRAME);
            } else {
                r.readFrame(&view);
                img = view.rgba;
                if (denoise) r.denoise(dnp, img);
            }
        } else {
            // checkpoint / resume of the accumulation (the reference's running mean lives in a GPU-private texture and is lost with the
            // process, R/Renderer/Renderer.cpp:236): header "MPTSUM2 W H samples seed rng depth bsdf scene-hash\n" + W * H * 4 raw floats.
            // The hash (FNV-1a over the packed primitive and material arrays) and the BSDF mode identify WHAT was accumulated: a resume on
            // another scene or material model is refused instead of mixing sums.  Written to a temporary file and renamed over the target,
            // so that a crash mid-write never destroys the checkpoint that --resume just read.
            uint32_t have = 0;
            unsigned neeClampBits = 0;   // the bits of the clamp in force (0: none)
            if (nee && neeClamp > 0.0f) std::memcpy(&neeClampBits, &neeClamp, sizeof neeClampBits);
            r.clearSum();
            const unsigned long long sceneHash = sceneFingerprint(*r.scene());
            if (!resume.empty()) {
                FILE* f = std::fopen(resume.c_str(), "rb");
                int w = 0, h = 0, rngm = 0, dep = 0, bs = 0;
                unsigned sd = 0;
                unsigned long long sh = 0;
                // (an --nee sum is another estimator's: its header is "MPTNEE1 ... scene-hash clamp-bits\n", which the plain format does not
                //  parse and the other way round, so neither run continues the other's sum, nor an --nee run one of another clamp; with
                //  cone sampling of the sphere lights it is "MPTNEE2 ... clamp-bits sampling\n": the two samplings do not mix either; with
                //  more than one light candidate it is "MPTNEE3 ... clamp-bits sampling candidates\n")
                unsigned cb = 0;
                int ls = 0, lc = 0;
                const bool parsed = f && (neeRis ? std::fscanf(f, "MPTNEE3 %d %d %u %u %d %d %d %llx %x %d %d", &w, &h, &have, &sd, &rngm, &dep, &bs, &sh, &cb, &ls, &lc) == 11 &&
                                                       ls == lightSampling && lc == lightCandidates
                                          : neeCone ? std::fscanf(f, "MPTNEE2 %d %d %u %u %d %d %d %llx %x %d", &w, &h, &have, &sd, &rngm, &dep, &bs, &sh, &cb, &ls) == 10 &&
                                                        ls == lightSampling
                                          : nee ? std::fscanf(f, "MPTNEE1 %d %d %u %u %d %d %d %llx %x", &w, &h, &have, &sd, &rngm, &dep, &bs, &sh, &cb) == 9
                                              : std::fscanf(f, "MPTSUM2 %d %d %u %u %d %d %d %llx", &w, &h, &have, &sd, &rngm, &dep, &bs, &sh) == 8);
                if (!parsed || std::fgetc(f) != '\n') {
                    if (f) std::fclose(f);
                    throw std::runtime_error("cannot read the checkpoint " + resume + (neeRis ? " as one of an --nee render with these light candidates and this light sampling"
                                                                                     : neeCone ? " as one of an --nee render with cone light sampling"
                                                                                     : nee   ? " as one of an --nee render with area light sampling" : " as one of a plain render"));
                }
                if (nee && cb != neeClampBits) {
                    std::fclose(f);
                    throw std::runtime_error("the checkpoint " + resume + " was written with another --nee-clamp");
                }
                if (w != width || h != height || sd != seed || rngm != prm.rng_mode || dep != depth || bs != prm.bsdf_mode || sh != sceneHash) {
                    std::fclose(f);
                    throw std::runtime_error("the checkpoint " + resume + " was written with another scene, size, seed, RNG, BSDF mode or depth");
                }
                std::vector<float> sum(static_cast<size_t>(w) * h * 4);
                const size_t got = std::fread(sum.data(), sizeof(float), sum.size(), f);
                std::fclose(f);
                if (got != sum.size()) throw std::runtime_error("the checkpoint " + resume + " is truncated");
                r.writeSum(sum);
            }
            if (nee) {
                const mpt_nee_info info = r.renderNee(static_cast<uint32_t>(spp), depth, neeWalk, neeClamp, have);
                char buf[320];
                std::snprintf(buf, sizeof buf, ", \"nee\": {\"paths\": %llu, \"rays\": %llu, \"shadow_rays\": %llu, \"shadow_rays_occluded\": %llu, \"lights\": %llu, \"device_ms\": %.3f",
                              (unsigned long long)info.paths, (unsigned long long)info.rays, (unsigned long long)info.shadow_rays,
                              (unsigned long long)info.shadow_rays_occluded, (unsigned long long)info.lights, info.device_ms);
                extraJson = buf + samplingJson + "}";
            } else {
                r.renderBatch(have, static_cast<uint32_t>(spp));
            }
            if (!display || !checkpoint.empty()) r.readSum(img);
            if (!checkpoint.empty()) {
                const std::string tmp = checkpoint + ".tmp";
                FILE* f = std::fopen(tmp.c_str(), "wb");
                if (!f) throw std::runtime_error("cannot write " + tmp);
                if (neeRis)
                    std::fprintf(f, "MPTNEE3 %d %d %u %u %d %d %d %llx %x %d %d\n", width, height, have + static_cast<uint32_t>(spp), seed, prm.rng_mode, depth,
                                 prm.bsdf_mode, sceneHash, neeClampBits, lightSampling, lightCandidates);
                else if (neeCone)
                    std::fprintf(f, "MPTNEE2 %d %d %u %u %d %d %d %llx %x %d\n", width, height, have + static_cast<uint32_t>(spp), seed, prm.rng_mode, depth,
                                 prm.bsdf_mode, sceneHash, neeClampBits, lightSampling);
                else if (nee)
                    std::fprintf(f, "MPTNEE1 %d %d %u %u %d %d %d %llx %x\n", width, height, have + static_cast<uint32_t>(spp), seed, prm.rng_mode, depth,
                                 prm.bsdf_mode, sceneHash, neeClampBits);
                else
                    std::fprintf(f, "MPTSUM2 %d %d %u %u %d %d %d %llx\n", width, height, have + static_cast<uint32_t>(spp), seed, prm.rng_mode, depth, prm.bsdf_mode,
                                 sceneHash);
                const bool ok = std::fwrite(img.data(), sizeof(float), img.size(), f) == img.size();
                if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), checkpoint.c_str()) != 0) {
                    std::remove(tmp.c_str());
                    throw std::runtime_error("cannot write " + checkpoint);
                }
            }
            scale = 1.0f / static_cast<float>(have + static_cast<uint32_t>(spp));
            if (display) {
                if (denoise) denoiseOnDevice(r, dnp, MPT_DENOISE_SUM, have + static_cast<uint32_t>(spp));
                present(r, shown, denoise ? MPT_DISPLAY_DENOISED : MPT_DISPLAY_SUM, have + static_cast<uint32_t>(spp));
            } else if (denoise) {   // the checkpoint above keeps the raw sum; the image is the denoised sum / samples
                mpt_denoise_params q = dnp;
                q.samples = have + static_cast<uint32_t>(spp);
                r.denoise(q, img);
                scale = 1.0f;
            }
        }
        double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        mpt_stats st = r.stats();
        std::printf("{\"paths\": %llu, \"rays\": %llu, \"seconds\": %.6f, \"device_ms\": %.3f, \"mrays_per_s\": %.1f%s}\n",
                    (unsigned long long)st.paths, (unsigned long long)st.rays, sec, st.total_ms,
                    st.total_ms > 0 ? st.rays / st.total_ms / 1e3 : 0.0, extraJson.c_str());
        if (!out.empty()) {
            int rc = display && shown.rgba8.empty() ? MPT_ERR_NOT_READY   // (a camera path without a frame)
                     : display ? mpt_write_ppm8(out.c_str(), shown.rgba8.data(), width, height)
                     : outPpm  ? mpt_write_ppm(out.c_str(), img.data(), width, height, scale, 2.2f)
                               : mpt_write_pfm(out.c_str(), img.data(), width, height, scale);
            if (rc) {
                std::fprintf(stderr, "cannot write %s\n", out.c_str());
                return 1;
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mpt_render: %s\n", e.what());
        return 1;
    }
    return 0;
}
