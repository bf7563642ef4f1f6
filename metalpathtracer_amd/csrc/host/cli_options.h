// cli_options.h — what mpt_render's command line says (Options), the table of flags that fills it (flagTable, parseOptions), and the
// combinations it refuses, as data (validate).
//   a new flag      one member of Options and one row of flagTable (and its line in usage())
//   a new conflict  one row in the Check of the mode that refuses it; a condition met in several modes is one of the named Conditions
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "Renderer.h"
#include "mpt.h"

using MetalCppPathTracer::Renderer;   // (for its BUILD_* words)

inline void usage() {
    std::puts(
        "mpt_render --scene scene.xml [--asset-root DIR] [--width 1280] [--height 720]\n"
        "           [--spp 64] [--depth 32] [--seed 1] [--rng philox|literal] [--bsdf lambert|scatter|scatter-all]\n"
        "           [--pipeline auto|ordered|wavelocal|wavefront|megakernel] [--frames N] [--device 0] [--out image.pfm|image.ppm]\n"
        "           [--camera-pos x,y,z] [--camera-dir x,y,z] [--camera-up x,y,z] [--vfov degrees]\n"
        "           [--gpus N | --devices a,b,...] [--camera-path FILE [--out-dir runs]] [--bvh reference|binned|gpu|auto]\n"
        "           [--checkpoint FILE] [--resume FILE] [--denoise [--denoise-iterations N]] [--ao N [--ao-radius R]]\n"
        "           [--direct N [--direct-walk reference|own|auto] [--restir K [--restir-radius R] [--restir-biased]]]\n"
        "           [--camera-path FILE --direct 1 --restir-temporal [--restir-history C] [--restir-biased]]\n"
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
        "  --restir-temporal with --camera-path and --direct 1: temporal reservoir reuse (mpt_direct_restir_temporal, include/mpt.h) — every\n"
        "                    frame of the path is one round of the direct pass in which a pixel merges the sample its --light-candidates\n"
        "                    pick with the reservoir of the pixel its surface point had in the frame before, which counts for at most\n"
        "                    --restir-history C frames' candidates (1..1024, default 20).  Unbiased by default: one more shadow ray per\n"
        "                    accepted history; --restir-biased omits it.  The frame's direct lighting goes to <out-dir>/frame_NNNN.ppm through\n"
        "                    the same writer, --out gets the last frame, the per-frame JSON line gains \"accepted\", \"from_history\" and\n"
        "                    \"reset\".  Not with --restir K, --light-sampling cone, --temporal, --svgf, --denoise, the display flags,\n"
        "                    --gpus > 1, --checkpoint or --resume.  Without it every file and line is what it was\n"
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

// Everything the command line says.  "Was given" is a member next to its value; what the API takes as a struct is that struct.
struct Options {
    std::string scene, assetRoot, out, cameraPath, outDir = "runs", checkpoint, resume;
    int width = 1280, height = 720, spp = 64, device = 0, frames = 0;
    mpt_render_params prm = {};   // --rng, --bsdf, --pipeline, --depth (max_depth), --seed (seed_lo)
    int gpusFlag = 1;             // --gpus N
    std::vector<int> deviceList;  // --devices a,b,...: the ordinals of a multi-GPU render, one rank each
    int bvhFlag = -1;             // --bvh; -1 = by mode, see bvh()
    float camPos[3] = {}, camDir[3] = {}, camUp[3] = {}, vfov = 0.0f;
    bool havePos = false, haveDir = false, haveUp = false;
    bool denoise = false;
    mpt_denoise_params dnp = {};
    bool temporal = false;
    mpt_temporal_params tpp = {};
    uint32_t temporalSpp = 1;
    bool svgf = false, haveSvgfIterations = false;
    int svgfIterations = -1;      // (the default of include/mpt.h)
    bool adaptive = false, neeAdaptive = false;   // --adaptive T, --nee-adaptive T: both thresholds go into adp, the last one wins
    mpt_adaptive_params adp = {}; // (0 = the defaults of include/mpt.h)
    int ao = 0;                   // --ao N: shadow rays per surface pixel
    bool haveAo = false;          // (with whatever count: 0 is refused, not ignored)
    float aoRadius = 0.0f;
    bool haveAoRadius = false;
    int direct = 0;               // --direct N: light samples per surface pixel
    bool haveDirect = false, haveDirectWalk = false;
    int32_t directWalk = MPT_WALK_AUTO;
    bool nee = false, haveNeeWalk = false, haveNeeClamp = false;
    int32_t neeWalk = MPT_WALK_AUTO;
    float neeClamp = 0.0f;
    bool haveLightSampling = false, haveLightCandidates = false;
    int lightSampling = MPT_LIGHT_SAMPLING_AREA, lightCandidates = 1;
    bool haveRestir = false, haveRestirRadius = false, restirBiased = false;
    int restirK = 0, restirRadius = 0;
    bool restirTemporal = false, haveRestirHistory = false;   // --restir-temporal, --restir-history C
    int restirHistory = 0;        // (0 = the default of include/mpt.h)
    bool display = false;         // a display flag was given: .ppm files come from mpt_display
    mpt_display_params shown = {};   // (clamp, srgb, and 0 = the defaults of include/mpt.h; source and samples are set per call)

    Options() {
        prm.rng_mode = MPT_RNG_PHILOX;
        prm.shard_count = 1;
        prm.pipeline = MPT_PIPE_AUTO;
        prm.max_depth = 32;
        prm.seed_lo = 1;
        dnp.iterations = -1;   // (the default of include/mpt.h)
    }

    bool outPpm() const { return out.size() > 4 && out.substr(out.size() - 4) == ".ppm"; }
    // a multi-GPU render is one rank per listed ordinal, or --device .. --device + N - 1
    int gpus() const { return deviceList.empty() ? gpusFlag : static_cast<int>(deviceList.size()); }
    std::vector<int> devices() const {
        if (!deviceList.empty()) return deviceList;
        std::vector<int> d(1, device);   // (a run on one GPU is on --device, whatever --gpus says)
        for (int g = 1; g < gpusFlag; ++g) d.push_back(device + g);
        return d;
    }
    // the reference's builder for the frame protocol and the literal RNG (the drop-in behaviour), auto for batch renders
    int bvh() const {
        if (bvhFlag >= 0) return bvhFlag;
        return prm.rng_mode == MPT_RNG_LITERAL || frames > 0 || !cameraPath.empty() ? Renderer::BUILD_REFERENCE : Renderer::BUILD_AUTO;
    }
    bool neeRis() const { return nee && lightCandidates > 1; }   // (resampled: the checkpoint names the sampling and the candidates)
    bool neeCone() const { return nee && !neeRis() && lightSampling == MPT_LIGHT_SAMPLING_CONE; }
    int32_t restirMode() const { return restirBiased ? MPT_RESTIR_BIASED : MPT_RESTIR_UNBIASED; }
};

// ---- parsing ----------------------------------------------------------------------------------------------------------------------------

constexpr int kParsed = -1;   // parseOptions and a row's function: go on (anything else is the exit status)

// A flag whose value is one of a few words.  What an unknown word does is the list's policy.
struct WordList {
    struct Word { const char* name; int value; };
    enum Unknown { FALLS_BACK, REFUSED_WITH_USAGE, REFUSED_WITH_MESSAGE };
    std::vector<Word> words;
    Unknown unknown;
    int fallback;          // FALLS_BACK: the value of an unknown word
    const char* message;   // REFUSED_WITH_MESSAGE

    int parse(const char* v, int* value) const {
        for (const Word& w : words)
            if (std::strcmp(v, w.name) == 0) {
                *value = w.value;
                return kParsed;
            }
        if (unknown == FALLS_BACK) {
            *value = fallback;
            return kParsed;
        }
        if (unknown == REFUSED_WITH_USAGE) usage();
        else std::fprintf(stderr, "mpt_render: %s\n", message);
        return 2;
    }
};
static const WordList
    kWalks = {{{"reference", MPT_WALK_REFERENCE}, {"own", MPT_WALK_OWN}, {"auto", MPT_WALK_AUTO}}, WordList::FALLS_BACK, MPT_WALK_AUTO, nullptr},
    kBuilders = {{{"reference", Renderer::BUILD_REFERENCE}, {"binned", Renderer::BUILD_BINNED}, {"gpu", Renderer::BUILD_GPU}, {"auto", Renderer::BUILD_AUTO}},
                 WordList::FALLS_BACK, Renderer::BUILD_AUTO, nullptr},
    kPipelines = {{{"megakernel", MPT_PIPE_MEGAKERNEL}, {"wavefront", MPT_PIPE_WAVEFRONT}, {"wavelocal", MPT_PIPE_WAVELOCAL}, {"ordered", MPT_PIPE_ORDERED},
                   {"auto", MPT_PIPE_AUTO}}, WordList::FALLS_BACK, MPT_PIPE_AUTO, nullptr},
    kBsdfs = {{{"lambert", MPT_BSDF_LAMBERT}, {"scatter", MPT_BSDF_SCATTER}, {"scatter-all", MPT_BSDF_SCATTER_ALL}}, WordList::FALLS_BACK, MPT_BSDF_LAMBERT, nullptr},
    kRngs = {{{"philox", MPT_RNG_PHILOX}, {"literal", MPT_RNG_LITERAL}}, WordList::FALLS_BACK, MPT_RNG_PHILOX, nullptr},
    kTones = {{{"clamp", MPT_TONE_CLAMP}, {"reinhard", MPT_TONE_REINHARD}, {"aces", MPT_TONE_ACES}}, WordList::REFUSED_WITH_USAGE, 0, nullptr},
    kTransfers = {{{"srgb", MPT_TRANSFER_SRGB}, {"gamma22", MPT_TRANSFER_GAMMA22}, {"linear", MPT_TRANSFER_LINEAR}}, WordList::REFUSED_WITH_USAGE, 0, nullptr},
    kLightSamplings = {{{"area", MPT_LIGHT_SAMPLING_AREA}, {"cone", MPT_LIGHT_SAMPLING_CONE}}, WordList::REFUSED_WITH_MESSAGE, 0,
                       "--light-sampling takes area or cone"};

// The values that are no plain number, word or triple.
inline int parseDevices(Options& o, const char* v) {
    for (const char* q = v; *q;) {
        char* end = nullptr;
        const long d = std::strtol(q, &end, 10);
        if (end == q || d < 0) {
            usage();
            return 2;
        }
        o.deviceList.push_back(static_cast<int>(d));
        q = *end == ',' ? end + 1 : end;
    }
    return kParsed;
}
inline int parseExposure(Options& o, const char* v) {   // --exposure EV: the multiplier is 2^EV
    o.shown.exposure = exp2f(static_cast<float>(std::atof(v)));
    return kParsed;
}
inline int parseLightCandidates(Options& o, const char* v) {   // (range-checked here: its message comes before a missing --scene and every conflict)
    o.lightCandidates = std::atoi(v);
    if (o.lightCandidates >= 1 && o.lightCandidates <= static_cast<int>(MPT_LIGHT_CANDIDATES_MAX)) return kParsed;
    std::fprintf(stderr, "mpt_render: --light-candidates takes a count in 1..32\n");
    return 2;
}
inline void switchAutoExposure(Options& o) { o.shown.auto_exposure = 1; }

// One row of the flag table: the spelling, the kind (which the constructor reads off the type of where the value goes), the "given" it
// sets, and whether it switches the display on.  Numbers go through atoi / strtoul / atof: `--spp x` is 0, not an error.
struct Flag {
    enum Kind { SWITCH, INT, UNSIGNED, FLOAT, STRING, WORD, TRIPLE, FUNCTION };
    const char* name;
    Kind kind;
    void* value = nullptr;                            // bool, int, unsigned, float, std::string, int (WORD) or float[3], by kind
    const WordList* words = nullptr;                  // WORD
    int (*function)(Options&, const char*) = nullptr; // FUNCTION
    void (*onSwitch)(Options&) = nullptr;             // SWITCH without a bool of its own
    bool* given = nullptr;
    bool display = false;

    Flag(const char* n, bool* v) : name(n), kind(SWITCH), value(v) {}
    Flag(const char* n, void (*f)(Options&), bool d) : name(n), kind(SWITCH), onSwitch(f), display(d) {}
    Flag(const char* n, int* v, bool* g = nullptr) : name(n), kind(INT), value(v), given(g) {}
    Flag(const char* n, unsigned* v) : name(n), kind(UNSIGNED), value(v) {}
    Flag(const char* n, float* v, bool* g = nullptr, bool d = false) : name(n), kind(FLOAT), value(v), given(g), display(d) {}
    Flag(const char* n, std::string* v) : name(n), kind(STRING), value(v) {}
    Flag(const char* n, const WordList& w, int* v, bool* g = nullptr, bool d = false) : name(n), kind(WORD), value(v), words(&w), given(g), display(d) {}
    Flag(const char* n, float (*v)[3], bool* g) : name(n), kind(TRIPLE), value(v), given(g) {}
    Flag(const char* n, int (*f)(Options&, const char*), bool* g = nullptr, bool d = false) : name(n), kind(FUNCTION), function(f), given(g), display(d) {}

    int store(Options& o, const char* v) const {
        switch (kind) {
        case SWITCH:
            if (value) *static_cast<bool*>(value) = true;
            else onSwitch(o);
            break;
        case INT: *static_cast<int*>(value) = std::atoi(v); break;
        case UNSIGNED: *static_cast<unsigned*>(value) = static_cast<unsigned>(std::strtoul(v, nullptr, 10)); break;
        case FLOAT: *static_cast<float*>(value) = static_cast<float>(std::atof(v)); break;
        case STRING: *static_cast<std::string*>(value) = v; break;
        case WORD: return words->parse(v, static_cast<int*>(value));
        case TRIPLE: {
            float* t = *static_cast<float(*)[3]>(value);
            if (std::sscanf(v, "%f,%f,%f", &t[0], &t[1], &t[2]) != 3) {
                usage();
                return 2;
            }
            break;
        }
        case FUNCTION: return function(o, v);
        }
        return kParsed;
    }
};

constexpr bool kDisplay = true;   // (a row's last word: the flag switches the display on)

static std::vector<Flag> flagTable(Options& o) {
    return {
        {"--scene", &o.scene},
        {"--asset-root", &o.assetRoot},
        {"--width", &o.width},
        {"--height", &o.height},
        {"--spp", &o.spp},
        {"--depth", &o.prm.max_depth},
        {"--seed", &o.prm.seed_lo},
        {"--device", &o.device},
        {"--frames", &o.frames},
        {"--gpus", &o.gpusFlag},
        {"--devices", parseDevices},
        {"--camera-path", &o.cameraPath},
        {"--out-dir", &o.outDir},
        {"--out", &o.out},
        {"--checkpoint", &o.checkpoint},
        {"--resume", &o.resume},
        {"--denoise", &o.denoise},
        {"--denoise-iterations", &o.dnp.iterations},
        {"--ao", &o.ao, &o.haveAo},
        {"--ao-radius", &o.aoRadius, &o.haveAoRadius},
        {"--direct", &o.direct, &o.haveDirect},
        {"--direct-walk", kWalks, &o.directWalk, &o.haveDirectWalk},
        {"--nee", &o.nee},
        {"--nee-walk", kWalks, &o.neeWalk, &o.haveNeeWalk},
        {"--nee-clamp", &o.neeClamp, &o.haveNeeClamp},
        {"--light-sampling", kLightSamplings, &o.lightSampling, &o.haveLightSampling},
        {"--light-candidates", parseLightCandidates, &o.haveLightCandidates},
        {"--restir", &o.restirK, &o.haveRestir},
        {"--restir-radius", &o.restirRadius, &o.haveRestirRadius},
        {"--restir-biased", &o.restirBiased},
        {"--restir-temporal", &o.restirTemporal},
        {"--restir-history", &o.restirHistory, &o.haveRestirHistory},
        {"--adaptive", &o.adp.threshold, &o.adaptive},
        {"--nee-adaptive", &o.adp.threshold, &o.neeAdaptive},
        {"--adaptive-min", &o.adp.min_samples},
        {"--adaptive-batch", &o.adp.batch_samples},
        {"--adaptive-floor", &o.adp.luminance_floor},
        {"--temporal", &o.temporal},
        {"--temporal-history", &o.tpp.max_history},
        {"--temporal-spp", &o.temporalSpp},
        {"--svgf", &o.svgf},
        {"--svgf-iterations", &o.svgfIterations, &o.haveSvgfIterations},
        {"--tonemap", kTones, &o.shown.tone, nullptr, kDisplay},
        {"--transfer", kTransfers, &o.shown.transfer, nullptr, kDisplay},
        {"--exposure", parseExposure, nullptr, kDisplay},
        {"--white", &o.shown.white, nullptr, kDisplay},
        {"--auto-exposure", switchAutoExposure, kDisplay},
        {"--key", &o.shown.key},   // (these three do not switch the display on: validate() sends them to --auto-exposure)
        {"--percentile", &o.shown.percentile},
        {"--adaptation", &o.shown.adaptation},
        {"--bvh", kBuilders, &o.bvhFlag},
        {"--camera-pos", &o.camPos, &o.havePos},
        {"--camera-dir", &o.camDir, &o.haveDir},
        {"--camera-up", &o.camUp, &o.haveUp},
        {"--vfov", &o.vfov},
        {"--rng", kRngs, &o.prm.rng_mode},
        {"--bsdf", kBsdfs, &o.prm.bsdf_mode},
        {"--pipeline", kPipelines, &o.prm.pipeline},
    };
}

// Fills `o` from the command line; kParsed, or the exit status of a run that ends here.  A flag without its value and an unknown flag
// print the usage and exit 2; --help is the unknown flag that exits 0, if no earlier argument has ended the run.
inline int parseOptions(int argc, char** argv, Options& o) {
    const std::vector<Flag> table = flagTable(o);
    for (int i = 1; i < argc; ++i) {
        const Flag* flag = nullptr;
        for (const Flag& f : table)
            if (!flag && std::strcmp(argv[i], f.name) == 0) flag = &f;
        if (!flag || (flag->kind != Flag::SWITCH && i + 1 >= argc)) {
            usage();
            return !flag && std::strcmp(argv[i], "--help") == 0 ? 0 : 2;
        }
        const int status = flag->store(o, flag->kind == Flag::SWITCH ? nullptr : argv[++i]);
        if (status != kParsed) return status;
        if (flag->given) *flag->given = true;
        if (flag->display) o.display = true;
    }
    return kParsed;
}

// ---- the combinations that are refused ---------------------------------------------------------------------------------------------------

// A fact about the command line, with the words that name it in a message.
struct Condition {
    bool (*holds)(const Options&);
    const char* words;
};
static const Condition
    kFrames = {[](const Options& o) { return o.frames > 0; }, "--frames"},
    kCameraPath = {[](const Options& o) { return !o.cameraPath.empty(); }, "--camera-path"},
    kNoCameraPath = {[](const Options& o) { return o.cameraPath.empty(); }, "a run without --camera-path"},
    kSeveralGpus = {[](const Options& o) { return o.gpus() > 1; }, "--gpus > 1"},
    kCheckpoint = {[](const Options& o) { return !o.checkpoint.empty(); }, "--checkpoint"},
    kResume = {[](const Options& o) { return !o.resume.empty(); }, "--resume"},
    kLiteralRng = {[](const Options& o) { return o.prm.rng_mode == MPT_RNG_LITERAL; }, "--rng literal"},
    kScatterAll = {[](const Options& o) { return o.prm.bsdf_mode == MPT_BSDF_SCATTER_ALL; }, "--bsdf scatter-all"},
    kAo = {[](const Options& o) { return o.haveAo || o.haveAoRadius; }, "--ao"},
    kDirect = {[](const Options& o) { return o.haveDirect || o.haveDirectWalk; }, "--direct"},
    kNee = {[](const Options& o) { return o.nee; }, "--nee"},
    kAdaptive = {[](const Options& o) { return o.adaptive; }, "--adaptive"},
    kDenoise = {[](const Options& o) { return o.denoise; }, "--denoise"},
    kDisplayFlags = {[](const Options& o) { return o.display; }, "the display flags"},
    kTemporal = {[](const Options& o) { return o.temporal; }, "--temporal"},
    kSvgf = {[](const Options& o) { return o.svgf; }, "--svgf"},
    kClampNoNumber = {[](const Options& o) { return o.neeClamp != o.neeClamp; }, "a --nee-clamp that is no number"},
    kOutNoPpm = {[](const Options& o) { return !o.outPpm(); }, "an --out that is no .ppm"},
    kNoTemporalSpp = {[](const Options& o) { return o.temporalSpp == 0; }, "--temporal-spp 0"};

// What one mode cannot be combined with: the first row that holds is the one the message names, so the order of the rows is behaviour.
struct Check {
    const char* flag;
    bool (*applies)(const Options&);
    std::vector<Condition> rows;

    int refuse(const Options& o) const {   // 0, or the exit status
        if (!applies(o)) return 0;
        for (const Condition& c : rows)
            if (c.holds(o)) {
                std::fprintf(stderr, "mpt_render: %s cannot be combined with %s\n", flag, c.words);
                return 2;
            }
        return 0;
    }
};
static const Check
    kNeeAdaptiveCheck = {"--nee-adaptive", [](const Options& o) { return o.neeAdaptive; },
                         {kNee, kAdaptive, kClampNoNumber, kSeveralGpus, kCameraPath, kFrames, kCheckpoint, kResume, kAo, kDirect, kLiteralRng, kScatterAll}},
    kNeeCheck = {"--nee", [](const Options& o) { return !o.neeAdaptive && (o.nee || o.haveNeeWalk || o.haveNeeClamp); },
                 {{[](const Options& o) { return !o.nee; }, "a run without --nee"}, kClampNoNumber, kAdaptive, kSeveralGpus, kCameraPath, kFrames, kAo, kDirect,
                  kLiteralRng, kScatterAll}},
    kDirectCheck = {"--direct", kDirect.holds,
                    {{[](const Options& o) { return o.direct < 1 || o.direct > static_cast<int>(MPT_DIRECT_MAX_SAMPLES); }, "a sample count outside 1..1024"},
                     {[](const Options& o) { return o.restirTemporal ? !o.out.empty() && !o.outPpm() : !o.outPpm(); }, kOutNoPpm.words}, kAo, kFrames,
                     {[](const Options& o) { return !o.restirTemporal && kCameraPath.holds(o); }, kCameraPath.words}, kSeveralGpus, kAdaptive, kDenoise, kDisplayFlags, kTemporal, kSvgf, kCheckpoint, kResume}},
    kAoCheck = {"--ao", kAo.holds,
                {{[](const Options& o) { return o.ao < 1 || o.ao > static_cast<int>(MPT_AO_MAX_SAMPLES); }, "a sample count outside 1..1024"},
                 kOutNoPpm, kFrames, kCameraPath, kSeveralGpus, kAdaptive, kDenoise, kDisplayFlags, kTemporal, kSvgf, kCheckpoint, kResume}},
    kAdaptiveCheck = {"--adaptive", kAdaptive.holds, {kFrames, kCameraPath, kSeveralGpus, kLiteralRng, kCheckpoint, kResume}},
    kTemporalCheck = {"--temporal", kTemporal.holds, {kNoCameraPath, kLiteralRng, kSeveralGpus, kAdaptive, kCheckpoint, kResume, kNoTemporalSpp}},
    // (--adaptive first: it needs a run without --camera-path, which --svgf cannot be)
    kSvgfCheck = {"--svgf", kSvgf.holds, {kAdaptive, kNoCameraPath, kTemporal, kDenoise, kLiteralRng, kSeveralGpus, kCheckpoint, kResume, kNoTemporalSpp}};

// --restir's refusals are whole sentences of their own
inline const char* restirRefusal(const Options& o) {
    if (!o.haveRestir && !o.haveRestirRadius && !(o.restirBiased && !o.restirTemporal)) return nullptr;   // (--restir-temporal takes --restir-biased too)
    return !o.haveRestir ? "--restir-radius and --restir-biased go with --restir K" : !o.haveDirect ? "--restir goes with --direct"
           : o.restirK < 0 || o.restirK > static_cast<int>(MPT_RESTIR_MAX_NEIGHBOURS) ? "--restir takes a count in 0..16"
           : o.haveRestirRadius && (o.restirRadius < 1 || o.restirRadius > static_cast<int>(MPT_RESTIR_MAX_RADIUS)) ? "--restir-radius takes a radius in 1..64"
           : o.lightSampling == MPT_LIGHT_SAMPLING_CONE ? "--restir cannot be combined with --light-sampling cone" : nullptr;
}

// ... and so are --restir-temporal's (before --direct's rows: with this flag the pass runs along a camera path)
inline const char* restirTemporalRefusal(const Options& o) {
    if (!o.restirTemporal) return o.haveRestirHistory ? "--restir-history goes with --restir-temporal" : nullptr;
    return o.cameraPath.empty() ? "--restir-temporal goes with --camera-path" : !o.haveDirect ? "--restir-temporal goes with --direct 1"
           : o.direct != 1 ? "--restir-temporal takes --direct 1: a frame is one round"
           : o.haveRestir || o.haveRestirRadius ? "--restir-temporal cannot be combined with --restir K"
           : o.lightSampling == MPT_LIGHT_SAMPLING_CONE ? "--restir-temporal cannot be combined with --light-sampling cone"
           : o.temporal ? "--restir-temporal cannot be combined with --temporal" : o.svgf ? "--restir-temporal cannot be combined with --svgf"
           : o.denoise ? "--restir-temporal cannot be combined with --denoise" : o.display ? "--restir-temporal cannot be combined with the display flags"
           : o.gpus() > 1 ? "--restir-temporal cannot be combined with --gpus > 1" : !o.checkpoint.empty() ? "--restir-temporal cannot be combined with --checkpoint"
           : !o.resume.empty() ? "--restir-temporal cannot be combined with --resume"
           : o.haveRestirHistory && (o.restirHistory < 1 || o.restirHistory > static_cast<int>(MPT_RESTIR_TEMPORAL_MAX_HISTORY))
               ? "--restir-history takes a count in 1..1024" : nullptr;
}

inline int refused(const char* sentence) {
    std::fprintf(stderr, "mpt_render: %s\n", sentence);
    return 2;
}

// The checks after parsing, in the order that decides which message a command line with several faults gets; 0, or the exit status.
inline int validate(const Options& o) {
    if (o.scene.empty()) {
        usage();
        return 2;
    }
    if (o.display && !o.out.empty() && !o.outPpm())
        return refused("the display flags (--tonemap, --transfer, --exposure, --white, --auto-exposure) need a .ppm --out");
    if (!o.display && (o.shown.key != 0.0f || o.shown.percentile != 0u || o.shown.adaptation != 0.0f))
        return refused("--key, --percentile and --adaptation go with --auto-exposure");
    if (const int status = kNeeAdaptiveCheck.refuse(o)) return status;   // (first: whatever it meets, the message names this flag)
    if (o.haveLightSampling && !o.nee && !o.haveDirect && !o.neeAdaptive) return refused("--light-sampling goes with --direct, --nee or --nee-adaptive");
    if (o.haveLightCandidates && (o.neeAdaptive ? o.lightCandidates > 1 : !o.nee && !o.haveDirect))
        return refused(o.neeAdaptive ? "--light-candidates above 1 cannot be combined with --nee-adaptive" : "--light-candidates goes with --direct or --nee");
    if (const char* why = restirTemporalRefusal(o)) return refused(why);
    if (const char* why = restirRefusal(o)) return refused(why);
    for (const Check* c : {&kNeeCheck, &kDirectCheck, &kAoCheck, &kAdaptiveCheck, &kTemporalCheck, &kSvgfCheck})
        if (const int status = c->refuse(o)) return status;
    if (o.svgf && o.haveSvgfIterations && (o.svgfIterations < 0 || o.svgfIterations > MPT_DENOISE_MAX_ITERATIONS)) {
        std::fprintf(stderr, "mpt_render: --svgf-iterations must be between 0 and %d\n", MPT_DENOISE_MAX_ITERATIONS);
        return 2;
    }
    return 0;
}
