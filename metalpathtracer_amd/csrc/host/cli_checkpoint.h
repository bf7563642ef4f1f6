// cli_checkpoint.h — the file mpt_render --checkpoint writes and --resume reads: one header line, then W * H * 4 raw floats (the HDR sum).
// (The reference's running mean lives in a GPU-private texture and is lost with the process, R/Renderer/Renderer.cpp:236.)
//
// The header says WHAT was accumulated, so that a resume on another scene, material model or estimator is refused instead of mixing sums.
// Its four kinds are one prefix chain — the magic, the eight common fields, then zero to three extras:
//     MPTSUM2 W H samples seed rng depth bsdf scene-hash                                  a plain render
//     MPTNEE1 ... scene-hash clamp-bits                                                   an --nee render, sphere lights sampled by area
//     MPTNEE2 ... scene-hash clamp-bits sampling                                          ... sampled by cone
//     MPTNEE3 ... scene-hash clamp-bits sampling candidates                               ... with more than one light candidate
// No kind parses as another, so neither estimator continues the other's sum.  A new kind is one more Kind, magic and wording below and,
// if it carries a new field, one more line in fields().  Standard library only: a CPU program can include this header.
#pragma once
#include <cstdint>
#include <cstdio>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

struct CheckpointHeader {
    enum Kind { PLAIN = 0, NEE = 1, NEE_CONE = 2, NEE_RIS = 3 };   // (the value is the number of extra fields)
    Kind kind = PLAIN;
    int width = 0, height = 0;
    uint32_t samples = 0;            // per pixel, in the sum that follows
    unsigned seed = 0;
    int rng = 0, depth = 0, bsdf = 0;
    unsigned long long sceneHash = 0;
    unsigned clampBits = 0;          // NEE...: the bits of the --nee-clamp in force (0: none)
    int sampling = 0;                // NEE_CONE, NEE_RIS: MPT_LIGHT_SAMPLING_*
    int candidates = 0;              // NEE_RIS

    static const char* magic(Kind k) {
        static const char* const names[] = {"MPTSUM2", "MPTNEE1", "MPTNEE2", "MPTNEE3"};
        return names[k];
    }
    static const char* wording(Kind k) {
        static const char* const names[] = {"a plain render", "an --nee render with area light sampling", "an --nee render with cone light sampling",
                                            "an --nee render with these light candidates and this light sampling"};
        return names[k];
    }

    // The fields in file order, each with the one conversion that both fprintf and fscanf take for it; `each` returns whether to go on.
    template <class Each>
    bool fields(Each&& each) {
        bool ok = each(" %d", &width) && each(" %d", &height) && each(" %u", &samples) && each(" %u", &seed) && each(" %d", &rng) &&
                  each(" %d", &depth) && each(" %d", &bsdf) && each(" %llx", &sceneHash);
        if (ok && kind >= NEE) ok = each(" %x", &clampBits);
        if (ok && kind >= NEE_CONE) ok = each(" %d", &sampling);
        if (ok && kind >= NEE_RIS) ok = each(" %d", &candidates);
        return ok;
    }
    bool write(FILE* f) const {
        CheckpointHeader h = *this;
        return std::fputs(magic(kind), f) >= 0 && h.fields([f](const char* conversion, auto* field) { return std::fprintf(f, conversion, *field) > 0; }) &&
               std::fputc('\n', f) == '\n';
    }
    // the header of kind `k` that `f` starts with: nothing if it starts with another kind's, or the line does not end where this kind's does
    static std::optional<CheckpointHeader> read(FILE* f, Kind k) {
        CheckpointHeader h;
        h.kind = k;
        char tag[8] = "";
        if (!f || std::fscanf(f, "%7[A-Z0-9]", tag) != 1 || std::string(tag) != magic(k)) return std::nullopt;
        if (!h.fields([f](const char* conversion, auto* field) { return std::fscanf(f, conversion, field) == 1; })) return std::nullopt;
        if (std::fgetc(f) != '\n') return std::nullopt;
        return h;
    }
    // why the sum under `got` (what read() gave for want.kind) cannot be continued by the run `want` describes; empty if it can.
    // `samples` is what the file is read for and is not compared.
    static std::string mismatch(const std::optional<CheckpointHeader>& got, const CheckpointHeader& want, const std::string& path) {
        if (!got || (want.kind >= NEE_CONE && got->sampling != want.sampling) || (want.kind >= NEE_RIS && got->candidates != want.candidates))
            return "cannot read the checkpoint " + path + " as one of " + wording(want.kind);
        if (want.kind >= NEE && got->clampBits != want.clampBits) return "the checkpoint " + path + " was written with another --nee-clamp";
        if (got->width != want.width || got->height != want.height || got->seed != want.seed || got->rng != want.rng || got->depth != want.depth ||
            got->bsdf != want.bsdf || got->sceneHash != want.sceneHash)
            return "the checkpoint " + path + " was written with another scene, size, seed, RNG, BSDF mode or depth";
        return std::string();
    }
};

// --resume: the sum of the checkpoint `path` into `sum`, if the run `want` describes continues it; returns the samples it holds.
inline uint32_t readCheckpoint(const std::string& path, const CheckpointHeader& want, std::vector<float>& sum) {
    FILE* f = std::fopen(path.c_str(), "rb");
    const std::optional<CheckpointHeader> got = CheckpointHeader::read(f, want.kind);
    const std::string why = CheckpointHeader::mismatch(got, want, path);
    if (!why.empty()) {
        if (f) std::fclose(f);
        throw std::runtime_error(why);
    }
    sum.resize(static_cast<size_t>(got->width) * got->height * 4);
    const size_t have = std::fread(sum.data(), sizeof(float), sum.size(), f);
    std::fclose(f);
    if (have != sum.size()) throw std::runtime_error("the checkpoint " + path + " is truncated");
    return got->samples;
}

// --checkpoint: written to a temporary file and renamed over the target, so that a crash or a full disk mid-write never destroys the
// checkpoint that --resume just read.
inline void writeCheckpoint(const std::string& path, const CheckpointHeader& header, const std::vector<float>& sum) {
    const std::string tmp = path + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + tmp);
    const bool ok = header.write(f) && std::fwrite(sum.data(), sizeof(float), sum.size(), f) == sum.size();
    if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path.c_str()) != 0) {
        std::remove(tmp.c_str());
        throw std::runtime_error("cannot write " + path);
    }
}
