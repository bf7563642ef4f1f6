// checkpoint_check.cpp — mpt_render's checkpoint file (metalpathtracer_amd/csrc/host/cli_checkpoint.h) on the CPU: stand-alone, built by
// tests/test_cli_cpu.py with AddressSanitizer and UndefinedBehaviorSanitizer.  The expected bytes and messages are string literals typed
// from the formats and texts of the main.cpp that wrote each kind out as an fprintf and an fscanf of its own:
//     "MPTSUM2 %d %d %u %u %d %d %d %llx\n"            width height samples seed rng depth bsdf scene-hash
//     "MPTNEE1 ... %llx %x\n"                          ... clamp-bits
//     "MPTNEE2 ... %llx %x %d\n"                       ... clamp-bits sampling
//     "MPTNEE3 ... %llx %x %d %d\n"                    ... clamp-bits sampling candidates
// Usage: checkpoint_check DIR (an empty directory it may write in; it leaves DIR/kept.ck).
#include <sys/resource.h>

#include <csignal>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_checkpoint.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

using Kind = CheckpointHeader::Kind;
static const Kind kKinds[4] = {CheckpointHeader::PLAIN, CheckpointHeader::NEE, CheckpointHeader::NEE_CONE, CheckpointHeader::NEE_RIS};
static const char* const kBytes[4] = {"MPTSUM2 48 32 12 7 1 4 2 cbf29ce484222325\n", "MPTNEE1 48 32 12 7 1 4 2 cbf29ce484222325 40800000\n",
                                      "MPTNEE2 48 32 12 7 1 4 2 cbf29ce484222325 40800000 1\n", "MPTNEE3 48 32 12 7 1 4 2 cbf29ce484222325 40800000 1 5\n"};
static const char* const kAsOneOf[4] = {" as one of a plain render", " as one of an --nee render with area light sampling",
                                        " as one of an --nee render with cone light sampling",
                                        " as one of an --nee render with these light candidates and this light sampling"};

static CheckpointHeader header(Kind kind) {
    CheckpointHeader h;
    h.kind = kind;
    h.width = 48;
    h.height = 32;
    h.samples = 12;
    h.seed = 7;
    h.rng = 1;
    h.depth = 4;
    h.bsdf = 2;
    h.sceneHash = 0xcbf29ce484222325ull;
    h.clampBits = 0x40800000u;   // 4.0f
    h.sampling = 1;
    h.candidates = 5;
    return h;
}
static std::string slurp(const std::string& path) {
    std::string s;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        char buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
        std::fclose(f);
    }
    return s;
}
static void spill(const std::string& path, const std::string& bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    std::fwrite(bytes.data(), 1, bytes.size(), f);
    std::fclose(f);
}
static bool exists(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (f) std::fclose(f);
    return f != nullptr;
}
// what a --resume of `path` by the run `want` describes says: "" and the samples if it goes through, else the message
static std::string resume(const std::string& path, const CheckpointHeader& want, uint32_t* samples = nullptr, std::vector<float>* sum = nullptr) {
    std::vector<float> mine;
    try {
        const uint32_t n = readCheckpoint(path, want, sum ? *sum : mine);
        if (samples) *samples = n;
        return "";
    } catch (const std::exception& e) {
        return e.what();
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1], file = dir + "/c.ck";
    const std::vector<float> payload(48 * 32 * 4, 0.25f);
    const std::string payloadBytes(reinterpret_cast<const char*>(payload.data()), payload.size() * sizeof(float));

    for (int k = 0; k < 4; ++k) {
        // written: the header's bytes, then the raw floats, and no temporary file left
        writeCheckpoint(file, header(kKinds[k]), payload);
        CHECK(slurp(file) == kBytes[k] + payloadBytes);
        CHECK(!exists(file + ".tmp"));
        // read back by the run that wrote it: every field, the samples and the sum
        FILE* f = std::fopen(file.c_str(), "rb");
        const std::optional<CheckpointHeader> got = CheckpointHeader::read(f, kKinds[k]);
        std::fclose(f);
        const CheckpointHeader want = header(kKinds[k]);
        CHECK(got && got->kind == want.kind && got->width == 48 && got->height == 32 && got->samples == 12 && got->seed == 7 && got->rng == 1 && got->depth == 4 &&
              got->bsdf == 2 && got->sceneHash == want.sceneHash);
        CHECK(got && got->clampBits == (k >= 1 ? 0x40800000u : 0u) && got->sampling == (k >= 2 ? 1 : 0) && got->candidates == (k >= 3 ? 5 : 0));
        uint32_t samples = 0;
        std::vector<float> sum;
        CheckpointHeader run = want;
        run.samples = 0;   // (what the run asks for is not compared)
        CHECK(resume(file, run, &samples, &sum) == "" && samples == 12 && sum == payload);
        // the twelve wrong-kind reads: no kind continues another's sum
        for (int j = 0; j < 4; ++j)
            if (j != k) CHECK(resume(file, header(kKinds[j])) == "cannot read the checkpoint " + file + kAsOneOf[j]);
        // another sampling or another count of candidates is another kind of sum, another clamp another sum
        if (k >= 2) {
            run = want;
            run.sampling = 0;
            CHECK(resume(file, run) == "cannot read the checkpoint " + file + kAsOneOf[k]);
        }
        if (k >= 3) {
            run = want;
            run.candidates = 4;
            CHECK(resume(file, run) == "cannot read the checkpoint " + file + kAsOneOf[k]);
        }
        run = want;
        run.clampBits = 0;
        CHECK(resume(file, run) == (k >= 1 ? "the checkpoint " + file + " was written with another --nee-clamp" : ""));
        // each of the seven common fields off by one (a wrong clamp is reported before them)
        for (int field = 0; field < 7; ++field) {
            run = want;
            switch (field) {
            case 0: ++run.width; break;
            case 1: ++run.height; break;
            case 2: ++run.seed; break;
            case 3: ++run.rng; break;
            case 4: ++run.depth; break;
            case 5: ++run.bsdf; break;
            default: ++run.sceneHash; break;
            }
            CHECK(resume(file, run) == "the checkpoint " + file + " was written with another scene, size, seed, RNG, BSDF mode or depth");
            run.clampBits += 1;
            if (k >= 1) CHECK(resume(file, run) == "the checkpoint " + file + " was written with another --nee-clamp");
        }
        // a header that does not end where this kind's does: no newline, a field too many, a field too few, a field that is no number
        const std::string line(kBytes[k], std::strlen(kBytes[k]) - 1);
        for (const std::string& bad : {line, line + " 1\n", line.substr(0, line.rfind(' ')) + "\n", line.substr(0, line.rfind(' ')) + " zz\n", std::string()}) {
            spill(file, bad + payloadBytes);
            CHECK(resume(file, want) == "cannot read the checkpoint " + file + kAsOneOf[k]);
        }
        // a payload that ends early
        spill(file, kBytes[k] + payloadBytes.substr(0, payloadBytes.size() - 1));
        CHECK(resume(file, want) == "the checkpoint " + file + " is truncated");
        std::remove(file.c_str());
        CHECK(resume(file, want) == "cannot read the checkpoint " + file + kAsOneOf[k]);   // (no such file)
    }

    // a write that fails (here: the file system takes no more than 64 bytes) leaves the old checkpoint and no temporary file
    const std::string kept = dir + "/kept.ck", old = std::string(kBytes[1]) + payloadBytes;
    spill(kept, old);
    rlimit before, small;
    getrlimit(RLIMIT_FSIZE, &before);
    small = before;
    small.rlim_cur = 64;
    std::signal(SIGXFSZ, SIG_IGN);
    setrlimit(RLIMIT_FSIZE, &small);
    std::string said;
    try {
        writeCheckpoint(kept, header(CheckpointHeader::PLAIN), payload);
    } catch (const std::exception& e) {
        said = e.what();
    }
    setrlimit(RLIMIT_FSIZE, &before);
    CHECK(said == "cannot write " + kept);
    CHECK(slurp(kept) == old && !exists(kept + ".tmp"));
    // ... and one that cannot begin says which file it could not open
    said.clear();
    try {
        writeCheckpoint(dir + "/none/c.ck", header(CheckpointHeader::PLAIN), payload);
    } catch (const std::exception& e) {
        said = e.what();
    }
    CHECK(said == "cannot write " + dir + "/none/c.ck.tmp");

    if (failures == 0) std::printf("all passed\n");
    return failures ? 1 : 0;
}
