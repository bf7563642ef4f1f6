// mpt_build_scratch.h — what the device builders (mpt_radix.h, mpt_sah.h, mpt_lbvh.h, mpt_devbuild.h) share on the HOST side: the scratch
// allocator and its pool, the pinned read-back block with the ONE definition of its layout, the wait for a stamped slot of that block, and
// the environment switches of a build — and the one hipcub idiom all of them use, the scan over scratch memory.  No kernel of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>

namespace mpt_build {
#define MPT_LB(call)                       \
    do {                                   \
        hipError_t e_ = (call);            \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

// ---- the pinned read-back block ---------------------------------------------------------------------------------------------------
// The pool holds ONE block of pinned host memory (hipHostMalloc per build: ~0.1 ms each; a pageable target costs ~0.3 ms per copy), of two
// parts of PIN_PART_WORDS 32-bit words: a scene build and the binary-tree build under it run at the same time and each reads back through
// its own.  Every region of a part is named here, and no reader or writer indexes the block by a bare number.
enum : uint32_t {
    PIN_PART_WORDS = 256u,        // 1 KiB per part
    PIN_PART_SCENE = 0u,          // mpt_devbuild.h build_pass (and the second SAH it may run over the leaves)
    PIN_PART_TREE = 1u,           // mpt_lbvh.h build_radix (and the SAH over the primitives)
    PIN_PARTS = 2u,
    // words of a part
    PIN_W_SMALL = 0u,             // a read-back of a few words, consumed before the next is made: a count (finish_radix, the leaves), the
    PIN_N_SMALL = 64u,            //   triangle and sphere counts of the top-down builder, the PLOC loop's state
    PIN_W_SAH_SLOTS = 64u,        // mpt_sah.h run_sah: PIN_SLOTS level slots of 3 eight-byte words
    PIN_SLOTS = 8u,
    PIN_SAH_SLOT_WORDS64 = 3u,
    PIN_W_COLLAPSE_SLOTS = 160u,  // mpt_devbuild.h collapse: PIN_SLOTS level slots of 1 eight-byte word
    PIN_W_SCALARS = 192u,         // mpt_devbuild.h: the copy of its Scalars, read once at the end ...
    PIN_N_SCALARS = 63u,
    PIN_W_LEAF_COUNT = 255u,      // ... with the number of reference leaves
};
static_assert(PIN_W_SMALL + PIN_N_SMALL <= PIN_W_SAH_SLOTS, "pinned map: the small read-backs run into run_sah's slots");
static_assert(PIN_W_SAH_SLOTS + 2u * PIN_SAH_SLOT_WORDS64 * PIN_SLOTS <= PIN_W_COLLAPSE_SLOTS, "pinned map: run_sah's slots run into the collapse's");
static_assert(PIN_W_COLLAPSE_SLOTS + 2u * PIN_SLOTS <= PIN_W_SCALARS, "pinned map: the collapse's slots run into the scalars");
static_assert(PIN_W_SCALARS + PIN_N_SCALARS <= PIN_W_LEAF_COUNT && PIN_W_LEAF_COUNT < PIN_PART_WORDS, "pinned map: the scalars do not fit the part");
static_assert(PIN_W_SAH_SLOTS % 2u == 0u && PIN_W_COLLAPSE_SLOTS % 2u == 0u, "pinned map: the slots are eight-byte words");
static_assert(PIN_PART_WORDS * 4u <= 1024u, "pinned map: a part is 1 KiB");

// Scratch memory of a build: a bump allocator over a few large chunks (a build makes ~90 arrays; one hipMalloc each cost a
// third of the 1 M-primitive build), handed back to the pool they came from on every exit path.  A ScratchPool
// (one per context) keeps the chunks between builds: a rebuild allocates nothing.
struct ScratchPool {
    std::vector<std::pair<void*, size_t>> chunks;
    size_t keep_bytes = (size_t)2 << 30;   // what stays allocated between builds at most
    uint32_t* pin = nullptr;               // the pinned read-back block (above)
    hipStream_t side = nullptr;            // a second stream for the chains of a build that need nothing of one another (mpt_devbuild.h) ...
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // ... and the events that fork and join it
    ScratchPool() = default;
    ScratchPool(const ScratchPool&) = delete;
    ~ScratchPool() {
        for (auto& c : chunks) hipFree(c.first);
        if (pin) hipHostFree(pin);
        if (side) hipStreamDestroy(side);
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
    }
    hipError_t side_stream(hipStream_t* out) {
        if (!side) {
            hipError_t e = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
            if (e != hipSuccess) return e;
            for (auto& v : ev)
                if ((e = hipEventCreateWithFlags(&v, hipEventDisableTiming)) != hipSuccess) return e;
        }
        *out = side;
        return hipSuccess;
    }
    hipError_t pinned(uint32_t part, uint32_t** out) {   // one builder's part (PIN_PART_*) of the pinned block
        if (!pin) MPT_LB(hipHostMalloc((void**)&pin, (size_t)PIN_PARTS * PIN_PART_WORDS * 4, hipHostMallocDefault));
        *out = pin + PIN_PART_WORDS * part;
        return hipSuccess;
    }
};
struct Scratch {
    ScratchPool& pool;
    std::vector<std::pair<void*, size_t>> mine;
    size_t off = 0;   // in the last chunk of mine
    explicit Scratch(ScratchPool& p) : pool(p) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        size_t kept = 0;
        for (auto& c : pool.chunks) kept += c.second;
        for (auto& c : mine) {
            if (kept + c.second <= pool.keep_bytes) {
                pool.chunks.push_back(c);
                kept += c.second;
            } else {
                hipFree(c.first);
            }
        }
    }
    // a chunk of at least `bytes` becomes the current one: the pool's smallest that fits, else a new allocation
    hipError_t chunk(size_t bytes) {
        int best = -1;
        for (int i = 0; i < (int)pool.chunks.size(); ++i)
            if (pool.chunks[i].second >= bytes && (best < 0 || pool.chunks[i].second < pool.chunks[best].second)) best = i;
        if (best >= 0) {
            mine.push_back(pool.chunks[best]);
            pool.chunks.erase(pool.chunks.begin() + best);
            off = 0;
            return hipSuccess;
        }
        void* q = nullptr;
        MPT_LB(hipMalloc(&q, bytes));
        mine.emplace_back(q, bytes);
        off = 0;
        return hipSuccess;
    }
    // (call once with an estimate of everything the build will ask for: one chunk instead of several)
    hipError_t reserve(size_t bytes) { return chunk(std::max<size_t>(bytes, (size_t)1 << 20)); }
    template <class T>
    hipError_t alloc(T** p, size_t count) {
        const size_t bytes = (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
        if (mine.empty() || off + bytes > mine.back().second) {
            *p = nullptr;
            MPT_LB(chunk(std::max<size_t>(bytes, (size_t)64 << 20)));
        }
        *p = (T*)((char*)mine.back().first + off);
        off += bytes;
        return hipSuccess;
    }
    template <class T, class... Ts>
    hipError_t allocs(size_t count, T** p, Ts**... more) {   // several arrays of `count` elements each, in this order
        MPT_LB(alloc(p, count));
        if constexpr (sizeof...(more) > 0) return allocs(count, more...);
        return hipSuccess;
    }
};

// ---- scans -------------------------------------------------------------------------------------------------------------------------
// An exclusive prefix sum of 32-bit words with hipcub, its temporary storage taken from the build's scratch.  Two phases — reserve() for the
// largest count, on the thread that owns the scratch; run() any number of times on counts up to that — for the loops and the chains that
// must not allocate on their way; once() is both, where nothing stands between them.
// (Here and plain, not a template and not in mpt_radix.h: the order in which a translation unit first names hipcub's kernels, and the order of
//  the headers that hold kernels, decide where kernels lie in the code object — profiles/r26_build_refactor.txt.  The build's one INCLUSIVE
//  sum, in mpt_devbuild.h's material chain, is a direct hipcub call for the same reason.)
struct Scan {
    char* tmp = nullptr;
    size_t bytes = 0;
    hipError_t reserve(Scratch& sc, size_t max_count, hipStream_t stream) {
        MPT_LB(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)max_count, stream));
        return sc.alloc(&tmp, bytes);
    }
    hipError_t run(uint32_t* in, uint32_t* out, size_t count, hipStream_t stream) const {
        size_t b = bytes;
        return hipcub::DeviceScan::ExclusiveSum(tmp, b, in, out, (int)count, stream);
    }
    static hipError_t once(Scratch& sc, uint32_t* in, uint32_t* out, size_t count, hipStream_t stream) {
        Scan s;
        MPT_LB(s.reserve(sc, count, stream));
        return s.run(in, out, count, stream);
    }
};

// ---- stamped slots ------------------------------------------------------------------------------------------------------------------
// A level loop that does not wait for the device (mpt_sah.h run_sah, mpt_devbuild.h collapse) has each level's first kernel leave its counts
// in a slot of the pinned block: PIN_SLOTS slots of `w` eight-byte words, each word (stamp << 32 | count) and ONE store, so that nothing has
// to order the words.  The host reads a slot a level or two late, to size the next grids and to end the loop.
struct StampedSlots {
    volatile unsigned long long* host = nullptr;
    unsigned long long* dev = nullptr;   // the same words as the kernels address them
    uint32_t w = 1;
    // `word`: PIN_W_SAH_SLOTS or PIN_W_COLLAPSE_SLOTS of the part `pin`; clears every slot
    hipError_t open(uint32_t* pin, uint32_t word, uint32_t words_per_slot) {
        w = words_per_slot;
        host = (volatile unsigned long long*)(pin + word);
        MPT_LB(hipHostGetDevicePointer((void**)&dev, pin + word, 0));
        for (uint32_t q = 0; q < PIN_SLOTS * w; ++q) host[q] = 0ull;
        return hipSuccess;
    }
    unsigned long long* dev_slot(uint32_t k) const { return dev + w * (k % PIN_SLOTS); }
    // all w words of slot k carry `stamp` (bits of `ignore` aside: a flag the kernel may set in its stamp)
    bool ready(uint32_t k, uint32_t stamp, uint32_t ignore = 0u) const {
        const volatile unsigned long long* sl = host + w * (k % PIN_SLOTS);
        for (uint32_t q = 0; q < w; ++q)
            if (((uint32_t)(sl[q] >> 32) & ~ignore) != stamp) return false;
        return true;
    }
    // Waits for that and copies the words to out[w].  The caller only waits for a level the device is at or past, with the next one queued:
    // the wait is short.  Every 4096 spins the stream is asked: an error ends the wait; so does a drained stream without the stamp
    // (hipErrorUnknown), and 20 s (hipErrorLaunchTimeOut — a level takes < 1 ms: a kernel hangs).
    hipError_t wait(hipStream_t stream, uint32_t k, uint32_t stamp, uint32_t ignore, unsigned long long* out) const {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned long long spin = 0; !ready(k, stamp, ignore); ++spin) {
            if ((spin & 0xFFFu) == 0xFFFu) {
                const hipError_t q = hipStreamQuery(stream);
                if (q != hipSuccess && q != hipErrorNotReady) return q;
                if (q == hipSuccess && !ready(k, stamp, ignore)) return hipErrorUnknown;   // the stream is drained and the stamp never came
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return hipErrorLaunchTimeOut;
            }
        }
        const volatile unsigned long long* sl = host + w * (k % PIN_SLOTS);
        for (uint32_t q = 0; q < w; ++q) out[q] = sl[q];
        return hipSuccess;
    }
};

// ---- the environment switches of a build --------------------------------------------------------------------------------------------
// Read once per build CALL (the tests flip them between builds) and passed down: no step reads the environment.
struct Switches {
    const bool one_stream = getenv("MPT_BUILD_ONE_STREAM") != nullptr;   // everything on the caller's stream
    const bool no_helper = getenv("MPT_BUILD_NO_HELPER") != nullptr;     // the material copy is enqueued by the calling thread
    const char* const key_bits = getenv("MPT_DEBUG_MAT_KEY_BITS");       // = 1..32: only that many (top) bits of the material sort key are kept, to force collisions
    const uint32_t mat_key_shift = key_bits ? 32u - (uint32_t)std::min(std::max(atoi(key_bits), 1), 32) : 0u;
    enum OwnTree { OWN_AUTO, OWN_REFIT, OWN_SAH };                        // the own binary tree: by refit of the builder's tree / by a second SAH
    const char* const own = getenv("MPT_OWN_TREE");                      // = refit | anything else
    const OwnTree own_tree = !own ? OWN_AUTO : strcmp(own, "refit") == 0 ? OWN_REFIT : OWN_SAH;
    const bool own_tree_walk = getenv("MPT_OWN_TREE_WALK") != nullptr;   // the refit walks up from every leaf even where a copy would do
    const bool keep_spheres = getenv("MPT_SAH_KEEP_SPHERES") != nullptr; // the top-down builder does not hang the spheres under the root
};

}  // namespace mpt_build
