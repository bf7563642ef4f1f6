// Stand-alone check of the (W, H) cache behind the lean kernels' constant division (metalpathtracer_amd/csrc/mpt_lean_cdiv.h) with the
// device check stubbed: the same pair twice makes one check, a changed pair a new one, a failed check (mismatches, or a check that
// could not run) turns the lean dispatch off for that pair and only for it.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer and run by tests/test_lean_cdiv_cache.py.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "mpt_lean_cdiv.h"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

struct Stub {   // the device check: counts its calls, remembers its operands, answers as told
    int calls = 0;
    float W = 0, H = 0;
    uint32_t mismatches = 0;
    bool runs = true;
    bool operator()(float w, float h, uint32_t* bad) {
        ++calls;
        W = w;
        H = h;
        *bad = mismatches;
        return runs;
    }
};

int main() {
    {   // same pair twice: one check; the operands reach the check as they are
        LeanCdivCache c;
        Stub s;
        CHECK(lean_cdiv_ok(c, 1920.0f, 1080.0f, s));
        CHECK(lean_cdiv_ok(c, 1920.0f, 1080.0f, s));
        CHECK(s.calls == 1 && c.checks == 1 && s.W == 1920.0f && s.H == 1080.0f);
        // a changed pair (either member): a new check each, and back again one more — the cache holds one pair
        CHECK(lean_cdiv_ok(c, 1920.0f, 1081.0f, s) && s.calls == 2);
        CHECK(lean_cdiv_ok(c, 1921.0f, 1081.0f, s) && s.calls == 3);
        CHECK(lean_cdiv_ok(c, 1921.0f, 1081.0f, s) && s.calls == 3);
        CHECK(lean_cdiv_ok(c, 1920.0f, 1080.0f, s) && s.calls == 4 && c.checks == 4);
        // W and H swapped is another pair
        CHECK(lean_cdiv_ok(c, 1080.0f, 1920.0f, s) && s.calls == 5);
    }
    {   // a failed check turns the lean dispatch off, is remembered, and does not outlive its pair
        LeanCdivCache c;
        Stub s;
        s.mismatches = 3;
        CHECK(!lean_cdiv_ok(c, 70.0f, 45.0f, s));
        CHECK(!lean_cdiv_ok(c, 70.0f, 45.0f, s));
        CHECK(s.calls == 1);
        s.mismatches = 0;
        CHECK(!lean_cdiv_ok(c, 70.0f, 45.0f, s) && s.calls == 1);   // (still the remembered answer)
        CHECK(lean_cdiv_ok(c, 71.0f, 45.0f, s) && s.calls == 2);
        CHECK(lean_cdiv_ok(c, 70.0f, 45.0f, s) && s.calls == 3);    // the pair is measured again when the context comes back to it
    }
    {   // a check that could not run counts as failed, whatever it left in the counter
        LeanCdivCache c;
        Stub s;
        s.runs = false;
        CHECK(!lean_cdiv_ok(c, 9.0f, 1023.0f, s) && s.calls == 1);
        CHECK(!lean_cdiv_ok(c, 9.0f, 1023.0f, s) && s.calls == 1);
        s.runs = true;
        CHECK(lean_cdiv_ok(c, 1023.0f, 9.0f, s) && s.calls == 2);
    }
    {   // a NaN size never matches the cache and is never handed to the device: generic kernels, no check
        LeanCdivCache c;
        Stub s;
        CHECK(!lean_cdiv_ok(c, NAN, 45.0f, s));
        CHECK(!lean_cdiv_ok(c, 70.0f, NAN, s));
        CHECK(s.calls == 0 && c.checks == 0);
        CHECK(lean_cdiv_ok(c, 70.0f, 45.0f, s) && s.calls == 1);
    }
    if (failures == 0) std::printf("all passed\n");
    return failures == 0 ? 0 : 1;
}
