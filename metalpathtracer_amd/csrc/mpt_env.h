// mpt_env.h — the one parser of the comma-list knobs (MPT_BUDGETS, MPT_MIN_ACTIVE, MPT_OT_BUDGETS, MPT_OT_MIN_ACTIVE).  Pure host C++, no
// HIP: mpt_hip.hip's create_impl calls it and applies each knob's own rule for the entries a list leaves out;
// tests/scene_layout/scene_layout_check.cpp checks both on the CPU.
#pragma once
#include <stdint.h>
#include <stdio.h>

// "a,b,c": reads up to `max` unsigned numbers (sscanf's %u), each followed by an optional comma, and stops at the first thing that is not
// one.  Returns how many it read.
static inline unsigned parse_uint_list(const char* s, unsigned* out, unsigned max) {
    unsigned n = 0;
    while (n < max) {
        unsigned v = 0;
        int used = 0;
        if (sscanf(s, "%u%n", &v, &used) != 1) break;
        out[n++] = v;
        s += used;
        if (*s == ',') ++s;
    }
    return n;
}

// MPT_BUDGETS, e.g. "8,20,50,125": box-test trips per step of ring 0 .. n-1.  An entry the list leaves out is twice the one before it
// (4 before the first); none is below 1.
static inline void fill_budgets(const char* s, uint32_t* b, unsigned n) {
    const unsigned given = parse_uint_list(s, b, n);
    unsigned prev = 4;
    for (unsigned k = 0; k < n; ++k) {
        const unsigned v = k < given ? b[k] : prev * 2;
        prev = b[k] = v < 1 ? 1 : v;
    }
}
// MPT_MIN_ACTIVE, "a,b,c": lanes that must still be traversing for a step of ring k to go on.  An entry the list leaves out repeats the
// last one given (0 when there is none); none is above 64.
static inline void fill_min_active(const char* s, uint32_t* m, unsigned n) {
    const unsigned given = parse_uint_list(s, m, n);
    unsigned v = 0;
    for (unsigned k = 0; k < n; ++k) {
        if (k < given) v = m[k];
        m[k] = v > 64 ? 64 : v;
    }
}
