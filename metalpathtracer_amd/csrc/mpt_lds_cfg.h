// mpt_lds_cfg.h — the configuration block of the persistent trace kernels (k_wavelocal*, k_ordered), slot by slot: the ONE definition.
//
// The block lies in every workgroup's LDS behind the material table, at float4 index mpt_lds_cfg_off_f4() (mpt_kernels.h), and is
// MPT_LDS_CFG_F4 float4 long.  Thread 0 of a workgroup writes it before the step loop; the loop reads from it what only some steps need,
// so that those values hold no scalar register across the loop.  Round 4 had two definitions of the block's START and faulted (the
// comment at mpt_lds_cfg_off_f4); every slot INSIDE it is named here, and no reader or writer indexes the block by a bare number.
//
//   float4 0..3    the camera as gen_primary reads it: (cam, W) (first, H) (vu, cdiv_recip(W)) (vv, cdiv_recip(H)); the two reciprocals
//                  are the lean kernels', 0 elsewhere
//   float4 4..9    CFG_N_WORDS 32-bit words, CFG_W_*
//   float4 10..11  lean kernels: where fresh queries enter the tree (mpt_lean_entry.h) — (ilo, entry) (ihi, entry_primary)
//   float4 12..15  lean ALL_LDS kernels: the tail leaf T (mpt_lean_entry.h) — (tlo, T's leaf word) (thi, tail_primary) and T's own two
//                  plane records, with T (0: the item is off) in the place of its miss link, which no box test reads
#pragma once
#include <stdint.h>

enum : uint32_t {
    // float4 slots, from the start of the block
    CFG_F4_CAM = 0u,
    CFG_F4_FIRST = 1u,
    CFG_F4_VU = 2u,
    CFG_F4_VV = 3u,
    CFG_F4_WORDS = 4u,
    CFG_F4_ENTRY_LO = 10u,
    CFG_F4_ENTRY_HI = 11u,
    CFG_F4_TAIL = 12u,              // four float4, CFG_TAIL_* from here (what closest_hit_resume gets as `tail_cfg`)
    CFG_F4_END = 16u,
    // words, from float4 CFG_F4_WORDS
    CFG_MAX_LEVELS = 8u,            // rings with a budget: MPT_WL_LEVELS of k_wavelocal, MPT_OT_MLEVELS of k_ordered
    CFG_W_BUDGET = 0u,              // + level: trips of the walk's loop a step of that ring may make
    CFG_W_MIN_ACTIVE = 8u,          // + level: ... and it ends once fewer lanes than this are still walking
    CFG_W_INPLACE_MIN = 15u,        // k_ordered: lanes that must need the tree for a step to walk it in place
    CFG_W_SKY_RESOLVE = 15u,        // lean ALL_LDS kernels of k_wavelocal (the same word: they have no such threshold and fewer than 8 rings): != 0 when
                                    // the pass's resolve sums the sky tiles' samples itself, so that a primary step elides them (mpt_kernels.h)
    CFG_W_CLAIM_BLOCK = 16u,        // a claim of path ids: its upper bound,
    CFG_W_CLAIM_MIN = 17u,          // ... its lower bound,
    CFG_W_CLAIM_DIV = 18u,          // ... the claim divisor x the waves per claim range,
    CFG_W_RANK_TILES = 19u,         // ... and this rank's tiles
    CFG_W_S_MUL = 20u,              // lean kernels: the division by a sample count that is no power of two (WlLean::s_mul, s_shift)
    CFG_W_S_SHIFT = 21u,
    CFG_W_CLASSES_LO = 22u,         // lean ALL_LDS kernels: the class table's address (mpt_lean_tiles.h; null: every tile is general)
    CFG_W_CLASSES_HI = 23u,
    CFG_N_WORDS = 24u,
    // the .w word of a float4 slot, as a word index from that slot
    CFG_W_OF_F4 = 3u,
    // the tail leaf's four float4, from CFG_F4_TAIL, and its two words as word indices from there
    CFG_TAIL_LO = 0u,
    CFG_TAIL_HI = 1u,
    CFG_TAIL_N0 = 2u,
    CFG_TAIL_N1 = 3u,
    CFG_TAIL_W_LEAF = 4u * CFG_TAIL_LO + CFG_W_OF_F4,
    CFG_TAIL_W_PRIMARY = 4u * CFG_TAIL_HI + CFG_W_OF_F4,
};
// What the lean k_wavelocal kernels do NOT read from the block: the trip budget and the lane minimum of their ring steps are constants
// of the kernels (the generic kernels read CFG_W_BUDGET / CFG_W_MIN_ACTIVE, which the environment can set; a context whose values differ
// from these runs the generic kernels — select_trace_kernel).  Swept together on the bench step, profiles/r28_ring0_rule.txt.
//   ring 0: a step makes at most MPT_LEAN_RING0_BUDGET box trips and ends — its unfinished rays parked in ring 1 — once fewer than
//           MPT_LEAN_RING0_N0 of its lanes still walk (asked after every leaf phase, where the generic kernels ask their minimum)
//   ring 1: no trip budget, and the step ends once fewer than MPT_LEAN_RING1_N lanes still walk (the generic kernels' default)
// A -DMPT_LEAN_RING_TESTING build (tests/test_gpu_ring0_rule.py) reads the block instead, so that a test can set any pair.
#ifndef MPT_LEAN_RING0_BUDGET
#define MPT_LEAN_RING0_BUDGET 8u
#endif
#ifndef MPT_LEAN_RING0_N0
#define MPT_LEAN_RING0_N0 8u
#endif
#define MPT_LEAN_RING1_N 24u
#if defined(MPT_LEAN_RING_CONTROL) && !defined(MPT_LEAN_RING_TESTING)
#error "MPT_LEAN_RING_CONTROL makes a parked ray forget what it had found: test builds only (-DMPT_LEAN_RING_TESTING)"
#endif
static_assert(CFG_W_BUDGET + CFG_MAX_LEVELS <= CFG_W_MIN_ACTIVE && CFG_W_MIN_ACTIVE + CFG_MAX_LEVELS - 1u <= CFG_W_INPLACE_MIN,
              "configuration block: the per-level words overlap (the last minimum shares its word with k_ordered's threshold: MPT_OT_MLEVELS < 8)");
static_assert(4u * CFG_F4_WORDS + CFG_N_WORDS <= 4u * CFG_F4_ENTRY_LO, "configuration block: the word area runs into the entry terms");
static_assert(CFG_F4_ENTRY_HI + 1u <= CFG_F4_TAIL && CFG_F4_TAIL + CFG_TAIL_N1 + 1u <= CFG_F4_END, "configuration block: the lean slots overlap");
