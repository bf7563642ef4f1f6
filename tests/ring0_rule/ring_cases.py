"""The views and the (N0, budget) pairs of tests/test_gpu_ring0_rule.py, shared with its child process (render_ring_cases.py): no pytest, no
GPU in here.

Every view renders scene.xml on the device-built tree at 70 x 45 (a partial tile column and row), 16 spp, depth 8, Philox.  scene.xml's mesh
stands in the box (-31.92, -0.15, -6.99) .. (-16.39, 15.23, 5.06): the two close views fill the image with it, so that no tile is a
`skip` tile and most bounce rays walk its sub-tree — the rays a ring-0 step parks; the view straight down sees the ground alone, whose
bounce rays all end within a trip or two."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lean_tail"))
import tail_cases as tc  # noqa: E402

SIZE, SPP, DEPTH = (70, 45), 16, 8
OWN = tc.OWN
UPZ = (0.0, 0.0, -1.0)

VIEWS = [dict(name="default", cam=OWN, shards=1),
         dict(name="bunny-close", cam=dict(OWN, pos=(-24.0, 8.0, 16.0), fwd=(0.0, -0.05, -1.0)), shards=1),
         dict(name="bunny-from-above", cam=dict(OWN, pos=(-24.0, 30.0, 0.0), fwd=(0.0, -1.0, 0.0), up=UPZ), shards=1),
         dict(name="ground-only", cam=dict(OWN, fwd=(0.0, -1.0, 0.0), up=UPZ), shards=1),
         dict(name="horizon-through-a-tile-row", cam=dict(OWN, fwd=(0.0, -0.03, -1.0)), shards=1),
         dict(name="two-shards", cam=OWN, shards=2)]

# MPT_LEAN_RING0_N0, MPT_LEAN_RING0_BUDGET and MPT_LEAN_RING1_N of metalpathtracer_amd/csrc/mpt_lds_cfg.h (the test reads them from the
# header and compares)
SHIPPED = (8, 8)
RING1_N = 24
# (name, N0, budget) of the test build, whose lean kernels read both from the configuration block: the shipped pair; the rule off; every
# unfinished ray parked after the first look at the loop's condition; the rule at its smallest; an odd budget, which the loop's pair of
# trips straddles; and a large N0 with a long budget, where the rule alone ends the steps
PAIRS = [("shipped",) + SHIPPED, ("off", 0, 8), ("n64-b1", 64, 1), ("n1", 1, 8), ("odd-budget", 8, 5), ("n24-b12", 24, 12)]
