"""The views and render items of tests/test_gpu_sky_resolve.py, shared with its child process (render_sky_cases.py): no pytest, no GPU in here.

VIEWS: six cases of tests/lean_tiles/tile_cases.py, by name, with what the class table read back must hold so that no view passes
vacuously — `sky`: at least one tile of class "skip, empty mask" (0x80000000), the tiles the trace kernel elides and the resolve sums;
`other`: at least one tile of another class, whose samples still go through the slots.  The mix was checked on the CPU classifier
(tests/lean_tiles/lean_tiles_check.cpp, 70 x 45): default 18 sky of 54, horizon 16, straight up 38 (the other 16 see the sphere at
y = 100 and nothing else), straight down 0 (52 see the ground alone, 2 the mesh), lone triangle 16.  Straight down is the view in which
the resolve gets a table and finds no sky tile in it.

ITEMS: what is rendered in every view at both sizes.  `renders`: (sample_begin, sample_count) of each call; `async`: by mpt_render_async
(both render lanes, the corun kernel, the sums chained in submission order), else by mpt_render.  Sample counts 1, 3, 5 and 17 are the
tails of the resolves' unrolled loops (two sky samples, four slots) and no powers of two."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lean_tiles"))
from tile_cases import CASES  # noqa: E402

_BY_NAME = {c["name"]: c for c in CASES}


def _view(name, sky, other):
    return dict(_BY_NAME[name], sky=sky, other=other)


VIEWS = [
    _view("default-classes", True, True),
    _view("straight-up", True, False),
    _view("straight-down", False, True),
    _view("horizon-through-a-tile-row", True, True),
    _view("light-silhouette", True, True),
    _view("lone-triangle-in-the-sky", True, True),
]


def _item(name, renders, depth=8, rank=0, shards=1, moments=False, async_=False):
    return dict(name=name, renders=renders, depth=depth, rank=rank, shards=shards, moments=moments, **{"async": async_})


ITEMS = [_item("spp%d_d%d" % (n, d), [(0, n)], depth=d) for n in (1, 3, 5, 17) for d in (1, 8)] + [
    _item("begin11", [(11, 5)]),
    _item("async3", [(0, 5), (5, 5), (10, 5)], async_=True),
    _item("rank1of2", [(0, 3)], rank=1, shards=2),
    _item("moments", [(0, 5)], moments=True),
]
