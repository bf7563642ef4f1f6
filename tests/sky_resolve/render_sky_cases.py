"""Child process of tests/test_gpu_sky_resolve.py: renders the views of sky_cases.py and writes every result to an .npz file.

usage: python render_sky_cases.py <out.npz>   (MPT_DEBUG_LAUNCH=1 is set by the caller; MPT_LEAN_SKY_RESOLVE=0 for the other arm)
For view k, size s (index into tile_cases.SIZES) and item `name` of sky_cases.ITEMS: `wl_k_s_name` = the HDR sum of the item's renders
with the wave-local pipeline, `mega_k_s_name` the megakernel's, `counts_*` = (rays, paths) of each, `m2wl_*` / `m2mega_*` the moments
buffer of the item with FLAG_MOMENTS, `table_k_s` = the class table read back after the first wave-local render; and `draw_wl` / `draw_mega`,
one frame of the frame protocol in the default view.  A marker line on stderr in front of every item separates the library's
MPT_DEBUG_LAUNCH lines."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE, os.path.join(ROOT, "tests", "lean_tiles")]
from metalpathtracer_amd import capi, host  # noqa: E402
from sky_cases import ITEMS, VIEWS  # noqa: E402
from tile_cases import SCENES, SIZES  # noqa: E402
import tail_cases as tc  # noqa: E402


def mark(text):
    sys.stderr.write(text + "\n")
    sys.stderr.flush()


def run_item(ctx, item, pipe):
    ctx.clear_sum()
    ctx.reset_stats()
    kw = dict(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, seed=(7, 1), pipeline=pipe, max_depth=item["depth"],
              shard_rank=item["rank"], shard_count=item["shards"], flags=capi.FLAG_MOMENTS if item["moments"] else 0)
    for begin, count in item["renders"]:
        (ctx.render_async if item["async"] else ctx.render)(sample_begin=begin, sample_count=count, **kw)
    ctx.wait()
    st = ctx.stats()
    return ctx.read_sum(), np.array([st["rays"], st["paths"]], np.int64), ctx.read_moments() if item["moments"] else None


out = {}
ctx = capi.Context(0)
loaded, counts_of, nodes = None, None, None
for k, c in enumerate(VIEWS):
    if loaded != c["scene"]:
        loaded = c["scene"]
        if loaded in SCENES:
            prims, mats = SCENES[loaded]()
            ctx.build_and_upload(prims, mats)
            counts_of = (prims.shape[0], int((prims[:, 3] == 1.0).sum()))
        else:
            sc = host.Scene()
            st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", loaded), sc)
            assert st == 0, log
            host.make_ready(ctx, sc, host.BVH_DEVICE)
            counts_of = (sc.getPrimitiveCount(), sc.getTriangleCount())
        nodes = ctx.read_scene_array(capi.SCENE_ARRAYS.index("nodes"))
    cam = tc.place(c["cam"], nodes, nodes.size // 8)
    for s, (W, H) in enumerate(SIZES):
        ctx.resize(W, H)
        u = host.make_uniforms(W, H, counts_of[0], counts_of[1], cam=cam)
        ctx.set_uniforms(u)
        for item in ITEMS:
            tag = "%d_%d_%s" % (k, s, item["name"])
            for name, pipe in (("wl", capi.PIPE_WAVELOCAL), ("mega", capi.PIPE_MEGAKERNEL)):
                mark("ITEM %s %s" % (tag, name))
                out["%s_%s" % (name, tag)], out["counts_%s_%s" % (name, tag)], m2 = run_item(ctx, item, pipe)
                if m2 is not None:
                    out["m2%s_%s" % (name, tag)] = m2
                if name == "wl" and "table_%d_%d" % (k, s) not in out:
                    out["table_%d_%d" % (k, s)], _ = ctx.read_lean_tile_classes()
        if k == 0 and s == 0:   # the frame protocol: one sample per draw, k_resolve_frame reads every slot
            for name, pipe in (("wl", capi.PIPE_WAVELOCAL), ("mega", capi.PIPE_MEGAKERNEL)):
                mark("ITEM draw %s" % name)
                u.frameCount = 0
                ctx.set_uniforms(u)
                ctx.draw(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, seed=(7, 1), pipeline=pipe, max_depth=8)
                out["draw_%s" % name] = ctx.read_frame()
mark("ITEM end")
ctx.close()
np.savez(sys.argv[1], **out)
