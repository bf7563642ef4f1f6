"""Child process of tests/test_gpu_wavelocal_lean.py: renders the cases of a JSON file and writes every result to an .npz file.

usage: python render_cases.py <cases.json> <out.npz>        (MPT_DEBUG_LAUNCH=1 is set by the caller; MPT_WL_LEAN=0 for the generic arm)
For case k: `sync_k` = the HDR sum of one mpt_render, `async_k` = the sum of two back-to-back mpt_render_async of consecutive sample
ranges, `counts_k` = (rays, paths) of each; with "mega": the same from the megakernel (`mega_sync_k`, ...).  A marker line on stderr in
front of every render separates the library's MPT_DEBUG_LAUNCH lines."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from metalpathtracer_amd import capi, host  # noqa: E402

cases = json.load(open(sys.argv[1]))
out = {}
ctx = capi.Context(0)
loaded = None
for k, c in enumerate(cases):
    if loaded != c["scene"]:
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", c["scene"]), sc)
        assert st == 0, log
        bvh = host.make_ready(ctx, sc, host.BVH_DEVICE)[0]
        loaded = c["scene"]
        out["nodes_" + c["scene"]] = np.array([np.asarray(bvh).size // 8], np.int64)   # 32-byte nodes of the reference-order tree
    W, H, spp = c["size"][0], c["size"][1], c["spp"]
    ctx.resize(W, H)
    ctx.set_uniforms(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount()))
    kw = dict(rng_mode=c["rng"], bsdf_mode=c["bsdf"], max_depth=c["depth"], seed=(7, 1), shard_rank=c["rank"], shard_count=c["shards"])
    for name, pipe in (("", capi.PIPE_WAVELOCAL),) + ((("mega_", capi.PIPE_MEGAKERNEL),) if c.get("mega") else ()):
        sys.stderr.write("CASE %d %ssync\n" % (k, name))
        sys.stderr.flush()
        ctx.clear_sum()
        ctx.reset_stats()
        ctx.render(sample_begin=0, sample_count=spp, pipeline=pipe, **kw)
        s = ctx.stats()
        out["%ssync_%d" % (name, k)] = ctx.read_sum()
        counts = [s["rays"], s["paths"]]
        sys.stderr.write("CASE %d %sasync\n" % (k, name))
        sys.stderr.flush()
        ctx.clear_sum()
        ctx.reset_stats()
        if pipe == capi.PIPE_WAVELOCAL:
            ctx.render_async(sample_begin=0, sample_count=spp, pipeline=pipe, **kw)
            ctx.render_async(sample_begin=spp, sample_count=spp, pipeline=pipe, **kw)
            ctx.wait()
        else:
            ctx.render(sample_begin=0, sample_count=spp, pipeline=pipe, **kw)
            ctx.render(sample_begin=spp, sample_count=spp, pipeline=pipe, **kw)
        s = ctx.stats()
        out["%sasync_%d" % (name, k)] = ctx.read_sum()
        out["%scounts_%d" % (name, k)] = np.array(counts + [s["rays"], s["paths"]], np.int64)
sys.stderr.write("CASE end\n")
sys.stderr.flush()
ctx.close()
np.savez(sys.argv[2], **out)
