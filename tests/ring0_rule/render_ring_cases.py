"""Child process of tests/test_gpu_ring0_rule.py: renders the views of ring_cases.py with the library MPT_LIB names and writes every
result to an .npz file.

usage: python render_ring_cases.py <out.npz> <arm> ...   (MPT_DEBUG_LAUNCH=1 is set by the caller)
An arm is `name:N0:budget` — a context made with MPT_MIN_ACTIVE="N0,<ring 1's>" and MPT_BUDGETS="budget" in the environment, which a
library reads when a context is made — or `name` alone: the environment as it is.  A name that ends in "+mega" also renders with the
megakernel, one that ends in "generic" gets MPT_WL_LEAN=0.  Per arm a and view v: `sync_a_v` the HDR sum of mpt_render with the wave-local
pipeline, `async_a_v` two back-to-back mpt_render_async steps of consecutive sample ranges into one sum (the corun kernel, both render
lanes), `counts_*` = (rays, paths) of each; a view with shards renders every rank into the one sum.  A render whose ring overflow flag is
set fails (MPT_ERR_OVERFLOW), and with it this process.  A marker line on stderr in front of every render separates the library's
MPT_DEBUG_LAUNCH lines."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
from metalpathtracer_amd import capi, host  # noqa: E402
from ring_cases import DEPTH, RING1_N, SIZE, SPP, VIEWS  # noqa: E402


def mark(text):
    sys.stderr.write(text + "\n")
    sys.stderr.flush()


out = {}
W, H = SIZE
for arm in sys.argv[2:]:
    name, _, pair = arm.partition(":")
    for k in ("MPT_MIN_ACTIVE", "MPT_BUDGETS", "MPT_WL_LEAN"):
        os.environ.pop(k, None)
    if pair:
        n0, budget = pair.split(":")
        os.environ["MPT_MIN_ACTIVE"] = "%s,%d" % (n0, RING1_N)
        os.environ["MPT_BUDGETS"] = budget
    if name.endswith("generic"):
        os.environ["MPT_WL_LEAN"] = "0"
    ctx = capi.Context(0)
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", "scene.xml"), sc)
    assert st == 0, log
    host.make_ready(ctx, sc, host.BVH_DEVICE)
    ctx.resize(W, H)
    kw = dict(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, max_depth=DEPTH, seed=(7, 1))
    pipes = [("", capi.PIPE_WAVELOCAL)] + ([("mega_", capi.PIPE_MEGAKERNEL)] if name.endswith("+mega") else [])
    for v, view in enumerate(VIEWS):
        ctx.set_uniforms(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=view["cam"]))
        n = view["shards"]
        for tag, pipe in pipes:
            mark("RENDER %s %d %ssync" % (name, v, tag))
            ctx.clear_sum()
            ctx.reset_stats()
            for r in range(n):
                ctx.render(sample_begin=0, sample_count=SPP, pipeline=pipe, shard_rank=r, shard_count=n, **kw)
            s = ctx.stats()
            out["%ssync_%s_%d" % (tag, name, v)] = ctx.read_sum()
            out["%scounts_sync_%s_%d" % (tag, name, v)] = np.array([s["rays"], s["paths"]], np.int64)
            mark("RENDER %s %d %sasync" % (name, v, tag))
            ctx.clear_sum()
            ctx.reset_stats()
            for half in (0, 1):
                for r in range(n):
                    if pipe == capi.PIPE_WAVELOCAL:
                        ctx.render_async(sample_begin=half * SPP, sample_count=SPP, pipeline=pipe, shard_rank=r, shard_count=n, **kw)
                    else:
                        ctx.render(sample_begin=half * SPP, sample_count=SPP, pipeline=pipe, shard_rank=r, shard_count=n, **kw)
            if pipe == capi.PIPE_WAVELOCAL:
                ctx.wait()
            s = ctx.stats()
            out["%sasync_%s_%d" % (tag, name, v)] = ctx.read_sum()
            out["%scounts_async_%s_%d" % (tag, name, v)] = np.array([s["rays"], s["paths"]], np.int64)
    mark("RENDER end")
    ctx.close()
np.savez(sys.argv[1], **out)
