"""Child process of tests/test_gpu_lean_tiles.py and tests/test_gpu_lean_tiles_device.py: renders the cases of tile_cases.py and writes
every result to an .npz file.

usage: python render_tile_cases.py <out.npz> [first_case last_case]   (MPT_DEBUG_LAUNCH=1 is set by the caller; MPT_WL_LEAN=0 / MPT_LEAN_TILES=0 for the other arms)
For case k and size s (index into tile_cases.SIZES): `wl_k_s` = the HDR sum of mpt_render with the wave-local pipeline, `mega_k_s` the
megakernel's, `async_k_s` two back-to-back mpt_render_async steps of consecutive sample ranges into one sum (the corun kernel, both render
lanes), `counts_*` = (rays, paths) of each, `table_k_s` = the class table read back after the wave-local render (empty: none),
`builds_k_s` = how many tables the context had built by then, `uniforms_k_s` = the fourteen camera words of the render, `n_nodes_k`,
`n_prims_k`; the device's node and primitive arrays go to <out.npz>.nodes_k.bin and .prims_k.bin.  A case with shards renders every
rank into the one sum.  A marker line on stderr in front of every render separates the library's MPT_DEBUG_LAUNCH lines."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
from metalpathtracer_amd import capi, host  # noqa: E402
from tile_cases import CASES, DEPTH, SCENES, SIZES, SPP  # noqa: E402
import tail_cases as tc  # noqa: E402


def mark(text):
    sys.stderr.write(text + "\n")
    sys.stderr.flush()


first, last = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (0, len(CASES))
out = {}
ctx = capi.Context(0)
loaded, counts_of, nodes, prims_dev = None, None, None, None
for k, c in enumerate(CASES):
    if not first <= k < last:
        continue
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
        prims_dev = ctx.read_scene_array(capi.SCENE_ARRAYS.index("prims"))
    nodes.tofile("%s.nodes_%d.bin" % (sys.argv[1], k))
    prims_dev.tofile("%s.prims_%d.bin" % (sys.argv[1], k))
    out["n_nodes_%d" % k], out["n_prims_%d" % k] = np.array([nodes.size // 8], np.int64), np.array([prims_dev.size // 12], np.int64)
    cam = tc.place(c["cam"], nodes, nodes.size // 8)
    kw = dict(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, max_depth=DEPTH, seed=(7, 1))
    for s, (W, H) in enumerate(SIZES):
        ctx.resize(W, H)
        u = host.make_uniforms(W, H, counts_of[0], counts_of[1], cam=cam)
        ctx.set_uniforms(u)
        out["uniforms_%d_%d" % (k, s)] = np.array(list(u.cameraPosition[:3]) + list(u.firstPixelPosition[:3]) + list(u.viewportU[:3]) +
                                                  list(u.viewportV[:3]) + list(u.screenSize[:2]), np.float32)
        n = c["shards"]
        for name, pipe in (("wl", capi.PIPE_WAVELOCAL), ("mega", capi.PIPE_MEGAKERNEL)):
            mark("CASE %d %d %s" % (k, s, name))
            ctx.clear_sum()
            ctx.reset_stats()
            for r in range(n):
                ctx.render(sample_begin=0, sample_count=SPP, pipeline=pipe, shard_rank=r, shard_count=n, **kw)
            st = ctx.stats()
            out["%s_%d_%d" % (name, k, s)] = ctx.read_sum()
            out["counts_%s_%d_%d" % (name, k, s)] = np.array([st["rays"], st["paths"]], np.int64)
            if name == "wl":
                out["table_%d_%d" % (k, s)], b = ctx.read_lean_tile_classes()
                out["builds_%d_%d" % (k, s)] = np.array([b], np.int64)
        mark("CASE %d %d async" % (k, s))
        ctx.clear_sum()
        ctx.reset_stats()
        for half in (0, 1):
            for r in range(n):
                ctx.render_async(sample_begin=half * SPP, sample_count=SPP, pipeline=capi.PIPE_WAVELOCAL, shard_rank=r, shard_count=n, **kw)
        ctx.wait()
        st = ctx.stats()
        out["async_%d_%d" % (k, s)] = ctx.read_sum()
        out["counts_async_%d_%d" % (k, s)] = np.array([st["rays"], st["paths"]], np.int64)
        mark("CASE %d %d mega2" % (k, s))
        ctx.clear_sum()
        for half in (0, 1):
            for r in range(n):
                ctx.render(sample_begin=half * SPP, sample_count=SPP, pipeline=capi.PIPE_MEGAKERNEL, shard_rank=r, shard_count=n, **kw)
        out["mega2_%d_%d" % (k, s)] = ctx.read_sum()
mark("CASE end")
ctx.close()
np.savez(sys.argv[1], **out)
