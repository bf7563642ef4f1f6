"""Child process of tests/test_gpu_lean_tail.py: renders the cases of tail_cases.py and writes every result to an .npz file.

usage: python render_tail_cases.py <out.npz>        (MPT_DEBUG_LAUNCH=1 is set by the caller; MPT_WL_LEAN=0 for the generic arm)
For case k and each of the wave-local pipeline ("") and the megakernel ("mega_"): `sync_k` / `sync_b_k` = the HDR sum of one mpt_render
with the case's first / second camera, `async_k` = the sum of two back-to-back mpt_render_async steps of consecutive sample ranges, the
first camera then the second (the megakernel: two mpt_render), `counts_k` = (rays, paths) after each of the three.  Per case also what a
launch's tail terms are computed from: the device's node array, written to <out.npz>.nodes_k.bin (8 words per node), `n_nodes_k`,
`cams_k` = the two camera positions as the uniforms carry them,
`root_box_k` = the root's box in the tree mpt_download_bvh returns, `node0_k` = the device array's first eight words.
A marker line on stderr in front of every render separates the library's MPT_DEBUG_LAUNCH lines."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
from metalpathtracer_amd import capi, host  # noqa: E402
from tail_cases import CASES, DEPTH, SCENES, SIZE, SPP, place  # noqa: E402


def mark(text):
    sys.stderr.write(text + "\n")
    sys.stderr.flush()


out = {}
ctx = capi.Context(0)
loaded, counts_of, nodes, n_nodes, root_box = None, None, None, 0, None
for k, c in enumerate(CASES):
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
        tree = ctx.download_bvh()[0]
        root_box = np.ascontiguousarray(tree[0], np.float32).reshape(8)
        nodes = ctx.read_scene_array(capi.SCENE_ARRAYS.index("nodes"))
        n_nodes = nodes.size // 8
    nodes.tofile("%s.nodes_%d.bin" % (sys.argv[1], k))
    W, H = SIZE
    ctx.resize(W, H)
    cams = [place(cam, nodes, n_nodes) for cam in c["cams"]]
    u = [host.make_uniforms(W, H, counts_of[0], counts_of[1], cam=cam) for cam in cams]
    out["node0_%d" % k], out["n_nodes_%d" % k], out["root_box_%d" % k] = nodes[:8].copy(), np.array([n_nodes], np.int64), root_box
    out["cams_%d" % k] = np.array([[x.cameraPosition[0], x.cameraPosition[1], x.cameraPosition[2]] for x in u], np.float32)
    kw = dict(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, max_depth=DEPTH, seed=(7, 1))
    for name, pipe in (("", capi.PIPE_WAVELOCAL), ("mega_", capi.PIPE_MEGAKERNEL)):
        counts = []
        for tag, which in (("sync", 0), ("sync_b", 1)):
            mark("CASE %d %s%s" % (k, name, tag))
            ctx.clear_sum()
            ctx.reset_stats()
            ctx.set_uniforms(u[which])
            ctx.render(sample_begin=0, sample_count=SPP, pipeline=pipe, **kw)
            s = ctx.stats()
            out["%s%s_%d" % (name, tag, k)] = ctx.read_sum()
            counts += [s["rays"], s["paths"]]
        mark("CASE %d %sasync" % (k, name))
        ctx.clear_sum()
        ctx.reset_stats()
        for which in (0, 1):
            ctx.set_uniforms(u[which])
            (ctx.render_async if pipe == capi.PIPE_WAVELOCAL else ctx.render)(sample_begin=which * SPP, sample_count=SPP, pipeline=pipe, **kw)
        if pipe == capi.PIPE_WAVELOCAL:
            ctx.wait()
        s = ctx.stats()
        out["%sasync_%d" % (name, k)] = ctx.read_sum()
        out["%scounts_%d" % (name, k)] = np.array(counts + [s["rays"], s["paths"]], np.int64)
mark("CASE end")
ctx.close()
np.savez(sys.argv[1], **out)
