"""Child process of tests/test_gpu_lean_primary.py: renders the cases of cases.py and writes every result to an .npz file.

usage: python render_cases.py <out.npz>        (MPT_DEBUG_LAUNCH=1 is set by the caller; MPT_WL_LEAN=0 for the generic arm)
For case k and each of the wave-local pipeline ("") and the megakernel ("mega_"): `sync_k` / `sync_b_k` = the HDR sum of one mpt_render
with the case's first / second camera, `async_k` = the sum of two back-to-back mpt_render_async steps of consecutive sample ranges, the
first camera then the second (the megakernel: two mpt_render), `counts_k` = (rays, paths) after each of the three.  For the soup scene
also the device's primitive records and one mpt_trace_rays ray from the camera to every sphere's centre.  A marker line on stderr in
front of every render separates the library's MPT_DEBUG_LAUNCH lines."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, HERE]
from metalpathtracer_amd import capi, host  # noqa: E402
from cases import CASES, SOUP_CAM, SOUP_SPHERES, soup_scene  # noqa: E402


def mark(text):
    sys.stderr.write(text + "\n")
    sys.stderr.flush()


out = {}
ctx = capi.Context(0)
loaded, counts_of = None, None
for k, c in enumerate(CASES):
    if loaded != c["scene"]:
        loaded = c["scene"]
        if loaded == "soup":
            prims, mats = soup_scene()
            ctx.build_and_upload(prims, mats)
            counts_of = (prims.shape[0], prims.shape[0] - SOUP_SPHERES)
            out["soup_prims"] = ctx.read_scene_array(capi.SCENE_ARRAYS.index("prims"))
            centres = prims[:SOUP_SPHERES, 0:3].astype(np.float64)
            d = centres - np.asarray(SOUP_CAM["pos"], np.float64)
            d /= np.linalg.norm(d, axis=1)[:, None]
            t, prim = ctx.trace_rays(np.tile(np.asarray(SOUP_CAM["pos"], np.float32), (SOUP_SPHERES, 1)), d.astype(np.float32))[:2]
            out["soup_ray_dirs"], out["soup_ray_prim"] = d.astype(np.float32), np.asarray(prim, np.int32)
        else:
            sc = host.Scene()
            st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", loaded), sc)
            assert st == 0, log
            host.make_ready(ctx, sc, host.BVH_DEVICE)
            counts_of = (sc.getPrimitiveCount(), sc.getTriangleCount())
        out["nodes_" + loaded] = np.array([ctx.build_info()["threaded_nodes"]], np.int64)
    W, H, spp = c["size"][0], c["size"][1], c["spp"]
    ctx.resize(W, H)
    u = [host.make_uniforms(W, H, counts_of[0], counts_of[1], cam=cam) for cam in c["cams"]]
    kw = dict(rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, max_depth=c["depth"], seed=(7, 1))
    for name, pipe in (("", capi.PIPE_WAVELOCAL), ("mega_", capi.PIPE_MEGAKERNEL)):
        counts = []
        for tag, which in (("sync", 0), ("sync_b", 1)):
            mark("CASE %d %s%s" % (k, name, tag))
            ctx.clear_sum()
            ctx.reset_stats()
            ctx.set_uniforms(u[which])
            ctx.render(sample_begin=0, sample_count=spp, pipeline=pipe, **kw)
            s = ctx.stats()
            out["%s%s_%d" % (name, tag, k)] = ctx.read_sum()
            counts += [s["rays"], s["paths"]]
        mark("CASE %d %sasync" % (k, name))
        ctx.clear_sum()
        ctx.reset_stats()
        for which in (0, 1):
            ctx.set_uniforms(u[which])
            (ctx.render_async if pipe == capi.PIPE_WAVELOCAL else ctx.render)(sample_begin=which * spp, sample_count=spp, pipeline=pipe, **kw)
        if pipe == capi.PIPE_WAVELOCAL:
            ctx.wait()
        s = ctx.stats()
        out["%sasync_%d" % (name, k)] = ctx.read_sum()
        out["%scounts_%d" % (name, k)] = np.array(counts + [s["rays"], s["paths"]], np.int64)
mark("CASE end")
ctx.close()
np.savez(sys.argv[1], **out)
