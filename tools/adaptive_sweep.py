"""Adaptive sampling measurements (profiles/r06_adaptive.txt).

  python tools/adaptive_sweep.py [--out FILE]   equal-time error: scene.xml and Cornell at 1920x1080, depth 8, MSE of the adaptive
                                                mean (N = 1024, min 16, batch 16) at several thresholds and of a uniform render of
                                                the same wall time, both against a 4096-spp plain render with another seed; and the
                                                fixed cost per pass that the uniform renders' time fit leaves over
  python tools/adaptive_sweep.py --moments      1920x1080 x 256 spp of scene.xml with and without MPT_FLAG_MOMENTS, five each, for
                                                rocprofv3 --kernel-trace --stats (k_resolve_sum_moments against k_resolve_sum)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, DEPTH = 1920, 1080, 8
CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)


def context(name, cam=None):
    from metalpathtracer_amd import capi, host
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
    assert st == 0, log
    ctx = capi.Context(0)
    host.make_ready(ctx, sc, host.BVH_DEVICE)   # (what bench.py and `mpt_render --bvh auto` render)
    ctx.resize(W, H)
    ctx.set_uniforms(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
    return ctx


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def mse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float((d * d).mean())


def uniform(ctx, spp, seed=(1, 0)):
    ctx.clear_sum()
    _, ms = timed(lambda: ctx.render(sample_count=spp, max_depth=DEPTH, seed=seed))
    return ctx.read_sum() / np.float32(spp), ms


def sweep(out):
    lines = ["# adaptive sampling on one MI355X at %dx%d, depth %d, philox; times are host wall ms of the synchronous call (one run "
             "each, after a warm-up)" % (W, H, DEPTH)]
    for name, cam in (("scene.xml", None), ("cornell.xml", CORNELL_CAM)):
        ctx = context(name, cam)
        ctx.clear_sum()
        for k in range(16):   # 4096 spp, another seed
            ctx.render(sample_begin=256 * k, sample_count=256, max_depth=DEPTH, seed=(9, 0))
        ref = ctx.read_sum() / np.float32(4096)
        uniform(ctx, 16)      # warm-up
        ctx.render_adaptive(0.05, sample_count=64, max_depth=DEPTH)
        spps, times, errs = [16, 32, 64, 128, 256, 512], [], []
        for s in spps:
            img, ms = uniform(ctx, s)
            times.append(ms)
            errs.append(mse(img, ref))
        b, a = np.polyfit(spps, times, 1)
        lines.append("")
        lines.append("%s: uniform renders  spp / ms / MSE: %s" % (name, ", ".join("%d %.2f %.3e" % v for v in zip(spps, times, errs))))
        lines.append("%s: time fit  ms = %.3f + %.5f * spp" % (name, a, b))
        lines.append("%s: threshold  passes  mean_spp  tiles_conv/at_max  ms  MSE  |  equal-time uniform spp  ms  MSE  |  MSE ratio  "
                     "fixed ms/pass" % name)
        for thr in (0.2, 0.1, 0.05, 0.025):
            ctx.reset_stats()
            info, ms = timed(lambda: ctx.render_adaptive(thr, min_samples=16, batch_samples=16, sample_count=1024, max_depth=DEPTH))
            img = ctx.read_adaptive_mean()
            e = mse(img, ref)
            mean_spp = info["samples"] / (W * H)
            eq = max(1, int(round((ms - a) / b)))
            uimg, ums = uniform(ctx, eq)
            ue = mse(uimg, ref)
            fixed = (ms - (a + b * mean_spp)) / info["passes"]
            lines.append("%s: %.3f  %d  %.1f  %d/%d  %.2f  %.3e  |  %d  %.2f  %.3e  |  %.2f  %.3f" % (
                name, thr, info["passes"], mean_spp, info["tiles_converged"], info["tiles_at_max"], ms, e, eq, ums, ue, ue / e, fixed))
            print(lines[-1], flush=True)
        ctx.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)


def moments():
    from metalpathtracer_amd import capi
    ctx = context("scene.xml")
    for flags in (0, capi.FLAG_MOMENTS) * 5:
        ctx.clear_sum()
        ctx.render(sample_count=256, max_depth=32, flags=flags)
    ctx.close()
    print("moments runs done")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--moments", action="store_true")
    args = ap.parse_args()
    moments() if args.moments else sweep(args.out)
