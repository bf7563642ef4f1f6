"""Timing of the two ways to sample a sphere light (mpt_set_light_sampling: AREA, CONE) on one GPU (profiles/r13_cone.txt), the sibling of
tools/nee_timing.py with its settings: HIP events throughout, the variants alternating in one process.
 (i)   Cornell box 1024x1024 and scene.xml 1920x1080, 16 spp at depth 8: the trace-kernel time of mpt_render at MPT_PIPE_AUTO, of
       mpt_render_nee and of mpt_direct_lighting (16 samples) with both walks under AREA and under CONE — the minimum and the median of
       REPS runs after WARMUP — with the rays and shadow rays of a run;
 (ii)  the variance of the estimators on the same workloads at a sixteenth of the pixels: BATCHES renders of 16 spp with different seeds
       each, the per-pixel variance of the batch means (the scalar is the mean of the three channels), summed over the image, mpt_render
       against mpt_render_nee under AREA and under CONE with the same per-sample clamp (1); variance x time is the product of that ratio
       and (i)'s;
 (iii) with --bench: bench.py's headline, RUNS times.
A library without mpt_set_light_sampling (an older build, through MPT_LIB and its own package) is timed under AREA alone: that is how the
area kernels of two builds are compared, the two processes alternating.
--area-only times this build the same way (the same sequence of kernels in the process).
Usage: python tools/cone_timing.py [--out profiles/r13_cone.txt] [--bench RUNS] [--quick] [--no-variance] [--area-only]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metalpathtracer_amd import capi, host  # noqa: E402

CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
WORKLOADS = (("cornell.xml", CORNELL_CAM, 1024, 1024), ("scene.xml", None, 1920, 1080))
SPP, DEPTH = 16, 8
REPS, WARMUP = 10, 3
BATCHES = 32
HAVE_SETTING = hasattr(capi.Context, "set_light_sampling")
ALL_MODES = (("area", 0), ("cone", 1)) if HAVE_SETTING else (("area", 0),)


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return "min %8.3f  median %8.3f ms" % (ms[0], ms[len(ms) // 2])


def set_mode(ctx, mode):
    if HAVE_SETTING:
        ctx.set_light_sampling(mode)


def batch_variance(ctx, run, batches, spp):
    """The per-pixel variance [H, W] of `batches` batch means; run(b) adds a batch's samples to the cleared sum."""
    x = np.empty((batches, ctx.height, ctx.width), np.float64)
    for b in range(batches):
        ctx.clear_sum()
        run(b)
        x[b] = ctx.read_sum()[..., :3].mean(-1, dtype=np.float64) / spp
    return x.var(0, ddof=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="a quarter of the width and height (a dry run of the tool itself)")
    ap.add_argument("--no-variance", action="store_true", help="part (i) alone")
    ap.add_argument("--area-only", action="store_true", help="AREA alone, as a build without the setting is timed")
    a = ap.parse_args()
    MODES = ALL_MODES[:1] if a.area_only else ALL_MODES
    lines = ["cone_timing: %d spp at depth %d, %d timed runs after %d warm-up runs, build %s, modes %s" % (
        SPP, DEPTH, REPS, WARMUP, capi.build_id()["source_sha256"][:16], "/".join(m for m, _ in MODES))]
    ctx = capi.Context(0)
    for name, cam, w, h in WORKLOADS:
        if a.quick:
            w, h = w // 4, h // 4
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        ctx.resize(w, h)
        ctx.set_uniforms(host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        lights = ctx.light_info()
        lines.append("")
        lines.append("%s %dx%dx%d: %d primitives, %d lights (%d spheres)" % (name, w, h, SPP, sc.getPrimitiveCount(), lights["lights"], lights["sphere_lights"]))
        kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=(1, 0))
        variants = [("mpt_render, MPT_PIPE_AUTO", 0, lambda: ctx.render(pipeline=capi.PIPE_AUTO, **kw))]
        for mode_name, mode in MODES:
            for walk_name, walk in (("reference order", capi.WALK_REFERENCE), ("own tree", capi.WALK_OWN)):
                variants.append(("mpt_render_nee, %s, %s" % (mode_name, walk_name), mode,
                                 lambda walk=walk: ctx.render_nee(walk=walk, clamp=1.0, **kw)))
                variants.append(("mpt_direct_lighting, %s, %s" % (mode_name, walk_name), mode,
                                 lambda walk=walk: ctx.direct_lighting(samples=SPP, seed=(1, 0), walk=walk)))
        ms = {label: [] for label, _, _ in variants}
        note = {}
        for r in range(WARMUP + REPS):
            for label, mode, run in variants:
                set_mode(ctx, mode)
                ctx.clear_sum()
                ctx.reset_stats()
                info = run()
                if r >= WARMUP:
                    ms[label].append(info["device_ms"] if info else ctx.stats()["trace_kernel_ms"])
                if not info:
                    note[label] = "%d rays" % ctx.stats()["rays"]
                elif "shadow_rays" in info:
                    note[label] = "%d rays, %d shadow rays (%.1f %% occluded)" % (info["rays"], info["shadow_rays"],
                                                                                 100.0 * info["shadow_rays_occluded"] / max(info["shadow_rays"], 1))
                else:
                    note[label] = "%d shadow rays (%.1f %% occluded)" % (info["rays"], 100.0 * info["rays_occluded"] / max(info["rays"], 1))
        for label, _, _ in variants:
            lines.append(" (i)  %-48s %s   %s" % (label + ":", stats(ms[label]), note[label]))
        print("\n".join(lines[-len(variants) - 1:]), flush=True)
        if a.no_variance:
            continue
        ctx.resize(w // 4, h // 4)
        ctx.set_uniforms(host.make_uniforms(w // 4, h // 4, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        vkw = dict(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP)
        v_pt = batch_variance(ctx, lambda b: ctx.render(seed=(b, 1), **vkw), BATCHES, SPP)
        t_pt = min(ms["mpt_render, MPT_PIPE_AUTO"])
        lines.append(" (ii) variance at %dx%d, %d batches of %d spp, all clamped at 1, summed over the image; time at the minima of (i), the faster walk" % (
            w // 4, h // 4, BATCHES, SPP))
        lines.append("      mpt_render: summed variance %.6g, %.3f ms" % (v_pt.sum(), t_pt))
        for k, (mode_name, mode) in enumerate(MODES):
            set_mode(ctx, mode)
            v = batch_variance(ctx, lambda b: ctx.render_nee(seed=(b, 2 + k), walk=capi.WALK_AUTO, clamp=1.0, **vkw), BATCHES, SPP)
            t = min(min(ms["mpt_render_nee, %s, reference order" % mode_name]), min(ms["mpt_render_nee, %s, own tree" % mode_name]))
            lines.append("      mpt_render_nee, %s: summed variance %.6g (pt / nee %.3f), %.3f ms (nee / pt %.2f); variance x time, pt / nee "
                         "(> 1: NEE wins per unit of noise): %.3f" % (mode_name, v.sum(), v_pt.sum() / v.sum(), t, t / t_pt, v_pt.sum() * t_pt / (v.sum() * t)))
        set_mode(ctx, 0)
        print("\n".join(lines[-2 - len(MODES):]), flush=True)
    ctx.close()
    if a.bench:
        lines.append("")
        for r in range(a.bench):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, check=True).stdout
            j = json.loads(out.strip().splitlines()[-1])
            lines.append(" (iii) bench.py run %d: %s" % (r, json.dumps({k: j[k] for k in j if not isinstance(j[k], (dict, list))})))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
