"""Timing and variance of resampled light sampling (mpt_set_light_candidates, include/mpt.h) on one GPU (profiles/r21_ris.txt), the
sibling of tools/nee_timing.py and tools/cone_timing.py: HIP events throughout, the variants alternating in one process.
 (i)   Cornell box 1024x1024 and scene.xml 1920x1080: the kernel time of the direct pass with 16 samples and of mpt_render_nee with
       16 spp at depth 8 (clamp 1), with both walks, both light samplings and M in {1, 2, 4, 8, 16, 32} candidates — the minimum of
       REPS runs after WARMUP — and mpt_render at MPT_PIPE_AUTO beside them;
 (ii)  the variance on the same workloads at a sixteenth of the pixels (MPT_WALK_AUTO): BATCHES results of 16 samples with different
       seeds each, the per-pixel variance of the batch means (the scalar is the mean of the three channels), summed over the pixels;
       mpt_render_nee and mpt_render clamped at 1 per sample (the direct pass has no clamp);
 (iii) per workload, walk and sampling one line per M: the time, the variance, and variance x time of M = 1 over that of M (> 1: M
       candidates win per unit of noise); for the render also variance x time of mpt_render over that of M, the figure of DESIGN.md §17;
 (iv)  with --bench: bench.py's headline, RUNS times.
Usage: python tools/ris_timing.py [--out profiles/r21_ris.txt] [--bench RUNS] [--quick]"""
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
MS = (1, 2, 4, 8, 16, 32)
WALKS = (("reference order", capi.WALK_REFERENCE), ("own tree", capi.WALK_OWN))
SAMPLINGS = (("area", capi.LIGHT_SAMPLING_AREA), ("cone", capi.LIGHT_SAMPLING_CONE))


def run_one(ctx, what, walk, seed, clamp=1.0):
    """One direct pass or one render onto a cleared sum under the context's settings: (kernel ms, info)."""
    if what == "direct":
        info = ctx.direct_lighting(samples=SPP, seed=seed, walk=walk)
    else:
        ctx.clear_sum()
        info = ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=seed, walk=walk, clamp=clamp)
    return info["device_ms"], info


def result(ctx, what):
    """[H, W] float64: the mean of the three channels of the direct pass's image, or of the sum per sample."""
    if what == "direct":
        return ctx.read_direct()[0][..., :3].mean(-1, dtype=np.float64)
    return ctx.read_sum()[..., :3].mean(-1, dtype=np.float64) / SPP


def summed_variance(batch):
    return float(np.asarray(batch).var(0, ddof=1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="a quarter of the width and height (a dry run of the tool itself)")
    a = ap.parse_args()
    lines = ["ris_timing: %d samples (depth %d for the render), the minimum of %d timed runs after %d warm-up runs, build %s" % (
        SPP, DEPTH, REPS, WARMUP, capi.build_id()["source_sha256"][:16])]
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
        acc, lights = ctx.accel_info(), ctx.light_info()
        lines.append("")
        lines.append("%s %dx%d: %d primitives, %d lights, MPT_WALK_AUTO = %s" % (
            name, w, h, sc.getPrimitiveCount(), lights["lights"], "own tree" if acc["auto_pipeline"] == capi.PIPE_ORDERED else "reference order"))
        # (i) the times: every variant once per round, the rounds one after the other
        variants = [(what, wl, wv, sl, sv, M) for what in ("direct", "nee") for wl, wv in WALKS for sl, sv in SAMPLINGS for M in MS]
        ms = {v: [] for v in variants}
        note = {}
        pt_ms = []
        for r in range(WARMUP + REPS):
            ctx.clear_sum()
            ctx.reset_stats()
            ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=(1, 0), pipeline=capi.PIPE_AUTO)
            if r >= WARMUP:
                pt_ms.append(ctx.stats()["trace_kernel_ms"])
            for v in variants:
                what, _, wv, _, sv, M = v
                ctx.set_light_sampling(sv)
                ctx.set_light_candidates(M)
                t, info = run_one(ctx, what, wv, (1, 0))
                if r >= WARMUP:
                    ms[v].append(t)
                note[v] = ("%d rays, %.1f %% occluded" % (info["rays"], 100.0 * info["rays_occluded"] / max(info["rays"], 1)) if what == "direct" else
                           "%d shadow rays, %.1f %% occluded" % (info["shadow_rays"], 100.0 * info["shadow_rays_occluded"] / max(info["shadow_rays"], 1)))
        t_pt = min(pt_ms)
        # (ii) the variances at a sixteenth of the pixels
        ctx.resize(w // 4, h // 4)
        ctx.set_uniforms(host.make_uniforms(w // 4, h // 4, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        var = {}
        pt = []
        for b in range(BATCHES):
            ctx.clear_sum()
            ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=(b, 1))
            pt.append(result(ctx, "nee"))
        v_pt = summed_variance(pt)
        for what in ("direct", "nee"):
            for sl, sv in SAMPLINGS:
                for M in MS:
                    ctx.set_light_sampling(sv)
                    ctx.set_light_candidates(M)
                    batch = []
                    for b in range(BATCHES):
                        run_one(ctx, what, capi.WALK_AUTO, (b, 2 + M))
                        batch.append(result(ctx, what))
                    var[(what, sl, M)] = summed_variance(batch)
        # (iii) the table
        lines.append(" mpt_render, MPT_PIPE_AUTO: min %8.3f ms; summed variance at %dx%d, %d batches of %d spp, clamp 1: %.6g" % (
            t_pt, w // 4, h // 4, BATCHES, SPP, v_pt))
        for what in ("direct", "nee"):
            for wl, wv in WALKS:
                for sl, sv in SAMPLINGS:
                    lines.append(" %s, %s, %s sampling" % ("direct pass" if what == "direct" else "mpt_render_nee", wl, sl))
                    t1, v1 = min(ms[(what, wl, wv, sl, sv, 1)]), var[(what, sl, 1)]
                    for M in MS:
                        t, v = min(ms[(what, wl, wv, sl, sv, M)]), var[(what, sl, M)]
                        row = "   M %2d: min %8.3f ms (x %.2f)  variance %.6g (1 / %.2f)  variance x time, M = 1 over M: %.3f" % (
                            M, t, t / t1, v, v1 / v, (v1 * t1) / (v * t))
                        if what == "nee":
                            row += "  mpt_render over M: %.3f" % ((v_pt * t_pt) / (v * t))
                        lines.append(row + "   " + note[(what, wl, wv, sl, sv, M)])
        print("\n".join(lines[-(2 + 8 * (1 + len(MS))):]), flush=True)
    ctx.close()
    if a.bench:
        lines.append("")
        for r in range(a.bench):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, check=True).stdout
            j = json.loads(out.strip().splitlines()[-1])
            lines.append(" (iv) bench.py run %d: %s" % (r, json.dumps({k: j[k] for k in j if not isinstance(j[k], (dict, list))})))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
