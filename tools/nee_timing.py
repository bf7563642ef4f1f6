"""Timing of the next-event-estimation render on one GPU (profiles/r12_nee.txt), HIP events throughout, the variants alternating in one
process:
 (i)   Cornell box 1024x1024x16 spp at depth 8 and scene.xml 1920x1080x16 spp at depth 8: the trace-kernel time of mpt_render at
       MPT_PIPE_AUTO, of mpt_render at MPT_PIPE_MEGAKERNEL (the comparable mapping: one lane per path, no rings) and of mpt_render_nee
       with both walks — the minimum and the median of REPS runs after WARMUP — with the rays and shadow rays of a run;
 (ii)  the variance of the two estimators on the same workloads at a sixteenth of the pixels: BATCHES renders of 16 spp with different
       seeds each, the per-pixel variance of the batch means (the scalar is the mean of the three channels), mpt_render against
       mpt_render_nee with the same per-sample clamp (1) — the mean over the pixels of s2_pt / s2_nee where both are positive, and the
       ratio of the summed variances; variance x time is the product of that and (i);
 (iii) the same ratio on the scene of tests/test_gpu_nee.py (the Cornell box with emissionPower 1 and a black light, 32x32, depth 4,
       64 x 64 spp, no clamp);
 (iv)  with --bench: bench.py's headline, RUNS times.
Usage: python tools/nee_timing.py [--out profiles/r12_nee.txt] [--bench RUNS] [--quick]"""
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


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return "min %8.3f  median %8.3f ms" % (ms[0], ms[len(ms) // 2])


def variance_ratio(ctx, batches, spp, depth, clamp):
    """(mean over pixels of s2_pt / s2_nee, ratio of the summed variances, pixels) from `batches` renders of `spp` samples each."""
    H, W = ctx.height, ctx.width
    pt = np.empty((batches, H, W), np.float64)
    ne = np.empty_like(pt)
    for b in range(batches):
        ctx.clear_sum()
        ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=depth, sample_count=spp, seed=(b, 1))
        pt[b] = ctx.read_sum()[..., :3].mean(-1, dtype=np.float64) / spp
        ctx.clear_sum()
        ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=depth, sample_count=spp, seed=(b, 2), walk=capi.WALK_AUTO, clamp=clamp)
        ne[b] = ctx.read_sum()[..., :3].mean(-1, dtype=np.float64) / spp
    v_pt, v_ne = pt.var(0, ddof=1), ne.var(0, ddof=1)
    both = (v_pt > 0) & (v_ne > 0)
    return float((v_pt[both] / v_ne[both]).mean()), float(v_pt[both].sum() / v_ne[both].sum()), int(both.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="a quarter of the width and height (a dry run of the tool itself)")
    a = ap.parse_args()
    lines = ["nee_timing: %d spp at depth %d, %d timed runs after %d warm-up runs, build %s" % (SPP, DEPTH, REPS, WARMUP, capi.build_id()["source_sha256"][:16])]
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
        lines.append("%s %dx%dx%d: %d primitives, %d lights, MPT_PIPE_AUTO / MPT_WALK_AUTO = %s" % (
            name, w, h, SPP, sc.getPrimitiveCount(), lights["lights"], "own tree" if acc["auto_pipeline"] == capi.PIPE_ORDERED else "reference order"))
        kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=(1, 0))
        variants = (("mpt_render, MPT_PIPE_AUTO", lambda: ctx.render(pipeline=capi.PIPE_AUTO, **kw)),
                    ("mpt_render, MPT_PIPE_MEGAKERNEL", lambda: ctx.render(pipeline=capi.PIPE_MEGAKERNEL, **kw)),
                    ("mpt_render_nee, reference order", lambda: ctx.render_nee(walk=capi.WALK_REFERENCE, clamp=1.0, **kw)),
                    ("mpt_render_nee, own tree", lambda: ctx.render_nee(walk=capi.WALK_OWN, clamp=1.0, **kw)))
        ms = {label: [] for label, _ in variants}
        note = {}
        for r in range(WARMUP + REPS):
            for label, run in variants:
                ctx.clear_sum()
                ctx.reset_stats()
                info = run()
                s = ctx.stats()
                if r >= WARMUP:
                    ms[label].append(s["trace_kernel_ms"])
                note[label] = "%d rays" % s["rays"] + (", %d shadow rays (%.1f %% occluded)" % (
                    info["shadow_rays"], 100.0 * info["shadow_rays_occluded"] / max(info["shadow_rays"], 1)) if info else "")
        for label, _ in variants:
            lines.append(" (i)  %-34s %s   %s" % (label + ":", stats(ms[label]), note[label]))
        ctx.resize(w // 4, h // 4)
        ctx.set_uniforms(host.make_uniforms(w // 4, h // 4, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        mean_ratio, sum_ratio, n = variance_ratio(ctx, BATCHES, SPP, DEPTH, 1.0)
        t_pt, t_ne = min(ms["mpt_render, MPT_PIPE_AUTO"]), min(min(ms["mpt_render_nee, reference order"]), min(ms["mpt_render_nee, own tree"]))
        lines.append(" (ii) variance at %dx%d, %d batches of %d spp, both clamped at 1: mean of s2_pt / s2_nee %.3f, summed variances %.3f (%d pixels)" % (
            w // 4, h // 4, BATCHES, SPP, mean_ratio, sum_ratio, n))
        lines.append("      time nee / pt %.2f at the minima; variance x time, pt / nee (> 1: NEE wins per unit of noise): %.3f" % (
            t_ne / t_pt, sum_ratio * t_pt / t_ne))
        print("\n".join(lines[-7:]), flush=True)
    # (iii) the scene of the statistical test
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", "cornell.xml"), sc)
    assert st == 0, log
    sc.buildBVH()
    buf = sc.buffers()
    mats = np.array(buf[2], np.float32).reshape(-1, 2, 4)
    lit = mats[:, 1, 3] > 0
    mats[lit, 1, 3] = 1.0
    mats[lit, 0, :3] = 0.0
    ctx.upload_scene(buf[0], buf[1], mats, buf[3])
    ctx.resize(32, 32)
    ctx.set_uniforms(host.make_uniforms(32, 32, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=CORNELL_CAM))
    mean_ratio, sum_ratio, n = variance_ratio(ctx, 64, 64, 4, 0.0)
    lines.append("")
    lines.append(" (iii) Cornell box, emissionPower 1, black light, 32x32, depth 4, 64 batches of 64 spp, no clamp: mean of s2_pt / s2_nee %.3f, "
                 "summed variances %.3f (%d pixels)" % (mean_ratio, sum_ratio, n))
    print(lines[-1], flush=True)
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
