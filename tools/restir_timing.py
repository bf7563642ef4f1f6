"""Timing and variance of spatial reservoir reuse in the direct pass on one GPU (profiles/r24_restir.txt), HIP events throughout, the
variants alternating in one process (the method of tools/nee_timing.py and DESIGN.md §19):
 (i)   Cornell box 1024x1024 and scene.xml 1920x1080, 16 rounds, MPT_WALK_AUTO: the device time of mpt_direct_lighting with m = 1 and
       m = 8 candidates and of mpt_direct_restir with m in (1, 8), K in (2, 4, 8), R in (4, 8, 16) in both modes — the minimum of REPS
       runs after WARMUP — with the rays of a run by kind;
 (ii)  the variance of every variant on the same workloads at a sixteenth of the pixels: BATCHES calls of 16 rounds with different
       seeds, the per-pixel variance of the batch images (the scalar is the mean of the three channels), summed over the pixels where
       the m = 8 direct pass has a variance; and the image mean over all batches (the biased mode's darkening shows there);
 (iii) variance x time of the m = 8 direct pass (RIS alone) over that of each variant: > 1, the variant wins per unit of noise;
 (iv)  with --bench RUNS [--parent DIR]: bench.py's headline, RUNS times, alternating with the bench.py of DIR, a built checkout of the
       commit before.
Usage: python tools/restir_timing.py [--out profiles/r24_restir.txt] [--bench RUNS] [--parent DIR] [--quick]"""
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
ROUNDS = 16
REPS, WARMUP = 10, 3
BATCHES = 32
MS, KS, RS = (1, 8), (2, 4, 8), (4, 8, 16)
MODES = ((capi.RESTIR_UNBIASED, "unbiased"), (capi.RESTIR_BIASED, "biased"))


def variants():
    """(label, m, None | (K, R, mode)) of every variant, the two direct passes first."""
    v = [("direct m=%d" % m, m, None) for m in MS]
    for m in MS:
        for K in KS:
            for R in RS:
                for mode, word in MODES:
                    v.append(("restir m=%d K=%d R=%-2d %s" % (m, K, R, word), m, (K, R, mode)))
    return v


def run(ctx, m, reuse, seed):
    """One call of a variant; returns (device ms, a note on its rays)."""
    ctx.set_light_candidates(m)
    if reuse is None:
        info = ctx.direct_lighting(samples=ROUNDS, seed=seed, walk=capi.WALK_AUTO)
        return info["device_ms"], "%d rays, %.1f %% occluded" % (info["rays"], 100.0 * info["rays_occluded"] / max(info["rays"], 1))
    K, R, mode = reuse
    info = ctx.direct_restir(samples=ROUNDS, seed=seed, walk=capi.WALK_AUTO, neighbours=K, radius=R, mode=mode)
    rays = info["rays_initial"] + info["rays_final"] + info["rays_correction"]
    return info["device_ms"], "%d rays = %d initial + %d final + %d correction, %.1f %% occluded, %.2f of %d neighbours accepted, %.1f %% of the rounds took a neighbour's sample" % (
        rays, info["rays_initial"], info["rays_final"], info["rays_correction"], 100.0 * info["rays_occluded"] / max(rays, 1),
        info["neighbours_accepted"] / max(info["pixels_surface"] * ROUNDS, 1), K, 100.0 * info["samples_from_neighbours"] / max(info["pixels_surface"] * ROUNDS, 1))


def image(ctx, reuse):
    rgba = ctx.read_direct()[0] if reuse is None else ctx.read_restir()[0]
    return rgba[..., :3].mean(-1, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--parent", default=None, help="a built checkout of the commit before: its bench.py alternates with this one's")
    ap.add_argument("--quick", action="store_true", help="a quarter of the width and height, 3 + 1 runs, 8 batches (a dry run of the tool itself)")
    a = ap.parse_args()
    reps, warmup, batches = (3, 1, 8) if a.quick else (REPS, WARMUP, BATCHES)
    lines = ["restir_timing: %d rounds, MPT_WALK_AUTO, %d timed runs after %d warm-up runs, %d batches, build %s" % (
        ROUNDS, reps, warmup, batches, capi.build_id()["source_sha256"][:16])]
    ctx = capi.Context(0)
    V = variants()
    for name, cam, w, h in WORKLOADS:
        if a.quick:
            w, h = w // 4, h // 4
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        ctx.resize(w, h)
        ctx.set_uniforms(host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        lines.append("")
        lines.append("%s %dx%d, %d rounds: %d primitives, %d lights" % (name, w, h, ROUNDS, sc.getPrimitiveCount(), ctx.light_info()["lights"]))
        ms = {label: [] for label, _, _ in V}
        note = {}
        for r in range(warmup + reps):
            for label, m, reuse in V:
                t, note[label] = run(ctx, m, reuse, (1, 0))
                if r >= warmup:
                    ms[label].append(t)
        ws, hs = max(w // 4, 1), max(h // 4, 1)
        ctx.resize(ws, hs)
        ctx.set_uniforms(host.make_uniforms(ws, hs, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        var, mean = {}, {}
        for i, (label, m, reuse) in enumerate(V):
            x = np.empty((batches, hs, ws), np.float64)
            for b in range(batches):
                run(ctx, m, reuse, (b, 100 + i))
                x[b] = image(ctx, reuse)
            var[label], mean[label] = x.var(0, ddof=1), float(x.mean())
        base = "direct m=8"
        lit = var[base] > 0
        t0, v0 = min(ms[base]), float(var[base][lit].sum())
        lines.append(" variance at %dx%d over %d pixels; vt = (variance x time of %s) / (variance x time of the variant)" % (ws, hs, int(lit.sum()), base))
        for label, _, _ in V:
            t, v = min(ms[label]), float(var[label][lit].sum())
            lines.append(" %-30s min %8.3f median %8.3f ms   sum var %.6e   image mean %.6f   vt %6.3f   %s" % (
                label, t, float(np.median(ms[label])), v, mean[label], (v0 * t0) / (v * t) if v > 0 else float("nan"), note[label]))
        print("\n".join(lines[-(len(V) + 2):]), flush=True)
    ctx.close()
    if a.bench:
        lines.append("")
        for r in range(a.bench):
            for who, root in (("parent", a.parent), ("this build", ROOT)):
                if not root:
                    continue
                out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
                                      "--no-extra-workloads"], capture_output=True, text=True, check=True, cwd=root, timeout=600).stdout
                j = json.loads(out.strip().splitlines()[-1])
                lines.append(" bench.py --steps 10 --warmup 3 (headline only), run %d, %s: %s" % (
                    r, who, json.dumps({k: j[k] for k in j if not isinstance(j[k], (dict, list))})))
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
