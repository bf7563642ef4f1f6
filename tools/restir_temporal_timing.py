"""Timing and variance of temporal reservoir reuse in the direct pass on one GPU (profiles/r29_restir_temporal.txt), HIP events
throughout, the variants alternating in one process (the method of tools/restir_timing.py and DESIGN.md §19, §20):
 (i)   Cornell box 1024x1024 and scene.xml 1920x1080, MPT_WALK_AUTO: the device time of ONE frame — mpt_direct_lighting with N = 1 and
       m in (1, 8) candidates, and mpt_direct_restir_temporal with m in (1, 8), C in (5, 20, 64) in both modes, as the second frame of a
       history, once after a camera step of tests/temporal_ref.py's PATHS (a reprojected tap) and once under the same camera (the tap is
       the pixel itself) — the minimum of REPS runs after WARMUP, with the rays of the frame by kind;
 (ii)  the variance of every variant on the same workloads at a sixteenth of the pixels: BATCHES histories with different seeds, each
       played from frame 0 to frame 24 of the path (and of a still camera), the per-pixel variance of the LAST frame's images (the
       scalar is the mean of the three channels), summed over the pixels where the m = 8 direct pass has a variance; and the image mean;
 (iii) variance x time of the m = 8, N = 1 direct pass (RIS alone) over that of each variant: > 1, the variant wins per unit of noise;
 (iv)  with --bench RUNS [--parent DIR]: bench.py's headline, RUNS times, alternating with the bench.py of DIR, a built checkout of the
       commit before.
Usage: python tools/restir_temporal_timing.py [--out profiles/r29_restir_temporal.txt] [--bench RUNS] [--parent DIR] [--quick]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from metalpathtracer_amd import capi, host  # noqa: E402
import temporal_ref  # noqa: E402  (the calibration paths and their cameras)

WORKLOADS = (("cornell.xml", 1024, 1024), ("scene.xml", 1920, 1080))
LAST = temporal_ref.PATH_FRAMES            # frame 24: the frame whose variance is taken
REPS, WARMUP = 10, 3
BATCHES = 32
MS, CS = (1, 8), (5, 20, 64)
MODES = ((capi.RESTIR_UNBIASED, "unbiased"), (capi.RESTIR_BIASED, "biased"))


def variants():
    """(label, m, None | (C, mode)) of every variant, the two direct passes first."""
    v = [("direct N=1 m=%d" % m, m, None) for m in MS]
    for m in MS:
        for C_ in CS:
            for mode, word in MODES:
                v.append(("temporal m=%d C=%-2d %s" % (m, C_, word), m, (C_, mode)))
    return v


def cameras(name, sc, w, h, still):
    P = temporal_ref.PATHS[name]
    cam0 = P["cam"] or host.camera_reset()
    return [host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=temporal_ref.path_camera(cam0, 0 if still else f, P["step"]))
            for f in range(LAST + 1)]


def play(ctx, us, m, reuse, seed, frames):
    """The frames `frames` of a variant from no history (the direct pass: the last of them alone); returns the last call's info."""
    ctx.set_light_candidates(m)
    if reuse is None:
        ctx.set_uniforms(us[frames[-1]])
        return ctx.direct_lighting(samples=1, sample_begin=frames[-1], seed=seed, walk=capi.WALK_AUTO)
    C_, mode = reuse
    ctx.restir_temporal_reset()
    for f in frames:
        ctx.set_uniforms(us[f])
        info = ctx.direct_restir_temporal(frame=f, seed=seed, walk=capi.WALK_AUTO, mode=mode, max_history=C_)
    return info


def note_of(info, reuse):
    if reuse is None:
        return "%d rays, %.1f %% occluded" % (info["rays"], 100.0 * info["rays_occluded"] / max(info["rays"], 1))
    rays = info["rays_initial"] + info["rays_final"] + info["rays_correction"]
    n = max(info["pixels_surface"], 1)
    return "%d rays = %d initial + %d final + %d correction, %.1f %% occluded, %.1f %% of the surface pixels accepted their tap, %.1f %% took the history's sample" % (
        rays, info["rays_initial"], info["rays_final"], info["rays_correction"], 100.0 * info["rays_occluded"] / max(rays, 1),
        100.0 * info["history_accepted"] / n, 100.0 * info["samples_from_history"] / n)


def image(ctx, reuse):
    rgba = ctx.read_direct()[0] if reuse is None else ctx.read_restir_temporal()[0]
    return rgba[..., :3].mean(-1, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--parent", default=None, help="a built checkout of the commit before: its bench.py alternates with this one's")
    ap.add_argument("--quick", action="store_true", help="a quarter of the width and height, 3 + 1 runs, 4 batches (a dry run of the tool itself)")
    a = ap.parse_args()
    reps, warmup, batches = (3, 1, 4) if a.quick else (REPS, WARMUP, BATCHES)
    lines = ["restir_temporal_timing: one frame, MPT_WALK_AUTO, %d timed runs after %d warm-up runs, %d batches of %d frames, build %s" % (
        reps, warmup, batches, LAST + 1, capi.build_id()["source_sha256"][:16])]
    ctx = capi.Context(0)
    V = variants()
    for name, w, h in WORKLOADS:
        if a.quick:
            w, h = w // 4, h // 4
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        ctx.resize(w, h)
        lines.append("")
        lines.append("%s %dx%d: %d primitives" % (name, w, h, sc.getPrimitiveCount()))
        ms = {(label, still): [] for label, _, _ in V for still in (False, True)}
        note = {}
        for still in (False, True):
            us = cameras(name, sc, w, h, still)
            for r in range(warmup + reps):
                for label, m, reuse in V:
                    info = play(ctx, us, m, reuse, (1, 0), (LAST - 1, LAST))
                    note[(label, still)] = note_of(info, reuse)
                    if r >= warmup:
                        ms[(label, still)].append(info["device_ms"])
        ws, hs = max(w // 4, 1), max(h // 4, 1)
        ctx.resize(ws, hs)
        base = "direct N=1 m=8"
        for still in (False, True):
            us = cameras(name, sc, ws, hs, still)
            var, mean = {}, {}
            for i, (label, m, reuse) in enumerate(V):
                x = np.empty((batches, hs, ws), np.float64)
                for b in range(batches):
                    play(ctx, us, m, reuse, (b, 100 + i), range(LAST + 1))
                    x[b] = image(ctx, reuse)
                var[label], mean[label] = x.var(0, ddof=1), float(x.mean())
            lit = var[base] > 0
            t0, v0 = min(ms[(base, still)]), float(var[base][lit].sum())
            lines.append(" %s: frame %d, variance at %dx%d over %d pixels; vt = (variance x time of %s) / (variance x time of the variant)" % (
                "still camera" if still else "the path of tests/temporal_ref.py", LAST, ws, hs, int(lit.sum()), base))
            for label, _, _ in V:
                t, v = min(ms[(label, still)]), float(var[label][lit].sum())
                lines.append("  %-30s min %7.3f median %7.3f ms   sum var %.6e   image mean %.6f   vt %6.3f   %s" % (
                    label, t, float(np.median(ms[(label, still)])), v, mean[label], (v0 * t0) / (v * t) if v > 0 else float("nan"), note[(label, still)]))
            print("\n".join(lines[-(len(V) + 1):]), flush=True)
    ctx.close()
    if a.bench:
        lines.append("")
        for r in range(a.bench):
            for who, root in (("parent", a.parent), ("this build", ROOT)):
                if not root:
                    continue
                root = os.path.abspath(root)
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
