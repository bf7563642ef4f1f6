"""Timing of the shadow-ray kernels on one GPU (profiles/r10_ao.txt), HIP events throughout, variants alternating in one process:
 (i)   the any-hit kernel against the closest-hit kernel of the same tree (k_trace_rays / k_trace_rays_ordered) on the SAME 2 M AO-style
       rays — origins and Lambert directions of mpt_ambient_occlusion's own samples, from the first hits of a 1920x1080 view — for
       scene.xml, the Cornell box and bunny x20, with no limit and with a limit of RADIUS (mpt_time_trace: 3 warm-up rounds, 20 timed);
 (ii)  mpt_ambient_occlusion at 1920x1080x16 on the three scenes, both walks alternating, in ms and rays/s, with the share of rays
       the own-tree walk hands to the reference-order walk;
 (iii) with --bench: bench.py's headline, RUNS times (the spread between the runs is what "unchanged" is judged by).
Usage: python tools/ao_timing.py [--out profiles/r10_ao.txt] [--bench RUNS] [--quick]"""
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

CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
SCENES = (("scene.xml", None), ("cornell.xml", CORNELL_CAM), ("bunny20.xml", None))
W, H, N = 1920, 1080, 16
RADIUS = {"scene.xml": 2.0, "cornell.xml": 0.25, "bunny20.xml": 2.0}
REPS, WARMUP = 20, 3


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return "min %8.3f  median %8.3f  max %8.3f ms" % (ms[0], ms[len(ms) // 2], ms[-1])


def ao_rays(ctx, u, n_rays):
    """n_rays AO-style rays of the view: the pass's own origins and directions (tests/ao_ref.py), two samples per surface pixel."""
    import ao_ref
    ad, nc, _ = ctx.read_aovs()
    surface, o, d = ao_ref.sample_rays(ad, nc, u, 0, 2, seed=(1, 0))
    d = d[surface].reshape(-1, 3)
    o = np.repeat(o[surface], 2, axis=0)
    keep = ~np.isnan(d).any(-1)
    o, d = o[keep], d[keep]
    reps = -(-n_rays // o.shape[0])
    return np.tile(o, (reps, 1))[:n_rays], np.tile(d, (reps, 1))[:n_rays]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="a tenth of the rays, 640x360 (a dry run of the tool itself)")
    a = ap.parse_args()
    n_rays = 200_000 if a.quick else 2_000_000
    w, h = (640, 360) if a.quick else (W, H)
    lines = ["ao_timing: %d rays, %dx%dx%d, %d timed repetitions after %d warm-up rounds, build %s" % (
        n_rays, w, h, N, REPS, WARMUP, capi.build_id()["source_sha256"][:16])]
    ctx = capi.Context(0)
    for name, cam in SCENES:
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        u = host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam)
        ctx.resize(w, h)
        ctx.set_uniforms(u)
        info = ctx.accel_info()
        lines.append("")
        lines.append("%s: %d primitives, own tree %s, MPT_WALK_AUTO = %s" % (
            name, sc.getPrimitiveCount(), "yes" if info["ordered_ok"] else "no", "own" if info["auto_pipeline"] == capi.PIPE_ORDERED else "reference"))
        o, d = ao_rays(ctx, u, n_rays)
        for tmax in (None, RADIUS[name]):
            ms = ctx.time_trace(o, d, tmax, warmup=WARMUP, reps=REPS)
            occ, flags = ctx.trace_occluded(o, d, tmax, walk=capi.WALK_OWN)
            lines.append(" (i) %d AO-style rays, tmax %s: %.1f %% occluded; own walk hands %.3f %% to the reference-order walk (%.3f %% stack overflow)" % (
                n_rays, "+inf" if tmax is None else "%g" % tmax, 100 * occ.mean(), 100 * (flags != 0).mean(), 100 * ((flags & 8) != 0).mean()))
            for k, label in enumerate(("closest hit, reference order (k_trace_rays)", "any hit,     reference order (k_occluded_ref)",
                                       "closest hit, own tree (k_trace_rays_ordered)", "any hit,     own tree (k_occluded_own)")):
                lines.append("     %-46s %s" % (label, stats(ms[:, k])))
            lines.append("     any hit / closest hit, medians: reference order %.3f, own tree %.3f" % (
                np.median(ms[:, 1]) / np.median(ms[:, 0]), np.median(ms[:, 3]) / max(np.median(ms[:, 2]), 1e-9)))
        res = {capi.WALK_REFERENCE: [], capi.WALK_OWN: []}
        for r in range(WARMUP + REPS):
            for walk in res:
                i = ctx.ambient_occlusion(samples=N, radius=0.0, seed=(1, 0), walk=walk)
                if r >= WARMUP:
                    res[walk].append(i["device_ms"])
        for walk, label in ((capi.WALK_REFERENCE, "reference order"), (capi.WALK_OWN, "own tree")):
            med = float(np.median(res[walk]))
            lines.append(" (ii) mpt_ambient_occlusion %dx%dx%d, no limit, %-15s %s  %.2f Grays/s (%d rays, %.1f %% occluded)" % (
                w, h, N, label + ":", stats(res[walk]), i["rays"] / med / 1e6, i["rays"], 100.0 * i["rays_occluded"] / max(i["rays"], 1)))
        print("\n".join(lines[-16:]), flush=True)
    ctx.close()
    if a.bench:
        lines.append("")
        vals = []
        for r in range(a.bench):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, check=True).stdout
            j = json.loads(out.strip().splitlines()[-1])
            vals.append(j)
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
