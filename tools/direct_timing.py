"""Timing of the direct-lighting pass on one GPU (profiles/r11_direct.txt), HIP events throughout, both walks alternating in one process:
 (i)  mpt_direct_lighting at 1920x1080x16 on scene.xml, the Cornell box and bunny x20 (trees built on the device): the minimum and the
      median of REPS passes after WARMUP, rays per second, the occluded share of the rays and the skipped share of the samples;
 (ii) with --bench: bench.py's headline, RUNS times (the spread between the runs is what "unchanged" is judged by).
Usage: python tools/direct_timing.py [--out profiles/r11_direct.txt] [--bench RUNS] [--quick]"""
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
SCENES = (("scene.xml", None), ("cornell.xml", CORNELL_CAM), ("bunny20.xml", None))
W, H, N = 1920, 1080, 16
REPS, WARMUP = 10, 3


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return "min %8.3f  median %8.3f  max %8.3f ms" % (ms[0], ms[len(ms) // 2], ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--quick", action="store_true", help="640x360 (a dry run of the tool itself)")
    a = ap.parse_args()
    w, h = (640, 360) if a.quick else (W, H)
    lines = ["direct_timing: %dx%dx%d, %d timed passes after %d warm-up passes, build %s" % (
        w, h, N, REPS, WARMUP, capi.build_id()["source_sha256"][:16])]
    ctx = capi.Context(0)
    for name, cam in SCENES:
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        ctx.resize(w, h)
        ctx.set_uniforms(host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        acc, lights = ctx.accel_info(), ctx.light_info()
        lines.append("")
        lines.append("%s: %d primitives, %d lights (%d triangles, %d spheres), MPT_WALK_AUTO = %s" % (
            name, sc.getPrimitiveCount(), lights["lights"], lights["triangle_lights"], lights["sphere_lights"],
            "own" if acc["auto_pipeline"] == capi.PIPE_ORDERED else "reference"))
        res = {capi.WALK_REFERENCE: [], capi.WALK_OWN: []}
        info = {}
        for r in range(WARMUP + REPS):
            for walk in res:
                info[walk] = ctx.direct_lighting(samples=N, seed=(1, 0), walk=walk)
                if r >= WARMUP:
                    res[walk].append(info[walk]["device_ms"])
        for walk, label in ((capi.WALK_REFERENCE, "reference order"), (capi.WALK_OWN, "own tree")):
            best, i = float(np.min(res[walk])), info[walk]
            lines.append(" (i) mpt_direct_lighting %dx%dx%d, %-16s %s  %.2f Grays/s at the minimum (%d rays, %.1f %% occluded; %.1f %% of %d samples skipped)" % (
                w, h, N, label + ":", stats(res[walk]), i["rays"] / best / 1e6, i["rays"], 100.0 * i["rays_occluded"] / max(i["rays"], 1),
                100.0 * (1.0 - i["rays"] / max(i["pixels_surface"] * N, 1)), i["pixels_surface"] * N))
        print("\n".join(lines[-4:]), flush=True)
    ctx.close()
    if a.bench:
        lines.append("")
        for r in range(a.bench):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, check=True).stdout
            j = json.loads(out.strip().splitlines()[-1])
            lines.append(" (ii) bench.py run %d: %s" % (r, json.dumps({k: j[k] for k in j if not isinstance(j[k], (dict, list))})))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
