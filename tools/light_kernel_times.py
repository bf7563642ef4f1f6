#!/usr/bin/env python3
"""Kernel times of every light-sampling kernel of ONE library build (MPT_LIB picks it), for comparing builds whose kernels should be the
same (tools/codeobj_compare.py says whether their code is): run it for the build before, the build after and the build before again
in one session — the two runs of the same build give the noise.

nee_timing.py's workloads and settings (Cornell box 1024x1024 and scene.xml 1920x1080, 16 samples, depth 8, HIP events, every variant once
per round, the minimum of --reps rounds, 10 by default, after 3 warm-up rounds): the direct pass and mpt_render_nee with both walks, both light samplings and
1 and 4 candidates (k_direct*, k_direct_ris*, k_nee*, k_nee_ris*), and mpt_render_nee_adaptive at threshold 0 with N = 16 and one
candidate (k_nee_adaptive*).  One line per variant: `name  min_ms`; --json FILE writes {name: min_ms} too.

Usage: MPT_LIB=path/to/libmpt_hip.so python tools/light_kernel_times.py [--json FILE] [--reps N] [--quick]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metalpathtracer_amd import capi, host  # noqa: E402

CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
WORKLOADS = (("cornell.xml", CORNELL_CAM, 1024, 1024), ("scene.xml", None, 1920, 1080))
SPP, DEPTH = 16, 8
REPS, WARMUP = 10, 3
MS = (1, 4)
WALKS = (("ref", capi.WALK_REFERENCE), ("own", capi.WALK_OWN))
SAMPLINGS = (("area", capi.LIGHT_SAMPLING_AREA), ("cone", capi.LIGHT_SAMPLING_CONE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=REPS, help="timed rounds (default %d)" % REPS)
    ap.add_argument("--quick", action="store_true", help="a quarter of the width and height (a dry run of the tool itself)")
    a = ap.parse_args()
    print("light_kernel_times: library %s, build %s" % (capi.LIB_PATH, capi.build_id()["source_sha256"][:16]), flush=True)
    ctx = capi.Context(0)
    best = {}
    for name, cam, w, h in WORKLOADS:
        if a.quick:
            w, h = w // 4, h // 4
        sc = host.Scene()
        st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", name), sc)
        assert st == 0, log
        host.make_ready(ctx, sc, host.BVH_DEVICE)
        ctx.resize(w, h)
        ctx.set_uniforms(host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        variants = [(what, wl, wv, sl, sv, M) for what in ("direct", "nee", "adaptive") for wl, wv in WALKS for sl, sv in SAMPLINGS
                    for M in (MS if what != "adaptive" else (1,))]
        ms = {v: [] for v in variants}
        for r in range(WARMUP + a.reps):
            for v in variants:
                what, _, wv, _, sv, M = v
                ctx.set_light_sampling(sv)
                ctx.set_light_candidates(M)
                if what == "direct":
                    t = ctx.direct_lighting(samples=SPP, seed=(1, 0), walk=wv)["device_ms"]
                elif what == "nee":
                    ctx.clear_sum()
                    t = ctx.render_nee(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=(1, 0), walk=wv, clamp=1.0)["device_ms"]
                else:
                    t = ctx.render_nee_adaptive(0.0, rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, sample_count=SPP, seed=(1, 0), walk=wv,
                                                clamp=1.0)["nee"]["device_ms"]
                if r >= WARMUP:
                    ms[v].append(t)
        for v in variants:
            what, wl, _, sl, _, M = v
            key = "%s %s %s %s M%d" % (name, what, wl, sl, M)
            best[key] = min(ms[v])
            print("%-44s %9.4f" % (key, best[key]), flush=True)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(best, f, indent=1)


if __name__ == "__main__":
    main()
