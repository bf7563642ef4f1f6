#!/usr/bin/env python3
"""CPU sweep of the four defaults of mpt_temporal_params over the three calibration paths of tests/temporal_ref.py (oracle renders,
the numpy restatement; no GPU).  Per setting: F = MSE(last 1-spp frame) / MSE(last history) against 1024 spp, and the share of the
last frame that lost its history.  Writes profiles/r07_temporal_sweep.txt.

    python tools/temporal_sweep.py [--out profiles/r07_temporal_sweep.txt] [--threads 16]
"""
import argparse
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import temporal_ref as tr  # noqa: E402
from conftest import oracle_scene  # noqa: E402

MAX_HISTORY = (8, 16, 32, 64)
DEPTH_TOL = (0.005, 0.02, 0.05, 0.1)
NORMAL_THR = (0.25, 0.5, 0.7, 0.9, 0.97)
MIN_WEIGHT = (0.01, 0.05, 0.25, 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_temporal_sweep.txt"))
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    names = list(tr.PATHS)
    paths = {}
    for n in names:
        sc, buf = oracle_scene(n)
        paths[n] = tr.oracle_path(n, sc, buf, threads=a.threads)
    lines = ["# temporal accumulation: sweep of the defaults (tools/temporal_sweep.py; oracle + numpy restatement, CPU)",
             "# paths: %d frames of 1 spp, %s; F = MSE(last frame) / MSE(last history) against 1024 spp; reset = share of the last frame"
             % (tr.PATH_FRAMES, ", ".join("%s %dx%d step %s" % (n, tr.PATHS[n]["W"], tr.PATHS[n]["H"], tr.PATHS[n]["step"]) for n in names)),
             "# max_history depth_tol normal_thr min_weight | " + " | ".join("%s F reset%%" % n for n in names) + " | geometric mean F"]
    rows = []
    for mh, zt, nt, mw in itertools.product(MAX_HISTORY, DEPTH_TOL, NORMAL_THR, MIN_WEIGHT):
        res = [tr.run_path(paths[n][0], paths[n][1], max_history=mh, depth_tolerance=zt, normal_threshold=nt, min_weight=mw)[:2] for n in names]
        gm = float(np.exp(np.mean([np.log(f) for f, _ in res])))
        rows.append(((mh, zt, nt, mw), res, gm))
        lines.append("%3d %6.3f %5.2f %5.2f | " % (mh, zt, nt, mw) + " | ".join("%7.2f %5.2f" % (f, 100 * r) for f, r in res) + " | %7.2f" % gm)
    ok = [r for r in rows if all(f >= 5 and s <= 0.05 for f, s in r[1])]
    best = max(ok, key=lambda r: r[2])
    lines.append("# best geometric mean among the settings with F >= 5 and reset <= 5 %% on every path: max_history %d depth_tolerance %g "
                 "normal_threshold %g min_weight %g (%.2f)" % (best[0] + (best[2],)))
    d = tr.DEFAULTS
    chosen = [r for r in rows if r[0] == (d["max_history"], d["depth_tolerance"], d["normal_threshold"], d["min_weight"])]
    if chosen:
        lines.append("# the defaults of include/mpt.h: max_history %d depth_tolerance %g normal_threshold %g min_weight %g: " % chosen[0][0]
                     + ", ".join("%s F %.2f reset %.2f %%" % (n, f, 100 * s) for n, (f, s) in zip(names, chosen[0][1])))
        lines += ["# The best row sits on the loose edge of every axis: on these slow paths the mean squared error rewards every kept",
                  "# sample and cannot see ghosting.  So each default moved from the prototype's (32, 0.02, 0.9, 0.05) only where the gain",
                  "# is large and stopped short of the edge: depth_tolerance 0.02 -> 0.05 (+9..32 %; 0.1 adds < 4 %), normal_threshold",
                  "# 0.9 -> 0.5 (+43 % on the bunnies, whose shading normals turn fast; 0.25 would accept taps across 75-degree creases),",
                  "# min_weight stays 0.05 (0.01 lets a pixel take its whole history from a tap almost a pixel away), max_history stays 32",
                  "# (64 cannot differ on 24 frames)."]
    open(a.out, "w").write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
