#!/usr/bin/env python3
"""CPU sweep of the filter defaults of mpt_svgf_params over the three calibration paths of tests/temporal_ref.py (oracle renders, the
numpy restatement tests/svgf_ref.py; no GPU).  Step A's four parameters stay at the temporal defaults.  Per setting:
F = MSE(last raw 1-spp frame) / MSE(last filtered frame) against 1024 spp, per path and as geometric mean; next to them two baselines
from the restatements the tree already had: F_hist (the unfiltered history of temporal_ref.run_path) and F_dt (that history through
denoise_ref with the mpt_denoise defaults: what --temporal --denoise gives).  Writes the table of profiles/r08_svgf_sweep.txt; the
reasoning under the table of that file is written by hand and has to be revisited when the table changes.

    python tools/svgf_sweep.py [--out profiles/r08_svgf_sweep.txt] [--threads 16] [--cache FILE.pkl]
"""
import argparse
import itertools
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import denoise_ref as dr  # noqa: E402
import svgf_ref as sr  # noqa: E402
import temporal_ref as tr  # noqa: E402

ITERATIONS = (1, 2, 3, 4, 5)
SIGMA_L = (1.0, 2.0, 4.0, 8.0)
SIGMA_N = (32.0, 128.0)
SIGMA_Z = (0.25, 1.0)
FEEDBACK = (0, 1)


def baselines(frames, hi):
    """(F_hist, F_dt) of a path: the parent's history, and that history through the parent's filter with its defaults."""
    f_hist, _, hist = tr.run_path(frames, hi)
    _, c, ad, nc = frames[-1]
    return f_hist, tr.mse(c, hi) / tr.mse(dr.denoise(hist, ad, nc), hi)


def load_paths(threads, cache=None):
    if cache and os.path.exists(cache):
        with open(cache, "rb") as f:
            return pickle.load(f)
    from conftest import oracle_scene
    from oracle import binding as ob
    paths = {}
    for n in tr.PATHS:
        sc, buf = oracle_scene(n)
        frames, hi = tr.oracle_path(n, sc, buf, threads=threads)
        paths[n] = ([(bytes(u), c, ad, nc) for u, c, ad, nc in frames], hi)
    if cache:
        with open(cache, "wb") as f:
            pickle.dump(paths, f)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_svgf_sweep.txt"))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cache", default=None, help="keep the oracle frames in this file between runs")
    a = ap.parse_args()
    from oracle import binding as ob
    names = list(tr.PATHS)
    paths = {n: ([(ob.Uniforms.from_buffer_copy(u), c, ad, nc) for u, c, ad, nc in fr], hi)
             for n, (fr, hi) in load_paths(a.threads, a.cache).items()}
    base = {n: baselines(*paths[n]) for n in names}
    lines = ["# SVGF: sweep of the filter defaults (tools/svgf_sweep.py; oracle + numpy restatement, CPU)",
             "# paths: %d frames of 1 spp, %s; step A at the temporal defaults" % (tr.PATH_FRAMES, ", ".join(
                 "%s %dx%d step %s" % (n, tr.PATHS[n]["W"], tr.PATHS[n]["H"], tr.PATHS[n]["step"]) for n in names)),
             "# F = MSE(last raw frame) / MSE(last filtered frame) against 1024 spp",
             "# baselines, same frames: " + "; ".join("%s F_hist %.2f F_dt %.2f" % (n, base[n][0], base[n][1]) for n in names),
             "# iterations sigma_l sigma_n sigma_z feedback | " + " | ".join("%s F" % n for n in names)
             + " | geometric mean F | beats both baselines on every path"]
    rows = []
    for it, sl, sn, sz, fb in itertools.product(ITERATIONS, SIGMA_L, SIGMA_N, SIGMA_Z, FEEDBACK):
        fs = [sr.run_path(paths[n][0], paths[n][1], iterations=it, sigma_luminance=sl, sigma_normal=sn, sigma_depth=sz, feedback=fb)[0]
              for n in names]
        gm = float(np.exp(np.mean(np.log(fs))))
        ok = all(f >= max(base[n]) for f, n in zip(fs, names))
        rows.append(((it, sl, sn, sz, fb), fs, gm, ok))
        lines.append("%d %5.1f %6.1f %5.2f %d | " % (it, sl, sn, sz, fb) + " | ".join("%7.2f" % f for f in fs) + " | %7.2f | %s" % (gm, "yes" if ok else "no"))
    good = [r for r in rows if r[3]]
    if good:
        best = max(good, key=lambda r: r[2])
        lines.append("# best geometric mean among the settings that beat both baselines on every path: iterations %d sigma_luminance %g "
                     "sigma_normal %g sigma_depth %g feedback %d (%.2f)" % (best[0] + (best[2],)))
    d = sr.DEFAULTS
    chosen = [r for r in rows if r[0] == (d["iterations"], d["sigma_luminance"], d["sigma_normal"], d["sigma_depth"], d["feedback"])]
    if chosen:
        lines.append("# the defaults of include/mpt.h: iterations %d sigma_luminance %g sigma_normal %g sigma_depth %g feedback %d: " % chosen[0][0]
                     + ", ".join("%s F %.2f" % (n, f) for n, f in zip(names, chosen[0][1])) + "; geometric mean %.2f" % chosen[0][2])
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


if __name__ == "__main__":
    main()
