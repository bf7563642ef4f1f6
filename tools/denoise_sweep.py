"""CPU calibration of the denoiser's defaults (include/mpt.h MPT_DENOISE_DEFAULT_*): the oracle renders Cornell and scene.xml at
128 x 128 with 4 and 1024 spp, guide data comes from the oracle's first_hit through every pixel centre, and the numpy restatement
(tests/denoise_ref.py) filters the 4-spp image over a grid of sigmas and levels.  Prints the table (profiles/r06_denoise_sweep.txt)
with the MSE against the 1024-spp image and the factor by which the filter cuts it.   python tools/denoise_sweep.py [--quick]"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import binding as ob  # noqa: E402
import denoise_ref as dr  # noqa: E402

CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
SCENES = (("cornell.xml", CORNELL_CAM), ("scene.xml", None))
SIZE, LOW, HIGH, DEPTH = 128, 4, 1024, 8


def case(name, cam, threads=16):
    sc = ob.OracleScene()
    assert sc.load_xml(os.path.join(ROOT, "assets", name)) == 0
    sc.build_bvh()
    buf = sc.buffers()
    u = ob.make_uniforms(SIZE, SIZE, sc.prim_count, sc.triangle_count, cam=cam)
    lo, _ = ob.render(u, buf, rng_mode=ob.RNG_PHILOX, max_depth=DEPTH, sample_count=LOW, seed=(1, 0), threads=threads)
    hi, _ = ob.render(u, buf, rng_mode=ob.RNG_PHILOX, max_depth=DEPTH, sample_count=HIGH, seed=(7, 0), threads=threads)
    ad, nc, _ = dr.first_hit_guides(u, buf, ob.first_hit)
    return lo / np.float32(LOW), hi / np.float32(HIGH), ad, nc


def mse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float((d * d).mean())


def main():
    quick = "--quick" in sys.argv
    cases = [(n,) + case(n, c) for n, c in SCENES]
    grid = itertools.product((5,) if quick else (3, 4, 5), (1.0, 4.0) if quick else (0.5, 1.0, 2.0, 4.0, 8.0),
                             (128.0,) if quick else (32.0, 128.0), (1.0,) if quick else (0.25, 1.0, 4.0))
    print("# denoiser sweep: oracle 4 spp vs 1024 spp (another seed), %dx%d, depth %d; factor = MSE(noisy) / MSE(denoised)" % (SIZE, SIZE, DEPTH))
    print("# %-4s %-6s %-6s %-6s %s" % ("N", "s_lum", "s_nrm", "s_dep", "  ".join("%-22s" % n for n, *_ in cases)) + "  min_factor")
    best = None
    for N, sl, sn, sz in grid:
        facs = []
        for name, lo, hi, ad, nc in cases:
            out = dr.denoise(lo, ad, nc, iterations=N, sigma_luminance=sl, sigma_normal=sn, sigma_depth=sz)
            facs.append((mse(out, hi), mse(lo, hi) / mse(out, hi)))
        m = min(f for _, f in facs)
        print("  %-4d %-6g %-6g %-6g %s  %.2f" % (N, sl, sn, sz, "  ".join("mse %.3e x%-7.2f" % f for f in facs), m))
        if best is None or m > best[0]:
            best = (m, N, sl, sn, sz)
    print("# best min factor %.2f at N=%d sigma_luminance=%g sigma_normal=%g sigma_depth=%g" % best)


if __name__ == "__main__":
    main()
