"""Measurements of mpt_render_nee_adaptive on one GPU (profiles/r19_nee_adaptive.txt), HIP-event time of the one trace kernel
(mpt_nee_info.device_ms) throughout, the variants alternating in one process.  Cornell box 1024x1024, depth 8, N = 256, the default
min_samples and batch_samples (16, 16), no per-sample clamp, tree built on the device, MPT_WALK_AUTO:
 (a) the cost of deciding in the wave: threshold 0 (every tile with any variance goes to N: the same samples there, the moments and
     the drained batch boundaries on top; a tile whose error is exactly 0 stops, and the tool says how many did) against
     mpt_render_nee at 256 spp — minimum, median and maximum of REPS runs after WARMUP, per call and per sample, and that the two sums
     are the same bits on the tiles at N;
 (b) equal time: for thresholds 0.1, 0.05, 0.02 the mean spp, device_ms (minimum of 3) and the RMSE of the per-pixel mean (rgb) against
     a 4096-spp mpt_render_nee image of OTHER samples (sample_begin 2^20); beside each, plain mpt_render_nee at the spp that takes the
     same time by (a)'s rate, its measured device_ms and its RMSE.
Usage: python tools/nee_adaptive_timing.py [--out profiles/r19_nee_adaptive.txt] [--quick]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metalpathtracer_amd import capi, host  # noqa: E402

CORNELL_CAM = dict(pos=(0.0, 1.0, 3.4), fwd=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0)
W = H = 1024
DEPTH, N, REF_SPP, REF_BEGIN = 8, 256, 4096, 1 << 20
REPS, WARMUP = 9, 3
THRESHOLDS = (0.1, 0.05, 0.02)


def spread(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return "min %8.3f  median %8.3f  max %8.3f ms" % (ms[0], ms[len(ms) // 2], ms[-1])


def rmse(mean, ref):
    d = mean[..., :3].astype(np.float64) - ref[..., :3]
    return float(np.sqrt((d * d).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the width, height and sample counts (a dry run of the tool itself)")
    a = ap.parse_args()
    w, h, n, ref_spp = (W // 16, H // 16, N // 8, REF_SPP // 16) if a.quick else (W, H, N, REF_SPP)
    ctx = capi.Context(0)
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", "cornell.xml"), sc)
    assert st == 0, log
    host.make_ready(ctx, sc, host.BVH_DEVICE)
    ctx.resize(w, h)
    ctx.set_uniforms(host.make_uniforms(w, h, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=CORNELL_CAM))
    kw = dict(rng_mode=capi.RNG_PHILOX, max_depth=DEPTH, seed=(1, 0), walk=capi.WALK_AUTO, clamp=0.0)
    lines = ["nee_adaptive_timing: cornell.xml %dx%d, depth %d, N = %d, min 16, batch 16, no clamp, build %s" % (
        w, h, DEPTH, n, capi.build_id()["source_sha256"][:16])]

    def plain(spp, begin=0):
        ctx.clear_sum()
        return ctx.render_nee(sample_begin=begin, sample_count=spp, **kw)

    # (a)
    ms = {"nee": [], "adaptive": [], "one": []}
    sums = {}
    for r in range(WARMUP + REPS):
        info = plain(n)
        sums["nee"] = ctx.read_sum() if r == 0 else sums["nee"]
        out = ctx.render_nee_adaptive(0.0, sample_count=n, **kw)
        sums["adaptive"] = ctx.read_sum() if r == 0 else sums["adaptive"]
        one = ctx.render_nee_adaptive(0.0, min_samples=n, sample_count=n, **kw)   # n_0 = N: one step, no boundary is drained
        assert one["adaptive"]["samples"] == info["paths"] and one["adaptive"]["passes"] == 1
        if r >= WARMUP:
            ms["nee"].append(info["device_ms"])
            ms["adaptive"].append(out["nee"]["device_ms"])
            ms["one"].append(one["nee"]["device_ms"])
    # threshold 0 stops a tile whose error is exactly 0 (error > threshold is the rule): tiles without any variance, the light's
    ctx.render_nee_adaptive(0.0, sample_count=n, **kw)
    at_n = capi.expand_tile_counts(ctx.read_tile_samples(), h, w) == n
    same = np.array_equal(sums["nee"][at_n].view(np.uint32), sums["adaptive"][at_n].view(np.uint32))
    ad = out["adaptive"]
    lines += ["", " (a) %d spp, %d timed runs after %d warm-ups, alternating; on the tiles at N the two sums are %s" % (
                  n, REPS, WARMUP, "the same bits" if same else "DIFFERENT"),
              "     threshold 0 leaves %d of %d tiles below N (no variance at all: error 0 is not > 0): %d samples against %d, %.4f of them" % (
                  ad["tiles_converged"], ad["tiles_converged"] + ad["tiles_at_max"], ad["samples"], info["paths"], ad["samples"] / info["paths"]),
              "     mpt_render_nee:                        %s" % spread(ms["nee"]),
              "     mpt_render_nee_adaptive, threshold 0:  %s   (%d schedule steps)" % (spread(ms["adaptive"]), out["adaptive"]["passes"]),
              "     the same with min_samples = N:         %s   (1 step: the moments and the registers, no boundary)" % spread(ms["one"]),
              "     one step / plain: %.4f at the minima, %.4f at the medians (all samples); the 16 steps' boundaries are the rest" % (
                  min(ms["one"]) / min(ms["nee"]), float(np.median(ms["one"]) / np.median(ms["nee"]))),
              "     adaptive / plain: %.4f at the minima, %.4f at the medians; per sample %.4f at the minima" % (
                  min(ms["adaptive"]) / min(ms["nee"]), float(np.median(ms["adaptive"]) / np.median(ms["nee"])),
                  min(ms["adaptive"]) / min(ms["nee"]) * info["paths"] / ad["samples"])]
    print("\n".join(lines), flush=True)
    ms_per_spp = min(ms["nee"]) / n
    # (b)
    plain(ref_spp, REF_BEGIN)
    ref = ctx.read_sum()[..., :3].astype(np.float64) / ref_spp
    lines += ["", " (b) RMSE of the mean (rgb) against %d spp of mpt_render_nee from sample %d on; device_ms the minimum of 3" % (ref_spp, REF_BEGIN)]
    for thr in THRESHOLDS:
        t_ad = []
        for _ in range(3):
            out = ctx.render_nee_adaptive(thr, sample_count=n, **kw)
            t_ad.append(out["nee"]["device_ms"])
        ad = out["adaptive"]
        e_ad = rmse(ctx.read_adaptive_mean(), ref)
        spp_eq = max(1, int(round(min(t_ad) / ms_per_spp)))
        t_pl = []
        for _ in range(3):
            t_pl.append(plain(spp_eq)["device_ms"])
        e_pl = rmse(ctx.read_sum() / np.float32(spp_eq), ref)
        lines.append("     threshold %-5g adaptive: mean spp %7.2f, %d steps, %d / %d tiles converged, %8.3f ms, RMSE %.6f | plain at %3d spp: %8.3f ms, RMSE %.6f | %s" % (
            thr, ad["samples"] / (w * h), ad["passes"], ad["tiles_converged"], ad["tiles_converged"] + ad["tiles_at_max"], min(t_ad), e_ad,
            spp_eq, min(t_pl), e_pl, "adaptive wins" if e_ad < e_pl else "plain wins"))
        print(lines[-1], flush=True)
    ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
