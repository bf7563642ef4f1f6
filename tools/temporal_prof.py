"""Kernel times of the temporal stage beside one a-trous level, from one rocprofv3 kernel trace (profiles/r07_temporal.txt).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/temporal_prof.py        the workload
    python tools/temporal_prof.py DIR/..._results.db                                  the reduction of its rocpd database
                                                                                      (or of ..._kernel_trace.csv)

Workload: scene.xml at 1920x1080 and 1280x720, one 1-spp render, then REPS x (mpt_temporal_accumulate + mpt_denoise with N = 2) with
a still camera — k_tp_reproject<1>, the same-camera rule — and REPS x the same with the camera alternating between two positions —
k_tp_reproject<2>, four taps per pixel, the guides traced again.  The first k_dn_level of every mpt_denoise is the level of step 1.
Reduction: dispatches in order, the first half of each kernel's dispatches is 1920x1080, the second 1280x720; medians in
microseconds without the first two; GB/s counts the compulsory 112 bytes per pixel of the temporal kernel."""
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
SIZES = ((1920, 1080), (1280, 720))
BYTES_PER_PIXEL = 112


def workload():
    sys.path.insert(0, ROOT)
    from metalpathtracer_amd import capi, host
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", "scene.xml"), sc)
    assert st == 0, log
    sc.buildBVH()
    ctx = capi.Context(0)
    ctx.upload_scene(*sc.buffers())
    for W, H in SIZES:
        ctx.resize(W, H)
        cams = []
        for dx in (0.0, 0.2):
            cam = host.camera_reset()
            cam["pos"] = (cam["pos"][0] + dx, cam["pos"][1], cam["pos"][2])
            cams.append(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=cam))
        ctx.set_uniforms(cams[0])
        ctx.render(sample_count=1, max_depth=8)
        ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=1)           # k_tp_reproject<0>: no history yet
        for moving in (False, True):
            for r in range(REPS):
                ctx.set_uniforms(cams[r & 1 if moving else 0])
                info = ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=1)
                ctx.denoise(source=capi.DENOISE_SUM, samples=1, iterations=2)
            print("%dx%d %s camera: %d of %d pixels reset in the last call" % (W, H, "moving" if moving else "still", info["pixels_reset"], W * H))
        ctx.synchronize()
    ctx.close()


def reduce(path):
    if path.endswith(".csv"):      # --output-format csv: ..._kernel_trace.csv
        import csv
        rows = sorted(((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))),
                      key=lambda r: r[1])
    else:
        rows = sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()
    series = {"still": [], "moving": [], "level": []}
    pair = 0
    for name, start, end in rows:
        us = (end - start) / 1e3
        if "k_tp_reprojectILi1E" in name or "k_tp_reproject<1>" in name:       # (mangled or demangled, by the profiler's version)
            series["still"].append(us)
        elif "k_tp_reprojectILi2E" in name or "k_tp_reproject<2>" in name:
            series["moving"].append(us)
        elif "k_dn_guide" in name or "k_tp_reproject" in name:
            pass
        elif "k_dn_level" in name:
            if pair % 2 == 0:            # N = 2: the first launch of every pair is step 1
                series["level"].append(us)
            pair += 1
    for i, (W, H) in enumerate(SIZES):
        out = []
        for key in ("still", "moving", "level"):
            s = series[key]
            half = len(s) // 2
            part = s[i * half:(i + 1) * half][2:]
            out.append((statistics.median(part), len(part)))
        mb = BYTES_PER_PIXEL * W * H / 1e6
        print("%-10s k_tp_reproject still %6.1f us (%5.0f GB/s) | moving %6.1f us (%5.0f GB/s) | k_dn_level step 1 %6.1f us  (medians of %d / %d / %d; %.0f MB compulsory)"
              % ("%dx%d" % (W, H), out[0][0], mb / out[0][0] * 1e3, out[1][0], mb / out[1][0] * 1e3, out[2][0], out[0][1], out[1][1], out[2][1], mb))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        reduce(sys.argv[1])
    else:
        workload()
