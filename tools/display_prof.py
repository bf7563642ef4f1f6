"""Times of the display stage (profiles/r10_display.txt): its three kernels from one rocprofv3 kernel trace, and a camera-path
playback with and without it.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/display_prof.py          the kernel workload
    python tools/display_prof.py DIR/..._results.db                                    the reduction of its rocpd database
                                                                                       (or of ..._kernel_trace.csv)
    python tools/display_prof.py e2e [FRAMES_DIR]                                      the playback comparison (profiler off)

Kernel workload: at 1920x1080 and 1280x720, for the default forms (aggregated histogram, four pixels per thread) and then for the
other ones (MPT_DISPLAY_HIST=plain, MPT_DISPLAY_PX=1; a context reads them when it is created), REPS x mpt_display with auto-exposure
and the ACES curve of: a scene.xml frame (the sum of 4 spp), a log-uniform random image and an image of one luminance (both written
into the sum: MPT_DISPLAY_SUM, the dividing load), then of an adaptive render (MPT_DISPLAY_ADAPTIVE, the load with the tile look-up).
Reduction: every kernel instantiation's dispatches in order are cut into runs of REPS; medians in microseconds without the first two
of each run; GB/s counts the compulsory bytes per pixel (16 read by the histogram, 16 read + 4 written by present) and "of peak" is
against HBM's 8 TB/s.  "gaps" is what one mpt_display's three kernels leave between them: from the histogram's start to present's end,
less the three kernel times.

Playback: mpt_render --camera-path over scene.xml at 1920x1080, philox, a fixed path of 64 frames, MPT_FRAME_TIMES=1 (the host's clock
around each call, in the frame's JSON line): today's path (float read-back, mpt_write_ppm) against --tonemap clamp --transfer gamma22,
alternating, two runs each in one session."""
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20
SIZES = ((1920, 1080), (1280, 720))
FORMS = (("wave", "4"), ("plain", "1"))
IMAGES = ("scene.xml frame", "log-uniform random", "one luminance")
HBM_PEAK = 8.0e12
PATH = "16 d\n16 w mouse 2 0\n16 a\n16 s mouse -2 0\n"


def workload():
    sys.path.insert(0, ROOT)
    import numpy as np
    from metalpathtracer_amd import capi, host
    sc = host.Scene()
    st, log = host.SceneLoader.LoadSceneFromXML(os.path.join(ROOT, "assets", "scene.xml"), sc)
    assert st == 0, log
    sc.buildBVH()
    rng = np.random.default_rng(1)
    kw = dict(auto_exposure=True, tone=capi.TONE_ACES)
    for W, H in SIZES:
        random = np.exp2(rng.uniform(-20, 20, (H, W, 4))).astype(np.float32)
        one = np.empty((H, W, 4), np.float32)
        one[...] = [0.3, 0.5, 0.2, 1.0]
        for hist, px in FORMS:
            os.environ["MPT_DISPLAY_HIST"], os.environ["MPT_DISPLAY_PX"] = hist, px
            ctx = capi.Context(0)
            ctx.upload_scene(*sc.buffers())
            ctx.resize(W, H)
            ctx.set_uniforms(host.make_uniforms(W, H, sc.getPrimitiveCount(), sc.getTriangleCount()))
            ctx.render(sample_count=4, max_depth=8)
            shown = []
            for r in range(REPS):
                info = ctx.display(source=capi.DISPLAY_SUM, samples=4, **kw)
            shown.append(ctx.read_display().copy())
            for img in (random, one):
                ctx.write_sum(img)
                for r in range(REPS):
                    info = ctx.display(source=capi.DISPLAY_SUM, samples=1, **kw)
                shown.append(ctx.read_display().copy())
            ctx.render_adaptive(0.05, sample_count=32, max_depth=8)
            for r in range(REPS):
                info = ctx.display(source=capi.DISPLAY_ADAPTIVE, **kw)
            shown.append(ctx.read_display().copy())
            print("%dx%d histogram %s, %s px per thread: adaptive frame scale %.6g, key bin %d, %d clipped; digest %s"
                  % (W, H, hist, px, info["scale"], info["key_bin"], info["pixels_clipped"],
                     " ".join("%08x" % (int(s.view(np.uint32).sum(dtype=np.uint64)) & 0xFFFFFFFF) for s in shown)))
            ctx.synchronize()
            ctx.close()


def _rows(path):
    if path.endswith(".csv"):      # --output-format csv: ..._kernel_trace.csv
        import csv
        return sorted(((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))),
                      key=lambda r: r[1])
    return sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()


def _kind(name):
    """('histogram' | 'exposure' | 'present', a label of the instantiation) from a mangled or demangled kernel name."""
    import re
    for key in ("k_dp_histogram", "k_dp_exposure", "k_dp_present"):
        if key in name:
            m = re.search(key + r"I((?:L[ib]\d+E)+)E", name)
            if m:
                return key[5:], " ".join(re.findall(r"L[ib](\d+)E", m.group(1)))
            m = re.search(key + r"<([^>]*)>", name)
            args = [a.strip() for a in m.group(1).split(",")] if m else []
            return key[5:], " ".join({"true": "1", "false": "0"}.get(a, a) for a in args)
    return None, None


def reduce(path):
    rows = [(n, s, e) for n, s, e in _rows(path) if "k_dp_" in n]
    by = {}
    for name, start, end in rows:
        kind, label = _kind(name)
        by.setdefault((kind, label), []).append((end - start) / 1e3)
    print("kernel (template arguments: source 1 = sum / samples, 2 = adaptive; histogram: aggregated; present: tone, pixels per thread)")
    for (kind, label), us in sorted(by.items()):
        if kind == "exposure":
            print("  k_dp_exposure                      %6.1f us (median of %d)" % (statistics.median(us), len(us)))
            continue
        runs = [us[i:i + REPS] for i in range(0, len(us), REPS)]
        bpp = 16 if kind == "histogram" else 20
        adaptive = label.split()[0] == "2"
        names = ["adaptive render"] if adaptive else list(IMAGES)
        per_size = len(names)
        for i, run in enumerate(runs):
            W, H = SIZES[min(i // per_size, len(SIZES) - 1)]
            med = statistics.median(run[2:]) if len(run) > 2 else statistics.median(run)
            mb = bpp * W * H / 1e6
            print("  k_dp_%-9s <%s> %9s %-18s %7.1f us  %6.0f GB/s  %.2f of peak (%.1f MB compulsory, %.1f us at 8 TB/s; %d dispatches)"
                  % (kind, label, "%dx%d" % (W, H), names[i % per_size], med, mb / med * 1e3, mb * 1e6 / HBM_PEAK / (med * 1e-6), mb,
                     mb * 1e6 / HBM_PEAK * 1e6, len(run)))
    # one call = histogram, exposure, present back to back: what is not kernel time between the first start and the last end
    gaps, i = [], 0
    while i + 2 < len(rows):
        k = [_kind(rows[i + j][0])[0] for j in range(3)]
        if k == ["histogram", "exposure", "present"]:
            span = rows[i + 2][2] - rows[i][1]
            gaps.append((span - sum(rows[i + j][2] - rows[i + j][1] for j in range(3))) / 1e3)
            i += 3
        else:
            i += 1
    if gaps:
        print("  gaps between the three kernels of one mpt_display: median %.1f us (of %d calls)" % (statistics.median(gaps), len(gaps)))


def e2e(keep=None):
    exe = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
    tmp = keep or tempfile.mkdtemp(prefix="display_e2e_")
    os.makedirs(tmp, exist_ok=True)
    path = os.path.join(tmp, "path.txt")
    open(path, "w").write(PATH)
    base = [exe, "--scene", os.path.join(ROOT, "assets", "scene.xml"), "--width", "1920", "--height", "1080", "--rng", "philox", "--depth", "32",
            "--camera-path", path]
    variants = (("today: read_frame + mpt_write_ppm", []), ("display: --tonemap clamp --transfer gamma22", ["--tonemap", "clamp", "--transfer", "gamma22"]))
    env = dict(os.environ, MPT_FRAME_TIMES="1")
    results = {name: [] for name, _ in variants}
    for rnd in range(2):
        for name, flags in variants:
            out_dir = os.path.join(tmp, "frames")
            t0 = time.perf_counter()
            r = subprocess.run(base + ["--out-dir", out_dir] + flags, env=env, capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-2000:]
            frames = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"frame"')]
            ms = [f["ms"] for f in frames][4:]                      # (without the first frames: code objects, first-touch of the buffers)
            results[name].append(dict(frames=len(frames), process_s=wall, **{k: statistics.median(m[k] for m in ms) for k in ("render", "read", "write")}))
            shutil.rmtree(out_dir, ignore_errors=True)
    for name, runs in results.items():
        for i, r in enumerate(runs):
            frame = r["render"] + r["read"] + r["write"]
            print("%-46s run %d: %d frames; per frame (medians, host ms) render %.3f  read-back%s %.3f  %s %.3f  = %.3f ms  (%.0f frames/s); process %.1f s"
                  % (name, i, r["frames"], r["render"], " + display" if "display" in name else "", r["read"],
                     "file write" if "display" in name else "conversion + file write", r["write"], frame, 1e3 / frame, r["process_s"]))
    if not keep:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "e2e":
        e2e(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1:
        reduce(sys.argv[1])
    else:
        workload()
