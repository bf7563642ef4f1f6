"""Per-kernel times of the denoiser from a rocprofv3 kernel trace of tools/denoise_timing.py (its rocpd database):
    python tools/denoise_prof.py DIR/..._results.db
Dispatches are taken in order: each k_dn_guide starts a repetition, the k_dn_level launches behind it are levels 0, 1, ...;
the first half of the repetitions is 1920x1080, the second 1280x720 (the workload's order).  Prints medians in microseconds."""
import sqlite3
import statistics
import sys


def main(path):
    rows = sqlite3.connect(path).execute("select name, start, end from kernels order by start").fetchall()
    reps, cur = [], None
    for name, start, end in rows:
        us = (end - start) / 1e3
        if "k_dn_guide" in name:
            cur = {"guide": us, "levels": []}
            reps.append(cur)
        elif "k_dn_level" in name and cur is not None:
            cur["levels"].append(us)
    half = len(reps) // 2
    for label, part in (("1920x1080", reps[:half]), ("1280x720", reps[half:])):
        part = part[2:]   # (the first repetitions include first-launch costs)
        g = statistics.median(p["guide"] for p in part)
        lv = [statistics.median(p["levels"][i] for p in part) for i in range(len(part[0]["levels"]))]
        print("%-10s guide pass %7.1f us | levels %s | filter total %7.1f us | guide + filter %7.1f us  (median of %d)" % (
            label, g, " ".join("%.1f" % v for v in lv), sum(lv), g + sum(lv), len(part)))


if __name__ == "__main__":
    main(sys.argv[1])
