"""numpy restatement of what a tile of mpt_render_nee_adaptive holds (include/mpt.h): the running float32 sums and the running float32
second moments of per-sample values, joined in sample order with one rounding per operation, as the kernel's `acc += v` and
add_moments (csrc/mpt_kernels.h) do.  The per-sample values themselves come from single-sample mpt_render_nee calls (0 + v is
exact); the stopping rule is tests/adaptive_ref.py's.  Test code."""
import numpy as np

import adaptive_ref as ar

F = np.float32


def running(values):
    """values [N, H, W, 4] float32, sample s at index s -> (sums, moments), each [N + 1, H, W, 4] float32: index n = what a pixel holds
    after its first n samples (index 0: zeros)."""
    v = np.asarray(values, F)
    sums = np.zeros((v.shape[0] + 1,) + v.shape[1:], F)
    moms = np.zeros_like(sums)
    for s in range(v.shape[0]):
        sums[s + 1] = sums[s] + v[s]
        l = ar.lum32(v[s])                                   # (0.2126f v.x + 0.7152f v.y) + 0.0722f v.z
        sq = np.concatenate([v[s][..., :3] * v[s][..., :3], (l * l)[..., None]], -1)
        moms[s + 1] = moms[s] + sq
    return sums, moms


def at_counts(run, per_px):
    """run [N + 1, H, W, 4] and per-pixel counts [H, W] -> [H, W, 4]: every pixel's entry at its own count."""
    idx = np.asarray(per_px, np.int64)[None, ..., None]
    return np.take_along_axis(run, np.broadcast_to(idx, (1,) + run.shape[1:]), 0)[0]


def schedule_errors(sums, moms, sched, luminance_floor=0.0):
    """The tile errors (adaptive_ref.tile_errors) at every step of the schedule."""
    return [ar.tile_errors(sums[n], moms[n], n, luminance_floor) for n in sched]


def steps_taken(count, n0, batch):
    """Schedule steps a tile that stopped at `count` took, the first included."""
    return 1 if count <= n0 else 1 + -(-(count - n0) // batch)
