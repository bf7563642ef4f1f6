"""numpy restatement of mpt_render_adaptive's schedule and stopping rule (include/mpt.h, csrc/mpt_adaptive.h).

Errors are computed in double precision from the float32 sum and moments, with the luminance weights as float32 constants widened to
double (the weights the moments' l^2 is formed with), exactly as k_adaptive_eval does."""
import numpy as np

DEFAULT_MIN_SAMPLES, DEFAULT_BATCH, DEFAULT_LUMINANCE_FLOOR = 16, 16, 0.05
LUM = tuple(np.float64(np.float32(c)) for c in (0.2126, 0.7152, 0.0722))


def schedule(N, min_samples=0, batch_samples=0):
    """Sample counts every active tile holds after pass 0, 1, ...: n_0 = min(min_samples, N), n_{k+1} = min(n_k + batch, N)."""
    m = min_samples or DEFAULT_MIN_SAMPLES
    b = batch_samples or DEFAULT_BATCH
    n = [min(m, N)]
    while n[-1] < N:
        n.append(min(n[-1] + b, N))
    return n


def lum64(rgb):
    rgb = np.asarray(rgb, np.float64)
    return (LUM[0] * rgb[..., 0] + LUM[1] * rgb[..., 1]) + LUM[2] * rgb[..., 2]


def lum32(v):
    """l of the moments (float32, operation order of dn_lum)."""
    v = np.asarray(v, np.float32)
    c = [np.float32(x) for x in (0.2126, 0.7152, 0.0722)]
    return (c[0] * v[..., 0] + c[1] * v[..., 1]) + c[2] * v[..., 2]


def pixel_errors(sum_, m2, n, luminance_floor=0.0):
    """err = sqrt(var / n) / max(mean, floor) per pixel of a sum holding n samples (n: a scalar or an [H, W] array)."""
    fl = np.float64(np.float32(luminance_floor if luminance_floor > 0 else DEFAULT_LUMINANCE_FLOOR))
    n = np.asarray(n, np.float64)
    s = lum64(sum_)
    mean = s / n
    var = np.maximum(0.0, (np.asarray(m2, np.float64)[..., 3] - s * mean) / (n - 1.0))
    return np.sqrt(var / n) / np.maximum(mean, fl)


def tile_max(e):
    """[H, W] per-pixel values -> [ceil(H/8), ceil(W/8)] maxima over the pixels of each 8x8 tile inside the image."""
    H, W = e.shape
    ty, tx = (H + 7) // 8, (W + 7) // 8
    pad = np.full((ty * 8, tx * 8), -np.inf)
    pad[:H, :W] = e
    return pad.reshape(ty, 8, tx, 8).max(axis=(1, 3))


def tile_errors(sum_, m2, n, luminance_floor=0.0):
    return tile_max(pixel_errors(sum_, m2, n, luminance_floor))


def stop_counts(errors, counts, threshold, N):
    """errors[k] = the tile errors after counts[k] samples: the count each tile stops at (first error <= threshold, else N)."""
    stop = np.full(errors[0].shape, N, np.int64)
    active = np.ones(errors[0].shape, bool)
    for e, n in zip(errors, counts):
        done = active & ~(e > threshold)
        stop[done] = n
        active &= ~done
        if n >= N:
            break
    return stop
