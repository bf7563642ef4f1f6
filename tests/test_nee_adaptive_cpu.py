"""The numpy helper of tests/test_gpu_nee_adaptive.py without a GPU: running sums and moments in float32 and in sample order."""
import numpy as np

import adaptive_ref as ar
import nee_adaptive_ref as nar

F = np.float32


def _values(N=12, H=5, W=7, seed=3):
    rng = np.random.default_rng(seed)
    v = np.exp2(rng.uniform(-12, 6, (N, H, W, 4))).astype(F)
    v[rng.random(v.shape) < 0.2] = 0                      # per-sample values are often exactly zero
    v[..., 3] = np.minimum(v[..., 3], 1)
    return v


def test_running_sums_and_moments_are_float32_in_sample_order():
    v = _values()
    sums, moms = nar.running(v)
    assert sums.dtype == F and moms.dtype == F and sums.shape == (13, 5, 7, 4)
    assert not sums[0].any() and not moms[0].any()
    assert np.array_equal(sums[1], v[0])                  # 0 + v is exact
    # one pixel by hand, scalar float32 operations
    y, x = 2, 3
    acc, m = np.zeros(4, F), np.zeros(4, F)
    c = [F(0.2126), F(0.7152), F(0.0722)]
    for s in range(v.shape[0]):
        p = v[s, y, x]
        acc = acc + p
        l = F(F(c[0] * p[0]) + F(c[1] * p[1])) + F(c[2] * p[2])
        m = m + np.array([p[0] * p[0], p[1] * p[1], p[2] * p[2], l * l], F)
        assert np.array_equal(sums[s + 1, y, x].view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(moms[s + 1, y, x].view(np.uint32), m.view(np.uint32))
    # close to the float64 totals, and not what another order of the samples gives everywhere (the order is part of the contract)
    np.testing.assert_allclose(sums[-1], v.astype(np.float64).sum(0), rtol=1e-5)
    back, _ = nar.running(v[::-1])
    assert not np.array_equal(back[-1].view(np.uint32), sums[-1].view(np.uint32))


def test_at_counts_picks_every_pixels_own_count():
    v = _values(N=8, H=16, W=11)
    sums, _ = nar.running(v)
    counts = np.array([[2, 8], [5, 0]], np.uint32)        # 2 x 2 tiles of a 16 x 11 image, the right column partial
    per_px = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:16, :11]
    got = nar.at_counts(sums, per_px)
    assert np.array_equal(got[:8, :8], sums[2][:8, :8]) and np.array_equal(got[:8, 8:], sums[8][:8, 8:])
    assert np.array_equal(got[8:, :8], sums[5][8:, :8]) and not got[8:, 8:].any()


def test_schedule_errors_and_steps():
    v = _values(N=16, H=16, W=16)
    sums, moms = nar.running(v)
    sched = ar.schedule(16, 4, 5)
    assert sched == [4, 9, 14, 16]
    errs = nar.schedule_errors(sums, moms, sched)
    assert len(errs) == 4 and errs[0].shape == (2, 2)
    assert np.array_equal(errs[1], ar.tile_errors(sums[9], moms[9], 9))
    assert [nar.steps_taken(c, 4, 5) for c in (4, 9, 14, 16)] == [1, 2, 3, 4]
    assert nar.steps_taken(3, 4, 5) == 1                  # N below min_samples: one step
