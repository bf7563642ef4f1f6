"""tests/restir_ref.py (the numpy restatement of mpt_direct_restir: spatial reservoir reuse in the direct pass) without a GPU:
  * with K = 0 it is tests/ris_ref.py's samples through tests/direct_ref.py's image — rgba and both counts bit for bit — for m = 1, 2, 5;
  * a reservoir's sample re-formed at its own pixel reproduces the stored factor fac_q bit for bit;
  * every neighbour offset stays within +-R over all 2^24 values u01 can take, for R = 1, 8, 64, and reaches both ends;
  * tainted pixels (a gap ray among the rays a pixel-round depends on) are at most 10 % of each GPU case's pixels;
  * the expectation of the specification itself: on `handmade` at 12 x 8 the UNBIASED reference against the m = 1 direct reference under
    different seeds, by the self-normalised batch statistic of tests/test_gpu_restir.py;
  * the entry points refuse a null context."""
import ctypes as C

import numpy as np
import pytest

import anyhit_ref
import direct_ref
import restir_cases as rsc
import restir_ref
import ris_cases as rcs
import ris_ref

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("M", (1, 2, 5))
@pytest.mark.parametrize("name", rsc.CASES)
def test_without_neighbours_it_is_the_resampled_direct_pass(name, M):
    r = rcs.direct_reference(name, M, rcs.AREA)
    for begin, N in rsc.RANGES:
        sampled, lower, _ = rcs.direct_sliced(r, begin, N)
        want = ris_ref.direct(r["ad"], r["nc"], r["u"], r["table"], begin, N, rsc.SEED, lower, sampled=sampled)
        got = rsc.reference(name, M, 0, 0, begin, N)
        for mode in restir_ref.MODES:
            g = got[mode]
            np.testing.assert_array_equal(bits(g["rgba"]), bits(want[0]))
            np.testing.assert_array_equal(g["traced"], want[1])
            np.testing.assert_array_equal(g["unoccluded"], want[2])
            assert g["info"]["rays_final"] == g["info"]["rays_correction"] == g["info"]["neighbours_accepted"] == 0
            assert g["info"]["rays_initial"] == want[1].sum()
            np.testing.assert_array_equal(g["pick"][..., :5], got["initial"][..., :5])          # the pick is the own reservoir
            np.testing.assert_array_equal(g["pick"][..., 5], got["initial"][..., 5] * 3)         # ... marked own
    assert (want[0][..., :3] > 0).any() and (want[1] > want[2]).any()


@pytest.mark.parametrize("name", rsc.CASES)
def test_a_sample_reformed_at_its_own_pixel_reproduces_its_factor(name):
    g = rsc.guides(name)
    H, W = g["ad"].shape[:2]
    o = direct_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, 1, rsc.SEED)[0].reshape(-1, 3)
    n = g["nc"][..., :3].reshape(-1, 3)
    seen = 0
    for begin, N in rsc.RANGES:
        w = rsc.reference(name, 5, 4, 8, begin, N)["initial"].reshape(-1, 6)
        holds = (w[:, 5] & 1) != 0
        with np.errstate(all="ignore"):
            f = restir_ref.form(w[:, 0].astype(np.int64), w[:, 1].view(np.float32), w[:, 2].view(np.float32), o, n, g["table"])
        np.testing.assert_array_equal(bits(f["fac"])[holds], w[holds, 4])
        assert f["ok"][holds].all() and not w[~holds].any()
        seen += int(holds.sum())
    assert seen > 0


@pytest.mark.parametrize("R", (1, 8, 64))
def test_every_offset_stays_within_the_radius(R):
    from ao_ref import u01
    u = u01(np.arange(1 << 24, dtype=np.uint32) << np.uint32(8))          # every value u01 can take
    assert u[0] == 0 and u[-1] < 1 and np.unique(u[:: 1 << 12]).size == 1 << 12
    d = restir_ref.offsets(u, R)
    assert d.min() == -R and d.max() == R
    assert np.unique(d).size == 2 * R + 1 and (np.diff(d) >= 0).all()


@pytest.mark.parametrize("name", rsc.CASES)
def test_tainted_pixels_are_at_most_a_tenth(name):
    """The cap is a condition on the cases, not a measurement of the code: the reference alone decides it."""
    worst = 0.0
    for M in rsc.MS:
        for K, R, begin, N in rsc.grid():
            r = rsc.reference(name, M, K, R, begin, N)
            for mode in restir_ref.MODES:
                worst = max(worst, r[mode]["tainted"].mean())
                assert r[mode]["tainted"].sum() <= rsc.TAINT_CAP * r[mode]["tainted"].size, (M, K, R, begin, N, mode)
    for W, H, R in rsc.SMALL_SIZES:
        r = rsc.reference(name, rsc.SMALL_M, rsc.SMALL_K, R, 7, 3, W, H)
        for mode in restir_ref.MODES:
            assert r[mode]["tainted"].sum() <= rsc.TAINT_CAP * r[mode]["tainted"].size, (W, H, mode)
    r = rsc.reference(name, 5, 4, 8, 7, 3)
    info = r[restir_ref.UNBIASED]["info"]
    print(name, "worst tainted fraction", worst, info)
    assert info["neighbours_accepted"] > 0 and info["samples_from_neighbours"] > 0 and info["rays_correction"] > 0      # the merge does something
    assert r[restir_ref.BIASED]["info"]["rays_correction"] == 0


def batch_statistic(x, y):
    """x, y [B, H, W]: D_b = the image mean of x - y per batch; returns (mean_b D_b, 5 * std_b(D_b) / sqrt(B))."""
    D = (x - y).reshape(x.shape[0], -1).mean(-1)
    return D.mean(), 5 * D.std(ddof=1) / np.sqrt(D.size)


def test_the_unbiased_rule_has_the_expectation_of_the_direct_pass():
    """The pixels of one ReSTIR image share samples, so the image mean is the unit: B batches under different seeds, D_b the image mean of
    (restir - direct) of batch b, |mean D_b| <= 5 std(D_b) / sqrt(B).  The bound comes from the batches themselves."""
    name, W, H, B, N, K, R, M = "handmade", 12, 8, 32, 4, 4, 8, 1
    g = rsc.guides(name, W, H)
    x = {k: np.empty((B, H, W)) for k in ("unbiased", "biased", "direct")}
    for b in range(B):
        r = restir_ref.restir(g["ad"], g["nc"], g["u"], g["table"], g["buf"], anyhit_ref.bounds, 0, N, M, K, R, (b, 11))
        x["unbiased"][b] = r[restir_ref.UNBIASED]["rgba"][..., :3].astype(np.float64).mean(-1)
        x["biased"][b] = r[restir_ref.BIASED]["rgba"][..., :3].astype(np.float64).mean(-1)
        sampled = direct_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, N, (b, 12))
        lower, _ = direct_ref.occlusion_bounds(sampled, g["buf"], anyhit_ref.bounds)
        x["direct"][b] = direct_ref.direct(g["ad"], g["nc"], g["u"], g["table"], 0, N, (b, 12), lower, sampled=sampled)[0][..., :3].astype(np.float64).mean(-1)
    mean, bound = batch_statistic(x["unbiased"], x["direct"])
    mean_b, bound_b = batch_statistic(x["biased"], x["direct"])
    print("image means", x["direct"].mean(), x["unbiased"].mean(), x["biased"].mean(), "unbiased: mean D", mean, "bound", bound,
          "biased (not asserted): mean D", mean_b, "bound", bound_b)
    assert x["direct"].mean() > 0 and bound > 0
    assert abs(mean) <= bound


def test_the_entry_points_refuse_a_null_context():
    from metalpathtracer_amd import capi
    L = capi.load()
    p = capi.restir_params(samples=1)
    out = (C.c_uint32 * 6)()
    assert capi.RESTIR_MAX_NEIGHBOURS == restir_ref.K_MAX and capi.RESTIR_MAX_RADIUS == restir_ref.R_MAX
    assert capi.RESTIR_DEFAULTS == restir_ref.DEFAULTS
    assert L.mpt_direct_restir(None, C.byref(p), None) == 1                  # MPT_ERR_INVALID_ARG, no crash
    assert L.mpt_read_restir(None, None, None, None) == 1
    assert L.mpt_restir_buffer(None, None, None) == 1
    assert L.mpt_read_restir_reservoirs(None, 0, out) == 1
