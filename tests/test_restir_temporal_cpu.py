"""tests/restir_temporal_ref.py (the numpy restatement of mpt_direct_restir_temporal: temporal reservoir reuse in the direct pass) without a
GPU:
  * with no history a frame is tests/restir_ref.py's K = 0, N = 1 round bit for bit — rgba, both counts, the reservoir — for m = 1, 2, 5;
  * a stored sample re-formed at its own pixel reproduces the stored factor bit for bit;
  * last frame's point o_q', rebuilt from the history guide and the history's camera, is bit for bit the origin frame f-1 used;
  * under the same camera the tap is the pixel itself;
  * Mh never exceeds m + C m, and with C = 2 the cap does scale a history;
  * tainted pixels (a gap ray among a pixel's own rays) are at most 10 % of each GPU case's pixels;
  * the cases do what they are for: every kind of rejection occurs in some case, taps are accepted, samples come from the history,
    correction rays are traced and some are occluded;
  * the expectation of the specification itself: on `handmade` at 12 x 8 the UNBIASED fifth frame against the m = 1 direct reference at
    the same camera under other seeds, by the self-normalised batch statistic of tests/test_restir_cpu.py;
  * the entry points refuse a null context, and capi's constants are the reference's."""
import ctypes as C

import numpy as np
import pytest

import anyhit_ref
import direct_ref
import restir_cases as rsc
import restir_ref
import restir_temporal_cases as rtc
import restir_temporal_ref as rtr
from test_restir_cpu import batch_statistic, bits

F = np.float32


@pytest.mark.parametrize("M", (1, 2, 5))
@pytest.mark.parametrize("name", rtc.CASES)
def test_without_a_history_a_frame_is_the_round_without_neighbours(name, M):
    g = rsc.guides(name)
    for f in (0, 7):
        want = rsc.reference(name, M, 0, 0, f, 1)
        got = rtr.frame(g["ad"], g["nc"], g["u"], g["table"], g["buf"], anyhit_ref.bounds, prev=None, frame=f, M=M, seed=rsc.SEED)
        surface = g["nc"][..., 3] == 0
        np.testing.assert_array_equal(got["initial"], want["initial"])
        for mode in rtr.MODES:
            a, b = got[mode], want[mode]
            np.testing.assert_array_equal(bits(a["rgba"]), bits(b["rgba"]))
            np.testing.assert_array_equal(a["traced"], b["traced"])
            np.testing.assert_array_equal(a["unoccluded"], b["unoccluded"])
            np.testing.assert_array_equal(a["res"][..., :6], b["pick"])              # the own reservoir, marked own ...
            np.testing.assert_array_equal(a["res"][..., 6], np.where(surface, M, 0))   # ... standing for its m candidates
            i = a["info"]
            assert i["history_accepted"] == i["samples_from_history"] == i["rays_final"] == i["rays_correction"] == 0
            assert i["pixels_reset"] == i["pixels_surface"] == surface.sum() and i["rays_initial"] == b["info"]["rays_initial"]
            assert i["rays_occluded"] == b["info"]["rays_occluded"]
    assert (want[0]["rgba"][..., :3] > 0).any() and want[0]["traced"].any()


def links_of(name):
    for M, C_, mode in rtc.grid():
        for link in rtc.chain(name, M, C_, mode):
            yield M, C_, mode, link


@pytest.mark.parametrize("name", rtc.CASES)
def test_a_stored_sample_reformed_at_its_own_pixel_reproduces_its_factor(name):
    seen = from_history = 0
    for M, C_, mode, link in links_of(name):
        g, ref = link["g"], link["ref"]
        w = ref[mode]["res"].reshape(-1, 7)
        holds = (w[:, 5] & 1) != 0
        with np.errstate(all="ignore"):
            f = restir_ref.form(w[:, 0].astype(np.int64), w[:, 1].copy().view(np.float32), w[:, 2].copy().view(np.float32), ref["o"].reshape(-1, 3),
                                g["nc"][..., :3].reshape(-1, 3), g["table"])
        np.testing.assert_array_equal(bits(f["fac"])[holds], w[holds, 4])
        assert f["ok"][holds].all() and not w[~holds, :6].any()
        seen += int(holds.sum())
        from_history += int((holds & ((w[:, 5] & 2) == 0)).sum())
    assert seen > 0 and from_history > 0


@pytest.mark.parametrize("name", rtc.CASES)
def test_last_frames_point_is_rebuilt_bit_for_bit(name):
    seen = 0
    for M, C_, mode, link in links_of(name):
        if link["prev"] is None:
            continue
        tap = link["ref"]["tap"]
        acc = tap["accepted"]
        gp = link["prev"][0]
        o_prev = direct_ref.samples(gp["ad"], gp["nc"], gp["u"], gp["table"], 0, 1, rtc.SEED)[0].reshape(-1, 3)
        np.testing.assert_array_equal(bits(tap["o_prev"][acc]), bits(o_prev[tap["q"][acc]]))
        seen += int(acc.sum())
    assert seen > 0


@pytest.mark.parametrize("name", rtc.CASES)
def test_with_the_same_camera_the_tap_is_the_pixel_itself(name):
    for M, C_, mode in rtc.grid():
        link = rtc.chain(name, M, C_, mode)[-1]
        tap = link["ref"]["tap"]
        surface = link["g"]["nc"][..., 3] == 0
        H, W = surface.shape
        np.testing.assert_array_equal(tap["accepted"], surface)                        # no test applies, and every surface pixel has Mh > 0
        np.testing.assert_array_equal(tap["q"][surface], np.arange(H * W).reshape(H, W)[surface])
        assert all(tap[k] == 0 for k in ("outside", "miss", "depth", "normal", "empty"))
        np.testing.assert_array_equal(bits(tap["o_prev"][surface]), bits(link["ref"]["o"][surface]))


@pytest.mark.parametrize("name", rtc.CASES)
def test_the_count_is_capped(name):
    scaled = 0
    for M, C_, mode, link in links_of(name):
        Mh = link["ref"][mode]["res"][..., 6]
        surface = link["g"]["nc"][..., 3] == 0
        assert Mh.max() <= M + C_ * M and (Mh[surface] >= M).all() and not Mh[~surface].any()
        if link["prev"] is not None:
            acc = link["ref"]["tap"]["accepted"]
            scaled += int((link["prev"][1].reshape(-1, 7)[link["ref"]["tap"]["q"][acc], 6] > C_ * M).sum())
    assert scaled > 0                                                                  # (C = 2 from frame 3 on)


@pytest.mark.parametrize("name", rtc.CASES)
def test_tainted_pixels_are_at_most_a_tenth(name):
    """The cap is a condition on the cases, not a measurement of the code: the reference alone decides it."""
    worst = 0.0
    for M, C_, mode, link in links_of(name):
        t = link["ref"][mode]["tainted"]
        worst = max(worst, t.mean())
        assert t.sum() <= rtc.TAINT_CAP * t.size, (M, C_, mode, link["frame"])
    for W, H in rtc.SMALL_SIZES:
        for mode in rtr.MODES:
            for link in rtc.chain(name, rtc.SMALL_M, rtc.SMALL_C, mode, W, H):
                t = link["ref"][mode]["tainted"]
                assert t.sum() <= rtc.TAINT_CAP * t.size, (W, H, mode, link["frame"])
    print(name, "worst tainted fraction", worst)


def test_the_cases_do_what_they_are_for():
    kinds = dict(outside=0, miss=0, depth=0, normal=0)
    for name in rtc.CASES:
        occluded_corrections = 0
        for M, C_, mode, link in links_of(name):
            if link["prev"] is None:
                continue
            ref = link["ref"]
            i = ref[mode]["info"]
            moved = link is not rtc.chain(name, M, C_, mode)[-1]
            if moved:
                for k in kinds:
                    kinds[k] += ref["tap"][k]
            assert i["history_accepted"] > 0 and i["samples_from_history"] > 0, (name, M, C_, mode, link["frame"])
            assert i["history_accepted"] + i["pixels_reset"] == i["pixels_surface"]
            assert i["rays_initial"] + i["rays_final"] + i["rays_correction"] == ref[mode]["traced"].sum()
            if mode == rtr.UNBIASED:
                assert i["rays_correction"] > 0
                u, b = ref[rtr.UNBIASED], ref[rtr.BIASED]
                occluded_corrections += int(i["rays_occluded"] - b["info"]["rays_occluded"])
            else:
                assert i["rays_correction"] == 0
        print(name, "occluded correction rays over the chains", occluded_corrections)
    print("rejections over the moved frames of all chains", kinds)
    assert all(v > 0 for v in kinds.values()), kinds


def test_the_unbiased_rule_has_the_expectation_of_the_direct_pass():
    """Frames share samples over time and pixels share them through the taps, so the image mean of the last frame is the unit: B batches
    of 5 frames under different seeds, D_b the image mean of (temporal - direct) of batch b at the last camera,
    |mean D_b| <= 5 std(D_b) / sqrt(B).  The bound comes from the batches themselves.  BIASED is printed, not asserted."""
    name, W, H, B, N, M = "handmade", 12, 8, 64, 5, 1
    gs = [rtc.guides(name, f, W, H) for f in range(N)]
    x = {k: np.empty((B, H, W)) for k in ("unbiased", "biased", "direct")}
    for b in range(B):
        for key, mode in (("unbiased", rtr.UNBIASED), ("biased", rtr.BIASED)):
            prev = None
            for f, g in enumerate(gs):
                r = rtc.one(g, prev, f, M, 0, seed=(b, 11))
                prev = (g, r[mode]["res"])
            x[key][b] = r[mode]["rgba"][..., :3].astype(np.float64).mean(-1)
        g = gs[-1]
        sampled = direct_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, 1, (b, 12))
        lower, _ = direct_ref.occlusion_bounds(sampled, g["buf"], anyhit_ref.bounds)
        x["direct"][b] = direct_ref.direct(g["ad"], g["nc"], g["u"], g["table"], 0, 1, (b, 12), lower, sampled=sampled)[0][..., :3].astype(np.float64).mean(-1)
    mean, bound = batch_statistic(x["unbiased"], x["direct"])
    mean_b, bound_b = batch_statistic(x["biased"], x["direct"])
    var = lambda a: a.var(0, ddof=1).sum()
    print("image means", x["direct"].mean(), x["unbiased"].mean(), x["biased"].mean(), "unbiased: mean D", mean, "bound", bound,
          "biased (not asserted): mean D", mean_b, "bound", bound_b, "variance ratio direct / unbiased", var(x["direct"]) / var(x["unbiased"]))
    assert x["direct"].mean() > 0 and bound > 0
    assert abs(mean) <= bound


def test_the_entry_points_refuse_a_null_context():
    from metalpathtracer_amd import capi
    L = capi.load()
    p = capi.restir_temporal_params(frame=1)
    out = (C.c_uint32 * 7)()
    assert capi.RESTIR_TEMPORAL_MAX_HISTORY == rtr.C_MAX and capi.RESTIR_TEMPORAL_DEFAULTS == rtr.DEFAULTS
    assert capi.RESTIR_TEMPORAL_DEFAULTS["max_history"] == rtr.C_DEFAULT == 20
    assert L.mpt_direct_restir_temporal(None, C.byref(p), None) == 1                 # MPT_ERR_INVALID_ARG, no crash
    assert L.mpt_read_restir_temporal(None, None, None, None) == 1
    assert L.mpt_restir_temporal_buffer(None, None, None) == 1
    assert L.mpt_read_restir_temporal_reservoirs(None, out) == 1
    assert L.mpt_restir_temporal_reset(None) == 1
    assert L.mpt_restir_temporal_image(None, 1, 1, None, None, None, None, None, None, None, C.byref(p), None, None, None, None, None) == 1
