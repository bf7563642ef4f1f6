"""GPU tests of mpt_direct_restir_temporal (include/mpt.h: temporal reservoir reuse in the direct pass over a camera path) against
tests/restir_temporal_ref.py.  Every frame is checked on its own through mpt_restir_temporal_image, which is fed the REFERENCE's
previous reservoirs: the image, the counts, the seven reservoir words and the info totals are compared bit for bit.  Occlusion is
tests/anyhit_ref.py's `lower` — what MPT_WALK_REFERENCE must answer — and MPT_WALK_OWN is held to the same on every pixel that is not
tainted (tests/test_restir_temporal_cpu.py caps those at 10 % of each case's pixels; measured, none of the cases has one).  Then the
small sizes, the context call against the hook chained on its own outputs (the state, the ping-pong, the camera key), identities that
need no reference, the state and its life, the refusals, the expectation on the device and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import restir_temporal_cases as rtc
import restir_temporal_ref as rtr
from conftest import ROOT, scene_path
from test_restir_cpu import batch_statistic

pytestmark = pytest.mark.gpu

SEED = rtc.SEED
INVALID, NOT_READY = 1, 5
EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
INFO_KEYS = rtr.INFO_KEYS


def same(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(autouse=True)
def _settings_restored(request):
    """One candidate and area sampling again after every test, whatever it did (other files share the session's context)."""
    ctx = request.getfixturevalue("gpu_ctx") if "gpu_ctx" in request.fixturenames else None
    yield
    if ctx is not None:
        from metalpathtracer_amd import capi
        ctx.set_light_candidates(1)
        ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)


def put(ctx, name, W=None, H=None, f=0):
    """The case's scene (through mpt_upload_scene with the host's tree), size and the uniforms of frame f; returns the uniforms."""
    _, buf = rtc.scene_of(name)
    ctx.upload_scene(*buf)
    u = rtc.uniforms_of(name, f, W, H)
    ctx.resize(int(u.screenSize[0]), int(u.screenSize[1]))
    ctx.set_uniforms(u)
    return u


def prev_of(link):
    p = link["prev"]
    return None if p is None else (p[0]["ad"], p[0]["nc"], p[0]["u"], p[1])


def check_link(ctx, link, M, C_, mode):
    """One frame through the hook with both walks, against the reference of the same arguments."""
    from metalpathtracer_amd import capi
    g, want = link["g"], link["ref"][mode]
    surface = g["nc"][..., 3] == 0
    for walk in (capi.WALK_REFERENCE, capi.WALK_OWN):
        rgba, traced, unocc, res, info = ctx.restir_temporal_image(g["ad"], g["nc"], g["u"], prev_of(link), frame=link["frame"], seed=SEED, walk=walk,
                                                                   mode=mode, max_history=C_)
        keep = np.ones_like(surface) if walk == capi.WALK_REFERENCE else ~want["tainted"]
        print("m", M, "C", C_, "mode", mode, "frame", link["frame"], "walk", walk, "pixels that differ:",
              int((rgba.view(np.uint32) != want["rgba"].view(np.uint32)).any(-1).sum()), {k: info[k] for k in INFO_KEYS}, "tainted",
              int(want["tainted"].sum()), "ms", info["device_ms"])
        same(rgba[keep], want["rgba"][keep])
        np.testing.assert_array_equal(traced[keep], want["traced"][keep])
        np.testing.assert_array_equal(unocc[keep], want["unoccluded"][keep])
        np.testing.assert_array_equal(res[keep], want["res"][keep])
        if keep.all():
            assert {k: info[k] for k in INFO_KEYS} == want["info"]
        assert traced.sum() == info["rays_initial"] + info["rays_final"] + info["rays_correction"]
        assert traced.sum() - unocc.sum() == info["rays_occluded"]
        assert info["history_accepted"] + info["pixels_reset"] == info["pixels_surface"] == surface.sum()
        assert (rgba[~surface] == (0, 0, 0, 1)).all() and (traced[~surface] == 0).all() and (unocc[~surface] == 0).all() and not res[~surface].any()


# ---- exactness through the hook ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", rtc.MS)
@pytest.mark.parametrize("name", rtc.CASES)
def test_every_frame_is_exact(gpu_ctx, name, M):
    u = put(gpu_ctx, name)
    ad, nc, _ = gpu_ctx.read_aovs()                                               # (the device's guides are the oracle's)
    g0 = rtc.guides(name, 0)
    same(ad, g0["ad"])
    same(nc, g0["nc"])
    gpu_ctx.set_light_candidates(M)
    merged = corrected = 0
    for C_ in rtc.CS:
        for mode in rtr.MODES:
            for link in rtc.chain(name, M, C_, mode):
                check_link(gpu_ctx, link, M, C_, mode)
                merged += link["ref"][mode]["info"]["samples_from_history"]
                corrected += link["ref"][mode]["info"]["rays_correction"]
    assert merged > 0 and corrected > 0 and u is not None


@pytest.mark.parametrize("W,H", rtc.SMALL_SIZES)
@pytest.mark.parametrize("name", rtc.CASES)
def test_every_frame_at_small_sizes(gpu_ctx, name, W, H):
    """1 x 1: one pixel, one lane.  7 x 3: a tile that is not full, taps that leave the image on every side."""
    put(gpu_ctx, name, W, H)
    gpu_ctx.set_light_candidates(rtc.SMALL_M)
    for mode in rtr.MODES:
        for link in rtc.chain(name, rtc.SMALL_M, rtc.SMALL_C, mode, W, H):
            check_link(gpu_ctx, link, rtc.SMALL_M, rtc.SMALL_C, mode)


# ---- the context call: the state, the ping-pong and the camera key ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene.xml", "manylights"])
def test_the_context_call_is_the_hook_chained(gpu_ctx, name):
    from metalpathtracer_amd import capi
    put(gpu_ctx, name)
    gpu_ctx.set_light_candidates(3)
    for mode in rtr.MODES:
        for walk in (capi.WALK_REFERENCE, capi.WALK_AUTO):
            gpu_ctx.restir_temporal_reset()
            prev = None
            from_history = 0
            # frames 0..3 along the path, then frame 4 under frame 3's camera: the same-camera rule through the camera key
            for frame, f in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 3)):
                u = rtc.uniforms_of(name, f)
                gpu_ctx.set_uniforms(u)
                kw = dict(frame=frame, seed=SEED, walk=walk, mode=mode, max_history=2)
                info = gpu_ctx.direct_restir_temporal(**kw)
                got = gpu_ctx.read_restir_temporal() + (gpu_ctx.read_restir_temporal_reservoirs(),)
                ad, nc, _ = gpu_ctx.read_aovs()
                want = gpu_ctx.restir_temporal_image(ad, nc, u, prev, **kw)
                for a, b in zip(got, want[:4]):
                    same(a, b)
                assert {k: info[k] for k in INFO_KEYS} == {k: want[4][k] for k in INFO_KEYS}
                assert (info["history_accepted"] > 0) == (frame > 0)
                if frame == 4:
                    assert info["pixels_reset"] == 0
                from_history += info["samples_from_history"]
                prev = (ad, nc, u, got[3])
            assert from_history > 0


# ---- identities that need no reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell.xml", "manylights"])
def test_identities(gpu_ctx, name):
    """The first frame and the frame after a reset are mpt_direct_restir with K = 0, N = 1; traced sums to the three kinds of ray; BIASED
    traces no correction ray from the same inputs; a frame repeated from the same state gives the same bits."""
    from metalpathtracer_amd import capi
    put(gpu_ctx, name, 40, 24)
    gpu_ctx.set_light_candidates(4)
    state = lambda: gpu_ctx.read_restir_temporal() + (gpu_ctx.read_restir_temporal_reservoirs(),)
    for frame in (0, 5):                                                          # (5: after a reset)
        gpu_ctx.restir_temporal_reset()
        for mode in rtr.MODES:
            gpu_ctx.restir_temporal_reset()
            gpu_ctx.set_uniforms(rtc.uniforms_of(name, 0, 40, 24))
            d = gpu_ctx.direct_restir(samples=1, sample_begin=frame, seed=SEED, neighbours=0, mode=mode)
            want = gpu_ctx.read_restir()
            info = gpu_ctx.direct_restir_temporal(frame=frame, seed=SEED, mode=mode)
            for a, b in zip(gpu_ctx.read_restir_temporal(), want):
                same(a, b)
            assert info["history_accepted"] == info["samples_from_history"] == info["rays_final"] == info["rays_correction"] == 0
            assert info["pixels_reset"] == info["pixels_surface"] == d["pixels_surface"] and info["rays_initial"] == d["rays_initial"]
            assert info["rays_occluded"] == d["rays_occluded"]
    assert want[0][..., :3].any()
    # two frames on, from one and the same history, in both modes and twice
    ad0, nc0, _ = gpu_ctx.read_aovs()
    u0 = rtc.uniforms_of(name, 0, 40, 24)
    res0 = gpu_ctx.read_restir_temporal_reservoirs()
    u1 = rtc.uniforms_of(name, 1, 40, 24)
    gpu_ctx.set_uniforms(u1)
    ad1, nc1, _ = gpu_ctx.read_aovs()
    kw = dict(frame=6, seed=SEED, walk=capi.WALK_AUTO)
    run = lambda mode: gpu_ctx.restir_temporal_image(ad1, nc1, u1, (ad0, nc0, u0, res0), mode=mode, **kw)
    u, b = run(capi.RESTIR_UNBIASED), run(capi.RESTIR_BIASED)
    for s in (u, b):
        info = s[4]
        assert s[1].sum() == info["rays_initial"] + info["rays_final"] + info["rays_correction"]
        assert s[1].sum() - s[2].sum() == info["rays_occluded"]
    iu, ib = u[4], b[4]
    assert ib["rays_correction"] == 0 and iu["rays_correction"] > 0 and iu["samples_from_history"] > 0
    assert all(ib[k] == iu[k] for k in ("rays_initial", "rays_final", "history_accepted", "samples_from_history", "pixels_reset"))
    np.testing.assert_array_equal(u[3][..., :3], b[3][..., :3])                   # the same picks: the modes part at step D
    np.testing.assert_array_equal(u[3][..., 4:], b[3][..., 4:])
    for x, y in zip(u[:4], run(capi.RESTIR_UNBIASED)[:4]):
        same(x, y)
    gpu_ctx.direct_restir_temporal(mode=capi.RESTIR_UNBIASED, **kw)               # ... and the context call from that history is the hook's
    for x, y in zip(u[:4], state()):
        same(x, y)
    print(name, iu, ib)


# ---- state ------------------------------------------------------------------------------------------------------------------------------------
def test_the_call_touches_no_other_stage_and_no_other_touches_it(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "scene.xml")
    gpu_ctx.clear_sum()
    gpu_ctx.draw(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(1, 0))
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(1, 0), flags=capi.FLAG_MOMENTS)
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.display(source=capi.DISPLAY_SUM, samples=2)
    gpu_ctx.ambient_occlusion(samples=4, seed=SEED)
    gpu_ctx.direct_lighting(samples=4, seed=SEED)
    gpu_ctx.set_light_candidates(4)
    gpu_ctx.direct_restir(samples=2, seed=SEED, neighbours=2)
    gpu_ctx.reset_stats()
    others = lambda: ((gpu_ctx.read_frame(), gpu_ctx.read_moments(), gpu_ctx.read_denoised(), gpu_ctx.read_temporal(), gpu_ctx.read_svgf(),
                       gpu_ctx.read_display(), gpu_ctx.read_ao()[0], gpu_ctx.read_ao()[1], gpu_ctx.read_sum()) + gpu_ctx.read_direct()
                      + gpu_ctx.read_restir() + (gpu_ctx.read_restir_reservoirs(0), gpu_ctx.read_restir_reservoirs(1)))
    before, stats = others(), gpu_ctx.stats()
    gpu_ctx.direct_restir_temporal(frame=0, seed=SEED)
    gpu_ctx.direct_restir_temporal(frame=1, seed=SEED)
    for a, b in zip(before, others()):
        np.testing.assert_array_equal(a, b)
    assert gpu_ctx.stats() == stats
    mine = lambda: gpu_ctx.read_restir_temporal() + (gpu_ctx.read_restir_temporal_reservoirs(),)
    kept = mine()
    assert kept[0][..., :3].any()
    gpu_ctx.clear_sum()                                                          # ... and the other stages leave this result and its history alone
    gpu_ctx.draw(rng_mode=capi.RNG_PHILOX, max_depth=4, seed=(2, 0))
    gpu_ctx.render(rng_mode=capi.RNG_PHILOX, max_depth=4, sample_count=2, seed=(2, 0), flags=capi.FLAG_MOMENTS)
    gpu_ctx.denoise(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=2)
    gpu_ctx.display(source=capi.DISPLAY_SUM, samples=2)
    gpu_ctx.ambient_occlusion(samples=3, seed=(5, 5))
    gpu_ctx.direct_lighting(samples=3, seed=(5, 5))
    gpu_ctx.direct_restir(samples=3, seed=(5, 5), neighbours=3)
    gpu_ctx.temporal_reset()
    gpu_ctx.svgf_reset()
    for a, b in zip(kept, mine()):
        same(a, b)
    ptr, nbytes = gpu_ctx.restir_temporal_buffer()
    assert ptr and nbytes == kept[0].size * 4 and ptr not in (gpu_ctx.direct_buffer()[0], gpu_ctx.restir_buffer()[0])
    assert gpu_ctx.direct_restir_temporal(frame=2, seed=SEED)["history_accepted"] > 0       # (the history is still there)


def test_the_history_is_dropped_by_resize_both_scene_calls_and_reset(gpu_ctx):
    name = "handmade"
    sc, buf = rtc.scene_of(name)
    u = put(gpu_ctx, name)
    W, H = int(u.screenSize[0]), int(u.screenSize[1])
    L, h = gpu_ctx.L, gpu_ctx.h
    out = np.empty((H, W, 4), np.float32)
    words = np.empty((H, W, 7), np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    def gone():
        p, n = C.c_void_p(), C.c_uint64()
        return (L.mpt_read_restir_temporal(h, out.ctypes.data_as(fp), None, None) == NOT_READY
                and L.mpt_restir_temporal_buffer(h, C.byref(p), C.byref(n)) == NOT_READY
                and L.mpt_read_restir_temporal_reservoirs(h, words.ctypes.data_as(up)) == NOT_READY)

    assert gone()                                                                # (put has made a scene and a size anew)
    for drop in (lambda: (gpu_ctx.resize(W + 1, H), gpu_ctx.resize(W, H)), lambda: gpu_ctx.upload_scene(*buf),
                 lambda: gpu_ctx.build_and_upload(*sc.packed_primitives()), gpu_ctx.restir_temporal_reset):
        assert gpu_ctx.direct_restir_temporal(frame=0, seed=SEED)["history_accepted"] == 0      # no history: the first frame
        assert gpu_ctx.direct_restir_temporal(frame=1, seed=SEED)["history_accepted"] > 0
        assert not gone() and gpu_ctx.read_restir_temporal()[0][..., :3].any()
        drop()
        assert gone()


def test_every_refusal_leaves_the_previous_result_and_history(gpu_ctx):
    from metalpathtracer_amd import capi
    put(gpu_ctx, "cornell.xml")
    gpu_ctx.set_light_candidates(3)
    gpu_ctx.direct_restir_temporal(frame=0, seed=SEED)
    gpu_ctx.direct_restir_temporal(frame=1, seed=SEED)
    state = lambda: gpu_ctx.read_restir_temporal() + (gpu_ctx.read_restir_temporal_reservoirs(),)
    before = state()
    L, h = gpu_ctx.L, gpu_ctx.h
    nan = float("nan")
    bad = [dict(walk=3), dict(walk=-1), dict(mode=2), dict(mode=-1), dict(max_history=capi.RESTIR_TEMPORAL_MAX_HISTORY + 1),
           dict(normal_threshold=nan), dict(depth_tolerance=nan)]
    for kw in bad:
        p = capi.restir_temporal_params(**dict(dict(frame=2, seed=SEED), **kw))
        assert L.mpt_direct_restir_temporal(h, C.byref(p), None) == INVALID, kw
        assert b"restir temporal" in L.mpt_last_error(h), kw
    assert L.mpt_direct_restir_temporal(h, None, None) == INVALID
    g = rtc.guides("cornell.xml", 0)
    with pytest.raises(capi.MptError):
        gpu_ctx.restir_temporal_image(g["ad"], g["nc"], g["u"], None, frame=2, max_history=1025)
    foreign = np.zeros(g["ad"].shape[:2] + (7,), np.uint32)
    foreign[..., 0], foreign[..., 5], foreign[..., 6] = 1 << 20, 1, 1            # a holding reservoir of a light the table does not have
    with pytest.raises(capi.MptError):
        gpu_ctx.restir_temporal_image(g["ad"], g["nc"], g["u"], (g["ad"], g["nc"], g["u"], foreign), frame=2)
    gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_CONE)                          # cone sampling in effect: refused
    p = capi.restir_temporal_params(frame=2, seed=SEED)
    assert L.mpt_direct_restir_temporal(h, C.byref(p), None) == INVALID and b"area" in L.mpt_last_error(h)
    gpu_ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)
    for a, b in zip(before, state()):
        same(a, b)
    info = gpu_ctx.direct_restir_temporal(frame=2, seed=SEED)                     # ... and the call goes on from the history it had
    assert info["history_accepted"] > 0 and info["pixels_reset"] == 0            # (the same camera: every surface pixel taps itself)


# ---- the expectation on the device ------------------------------------------------------------------------------------------------------------
B, FRAMES_B = 48, 6


@pytest.mark.parametrize("name", ["manylights", "cornell.xml"])
def test_unbiased_reuse_has_the_expectation_of_the_direct_pass(gpu_ctx, name):
    """tests/test_gpu_ris.py's scenes at 32 x 32; B batches of FRAMES_B frames along the case's path under different seeds, m = 1.  Frames
    share samples over time and pixels through the taps, so the image mean of the last frame is the unit: D_b = the image mean of
    (temporal - direct N = 1) of batch b at the last camera and |mean_b D_b| <= 5 std_b(D_b) / sqrt(B).  The same figures are printed
    for BIASED and not asserted."""
    from metalpathtracer_amd import capi, host
    from test_gpu_ris import STAT_W, stat_scene
    stat_scene(gpu_ctx, name)
    sc, _ = rtc.scene_of(name)
    us = [host.make_uniforms(STAT_W, STAT_W, sc.getPrimitiveCount(), sc.getTriangleCount(), cam=rtc.camera(name, f)) for f in range(FRAMES_B)]
    gpu_ctx.set_light_candidates(1)
    x = {k: np.empty((B, STAT_W, STAT_W)) for k in ("direct", "unbiased", "biased")}
    ms = dict.fromkeys(x, 0.0)
    accepted = 0
    for b in range(B):
        for key, mode in (("unbiased", capi.RESTIR_UNBIASED), ("biased", capi.RESTIR_BIASED)):
            gpu_ctx.restir_temporal_reset()
            for f, u in enumerate(us):
                gpu_ctx.set_uniforms(u)
                info = gpu_ctx.direct_restir_temporal(frame=f, seed=(b, 2 + mode), walk=capi.WALK_AUTO, mode=mode)
            x[key][b] = gpu_ctx.read_restir_temporal()[0][..., :3].astype(np.float64).mean(-1)
            ms[key] += info["device_ms"]
            accepted += info["history_accepted"]
        info = gpu_ctx.direct_lighting(samples=1, seed=(b, 1), walk=capi.WALK_AUTO)
        x["direct"][b] = gpu_ctx.read_direct()[0][..., :3].astype(np.float64).mean(-1)
        ms["direct"] += info["device_ms"]
    v1 = x["direct"].var(0, ddof=1)
    figures = {}
    for key in ("unbiased", "biased"):
        figures[key] = batch_statistic(x[key], x["direct"])
        v = x[key].var(0, ddof=1)
        print(name, key, "mean D", figures[key][0], "bound", figures[key][1], "image means", x["direct"].mean(), x[key].mean(),
              "sum var(direct) / sum var:", v1.sum() / v.sum(), "device ms of the last frames", ms["direct"], ms[key])
    mean, bound = figures["unbiased"]
    assert accepted > 0 and x["direct"].mean() > 0
    assert bound > 0 and abs(mean) <= bound


# ---- the CLI --------------------------------------------------------------------------------------------------------------------------------------
def run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


W_CLI, H_CLI = 48, 32
PATH_LINES = ("d", "2 d", "mouse 40 0")          # four frames: one step right, two more, a turn
PATH_INPUTS = (dict(move=(1, 0, 0)), dict(move=(1, 0, 0)), dict(move=(1, 0, 0)), dict(rotate=(40, 0)))


def cli_base():
    return [EXE, "--scene", scene_path("scene.xml"), "--width", str(W_CLI), "--height", str(H_CLI), "--seed", "1", "--bvh", "reference"]


def test_cli_restir_temporal(tmp_path):
    """mpt_render --camera-path F --direct 1 --restir-temporal writes, frame by frame, what the host layer returns through the same writer,
    and --out gets the last frame; each refusal prints its sentence and exits 2; without the flag --direct N --camera-path F is refused
    as before."""
    from metalpathtracer_amd import capi, host
    p = lambda name: str(tmp_path / name)
    read = lambda name: open(p(name), "rb").read()
    path = p("path.txt")
    with open(path, "w") as f:
        f.write("# three lines\n" + "\n".join(PATH_LINES) + "\n")
    runs = (("u", ["--light-candidates", "4"], dict(max_history=0, mode=capi.RESTIR_UNBIASED)),
            ("b", ["--light-candidates", "4", "--restir-history", "2", "--restir-biased", "--direct-walk", "reference"],
             dict(max_history=2, mode=capi.RESTIR_BIASED, walk=capi.WALK_REFERENCE)))
    for key, extra, kw in runs:
        r = run(cli_base() + ["--camera-path", path, "--out-dir", p(key), "--out", p(key + ".ppm"), "--direct", "1", "--restir-temporal"] + extra)
        assert r.returncode == 0, (key, r.stderr[-2000:])
        lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]       # (the scene loader prints a line of its own)
        frames, last = lines[:-1], lines[-1]
        assert [l["frame"] for l in frames] == [0, 1, 2, 3] and "restir" not in last and "direct" not in last
        assert frames[0]["accepted"] == 0 and frames[0]["from_history"] == 0 and frames[0]["reset"] > 0
        assert all(l["accepted"] > 0 for l in frames[1:]) and sum(l["from_history"] for l in frames) > 0
        rr = host.Renderer(0, scene_path("scene.xml"))
        try:
            rr.drawableSizeWillChange(W_CLI, H_CLI)
            rr.setRenderParams(rng_mode=capi.RNG_PHILOX, seed=(1, 0))
            rr.setLightCandidates(4)
            for f, inp in enumerate(PATH_INPUTS):
                rr.input(**inp)
                rgba, info = rr.drawDirectRestirTemporal(f, **kw)
                assert (frames[f]["accepted"], frames[f]["from_history"], frames[f]["reset"]) == (
                    info["history_accepted"], info["samples_from_history"], info["pixels_reset"]), (key, f)
                assert host.write_ppm(p("mine.ppm"), rgba) == 0
                assert read("mine.ppm") == open(os.path.join(p(key), "frame_%04d.ppm" % f), "rb").read(), (key, f)
            assert read("mine.ppm") == read(key + ".ppm")                         # --out: the last frame
            with pytest.raises(Exception):
                rr.drawDirectRestirTemporal(4, 1025)
        finally:
            rr.close()
    assert read("u.ppm") != read("b.ppm")
    on = ["--camera-path", path, "--out-dir", p("x"), "--direct", "1", "--restir-temporal"]
    for bad, word in ((["--direct", "1", "--restir-temporal", "--out", p("x.ppm")], "--camera-path"),
                      (["--camera-path", path, "--restir-temporal"], "--direct"),
                      (["--camera-path", path, "--direct", "4", "--restir-temporal"], "a frame is one round"),
                      (on + ["--restir", "4"], "--restir K"), (on + ["--light-sampling", "cone"], "cone"), (on + ["--temporal"], "--temporal"),
                      (on + ["--svgf"], "--svgf"), (on + ["--denoise"], "--denoise"), (on + ["--tonemap", "aces"], "the display flags"),
                      (on + ["--gpus", "2"], "--gpus > 1"), (on + ["--checkpoint", p("c")], "--checkpoint"), (on + ["--resume", p("c")], "--resume"),
                      (on + ["--restir-history", "0"], "1..1024"), (on + ["--restir-history", "1025"], "1..1024"),
                      (["--camera-path", path, "--out-dir", p("x"), "--restir-history", "4"], "--restir-temporal")):
        r = run(cli_base() + bad)
        assert r.returncode == 2 and "--restir-" in r.stderr and word in r.stderr, (bad, r.stderr[-500:])
    r = run(cli_base() + ["--camera-path", path, "--out-dir", p("x"), "--direct", "1", "--light-candidates", "8", "--out", p("x.ppm")])
    assert r.returncode == 2 and r.stderr.strip() == "mpt_render: --direct cannot be combined with --camera-path"      # today's sentence
