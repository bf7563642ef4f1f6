"""The display stage on the device (include/mpt.h, "display") against its numpy restatement (tests/display_ref.py): bytes, histogram
and every info field bit for bit — the stage runs no pow, exp or log, so there is nothing to tolerate."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import display_ref as dr
from conftest import CORNELL_CAM, ROOT, oracle_scene, scene_path

pytestmark = pytest.mark.gpu
F = np.float32
TONES = (dr.CLAMP, dr.REINHARD, dr.ACES)
TRANSFERS = (dr.SRGB, dr.GAMMA22, dr.LINEAR)
NOT_READY, INVALID = 5, 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cu(u):
    from metalpathtracer_amd import capi
    return capi.Uniforms.from_buffer_copy(bytes(u))


def _ref_kw(kw):
    """display_ref.display's keywords from capi.display_params' (the restatement calls its exposure argument exposure_)."""
    kw = dict(kw)
    kw.pop("source", None)
    kw.pop("samples", None)
    if "exposure" in kw:
        kw["exposure_"] = kw.pop("exposure")
    return kw


def _special_values():
    """What a frame can hold besides ordinary radiance, and where the encoding can go wrong: zero, negatives, NaN, the infinities,
    denormals, every threshold of every table with both of its float neighbours, and the tone curves' cap with its neighbours."""
    v = [np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 1e-42, -1e-42, 1.1754942e-38, 1.0, 65504.0, 3.4e38], F)]
    for x in [F(65504.0), F(1.0)] + [t for tr in TRANSFERS for t in dr.table(tr)]:
        v.append(np.array([np.nextafter(x, F(0)), x, np.nextafter(x, F(np.inf))], F))
    return np.concatenate(v)


def _test_image(W, H, seed):
    """Log-uniform over 2^-40 .. 2^40, with the special values scattered over a third of the channels (all of them where they fit)."""
    rng = np.random.default_rng(seed)
    c = np.exp2(rng.uniform(-40, 40, (H, W, 4))).astype(F)
    flat = c[..., :3].reshape(-1).copy()
    sp = _special_values()
    n = min(sp.size, max(1, flat.size // 3)) if flat.size >= 9 else 0
    where = rng.choice(flat.size, n, replace=False)
    flat[where] = sp if n == sp.size else rng.choice(sp, n, replace=False)
    c[..., :3] = flat.reshape(H, W, 3)
    return c


def _check(got, want, what):
    out, hist, info = got
    wout, whist, winfo, _ = want
    assert np.array_equal(hist, whist), what
    assert dr.same_info(info, winfo), (what, info, winfo)
    assert np.array_equal(out, wout), (what, int((out != wout).sum()))


@pytest.mark.parametrize("W,H", [(1, 1), (37, 23), (128, 64)])
def test_display_image_matches_restatement_bit_for_bit(gpu_ctx, W, H):
    c = _test_image(W, H, 100 + W)
    if W == 128:
        assert np.isin(_bits(_special_values()), _bits(c[..., :3])).all()
    for tone, transfer in itertools.product(TONES, TRANSFERS):
        for kw in (dict(), dict(exposure=0.37), dict(auto_exposure=True), dict(auto_exposure=True, exposure=3.0, white=1.5, percentile=90, key=0.5)):
            kw = dict(kw, tone=tone, transfer=transfer)
            _check(gpu_ctx.display_image(c, **kw), dr.display(c, **_ref_kw(kw)), (W, H, kw))
    # the thresholds themselves, unscaled: the values that decide whether the code is the correctly rounded one
    for transfer in TRANSFERS:
        T = dr.table(transfer)
        t = np.zeros((H, W, 4), F)
        near = np.concatenate([np.nextafter(T, F(0)), T, np.nextafter(T, F(1))])
        t[..., :3] = np.resize(near, H * W * 3).reshape(H, W, 3)
        _check(gpu_ctx.display_image(t, transfer=transfer), dr.display(t, transfer=transfer), (W, H, transfer))
        if W == 128:
            k = np.arange(1, 256)
            tt = np.zeros((1, 255 * 3, 4), F)
            tt[0, :, 0] = near
            code = gpu_ctx.display_image(tt, transfer=transfer)[0][0, :, 0].astype(int)
            assert np.array_equal(code[:255], k - 1) and np.array_equal(code[255:510], k) and np.array_equal(code[510:], k)


def test_histogram_corners(gpu_ctx):
    from metalpathtracer_amd import capi
    # one luminance: every lane of every wave in one bin
    c = np.empty((256, 256, 4), F)
    c[...] = [0.3, 0.5, 0.2, 1.0]
    out, hist, info = gpu_ctx.display_image(c, auto_exposure=True, tone=dr.REINHARD)
    _check((out, hist, info), dr.display(c, auto_exposure=True, tone=dr.REINHARD), "one luminance")
    assert hist.max() == 256 * 256 == info["pixels_counted"] and np.count_nonzero(hist) == 1 and info["key_bin"] == int(np.argmax(hist))
    # two luminances side by side in every wave, and an uncounted one
    c[:, 1::2, :3] = [4.0, 5.0, 6.0]
    c[:, ::7, :3] = 0
    _check(gpu_ctx.display_image(c, auto_exposure=True), dr.display(c, auto_exposure=True), "two luminances")
    # all black: nothing counted, the scale is the exposure
    z = np.zeros((48, 40, 4), F)
    out, hist, info = gpu_ctx.display_image(z, auto_exposure=True, exposure=2.0)
    assert not hist.any() and info["pixels_counted"] == 0 and info["key_bin"] == capi.DISPLAY_NO_BIN
    assert info["scale"] == 2 and info["auto_scale"] == 1 and not out[..., :3].any() and (out[..., 3] == 255).all()
    # the percentiles, over bins 0 and 255 too: values below 2^-32 and above 2^32
    rng = np.random.default_rng(3)
    r = np.exp2(rng.uniform(-45, 45, (40, 70, 4))).astype(F)
    r[0, :5, :3] = 2.0 ** -40
    r[1, :5, :3] = 2.0 ** 40
    keys = []
    for p in (1, 50, 100):
        got = gpu_ctx.display_image(r, auto_exposure=True, percentile=p)
        _check(got, dr.display(r, auto_exposure=True, percentile=p), ("percentile", p))
        keys.append(got[2]["key_bin"])
    assert got[1][0] > 0 and got[1][255] > 0 and keys[0] < keys[1] < keys[2] and keys[2] == 255
    lo = np.full((8, 8, 4), 2.0 ** -60, F)
    hi = np.full((8, 8, 4), 2.0 ** 60, F)
    assert gpu_ctx.display_image(lo, auto_exposure=True)[1][0] == 64 and gpu_ctx.display_image(hi, auto_exposure=True)[1][255] == 64


def _show_sum(ctx, img, **kw):
    """A frame through the context's own state, without a scene: the image is written into the HDR sum (x / 1 is x)."""
    ctx.write_sum(img)
    info = ctx.display(source=0, samples=1, **kw)
    return ctx.read_display(), ctx.read_display_histogram(), info


def test_adaptation_and_what_forgets_it():
    from metalpathtracer_amd import capi
    W, H = 40, 24
    rng = np.random.default_rng(9)
    imgs = [np.exp2(rng.uniform(lo, lo + 12, (H, W, 4))).astype(F) for lo in (-8, 0, -14, -3, 2, -6, -1, -9, 1, -4)]
    kw = dict(auto_exposure=True, adaptation=0.25, tone=dr.ACES)
    ctx = capi.Context(0)
    try:
        for call in (ctx.read_display, ctx.display_buffer, ctx.read_display_histogram):
            with pytest.raises(capi.MptError) as e:
                call()
            assert e.value.status == NOT_READY                   # before mpt_resize
        with pytest.raises(capi.MptError) as e:
            ctx.display(source=0, samples=1)
        assert e.value.status == NOT_READY
        ctx.resize(W, H)
        for call in (ctx.read_display, ctx.display_buffer, ctx.read_display_histogram):
            with pytest.raises(capi.MptError) as e:
                call()
            assert e.value.status == NOT_READY                   # before the first mpt_display
        ctx.display_reset()                                      # (nothing to forget yet: not an error)
        kept = None
        scales = []
        for i in range(3):                                       # three smoothed calls: the restatement's three scales
            want = dr.display(imgs[i], prev=kept, **_ref_kw(kw))
            _check(_show_sum(ctx, imgs[i], **kw), want, ("adaptation", i))
            kept = want[3]
            scales.append(want[2]["auto_scale"])
        assert len({float(s) for s in scales}) == 3
        assert ctx.display_buffer()[1] == W * H * 4
        # a call without auto_exposure leaves the kept scale and the histogram alone
        h_before = ctx.read_display_histogram()
        out, h_after, info = _show_sum(ctx, imgs[3], exposure=0.5)
        assert np.array_equal(out, dr.display(imgs[3], exposure_=0.5)[0]) and np.array_equal(h_before, h_after)
        assert info["auto_scale"] == 1 and info["scale"] == 0.5 and info["key_bin"] == capi.DISPLAY_NO_BIN and info["pixels_counted"] == 0
        want = dr.display(imgs[4], prev=kept, **_ref_kw(kw))
        _check(_show_sum(ctx, imgs[4], **kw), want, "after a call without auto_exposure")
        kept = want[3]
        # what makes the next call unsmoothed
        sc, buf = oracle_scene("cornell.xml")
        forgets = [("display_reset", ctx.display_reset), ("resize", lambda: ctx.resize(W, H)), ("upload_scene", lambda: ctx.upload_scene(*buf)),
                   ("build_and_upload", lambda: ctx.build_and_upload(buf[1], buf[2]))]
        for i, (what, forget) in enumerate(forgets):
            forget()
            if what != "display_reset":
                with pytest.raises(capi.MptError) as e:
                    ctx.read_display()
                assert e.value.status == NOT_READY, what         # the buffers were dropped with the state
            want = dr.display(imgs[5 + i], prev=None, **_ref_kw(kw))
            _check(_show_sum(ctx, imgs[5 + i], **kw), want, what)
            assert _bits(want[2]["auto_scale"]) != _bits(dr.display(imgs[5 + i], prev=kept, **_ref_kw(kw))[2]["auto_scale"]), what
            kept = want[3]
        want = dr.display(imgs[9], prev=kept, **_ref_kw(kw))     # ... and the one after that is smoothed again
        _check(_show_sum(ctx, imgs[9], **kw), want, "smoothed again")
        # the unit hook takes the kept scale as an argument and leaves the context's alone
        _check(ctx.display_image(imgs[0], prev_auto_scale=kept, **kw), dr.display(imgs[0], prev=kept, **_ref_kw(kw)), "hook with a previous scale")
    finally:
        ctx.close()


def _cornell(W, H):
    from metalpathtracer_amd import capi
    from oracle import binding as ob
    sc, buf = oracle_scene("cornell.xml")
    ctx = capi.Context(0)
    ctx.upload_scene(*buf)
    ctx.resize(W, H)
    u0 = _cu(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=CORNELL_CAM))
    cam1 = dict(CORNELL_CAM, pos=(0.05, 1.0, 3.4))
    u1 = _cu(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=cam1))
    return ctx, u0, u1


def test_every_source_on_the_cornell_box():
    from metalpathtracer_amd import capi
    W, H, spp = 64, 48, 8
    ctx, u0, u1 = _cornell(W, H)
    kw = dict(tone=dr.ACES, auto_exposure=True)
    rk = _ref_kw(kw)
    try:
        ctx.set_uniforms(u0)
        for src in (capi.DISPLAY_DENOISED, capi.DISPLAY_TEMPORAL, capi.DISPLAY_SVGF, capi.DISPLAY_ADAPTIVE):
            with pytest.raises(capi.MptError) as e:
                ctx.display(source=src, **kw)
            assert e.value.status == NOT_READY, src
        with pytest.raises(capi.MptError) as e:
            ctx.read_display()
        assert e.value.status == NOT_READY                      # (a refused call shows nothing)

        def shown(src, samples=0):
            ctx.display_reset()
            info = ctx.display(source=src, samples=samples, **kw)
            return ctx.read_display(), ctx.read_display_histogram(), info

        ctx.render(sample_count=spp, max_depth=8)
        total = ctx.read_sum()
        _check(shown(capi.DISPLAY_SUM, spp), dr.display(dr.source_sum(total, spp), **rk), "SUM")
        assert 0 < dr.display(dr.source_sum(total, spp), **rk)[2]["pixels_counted"] <= W * H
        ctx.draw(max_depth=8)
        _check(shown(capi.DISPLAY_FRAME), dr.display(ctx.read_frame(), **rk), "FRAME")
        ctx.denoise(source=capi.DENOISE_SUM, samples=spp)
        _check(shown(capi.DISPLAY_DENOISED), dr.display(ctx.read_denoised(), **rk), "DENOISED")
        for f, u in enumerate((u0, u1)):                         # two frames each, the second from a moved camera
            ctx.set_uniforms(u)
            ctx.clear_sum()
            ctx.render(sample_begin=2 * f, sample_count=2, max_depth=8)
            ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=2)
            ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=2)
        hist_t, hist_s = ctx.read_temporal(), ctx.read_svgf()
        assert hist_t[..., 3].max() > 1 and not np.array_equal(_bits(hist_t[..., :3]), _bits(hist_s[..., :3]))
        _check(shown(capi.DISPLAY_TEMPORAL), dr.display(hist_t, **rk), "TEMPORAL")
        _check(shown(capi.DISPLAY_SVGF), dr.display(hist_s, **rk), "SVGF")
        ctx.denoise_temporal()
        _check(shown(capi.DISPLAY_DENOISED), dr.display(ctx.read_denoised(), **rk), "DENOISED (temporal)")
        ctx.set_uniforms(u0)
        for thr in (0.4, 0.25, 0.15, 0.08):                      # a threshold that leaves the tiles at different counts
            ctx.render_adaptive(thr, min_samples=2, batch_samples=2, sample_count=16, max_depth=8)
            counts = ctx.read_tile_samples()
            if len(np.unique(counts)) >= 3:
                break
        assert len(np.unique(counts)) >= 2, np.unique(counts)
        mean = dr.source_adaptive(ctx.read_sum(), capi.expand_tile_counts(counts, H, W))
        _check(shown(capi.DISPLAY_ADAPTIVE), dr.display(mean, **rk), "ADAPTIVE")
        assert np.array_equal(_bits(mean), _bits(ctx.read_adaptive_mean()[..., :3]))
        # every tone curve and transfer function from a real source too, without auto-exposure
        for tone, transfer in itertools.product(TONES, TRANSFERS):
            k2 = dict(tone=tone, transfer=transfer, exposure=1.7)
            info = ctx.display(source=capi.DISPLAY_ADAPTIVE, **k2)
            want = dr.display(mean, **_ref_kw(k2))
            assert np.array_equal(ctx.read_display(), want[0]) and dr.same_info(info, want[2]), (tone, transfer)
    finally:
        ctx.close()


def test_odd_size_adaptive_tiles_and_both_store_widths(tmp_path):
    """37 x 23: edge tiles cut by the border and a pixel count that is no multiple of four, through the forms the other tests do not run
    — the one-pixel k_dp_present and the plain k_dp_histogram, which must give the same bytes as the defaults (a child process: the
    forms are chosen from the environment when a context is created)."""
    import sys
    script = tmp_path / "forms.py"
    script.write_text(
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import display_ref as dr\n"
        "from metalpathtracer_amd import capi\n"
        "from conftest import CORNELL_CAM, oracle_scene\n"
        "from oracle import binding as ob\n"
        "W, H = 37, 23\n"
        "sc, buf = oracle_scene('cornell.xml')\n"
        "ctx = capi.Context(0)\n"
        "ctx.upload_scene(*buf); ctx.resize(W, H)\n"
        "ctx.set_uniforms(capi.Uniforms.from_buffer_copy(bytes(ob.make_uniforms(W, H, sc.prim_count, sc.triangle_count, cam=CORNELL_CAM))))\n"
        "ctx.render_adaptive(0.3, min_samples=2, batch_samples=2, sample_count=12, max_depth=8)\n"
        "counts = ctx.read_tile_samples()\n"
        "mean = dr.source_adaptive(ctx.read_sum(), capi.expand_tile_counts(counts, H, W))\n"
        "for kw in (dict(tone=2, auto_exposure=True), dict(tone=1, transfer=1, exposure=2.0)):\n"
        "    info = ctx.display(source=capi.DISPLAY_ADAPTIVE, **kw)\n"
        "    rk = dict(kw); rk['exposure_'] = rk.pop('exposure', 0.0)\n"
        "    want = dr.display(mean, **rk)\n"
        "    assert np.array_equal(ctx.read_display(), want[0]) and dr.same_info(info, want[2]), kw\n"
        "    assert not kw.get('auto_exposure') or np.array_equal(ctx.read_display_histogram(), want[1])\n"
        "rng = np.random.default_rng(1)\n"
        "c = np.exp2(rng.uniform(-20, 20, (H, W, 4))).astype(np.float32)\n"
        "out, hist, info = ctx.display_image(c, tone=2, auto_exposure=True)\n"
        "want = dr.display(c, tone=2, auto_exposure=True)\n"
        "assert np.array_equal(out, want[0]) and np.array_equal(hist, want[1]) and dr.same_info(info, want[2])\n"
        "ctx.close()\n"
        "print('forms ok', len(np.unique(counts)))\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, MPT_DISPLAY_PX="1", MPT_DISPLAY_HIST="plain")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "forms ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_no_side_effects_and_async():
    """(A queued render that FAILS is reported by mpt_display through the same drain-then-wait path as mpt_denoise; it is not exercised
    here: only a HIP error or a ring overflow makes a queued render fail, and neither can be had harmlessly.)"""
    from metalpathtracer_amd import capi
    W, H = 64, 48
    ctx, u0, u1 = _cornell(W, H)
    try:
        ctx.set_uniforms(u0)
        ctx.draw(max_depth=8)
        ctx.render(sample_count=4, max_depth=8, flags=capi.FLAG_MOMENTS)
        ctx.denoise(source=capi.DENOISE_SUM, samples=4)
        ctx.temporal_accumulate(source=capi.DENOISE_SUM, samples=4)
        ctx.svgf_accumulate(source=capi.DENOISE_SUM, samples=4)

        def state():
            return [ctx.read_sum(), ctx.read_frame(), ctx.read_moments(), ctx.read_denoised(), ctx.read_temporal(), ctx.read_svgf(),
                    *ctx.read_svgf_state()], ctx.stats()

        before, st0 = state()
        for src in (capi.DISPLAY_SUM, capi.DISPLAY_FRAME, capi.DISPLAY_DENOISED, capi.DISPLAY_TEMPORAL, capi.DISPLAY_SVGF):
            ctx.display(source=src, samples=4, tone=dr.REINHARD, auto_exposure=True, adaptation=0.5)
            ctx.read_display()
        after, st1 = state()
        assert st0 == st1
        for a, b in zip(before, after):
            assert np.array_equal(_bits(a), _bits(b))
        # asynchronous renders, displayed without an explicit wait: the finished sum
        ctx.clear_sum()
        ctx.render_async(sample_count=2, max_depth=8)
        ctx.render_async(sample_begin=2, sample_count=2, max_depth=8)
        info = ctx.display(source=capi.DISPLAY_SUM, samples=4, tone=dr.ACES)
        got = ctx.read_display()
        ctx.wait()
        want = dr.display(dr.source_sum(ctx.read_sum(), 4), tone=dr.ACES)
        assert np.array_equal(got, want[0]) and dr.same_info(info, want[2])
    finally:
        ctx.close()


def test_argument_errors_change_nothing():
    from metalpathtracer_amd import capi
    import ctypes as C
    W, H = 24, 16
    rng = np.random.default_rng(2)
    img = np.exp2(rng.uniform(-6, 3, (H, W, 4))).astype(F)
    nan = float("nan")
    bad = [dict(source=6), dict(source=-1), dict(tone=3), dict(tone=-1), dict(transfer=3), dict(transfer=-1), dict(source=0, samples=0),
           dict(percentile=101), dict(exposure=nan), dict(white=nan), dict(key=nan), dict(adaptation=nan)]
    ctx = capi.Context(0)
    try:
        ctx.resize(W, H)
        ctx.write_sum(img)
        kw = dict(source=0, samples=1, auto_exposure=True, adaptation=0.5)
        ctx.display(**kw)
        shown, hist = ctx.read_display(), ctx.read_display_histogram()
        for b in bad:
            with pytest.raises(capi.MptError) as e:
                ctx.display(**dict(dict(source=0, samples=1, auto_exposure=True), **b))
            assert e.value.status == INVALID, b
            assert np.array_equal(ctx.read_display(), shown) and np.array_equal(ctx.read_display_histogram(), hist), b
            if "source" not in b:                                  # (the unit hook ignores source and samples)
                with pytest.raises(capi.MptError) as e:
                    ctx.display_image(img, **b)
                assert e.value.status == INVALID, b
        assert ctx.L.mpt_display(ctx.h, None, None) == INVALID and ctx.L.mpt_display(None, None, None) == INVALID
        assert ctx.L.mpt_read_display(ctx.h, None) == INVALID and ctx.L.mpt_read_display_histogram(ctx.h, None) == INVALID
        assert ctx.L.mpt_display_buffer(ctx.h, None, None) == INVALID and ctx.L.mpt_display_reset(None) == INVALID
        p = capi.display_params()
        out = (C.c_uint8 * (W * H * 4))()
        assert ctx.L.mpt_display_image(ctx.h, W, H, None, C.byref(p), None, out, None, None) == INVALID
        assert ctx.L.mpt_display_image(ctx.h, 0, H, img.ctypes.data_as(C.POINTER(C.c_float)), C.byref(p), None, out, None, None) == INVALID
        assert ctx.L.mpt_display_image(ctx.h, W, H, img.ctypes.data_as(C.POINTER(C.c_float)), None, None, out, None, None) == INVALID
        assert np.array_equal(ctx.read_display(), shown)
        # the refused calls left the kept auto scale alone as well: the next call smooths from the first one's
        first = dr.display(img, auto_exposure=True)
        img2 = (img * F(8)).astype(F)
        ctx.write_sum(img2)
        info = ctx.display(**kw)
        assert dr.same_info(info, dr.display(img2, auto_exposure=True, adaptation=0.5, prev=first[3])[2])
    finally:
        ctx.close()


EXE = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")


def _ppm(path, W, H):
    raw = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 3, path
    return np.frombuffer(raw[len(head):], np.uint8).reshape(H, W, 3)


def test_cli_batch_with_and_without_the_flags(tmp_path):
    from metalpathtracer_amd import capi, host
    W, H, spp = 64, 48, 8
    base = [EXE, "--scene", scene_path("cornell.xml"), "--width", str(W), "--height", str(H), "--spp", str(spp), "--depth", "8", "--seed", "1",
            "--bvh", "reference"]
    a, b = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    r = subprocess.run(base + ["--out", a, "--tonemap", "aces", "--auto-exposure"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["--out", b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["--out", str(tmp_path / "c.pfm"), "--tonemap", "aces"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and ".ppm" in r.stderr               # a display flag with a .pfm output is an error
    rr = host.Renderer(0, scene_path("cornell.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        rr.clearSum()
        rr.renderBatch(0, spp)
        total = rr.readSum()
        want = dr.display(dr.source_sum(total, spp), tone=dr.ACES, auto_exposure=True)
        assert np.array_equal(_ppm(a, W, H), want[0][..., :3])
        out, info = rr.display(source=capi.DISPLAY_SUM, tone=dr.ACES, auto_exposure=True)   # (samples = 0: what renderBatch added)
        assert np.array_equal(out, want[0]) and dr.same_info(info, want[2])
        today = str(tmp_path / "today.ppm")                        # without the flags: today's path, byte for byte
        assert host.write_ppm(today, total, scale=1.0 / spp) == 0
        assert open(today, "rb").read() == open(b, "rb").read()
        assert not np.array_equal(_ppm(a, W, H), _ppm(b, W, H))
    finally:
        rr.close()


def test_cli_camera_path_temporal_with_adaptation(tmp_path):
    from metalpathtracer_amd import capi, host
    W, H = 64, 48
    path = tmp_path / "path.txt"
    path.write_text("1\n1 d mouse 6 0\n1 w\n")
    out_dir = tmp_path / "runs"
    last = str(tmp_path / "last.ppm")
    r = subprocess.run([EXE, "--scene", scene_path("cornell.xml"), "--width", str(W), "--height", str(H), "--depth", "8", "--seed", "1",
                        "--bvh", "reference", "--camera-path", str(path), "--out-dir", str(out_dir), "--out", last, "--temporal",
                        "--tonemap", "reinhard", "--auto-exposure", "--adaptation", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    frames = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"frame"')]
    assert [f["frame"] for f in frames] == [0, 1, 2]
    rr = host.Renderer(0, scene_path("cornell.xml"))
    try:
        rr.drawableSizeWillChange(W, H)
        rr.setRenderParams(rng_mode=capi.RNG_PHILOX, max_depth=8, seed=(1, 0))
        kept = None
        for f, inp in enumerate([dict(), dict(move=(1, 0, 0), rotate=(6, 0)), dict(move=(0, 0, 1))]):
            rr.input(**inp)
            rr.drawTemporal(1)
            want = dr.display(rr.readTemporal(), tone=dr.REINHARD, auto_exposure=True, adaptation=0.5, prev=kept)
            kept = want[3]
            assert np.array_equal(_ppm(out_dir / ("frame_%04d.ppm" % f), W, H), want[0][..., :3]), f
            assert frames[f]["key_bin"] == want[2]["key_bin"] and frames[f]["clipped"] == want[2]["pixels_clipped"], f
            assert F(frames[f]["scale"]) == want[2]["scale"], f
        assert open(last, "rb").read() == open(out_dir / "frame_0002.ppm", "rb").read()
    finally:
        rr.close()
