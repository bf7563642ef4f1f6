"""GPU tests of the light-sampling kernels on trees that do not fit in LDS (tests/light_big_cases.py): 15,260 primitives whose reference
tree exceeds the largest LDS image the context grants, so MPT_WALK_REFERENCE launches the MPT_AO_REF instantiations (threaded nodes and
primitive records beyond the staged ones come from global memory), and whose own tree does not fit either; 87 material rows, so shading
reads rows from global memory; a patch of coplanar copies, so a good share of the closest-first walks is flagged and re-traced through
the reference tree.  Both routes put the scene on the device: mpt_upload_scene with the host's tree, and mpt_build_and_upload, whose
downloaded tree is the one the references then walk.

Every kernel family — the direct pass and mpt_render_nee, each plain, with the cone, resampled, and resampled with the cone; the
adaptive render with and without the cone; ReSTIR's initial and both merge kernels — is compared bit for bit with the existing
references and count for count with its info struct, under MPT_WALK_REFERENCE on every pixel and under MPT_WALK_OWN on every pixel
without a gap ray (ReSTIR: untainted); MPT_WALK_AUTO must be MPT_WALK_OWN.  tests/test_light_big_cpu.py shows for the host tree that
the exempted pixels stay below their caps; here the same caps are asserted for the downloaded tree before anything is compared."""
import numpy as np
import pytest

import adaptive_ref as ar
import light_big_cases as lb
import nee_adaptive_ref as nar
import nee_ref
import restir_ref

pytestmark = pytest.mark.gpu

SEED = lb.SEED
ROUTES = ("upload", "build")
N_AD, MIN_AD, BATCH_AD = 16, 4, 4           # the schedule of tests/test_gpu_nee_adaptive.py
SCHED = ar.schedule(N_AD, MIN_AD, BATCH_AD)
RESTIR_KEYS = ("pixels_surface", "rays_initial", "rays_final", "rays_correction", "rays_occluded", "neighbours_accepted", "samples_from_neighbours",
               "lights")

_built = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    np.testing.assert_array_equal(bits(a), bits(b))


def walks():
    from metalpathtracer_amd import capi
    return (capi.WALK_REFERENCE, capi.WALK_OWN, capi.WALK_AUTO)


@pytest.fixture(autouse=True)
def _defaults(request, monkeypatch):
    """No build or LDS knob from outside; one candidate and area sampling again afterwards (other files share the session's context)."""
    from metalpathtracer_amd import capi
    for env in capi.knob_env():
        monkeypatch.delenv(env, raising=False)
    ctx = request.getfixturevalue("gpu_ctx")
    yield
    ctx.set_light_candidates(1)
    ctx.set_light_sampling(capi.LIGHT_SAMPLING_AREA)


def put(ctx, route):
    """The scene on the device by `route`, the case's size and camera; returns the Refs over the tree the device holds.  Neither tree
    fits: the reference tree by its size alone, the own tree by what mpt_accel_info reports."""
    from metalpathtracer_amd import capi
    bvh, prims, mats, idx = lb.host_buffers()
    if route == "upload":
        ctx.upload_scene(bvh, prims, mats, idx)
        refs = lb.host_refs()
    else:
        ctx.build_and_upload(prims, mats)
        dbvh, didx = ctx.download_bvh()
        if "refs" not in _built:
            _built["refs"] = lb.Refs((dbvh, prims, mats, didx))
        refs = _built["refs"]
        same(dbvh, refs.buf[0])                                              # every build of these arrays is the same tree
        np.testing.assert_array_equal(didx, refs.buf[3])
    ctx.resize(lb.W, lb.H)
    ctx.set_uniforms(refs.u)
    ai, bi = ctx.accel_info(), ctx.build_info()
    assert refs.buf[0].shape[0] * 32 > lb.LDS_MOST
    assert bi["prims"] == prims.shape[0] >= bi["auto_ordered_prims"] == lb.AUTO_ORDERED_PRIMS
    assert bi["threaded_nodes"] >= refs.buf[0].shape[0] and bi["materials"] > lb.LDS_MATS
    assert ai["ordered_ok"] == 1 and ai["auto_pipeline"] == capi.PIPE_ORDERED
    assert ai["lds_nodes"] < ai["nodes"] and ai["lds_prims"] < prims.shape[0]
    return refs


def guides_match(ctx, refs):
    ad, nc, prim = ctx.read_aovs()
    want = refs.guides()
    same(ad, want[0])
    same(nc, want[1])
    np.testing.assert_array_equal(prim, want[2])
    return want


def auto_is_own(results):
    """results: walk -> (arrays, counts).  MPT_WALK_AUTO on a scene of this size is MPT_WALK_OWN, bit for bit."""
    from metalpathtracer_amd import capi
    (a_arr, a_cnt), (o_arr, o_cnt) = results[capi.WALK_AUTO], results[capi.WALK_OWN]
    for x, y in zip(a_arr, o_arr):
        same(x, y)
    assert a_cnt == o_cnt


# ---- the scene on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_the_scene_on_the_device(gpu_ctx, route):
    """The light table is direct_ref.light_table bit for bit; the guides are the oracle's; Lambert and emitter rows beyond the 32 that LDS
    holds are first hits by this route's own numbering of the rows."""
    refs = put(gpu_ctx, route)
    want = refs.table
    ids, rec, cdf = gpu_ctx.read_lights()
    np.testing.assert_array_equal(ids, want.ids)
    same(rec, want.rec)
    same(cdf, want.cdf)
    assert gpu_ctx.light_info() == dict(lights=want.n, emissive_prims=want.seen, triangle_lights=int((want.rec[:, 0, 3] == 1).sum()),
                                        sphere_lights=int((want.rec[:, 0, 3] == 0).sum()))
    assert want.n == 1 + lb.N_TRI_LIGHTS
    _, _, prim = guides_match(gpu_ctx, refs)
    arrays, counts = gpu_ctx.read_scene()
    lambert, emitter = lb.material_rows_seen(prim, lb.rows_of_records(arrays["prims"]), refs.buf[2])
    ai = gpu_ctx.accel_info()
    print(route, counts, "own nodes", ai["nodes"], "lds_nodes", ai["lds_nodes"], "lds_prims", ai["lds_prims"], "reference nodes", refs.buf[0].shape[0],
          "Lambert rows seen", lambert.size, "beyond the LDS table", int((lambert >= lb.LDS_MATS).sum()), "emitter rows seen", emitter.size, "beyond",
          int((emitter >= lb.LDS_MATS).sum()))
    assert counts["n_mats"] > lb.LDS_MATS
    assert (lambert >= lb.LDS_MATS).any() and (emitter >= lb.LDS_MATS).any()


@pytest.mark.parametrize("route", ROUTES)
def test_closest_hits_of_the_primary_rays(gpu_ctx, route):
    """mpt_trace_rays and mpt_trace_rays_ordered against the oracle on the case's primary rays: t, primitive, normal and face.  At
    least 5 % of the closest-first walks are flagged — the copies tie — so the re-trace through the reference tree in global memory
    is exercised by every render below."""
    refs = put(gpu_ctx, route)
    o, d = lb.primary_rays(refs.u)
    want = [refs.first_hit(o[i], d[i], refs.buf) for i in range(o.shape[0])]
    t_w = np.array([np.float32(w[0]) for w in want], np.float32)
    p_w = np.array([w[1] for w in want], np.int32)
    n_w = np.array([w[2] for w in want], np.float32)
    f_w = np.array([w[3] for w in want], np.int32)
    hit = p_w >= 0
    np.testing.assert_array_equal(p_w.reshape(lb.H, lb.W), refs.guides()[2])      # (these are the guides' rays)
    t0, p0, n0, f0 = gpu_ctx.trace_rays(o, d)
    t1, p1, n1, f1, flags = gpu_ctx.trace_rays_ordered(o, d)
    for t, p, n, f in ((t0, p0, n0, f0), (t1, p1, n1, f1)):
        np.testing.assert_array_equal(p, p_w)
        same(t[hit], t_w[hit])
        same(n[hit], n_w[hit])
        np.testing.assert_array_equal(f[hit] != 0, f_w[hit] != 0)
        assert np.isinf(t[~hit]).all()
    share = float((flags != 0).mean())
    print(route, "flagged share of the primary rays", share, "flags", dict(zip(*np.unique(flags, return_counts=True))), "hits", int(hit.sum()))
    assert share >= 0.05


# ---- the direct pass: k_direct, k_direct_cone, k_direct_ris, k_direct_ris_cone ---------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name,M,sampling", lb.DIRECT_FAMILIES, ids=[f[0] for f in lb.DIRECT_FAMILIES])
def test_the_direct_pass(gpu_ctx, name, M, sampling, route):
    from metalpathtracer_amd import capi
    refs = put(gpu_ctx, route)
    _, nc, _ = guides_match(gpu_ctx, refs)
    gpu_ctx.set_light_candidates(M)
    gpu_ctx.set_light_sampling(sampling)
    r = refs.direct(M, sampling)
    want, gap = r["want"], r["gap"]
    surface = nc[..., 3] == 0
    print(name, route, "gap pixels", int(gap.sum()), "of", gap.size)
    assert gap.sum() <= lb.GAP_CAP * gap.size
    assert want[1].sum() > want[2].sum() > 0                                 # open and occluded shadow rays both occur
    results = {}
    for walk in walks():
        info = gpu_ctx.direct_lighting(samples=lb.DIRECT_N, sample_begin=0, seed=SEED, walk=walk)
        got = gpu_ctx.read_direct()
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        print(name, route, "walk", walk, "pixels that differ:", int((bits(got[0]) != bits(want[0])).any(-1).sum()), "traced", info["rays"], "occluded",
              info["rays_occluded"], "ms", info["device_ms"])
        same(got[0][keep], want[0][keep])
        np.testing.assert_array_equal(got[1], want[1])                       # (what is traced does not depend on the walk)
        np.testing.assert_array_equal(got[2][keep], want[2][keep])
        assert info["pixels_surface"] == surface.sum() and info["rays"] == want[1].sum() and info["lights"] == refs.table.n
        assert info["rays_occluded"] == int(got[1].sum()) - int(got[2].sum())
        if keep.all():
            assert info["rays_occluded"] == int(want[1].sum()) - int(want[2].sum())
        assert (got[0][~surface] == (0, 0, 0, 1)).all() and (got[1][~surface] == 0).all() and (got[2][~surface] == 0).all()
        info.pop("device_ms")
        results[walk] = (got, info)
    auto_is_own(results)


# ---- mpt_render_nee: k_nee, k_nee_cone, k_nee_ris, k_nee_ris_cone ----------------------------------------------------------------------------
def nee_kw(walk, **more):
    from metalpathtracer_amd import capi
    return dict(walk=walk, clamp=0.0, rng_mode=capi.RNG_PHILOX, bsdf_mode=capi.BSDF_LAMBERT, max_depth=lb.NEE_DEPTH, seed=SEED, **more)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name,M,sampling", lb.NEE_FAMILIES, ids=[f[0] for f in lb.NEE_FAMILIES])
def test_the_render(gpu_ctx, name, M, sampling, route):
    from metalpathtracer_amd import capi
    refs = put(gpu_ctx, route)
    gpu_ctx.set_light_candidates(M)
    gpu_ctx.set_light_sampling(sampling)
    r = refs.nee(M, sampling)
    want = nee_ref.accumulate(r["value"])
    gap = r["gap"].any(-1)
    rays, shadow, occluded = (int(r[k].sum()) for k in ("rays", "shadow", "occluded"))
    print(name, route, "gap pixels", int(gap.sum()), "of", gap.size)
    assert gap.sum() <= lb.GAP_CAP * gap.size
    assert shadow > occluded > 0
    results = {}
    for walk in walks():
        gpu_ctx.clear_sum()
        gpu_ctx.reset_stats()
        info = gpu_ctx.render_nee(sample_count=lb.NEE_SPP, **nee_kw(walk))
        got = gpu_ctx.read_sum()
        keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
        print(name, route, "walk", walk, "pixels that differ:", int((bits(got) != bits(want)).any(-1).sum()), "rays", info["rays"], "shadow",
              info["shadow_rays"], "occluded", info["shadow_rays_occluded"], "ms", info["device_ms"])
        same(got[keep], want[keep])
        assert info["paths"] == gap.size * lb.NEE_SPP and info["rays"] == rays and info["shadow_rays"] == shadow and info["lights"] == refs.table.n
        if keep.all():
            assert info["shadow_rays_occluded"] == occluded
        st = gpu_ctx.stats()
        assert st["paths"] == info["paths"] and st["rays"] == info["rays"]
        info.pop("device_ms")
        results[walk] = ((got,), info)
    auto_is_own(results)


# ---- mpt_render_nee_adaptive: k_nee_adaptive, k_nee_adaptive_cone ----------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("sampling", (lb.AREA, lb.CONE), ids=("nee_adaptive", "nee_adaptive_cone"))
def test_the_adaptive_render(gpu_ctx, sampling, route):
    """As tests/test_gpu_nee_adaptive.py: the per-sample values of every pixel from single-sample mpt_render_nee calls with the same walk
    (the first NEE_SPP of them are the reference's own, checked here), joined by tests/nee_adaptive_ref.py into running sums and moments;
    every tile holds both at its own count.  With a threshold of 0 every tile runs to the end and the call is mpt_render_nee's, counts
    included."""
    from metalpathtracer_amd import capi
    refs = put(gpu_ctx, route)
    gpu_ctx.set_light_sampling(sampling)
    r = refs.nee(1, sampling)
    gap = r["gap"].any(-1)
    assert gap.sum() <= lb.GAP_CAP * gap.size
    results = {}
    thr = None
    for walk in walks():
        if walk != capi.WALK_AUTO:
            vs = []
            for s in range(N_AD):
                gpu_ctx.clear_sum()
                gpu_ctx.render_nee(sample_begin=s, sample_count=1, **nee_kw(walk))
                vs.append(gpu_ctx.read_sum())
            keep = np.ones_like(gap) if walk == capi.WALK_REFERENCE else ~gap
            for s in range(lb.NEE_SPP):
                same(vs[s][keep], r["value"][:, :, s][keep])
            sums, moms = nar.running(np.stack(vs))
            thr = float(np.float32(np.quantile(ar.tile_errors(sums[MIN_AD], moms[MIN_AD], MIN_AD), 0.3)))
        kw = dict(min_samples=MIN_AD, batch_samples=BATCH_AD, sample_begin=0, sample_count=N_AD)
        out = gpu_ctx.render_nee_adaptive(thr, **nee_kw(walk, **kw))
        counts, got_s, got_m = gpu_ctx.read_tile_samples(), gpu_ctx.read_sum(), gpu_ctx.read_moments()
        if walk != capi.WALK_AUTO:
            per_px = capi.expand_tile_counts(counts, lb.H, lb.W)
            want_s, want_m = nar.at_counts(sums, per_px), nar.at_counts(moms, per_px)
            print(route, "sampling", sampling, "walk", walk, "threshold", thr, "counts", dict(zip(*np.unique(counts, return_counts=True))),
                  "pixels that differ: sum", int((bits(got_s) != bits(want_s)).any(-1).sum()), "moments", int((bits(got_m) != bits(want_m)).any(-1).sum()), out)
            assert np.isin(counts, SCHED).all() and len(np.unique(counts)) >= 2
            same(got_s, want_s)
            same(got_m, want_m)
            a = out["adaptive"]
            assert a["samples"] == int(per_px.astype(np.int64).sum()) == out["nee"]["paths"]
            assert a["tiles_at_max"] == int((counts == N_AD).sum()) and a["tiles_converged"] == int((counts != N_AD).sum())
            assert a["passes"] == max(nar.steps_taken(int(c), MIN_AD, BATCH_AD) for c in counts.ravel())
            assert out["nee"]["lights"] == refs.table.n
        # threshold 0: every tile takes all N_AD samples; the sum and every count are mpt_render_nee's
        full = gpu_ctx.render_nee_adaptive(0.0, **nee_kw(walk, **kw))
        full_s, full_m = gpu_ctx.read_sum(), gpu_ctx.read_moments()
        assert (gpu_ctx.read_tile_samples() == N_AD).all()
        assert full["adaptive"]["tiles_at_max"] == counts.size and full["adaptive"]["tiles_converged"] == 0 and full["adaptive"]["passes"] == len(SCHED)
        gpu_ctx.clear_sum()
        plain = gpu_ctx.render_nee(sample_begin=0, sample_count=N_AD, **nee_kw(walk))
        same(full_s, gpu_ctx.read_sum())
        for k in ("paths", "rays", "shadow_rays", "shadow_rays_occluded", "lights"):
            assert full["nee"][k] == plain[k], k
        assert full["adaptive"]["samples"] == plain["paths"] == gap.size * N_AD
        if walk != capi.WALK_AUTO:
            same(full_s, sums[N_AD])
            same(full_m, moms[N_AD])
        for o in (out, full):
            o["nee"].pop("device_ms")
        results[walk] = ((counts, got_s, got_m, full_s, full_m), (out, full))
    auto_is_own(results)


# ---- mpt_direct_restir: k_restir_initial, k_restir_merge<unbiased>, k_restir_merge<biased> ---------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mode", restir_ref.MODES, ids=("restir_unbiased", "restir_biased"))
def test_restir(gpu_ctx, mode, route):
    """The image, the counts, the info totals and both reservoir read-backs (the initial ones are k_restir_initial's)."""
    from metalpathtracer_amd import capi
    refs = put(gpu_ctx, route)
    _, nc, _ = guides_match(gpu_ctx, refs)
    p = lb.RESTIR
    gpu_ctx.set_light_candidates(p["M"])
    ref = refs.restir()
    want = ref[mode]
    surface = nc[..., 3] == 0
    tainted = want["tainted"]
    print("restir", route, "mode", mode, "tainted", int(tainted.sum()), "of", tainted.size)
    assert tainted.sum() <= lb.TAINT_CAP * tainted.size
    assert want["info"]["samples_from_neighbours"] > 0 and want["traced"].sum() > want["unoccluded"].sum() > 0
    results = {}
    for walk in walks():
        info = gpu_ctx.direct_restir(walk=walk, samples=p["N"], sample_begin=p["begin"], seed=SEED, neighbours=p["K"], radius=p["R"], mode=mode)
        rgba, traced, unocc = gpu_ctx.read_restir()
        initial, pick = gpu_ctx.read_restir_reservoirs(0), gpu_ctx.read_restir_reservoirs(1)
        keep = np.ones_like(surface) if walk == capi.WALK_REFERENCE else ~tainted
        print("restir", route, "mode", mode, "walk", walk, "pixels that differ:", int((bits(rgba) != bits(want["rgba"])).any(-1).sum()),
              {k: info[k] for k in RESTIR_KEYS}, "ms", info["device_ms"])
        same(rgba[keep], want["rgba"][keep])
        np.testing.assert_array_equal(traced[keep], want["traced"][keep])
        np.testing.assert_array_equal(unocc[keep], want["unoccluded"][keep])
        np.testing.assert_array_equal(initial[keep], ref["initial"][keep])
        np.testing.assert_array_equal(pick[keep], want["pick"][keep])
        if keep.all():
            assert {k: info[k] for k in RESTIR_KEYS} == want["info"]
        assert traced.sum() == info["rays_initial"] + info["rays_final"] + info["rays_correction"]
        assert traced.sum() - unocc.sum() == info["rays_occluded"]
        assert (rgba[~surface] == (0, 0, 0, 1)).all() and (traced[~surface] == 0).all() and (unocc[~surface] == 0).all()
        assert not initial[~surface].any() and not pick[~surface].any()
        results[walk] = ((rgba, traced, unocc, initial, pick), {k: info[k] for k in RESTIR_KEYS})
    auto_is_own(results)
