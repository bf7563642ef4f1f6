"""The lean wave-local trace kernels (k_wavelocal_lean*, mpt_kernels.h) against the megakernel and against the generic kernels.

Renders with the wave-local pipeline, Philox and Lambert run the lean kernels whenever the pass is inside the ranges of their 24-bit index
arithmetic (wl_lean_ok, mpt_wl_lean.h).  Every case is rendered three ways — this build, this build with MPT_WL_LEAN=0 in a fresh child
process (the knob is read when a context is created), the megakernel — by mpt_render and by two back-to-back mpt_render_async into one
sum (the variants that run beside a resolve), and HDR sum, ray count and path count must agree bit for bit.  The MPT_DEBUG_LAUNCH line
names the kernel that ran.

Shapes: the smallest that exercise every changed expression — 70 x 45 is off the tile grid in both axes, 264 x 8 has many tile columns in
one row, 3 and 17 spp take the division by a sample count that is no power of two, 3 shards put nranks and rank into the tile arithmetic,
16 x 1032 makes T * tile_mul pass 2^31 (two tile columns: tile_mul = 2^23, tile rows >= 128).  8 x 8 is ONE tile column: the host
has no tile arithmetic for it (no tile_magic), so that size is outside the lean kernels' range and must report the generic kernel.
bunny20.xml does not fit LDS: ALL_LDS = false and the global primitive records.  (mpt_accel_info describes the closest-first tree; whether the
reference-order tree is resident is read from the launch line instead: the workgroup's LDS bytes against 32 bytes per node.)"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

RNG_LITERAL, RNG_PHILOX, BSDF_LAMBERT, BSDF_SCATTER = 0, 1, 0, 1


def _case(size, spp, depth=8, shards=1, rank=0, scene="scene.xml", rng=RNG_PHILOX, bsdf=BSDF_LAMBERT, lean=True):
    return dict(scene=scene, size=size, spp=spp, depth=depth, shards=shards, rank=rank, rng=rng, bsdf=bsdf, lean=lean, mega=True)


CASES = ([_case(size, spp, lean=size != (8, 8)) for size in ((8, 8), (70, 45), (264, 8)) for spp in (1, 3, 17, 64)] +
         [_case((70, 45), 3, depth=1), _case((264, 8), 64, depth=1),
          _case((70, 45), 17, shards=3, rank=2), _case((264, 8), 64, shards=3, rank=2), _case((70, 45), 1, shards=3, rank=2),
          _case((16, 1032), 1),
          _case((70, 45), 3, rng=RNG_LITERAL, lean=False), _case((70, 45), 3, bsdf=BSDF_SCATTER, lean=False),
          _case((64, 48), 1, scene="bunny20.xml")])


def _run(tmp_path, tag, env):
    cases, out, err = tmp_path / "cases.json", tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    cases.write_text(json.dumps(CASES))
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1", **env)
    with open(err, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wl_lean", "render_cases.py"), str(cases), str(out)], env=e, stderr=f, timeout=300)
    text = err.read_text()
    assert r.returncode == 0, text[-2000:]
    kernels, cur, lds = {}, None, {}   # (case, "sync" / "async" / ..) -> kernel names of the launches behind that marker; LDS bytes per workgroup
    for line in text.splitlines():
        m = re.match(r"CASE (\d+) (\w+)$", line)
        if m:
            cur = (int(m.group(1)), m.group(2))
            kernels[cur] = []
        elif line.startswith("CASE end"):
            cur = None
        elif cur is not None:
            m = re.search(r"\[mpt\] pipeline \d+:.* kernel (\w+)$", line)
            if m:
                kernels[cur].append(m.group(1))
                lds[cur] = int(re.search(r"(\d+) B of LDS", line).group(1))
    return np.load(out), kernels, lds


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    d = tmp_path_factory.mktemp("wl_lean")
    return _run(d, "lean", {}), _run(d, "generic", {"MPT_WL_LEAN": "0"})


@pytest.mark.gpu
def test_bunny20_spills_out_of_lds(renders):
    (lean, _, lds), _ = renders
    k = [i for i, c in enumerate(CASES) if c["scene"] == "bunny20.xml"][0]
    assert int(lean["nodes_bunny20.xml"][0]) * 32 > lds[(k, "sync")] > 0      # ALL_LDS = false: nodes and primitive records from global memory
    assert int(lean["nodes_scene.xml"][0]) * 32 <= lds[(1, "sync")]           # scene.xml: the whole tree is resident


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=["%s-%dx%d-%dspp-d%d-%d/%d-rng%d-bsdf%d" % (c["scene"], c["size"][0], c["size"][1], c["spp"], c["depth"],
                                                                                                 c["rank"], c["shards"], c["rng"], c["bsdf"]) for c in CASES])
def test_lean_kernels_match_megakernel_and_generic(renders, k):
    (lean, lean_k, _), (gen, gen_k, _) = renders
    c = CASES[k]
    want_sync, want_async = ("k_wavelocal_lean", "k_wavelocal_lean_corun") if c["lean"] else ("k_wavelocal", "k_wavelocal_corun")
    assert lean_k[(k, "sync")] and set(lean_k[(k, "sync")]) == {want_sync}, lean_k[(k, "sync")]
    assert len(lean_k[(k, "async")]) >= 2 and set(lean_k[(k, "async")]) == {want_async}, lean_k[(k, "async")]
    assert set(gen_k[(k, "sync")]) == {"k_wavelocal"} and set(gen_k[(k, "async")]) == {"k_wavelocal_corun"}, (gen_k[(k, "sync")], gen_k[(k, "async")])
    assert set(lean_k[(k, "mega_sync")]) == {"k_megakernel"}
    for how in ("sync", "async"):
        a, m, g = lean["%s_%d" % (how, k)], lean["mega_%s_%d" % (how, k)], gen["%s_%d" % (how, k)]
        assert a[..., 3].max() > 0, "nothing rendered"
        assert a.tobytes() == m.tobytes(), "%s: differs from the megakernel in %d pixels" % (how, int((a != m).any(-1).sum()))
        assert a.tobytes() == g.tobytes(), "%s: differs from the generic kernel in %d pixels" % (how, int((a != g).any(-1).sum()))
    assert lean["counts_%d" % k].tolist() == lean["mega_counts_%d" % k].tolist() == gen["counts_%d" % k].tolist()
    assert lean["counts_%d" % k][0] > 0
