"""Renders through the lean kernels' short arithmetic (normalize3<true>, cdiv_chain: mpt_device.h) at sizes that change inside
one context, against the generic kernels (MPT_WL_LEAN=0, a fresh child process) and the megakernel, bit for bit.

The division of the sub-pixel jitter by the image's width and height is admitted per (W, H) by a device check whose answer the context
keeps (mpt_lean_cdiv.h).  The cases run one after another in ONE context — 1023 x 9 and 9 x 1023 at 1 spp (odd sizes, two tile columns
at least, W and H swapped), 70 x 45 at 3 spp, and 70 x 45 again — so that every resize has to refresh that answer and the last case finds
it cached; each must still name the lean kernels on its launch line.  Driven by tests/wl_lean/render_cases.py, as
tests/test_gpu_wavelocal_lean.py is."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SIZES = (((1023, 9), 1), ((9, 1023), 1), ((70, 45), 3), ((70, 45), 3))
CASES = [dict(scene="scene.xml", size=size, spp=spp, depth=8, shards=1, rank=0, rng=1, bsdf=0, mega=True) for size, spp in SIZES]


def _run(d, tag, env):
    cases, out, err = d / "cases.json", d / (tag + ".npz"), d / (tag + ".err")
    cases.write_text(json.dumps(CASES))
    with open(err, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wl_lean", "render_cases.py"), str(cases), str(out)],
                           env=dict(os.environ, MPT_DEBUG_LAUNCH="1", **env), stderr=f, timeout=300)
    text = err.read_text()
    assert r.returncode == 0, text[-2000:]
    kernels, cur = {}, None   # (case, "sync" / "async" / "mega_sync" / ..) -> kernel names of the launches behind that marker
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
    return np.load(out), kernels


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean_math")
    return _run(d, "lean", {}), _run(d, "generic", {"MPT_WL_LEAN": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=["%d-%dx%d-%dspp" % (i, s[0], s[1], spp) for i, (s, spp) in enumerate(SIZES)])
def test_lean_renders_match_generic_and_megakernel_across_resizes(renders, k):
    (lean, lean_k), (gen, gen_k) = renders
    assert lean_k[(k, "sync")] and set(lean_k[(k, "sync")]) == {"k_wavelocal_lean"}, lean_k[(k, "sync")]
    assert len(lean_k[(k, "async")]) >= 2 and set(lean_k[(k, "async")]) == {"k_wavelocal_lean_corun"}, lean_k[(k, "async")]
    assert set(gen_k[(k, "sync")]) == {"k_wavelocal"} and set(gen_k[(k, "async")]) == {"k_wavelocal_corun"}, (gen_k[(k, "sync")], gen_k[(k, "async")])
    assert set(lean_k[(k, "mega_sync")]) == {"k_megakernel"}
    for how in ("sync", "async"):
        a, m, g = lean["%s_%d" % (how, k)], lean["mega_%s_%d" % (how, k)], gen["%s_%d" % (how, k)]
        assert a[..., 3].max() > 0, "nothing rendered"
        assert a.tobytes() == m.tobytes(), "%s: differs from the megakernel in %d pixels" % (how, int((a != m).any(-1).sum()))
        assert a.tobytes() == g.tobytes(), "%s: differs from the generic kernel in %d pixels" % (how, int((a != g).any(-1).sum()))
    assert lean["counts_%d" % k].tolist() == lean["mega_counts_%d" % k].tolist() == gen["counts_%d" % k].tolist()
    assert lean["counts_%d" % k][0] > 0


@pytest.mark.gpu
def test_the_repeated_size_renders_the_same_bytes(renders):
    (lean, _), _ = renders
    for how in ("sync", "async"):
        assert lean["%s_2" % how].tobytes() == lean["%s_3" % how].tobytes()
