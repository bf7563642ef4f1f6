"""Ring-0 steps of the lean wave-local kernels park their few long walks at once (closest_hit_resume, metalpathtracer_amd/csrc/mpt_device.h;
the constants in mpt_lds_cfg.h): a budgeted ring-0 step ends once fewer than N0 of its lanes still walk, the box loop's control runs
every second trip, and N0 and the trip budget are constants of the kernels.  A parked ray resumes with the state it stopped with and
sees the same sequence of tests, so nothing may change.

Six views of tests/ring0_rule/ring_cases.py, 70 x 45, 16 spp, depth 8, Philox, device-built tree — the default view, two close views of
the mesh (every tile general, most bounce rays walk the sub-tree), the ground alone, the horizon through a tile row, two shards — each
by mpt_render (k_wavelocal_lean) and by two back-to-back mpt_render_async steps into one sum (k_wavelocal_lean_corun).  The shipped
library's HDR sum and its ray and path counts must equal, byte for byte, the megakernel's, the generic k_wavelocal's (MPT_WL_LEAN=0), and
those of a -DMPT_LEAN_RING_TESTING build of the library (tests/ring0_rule/_build, made by `make`), whose lean kernels read N0 and the
budget from the configuration block, at the shipped pair, with the rule off (N0 = 0), at N0 = 64 with budget 1 (every unfinished ray is
parked at the first look), N0 = 1, an odd budget (the pair of trips straddles it) and N0 = 24 with budget 12.  A render whose ring
overflow flag is set fails with MPT_ERR_OVERFLOW, and the child process with it: overflow == 0 in all of them.  The shipped library with
a ring knob in the environment must run the generic kernels, since the lean kernels no longer read the knobs.

Control, run once by hand (profiles/r28_ring0_rule.txt): a test build with -DMPT_LEAN_RING_CONTROL, in which a ray parked by the rule's
exit loses its walk, fails all six views.  (Resetting such a ray's node to the entry, or its best hit to none, fails nothing: the first
repeats tests that cannot change the winner, and a ray parked within eight trips has tested boxes, not yet a leaf.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "ring0_rule"))
from ring_cases import PAIRS, RING1_N, SHIPPED, SIZE, SPP, VIEWS  # noqa: E402

TEST_LIB = os.path.join(ROOT, "tests", "ring0_rule", "_build", "libmpt_hip_ringtest.so")


def _run(tmp_path, tag, arms, lib=None):
    out, err = tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1")
    if lib:
        e["MPT_LIB"] = lib
    with open(err, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ring0_rule", "render_ring_cases.py"), str(out)] + arms, env=e, stderr=f, timeout=300)
    text = err.read_text()
    assert r.returncode == 0, text[-2000:]
    kernels, cur = {}, None   # (arm, view, "sync" / "async" / "mega_sync" ..) -> kernel names of the launches behind that marker
    for line in text.splitlines():
        m = re.match(r"RENDER (\S+) (\d+) (\w+)$", line)
        if m:
            cur = (m.group(1), int(m.group(2)), m.group(3))
            kernels[cur] = []
        elif line.startswith("RENDER end"):
            cur = None
        elif cur is not None:
            m = re.search(r"\[mpt\] pipeline \d+:.* kernel (\w+)$", line)
            if m:
                kernels[cur].append(m.group(1))
    return np.load(out), kernels


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    d = tmp_path_factory.mktemp("ring0_rule")
    assert os.path.exists(TEST_LIB), "tests/ring0_rule/_build/libmpt_hip_ringtest.so is not built (make)"
    shipped = _run(d, "shipped", ["lean+mega", "generic", "knob:%d:%d" % SHIPPED])
    test = _run(d, "test", ["%s:%d:%d" % p for p in PAIRS], lib=TEST_LIB)
    return shipped, test


def test_shipped_pair_is_the_header():
    text = open(os.path.join(ROOT, "metalpathtracer_amd", "csrc", "mpt_lds_cfg.h")).read()
    got = [int(re.search(r"#define %s (\d+)u" % n, text).group(1)) for n in ("MPT_LEAN_RING0_N0", "MPT_LEAN_RING0_BUDGET", "MPT_LEAN_RING1_N")]
    assert got == [SHIPPED[0], SHIPPED[1], RING1_N]


@pytest.mark.gpu
@pytest.mark.parametrize("v", range(len(VIEWS)), ids=[x["name"] for x in VIEWS])
def test_ring0_rule_changes_no_bit(renders, v):
    (ship, ship_k), (test, test_k) = renders
    n = VIEWS[v]["shards"]
    W, H = SIZE
    for how, lean_kernel, generic_kernel in (("sync", "k_wavelocal_lean", "k_wavelocal"), ("async", "k_wavelocal_lean_corun", "k_wavelocal_corun")):
        runs = n * (2 if how == "async" else 1)
        assert ship_k[("lean+mega", v, how)] == [lean_kernel] * runs, ship_k[("lean+mega", v, how)]
        assert ship_k[("lean+mega", v, "mega_" + how)] == ["k_megakernel"] * runs
        assert ship_k[("generic", v, how)] == [generic_kernel] * runs
        assert ship_k[("knob", v, how)] == [generic_kernel] * runs, "a ring knob is set: the generic kernels read it, the lean ones do not"
        a, ca = ship["%s_lean+mega_%d" % (how, v)], ship["counts_%s_lean+mega_%d" % (how, v)]
        assert ca[1] == W * H * SPP * (2 if how == "async" else 1) and ca[0] > ca[1], ca
        assert a[..., :3].max() > 0, "nothing rendered"
        others = [("the megakernel", ship["mega_%s_lean+mega_%d" % (how, v)], ship["mega_counts_%s_lean+mega_%d" % (how, v)])]
        others += [("the generic kernel" + (" with the knobs" if arm == "knob" else ""), ship["%s_%s_%d" % (how, arm, v)], ship["counts_%s_%s_%d" % (how, arm, v)])
                   for arm in ("generic", "knob")]
        for name, n0, budget in PAIRS:
            assert test_k[(name, v, how)] == [lean_kernel] * runs, (name, test_k[(name, v, how)])
            others.append(("the test build at N0 = %d, budget %d" % (n0, budget), test["%s_%s_%d" % (how, name, v)], test["counts_%s_%s_%d" % (how, name, v)]))
        for what, b, cb in others:
            assert a.tobytes() == b.tobytes(), "%s %s: differs from %s in %d pixels" % (VIEWS[v]["name"], how, what, int((a != b).any(-1).sum()))
            assert ca.tolist() == cb.tolist(), "%s %s: counts differ from %s: %s, %s" % (VIEWS[v]["name"], how, what, ca.tolist(), cb.tolist())
