"""Fresh rays of the lean wave-local kernels enter the walk below the root (the entry node, metalpathtracer_amd/csrc/mpt_lean_entry.h) against
the generic kernels and the megakernel.

Every case of tests/lean_entry/entry_cases.py is rendered three ways — this build, this build with MPT_WL_LEAN=0 in a fresh child process (the
knob is read when a context is created), the megakernel — by mpt_render (k_wavelocal_lean) and by two back-to-back mpt_render_async
steps into one sum (k_wavelocal_lean_corun); HDR sum, ray count and path count must agree bit for bit.

Cases, 70 x 45, 3 spp, depth 1 and 8: scene.xml from its own camera; at 1023 x 9; from a camera above the root box (primary rays start
at the root, bounce rays below it); from a camera exactly on the shrunk box's lower x plane and one ulp outside it, both taken from the
node array read back; a two-triangle scene whose root is a leaf record; 300 triangles at 2e7, where the staging check fails; two
cameras in one context, one inside the shrunk box and one outside — two mpt_render, then one async step each on the two render lanes;
bunny20.xml at 1 spp, whose tree does not fit LDS (ALL_LDS = false).  For every case the child reads node 0 back (the device's node
array, and the root's box of mpt_download_bvh, which must be the same planes) and the stand-alone program of test_lean_entry_cpu.py
evaluates lean_entry_terms on it with each camera: the case must be on or off as entry_cases.py intends, so none passes vacuously."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "lean_entry"))
from entry_cases import CASES, OFF, ON, PRIMARY_OFF  # noqa: E402


def _run(tmp_path, tag, env):
    out, err = tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1", **env)
    with open(err, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lean_entry", "render_entry_cases.py"), str(out)], env=e, stderr=f, timeout=300)
    text = err.read_text()
    assert r.returncode == 0, text[-2000:]
    kernels, cur = {}, None   # (case, "sync" / "async" / ..) -> kernel names of the launches behind that marker
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
    d = tmp_path_factory.mktemp("lean_entry")
    return _run(d, "lean", {}), _run(d, "generic", {"MPT_WL_LEAN": "0"})


@pytest.fixture(scope="module")
def terms_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lean_entry_terms") / "lean_entry_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lean_entry", "lean_entry_check.cpp"), "-o", exe], check=True)
    return exe


def _terms(exe, node0, n_nodes, cam):
    words = ["%08x" % w for w in node0] + [str(int(n_nodes))] + ["%08x" % w for w in np.asarray(cam, np.float32).view(np.uint32)]
    f = subprocess.run([exe, "terms"] + words, capture_output=True, text=True, check=True).stdout.split()
    return int(f[0]), int(f[1])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_lean_entry_matches_megakernel_and_generic(renders, terms_program, k):
    (lean, lean_k), (gen, gen_k) = renders
    # the case is what it is meant to be: the entry terms of a launch with each camera, from the tree the device holds
    node0, n_nodes = lean["node0_%d" % k], int(lean["n_nodes_%d" % k][0])
    box = lean["root_box_%d" % k].view(np.uint32)
    assert box[0:3].tolist() == node0[0:3].tolist() and box[4:7].tolist() == node0[4:7].tolist(), (box, node0)
    for cam, expect in zip(lean["cams_%d" % k], CASES[k]["expect"]):
        entry, entry_primary = _terms(terms_program, node0, n_nodes, cam)
        print(CASES[k]["name"], "camera", cam.tolist(), "A0 %#x of %d nodes -> entry %d, primary entry %d; intended: %s" % (node0[3], n_nodes, entry, entry_primary, expect))
        if expect == ON:
            assert entry == node0[3] != 0 and entry_primary == entry
        elif expect == PRIMARY_OFF:
            assert entry == node0[3] != 0 and entry_primary == 0
        elif expect == OFF:
            assert entry == 0 and entry_primary == 0
        else:   # (bunny20.xml: the tree that does not fit LDS; the item is on for its bounce rays)
            assert entry == node0[3] != 0
    if "leaf" in CASES[k]["name"]:
        assert node0[3] & 0x80000000
    for how in ("sync", "sync_b"):
        assert lean_k[(k, how)] and set(lean_k[(k, how)]) == {"k_wavelocal_lean"}, lean_k[(k, how)]
        assert set(gen_k[(k, how)]) == {"k_wavelocal"}, gen_k[(k, how)]
        assert set(lean_k[(k, "mega_" + how)]) == {"k_megakernel"}
    assert len(lean_k[(k, "async")]) >= 2 and set(lean_k[(k, "async")]) == {"k_wavelocal_lean_corun"}, lean_k[(k, "async")]
    assert set(gen_k[(k, "async")]) == {"k_wavelocal_corun"}, gen_k[(k, "async")]
    for how in ("sync", "sync_b", "async"):
        a, m, g = lean["%s_%d" % (how, k)], lean["mega_%s_%d" % (how, k)], gen["%s_%d" % (how, k)]
        assert a.tobytes() == m.tobytes(), "%s: differs from the megakernel in %d pixels" % (how, int((a != m).any(-1).sum()))
        assert a.tobytes() == g.tobytes(), "%s: differs from the generic kernel in %d pixels" % (how, int((a != g).any(-1).sum()))
    assert lean["counts_%d" % k].tolist() == lean["mega_counts_%d" % k].tolist() == gen["counts_%d" % k].tolist()
    assert lean["counts_%d" % k][0] > 0
    if "far" not in CASES[k]["scene"]:
        assert lean["sync_%d" % k][..., :3].max() > 0, "nothing rendered"
    if CASES[k]["cams"][0] is not CASES[k]["cams"][1]:   # the two cameras really give two images
        assert lean["sync_%d" % k].tobytes() != lean["sync_b_%d" % k].tobytes()
