"""The lean wave-local kernels test the walk's last leaf once, behind the loop (the tail leaf, metalpathtracer_amd/csrc/mpt_lean_entry.h),
against the generic kernels and the megakernel.

Every case of tests/lean_tail/tail_cases.py is rendered three ways — this build, this build with MPT_WL_LEAN=0 in a fresh child process
(the knob is read when a context is created), the megakernel — by mpt_render (k_wavelocal_lean) and by two back-to-back
mpt_render_async steps into one sum (k_wavelocal_lean_corun); HDR sum, ray count and path count must agree bit for bit.

Cases, 70 x 45, 16 spp, depth 8 (ring 1 and the drain are used): scene.xml from its own camera; from a camera above the sphere leaf's
box (tail_primary off: every primary lane makes the box test); from a camera exactly on the shrunk box's upper y plane and one ulp
above it, both taken from the node array read back; two cameras in one context, one inside and one outside — two mpt_render, then one
async step each on the two render lanes; three spheres with a triangle floating above all of them (bounce origins outside the leaf's
box: a build without the box test of the uncertain lanes renders this one and the camera above differently); seven spheres (the last
node is a chain node: off); no sphere; a two-triangle scene whose root is a leaf record; 300 triangles and three spheres at 2e7, where the
staging check fails; bunny20.xml, whose tree does not fit LDS (ALL_LDS = false: the kernels of the parent).  For every case the child writes the
device's node array to a file and the stand-alone program of test_lean_tail_cpu.py evaluates lean_tail_terms on it with each camera:
the result must be what tail_cases.find_tail — the same walk written again in Python — finds, and on or off as tail_cases.py intends,
so none passes vacuously."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "lean_tail"))
from tail_cases import CASES, HOLD, OFF, ON, PRIMARY_OFF, find_tail  # noqa: E402


def _run(tmp_path, tag, env):
    out, err = tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1", **env)
    with open(err, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lean_tail", "render_tail_cases.py"), str(out)], env=e, stderr=f, timeout=300)
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
    return np.load(out), kernels, str(out)


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean_tail")
    return _run(d, "lean", {}), _run(d, "generic", {"MPT_WL_LEAN": "0"})


@pytest.fixture(scope="module")
def terms_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lean_tail_terms") / "lean_tail_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lean_tail", "lean_tail_check.cpp"), "-o", exe], check=True)
    return exe


def _terms(exe, nodes_file, n_nodes, cam):
    words = [nodes_file, str(int(n_nodes))] + ["%08x" % w for w in np.asarray(cam, np.float32).view(np.uint32)]
    f = subprocess.run([exe, "terms"] + words, capture_output=True, text=True, check=True).stdout.split()
    return int(f[0]), int(f[1], 16), int(f[2])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_lean_tail_matches_megakernel_and_generic(renders, terms_program, k):
    (lean, lean_k, lean_out), (gen, gen_k, _) = renders
    # the case is what it is meant to be: the tail terms of a launch with each camera, from the tree the device holds
    nodes_file, n_nodes = "%s.nodes_%d.bin" % (lean_out, k), int(lean["n_nodes_%d" % k][0])
    nodes = np.fromfile(nodes_file, np.uint32)
    assert nodes.size == 8 * n_nodes and nodes[:8].tolist() == lean["node0_%d" % k].tolist()
    box, node0 = lean["root_box_%d" % k].view(np.uint32), nodes[:8]
    assert box[0:3].tolist() == node0[0:3].tolist() and box[4:7].tolist() == node0[4:7].tolist(), (box, node0)
    want_t, why = find_tail(nodes, n_nodes)
    assert CASES[k]["why"] is None or CASES[k]["why"] in why, why
    for cam, expect in zip(lean["cams_%d" % k], CASES[k]["expect"]):
        t, leaf, primary = _terms(terms_program, nodes_file, n_nodes, cam)
        print(CASES[k]["name"], "camera", cam.tolist(), "%d nodes -> T %d (%s), leaf word %#x, tail_primary %d; intended: %s" % (n_nodes, t, why, leaf, primary, expect))
        assert t == want_t
        if t:
            assert leaf & HOLD and leaf == nodes[8 * t + 3] and nodes[8 * t + 7] >= n_nodes
        else:
            assert leaf == 0 and primary == 0
        if expect == ON:
            assert t != 0 and primary == 1
        elif expect == PRIMARY_OFF:
            assert t != 0 and primary == 0
        elif expect == OFF:
            assert t == 0
    if "leaf" in CASES[k]["name"]:
        assert node0[3] & HOLD
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
