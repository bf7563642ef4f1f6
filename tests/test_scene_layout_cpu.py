"""mpt_upload_scene's host side (layout_scene, metalpathtracer_amd/csrc/mpt_scene_layout.h) and the comma-list knobs (mpt_env.h), on the CPU.

tests/scene_layout/scene_layout_check.cpp is a stand-alone program that includes only those pure host headers.  Without arguments it lays
out hand-made trees that reach every branch, feeds the parser of the caller's indices every malformed tree it must refuse (status, exact
message) and checks the fill rules of the three list knobs.  In golden mode it lays out the arrays of one asset scene and prints
mpt_scene_digest's words for the six host-made arrays and the seven counts, which must be the ones tests/golden/upload_digests.json
records — from the device, by tools/gpu_scene_digest.py --upload at commit be3643d, the last one whose mpt_upload_scene made the layout
inside mpt_hip.hip.  Built with the host compiler, AddressSanitizer and UndefinedBehaviorSanitizer; nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_scene

NAMES = "nodes prims mats own refleaf refbox always ref_bvh ref_idx n_nodes n_prims n_mats n_own n_leaves n_always depth".split()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("scene_layout") / "scene_layout_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "scene_layout", "scene_layout_check.cpp"), "-o", exe], check=True)
    return exe


def test_hand_made_trees_rejections_and_list_knobs(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all passed" in r.stdout and not r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["scene.xml", "cornell.xml", "glass.xml", "bunny20.xml"])
def test_layout_has_the_recorded_digests(checker, tmp_path, name):
    want = json.load(open(os.path.join(GOLDEN, "upload_digests.json")))[name]
    bvh, prims, mats, idx = host_scene(name)[1]
    files = []
    for tag, arr, dtype in (("bvh", bvh, np.float32), ("prims", prims, np.float32), ("mats", mats, np.float32), ("idx", idx, np.int32)):
        files.append(str(tmp_path / tag))
        np.ascontiguousarray(np.asarray(arr), dtype=dtype).tofile(files[-1])
    r = subprocess.run([checker, "golden"] + files, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines())
    assert got.pop("acc_ok") == "1"
    assert sorted(got) == sorted(n for n in NAMES if n not in ("refbox", "ref_bvh", "ref_idx"))   # (refbox is made on the device)
    assert {n: want[NAMES.index(n)] for n in got} == got
