"""The tail leaf of the lean wave-local kernels (lean_tail_terms, metalpathtracer_amd/csrc/mpt_lean_entry.h), on the CPU.

tests/lean_tail/lean_tail_check.cpp is a stand-alone program that includes the header.  It checks the off-switch at each edge — the root
is a leaf record, no nodes, T an internal node, A0 = 0, a miss link to node 0, miss links that never end, A0 = n_nodes, n_nodes at the
marker, a box thinner than 4m (and one exactly 4m thick, accepted), planes at 1.6e7 where an ulp exceeds 2m, a NaN or infinite plane,
the camera exactly on tlo / thi (inside) and one ulp outside each — and then the implication the kernels rely on, in float32 with the
IEEE 1 / d: for 2^21 origins per box (in the shrunk box, on its faces, between the two boxes, on T's faces, around it) and directions
with exact zeros, -0, denormals, tiny components, |d| = 2 and components past 2, whenever the guard says certain T's slab test says hit
and the minimum of its far terms exceeds 0.0001f.  Four boxes the function accepts, among them scene.xml's sphere leaf, [-1e4, 1e4] x
[-2e4, 140] x [-1e4, 1e4].  The program asserts that at least half of the origins are inside the shrunk box and that the guard says
certain for at least a fifth, so it cannot pass by declining.

Built twice with the host compiler, plain and with AddressSanitizer + UndefinedBehaviorSanitizer, and run directly; nothing is loaded
into Python."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lean_tail", "lean_tail_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc")]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_tail_terms_edges_and_implication(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lean_tail_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([cxx] + FLAGS + extra + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all passed" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert "edges: 0 failures" in r.stdout
    boxes = re.findall(r"box \d: (\d+) origins, (\d+) inside the shrunk box, (\d+) certain, (\d+) failures, least far term (\S+)", r.stdout)
    assert len(boxes) == 4
    for n, inside, certain, bad, least in boxes:
        assert int(n) >= 2 ** 21 and 2 * int(inside) >= int(n) and 5 * int(certain) >= int(n) and int(bad) == 0 and float(least) > 1e-4
