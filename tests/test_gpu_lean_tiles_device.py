"""The class table the device builds (k_lean_tile_classes) equals the table the same header gives on the host, word for word.

lean_tile_class (metalpathtracer_amd/csrc/mpt_lean_tiles.h) is double-precision interval arithmetic: +, -, *, / and sqrt are correctly
rounded on both sides and both builds use -ffp-contract=off, so the words must be identical.  For the default view, the horizon case,
straight down and the sphere at y = 100 (tests/lean_tiles/tile_cases.py), at both sizes: the child process renders with the lean kernels,
reads the table back through mpt_read_lean_tile_classes and writes the device's node and primitive arrays and the render's camera
words to files; tests/lean_tiles/lean_tiles_check.cpp, built with the host compiler, prints the host's table from those files.

And the implication the kernels rely on, with the device's own functions: tests/lean_tiles/lean_tiles_harness.hip (built by `make`) runs
gen_primary<true>, mpt_rcp3, slab_hit and leaf_test<.., LEAN, PRIMARY> on 2^18 primary rays — 64 pixels x 4096 Philox samples — of every
`skip` tile of the default view and of the horizon case, from the arrays the device holds.  No ray may hit a chain box or a sphere
outside its tile's mask, have a NaN or a component beyond 2; some rays must hit a sphere of their mask, so the masks are not simply full.
The same for a hand-made tree whose chain has two nodes — the mesh's box and the box of a lone triangle in the sky, which the device's
builder (binary, the tail leaf a child of the root) never produces: the second node takes skip tiles away and nothing is violated."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "lean_tiles"))
from tile_cases import CASES, SIZES, class_counts  # noqa: E402

NAMES = ("default-classes", "horizon-through-a-tile-row", "straight-down", "sphere-at-100-in-view")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("lean_tiles_table") / "lean_tiles_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lean_tiles", "lean_tiles_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    names = [c["name"] for c in CASES]
    first, last = names.index(NAMES[0]), names.index(NAMES[-1]) + 1
    out = str(tmp_path_factory.mktemp("lean_tiles_device") / "dev.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lean_tiles", "render_tile_cases.py"), out, str(first), str(last)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out), out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_table_equals_host_table(program, rendered, name):
    data, out = rendered
    k = [c["name"] for c in CASES].index(name)
    for s, (W, H) in enumerate(SIZES):
        dev = data["table_%d_%d" % (k, s)]
        words = ["%08x" % w for w in data["uniforms_%d_%d" % (k, s)].view(np.uint32)]
        cmd = [program, "table", str(W), str(H), "%s.nodes_%d.bin" % (out, k), str(int(data["n_nodes_%d" % k][0])),
               "%s.prims_%d.bin" % (out, k), str(int(data["n_prims_%d" % k][0])), "-"] + words
        host = np.array([int(x, 16) for x in subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.split()], np.uint32)
        print(name, (W, H), class_counts(dev))
        assert dev.size == host.size == ((W + 7) // 8) * ((H + 7) // 8)
        assert class_counts(dev)["skip"] > 0
        assert dev.tolist() == host.tolist(), "differ in %d words" % int((dev != host).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES[:2])
def test_skip_tiles_hold_for_the_device_primary_path(rendered, name):
    data, out = rendered
    L = C.CDLL(os.path.join(ROOT, "tests", "lean_tiles", "_build", "libleantiles.so"))
    fp = C.POINTER(C.c_float)
    L.lean_tiles_violations.argtypes = [fp, C.c_uint32, fp, C.c_uint32, fp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    k = [c["name"] for c in CASES].index(name)
    nodes = np.fromfile("%s.nodes_%d.bin" % (out, k), np.float32)
    prims = np.fromfile("%s.prims_%d.bin" % (out, k), np.float32)
    for s, (W, H) in enumerate(SIZES):
        cam = np.ascontiguousarray(data["uniforms_%d_%d" % (k, s)], np.float32)
        res = (C.c_uint64 * 4)()
        rc = L.lean_tiles_violations(nodes.ctypes.data_as(fp), nodes.size // 8, prims.ctypes.data_as(fp), prims.size // 12, cam.ctypes.data_as(fp), W, H, 7, res)
        tiles, rays, bad, lit = [int(v) for v in res]
        print(name, (W, H), "skip tiles %d, rays %d, violations %d, rays that hit a sphere of their mask %d" % (tiles, rays, bad, lit))
        assert rc == 0
        assert tiles == class_counts(data["table_%d_%d" % (k, s)])["skip"] and tiles > 0 and rays == tiles << 18
        assert bad == 0 and lit > 0


def _hand_tree(chain):
    """scene.xml's three spheres as the tail leaf (node 1) behind a chain of leaf records, one triangle each (nodes 2..), in the device's layout"""
    spheres = (((0.0, -10000.0, 0.0), 10000.0), ((0.0, 100.0, 0.0), 40.0), ((0.0, 20.0, 0.0), 10.0))
    n_nodes, hold = 2 + len(chain), 0x80000000
    nodes, prims = np.zeros((n_nodes, 8), np.float32), np.zeros((len(spheres) + len(chain), 12), np.float32)
    links = nodes.view(np.uint32)
    for k, (c, r) in enumerate(spheres):
        prims[k, 0:3], prims[k, 4] = c, r
    lo = np.min([np.array(c) - r for c, r in spheres], 0)
    hi = np.max([np.array(c) + r for c, r in spheres], 0)
    nodes[1, 0:3], nodes[1, 4:7] = lo, hi
    links[1, 3], links[1, 7] = hold | (len(spheres) - 1), n_nodes
    for k, (blo, bhi) in enumerate(chain):
        n, p = 2 + k, len(spheres) + k
        nodes[n, 0:3], nodes[n, 4:7] = blo, bhi
        links[n, 3], links[n, 7] = hold | (p << 4), n + 1 if k + 1 < len(chain) else 1
        prims[p, 0:3], prims[p, 4:7], prims[p, 8:11] = blo, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
        prims.view(np.uint32)[p, 3] = 1
        lo, hi = np.minimum(lo, blo), np.maximum(hi, bhi)
    nodes[0, 0:3], nodes[0, 4:7] = lo, hi
    links[0, 3], links[0, 7] = 2 if chain else 1, n_nodes
    return nodes, prims


@pytest.mark.gpu
def test_two_node_chain_on_the_device():
    from metalpathtracer_amd import host
    L = C.CDLL(os.path.join(ROOT, "tests", "lean_tiles", "_build", "libleantiles.so"))
    fp = C.POINTER(C.c_float)
    L.lean_tiles_violations.argtypes = [fp, C.c_uint32, fp, C.c_uint32, fp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    mesh, tri = ((-31.92, -0.15, -6.99), (-16.39, 15.23, 5.06)), ((10.0, 40.0, -5.0), (14.0, 44.0, -4.0))
    W, H = 70, 45
    u = host.make_uniforms(W, H, 5, 2)
    cam = np.array(list(u.cameraPosition[:3]) + list(u.firstPixelPosition[:3]) + list(u.viewportU[:3]) + list(u.viewportV[:3]) + list(u.screenSize[:2]), np.float32)
    got = []
    for chain in ((mesh,), (mesh, tri)):
        nodes, prims = _hand_tree(chain)
        res = (C.c_uint64 * 4)()
        rc = L.lean_tiles_violations(nodes.ctypes.data_as(fp), nodes.shape[0], prims.ctypes.data_as(fp), prims.shape[0], cam.ctypes.data_as(fp), W, H, 7, res)
        tiles, rays, bad, lit = [int(v) for v in res]
        print("chain of %d: skip tiles %d, rays %d, violations %d, rays that hit a sphere of their mask %d" % (len(chain), tiles, rays, bad, lit))
        assert rc == 0 and tiles > 0 and rays == tiles << 18 and bad == 0 and lit > 0
        got.append(tiles)
    assert 5 * got[0] >= 54 and got[1] < got[0]   # (the triangle's box, in the sky right of the centre, makes tiles general)
