"""Primary steps of the lean wave-local kernels skip the walk a tile's rays cannot need (metalpathtracer_amd/csrc/mpt_lean_tiles.h),
against the generic kernels and the megakernel.

Every case of tests/lean_tiles/tile_cases.py — the eleven of tests/lean_tail/tail_cases.py with their first camera and the second camera of the
one that has two, the horizon through a tile row, the light's silhouette, straight up and straight down, the sphere at y = 100 in view, a
lone triangle in the sky, a scene without spheres (one of the eleven), and one render in two shards: twenty in all — is rendered at 70 x 45 and 64 x 64 (the centre column of the second has d.x = 0), 16 spp,
depth 8, three ways: this build, this build with MPT_WL_LEAN=0 in a fresh child process, the megakernel; by mpt_render (k_wavelocal_lean)
and by two back-to-back mpt_render_async steps into one sum (k_wavelocal_lean_corun, both render lanes, each with a table of its own).
HDR sum, ray count and path count must agree bit for bit.  The class table is read back after every wave-local render and must hold the
classes the case is meant to exercise (tile_cases.py), so none passes vacuously; with MPT_LEAN_TILES=0 there is no table and the sums
are the same again."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "lean_tiles"))
from tile_cases import CASES, NONE, OFF, SIZES, chain_length, class_counts, tile_of  # noqa: E402


def _run(tmp_path, tag, env, cases=None):
    out, err = tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1", **env)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "lean_tiles", "render_tile_cases.py"), str(out)] + ([str(c) for c in cases] if cases else [])
    with open(err, "w") as f:
        r = subprocess.run(cmd, env=e, stderr=f, timeout=600)
    text = err.read_text()
    assert r.returncode == 0, text[-2000:]
    kernels, cur = {}, None   # (case, size, "wl" / "mega" / ..) -> kernel names of the launches behind that marker
    for line in text.splitlines():
        m = re.match(r"CASE (\d+) (\d+) (\w+)$", line)
        if m:
            cur = (int(m.group(1)), int(m.group(2)), m.group(3))
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
    d = tmp_path_factory.mktemp("lean_tiles")
    return _run(d, "lean", {}), _run(d, "generic", {"MPT_WL_LEAN": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_lean_tiles_match_megakernel_and_generic(renders, k):
    (lean, lean_k, lean_out), (gen, gen_k, _) = renders
    c = CASES[k]
    for s, (W, H) in enumerate(SIZES):
        tag = "%d_%d" % (k, s)
        table = lean["table_" + tag]
        n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
        if c["expect"] == NONE:
            assert table.size == 0
        else:
            assert table.size == n_tiles, (table.size, n_tiles)
            got = class_counts(table)
            print(c["name"], (W, H), got, "intended:", c["expect"])
            if c["expect"] == OFF:
                assert got["skip"] == 0, got
            else:
                for key, least in c["expect"].items():
                    if key == "no_sky":
                        assert got["sky"] == 0, got
                    elif key == "chain":
                        n_nodes = int(lean["n_nodes_%d" % k][0])
                        length = chain_length(np.fromfile("%s.nodes_%d.bin" % (lean_out, k), np.uint32), n_nodes)
                        print(c["name"], "chain of", length)
                        assert length is not None and length >= least
                    elif key == "general_at":
                        tx, ty = tile_of(least, c["cam"], W, H)
                        assert table[ty * ((W + 7) // 8) + tx] == 0, (tx, ty, hex(int(table[ty * ((W + 7) // 8) + tx])))
                    else:
                        assert got[key] >= least, (key, got)
            assert set(lean_k[(k, s, "wl")]) == {"k_wavelocal_lean"}, lean_k[(k, s, "wl")]
            assert set(lean_k[(k, s, "async")]) == {"k_wavelocal_lean_corun"}, lean_k[(k, s, "async")]
        assert gen["table_" + tag].size == 0
        assert set(gen_k[(k, s, "wl")]) == {"k_wavelocal"} and set(gen_k[(k, s, "async")]) == {"k_wavelocal_corun"}
        assert set(lean_k[(k, s, "mega")]) == {"k_megakernel"}
        for a, m in (("wl", "mega"), ("async", "mega2")):
            x, y, z = lean["%s_%s" % (a, tag)], lean["%s_%s" % (m, tag)], gen["%s_%s" % (a, tag)]
            assert x.tobytes() == y.tobytes(), "%s %s: differs from the megakernel in %d pixels" % (a, (W, H), int((x != y).any(-1).sum()))
            assert x.tobytes() == z.tobytes(), "%s %s: differs from the generic kernel in %d pixels" % (a, (W, H), int((x != z).any(-1).sum()))
        assert lean["counts_wl_" + tag].tolist() == lean["counts_mega_" + tag].tolist() == gen["counts_wl_" + tag].tolist()
        assert lean["counts_async_" + tag].tolist() == gen["counts_async_" + tag].tolist()
        assert lean["counts_wl_" + tag][0] > 0
        if "far" not in c["scene"]:
            assert lean["wl_" + tag][..., :3].max() > 0, "nothing rendered"


@pytest.mark.gpu
def test_lean_tiles_environment_switch(tmp_path, renders):
    """MPT_LEAN_TILES=0: the lean kernels run without a table and render the same sums (the default view and the horizon case)."""
    first = [c["name"] for c in CASES].index("default-classes")
    off, off_k, _ = _run(tmp_path, "tiles_off", {"MPT_LEAN_TILES": "0"}, cases=(first, first + 2))
    lean = renders[0][0]
    for k in (first, first + 1):
        for s in range(len(SIZES)):
            tag = "%d_%d" % (k, s)
            assert off["table_" + tag].size == 0 and lean["table_" + tag].size != 0
            assert set(off_k[(k, s, "wl")]) == {"k_wavelocal_lean"}
            assert off["wl_" + tag].tobytes() == lean["wl_" + tag].tobytes() and off["async_" + tag].tobytes() == lean["async_" + tag].tobytes()
            assert off["counts_wl_" + tag].tolist() == lean["counts_wl_" + tag].tolist()
