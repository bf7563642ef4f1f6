"""Sky tiles are summed by the resolve, not through result slots (k_resolve_sum, k_resolve_sum_moments and the elision in the primary steps
of the lean wave-local kernels: metalpathtracer_amd/csrc/mpt_kernels.h).

Six views of tests/sky_resolve/sky_cases.py — the default view, straight up, straight down, the horizon through a tile row, the light's
silhouette, a lone triangle in the sky — at 70 x 45 and 64 x 64, each with twelve items: 1, 3, 5 and 17 spp at depth 1 and 8, a
non-zero sample_begin, three mpt_render_async renders into one sum, rank 1 of 2 shards, and MPT_FLAG_MOMENTS.  Every item is rendered by
this build, by this build with MPT_LEAN_SKY_RESOLVE=0 in a fresh child process, and by the megakernel: the HDR sum, the moments buffer and
the ray and path counts must agree byte for byte.  The class table is read back and must hold the sky tiles (and the tiles of another
class) the view is meant to have, and the library must say that it left the sky tiles to the resolve in one arm and not in the other, so
that nothing passes vacuously.  The frame protocol and the generic kernels never elide: same bytes, no such line.

Control, run once by hand (profiles/r25_sky_resolve.txt): a library built with -DMPT_SKY_RESOLVE_CONTROL -DMPT_SKY_RESOLVE_TESTING, whose
resolve computes sample s + 1 in the place of s, fails every view that has a sky tile."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "sky_resolve"))
from sky_cases import ITEMS, VIEWS  # noqa: E402
from tile_cases import SIZES, class_counts  # noqa: E402

SKY_LINE = "[mpt] sky tiles: summed by the resolve"


def _run(tmp_path, tag, env):
    out, err = tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1", **env)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "sky_resolve", "render_sky_cases.py"), str(out)]
    with open(err, "w") as f:
        r = subprocess.run(cmd, env=e, stderr=f, timeout=600)
    text = err.read_text()
    assert r.returncode == 0, text[-2000:]
    launches, cur = {}, None   # "k_s_item wl" -> (kernel names, launches left to the resolve) behind that marker
    for line in text.splitlines():
        m = re.match(r"ITEM (.+)$", line)
        if m:
            cur = m.group(1)
            launches[cur] = ([], [])
        elif cur is not None:
            m = re.search(r"\[mpt\] pipeline \d+:.* kernel (\w+)$", line)
            if m:
                launches[cur][0].append(m.group(1))
            elif line.strip() == SKY_LINE:
                launches[cur][1].append(line)
    return np.load(out), launches


@pytest.fixture(scope="module")
def renders(tmp_path_factory):
    d = tmp_path_factory.mktemp("sky_resolve")
    return _run(d, "on", {}), _run(d, "off", {"MPT_LEAN_SKY_RESOLVE": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(VIEWS)), ids=[v["name"] for v in VIEWS])
def test_sky_tiles_summed_by_the_resolve(renders, k):
    (on, on_l), (off, off_l) = renders
    v = VIEWS[k]
    for s, (W, H) in enumerate(SIZES):
        table = on["table_%d_%d" % (k, s)]
        assert table.size == ((W + 7) // 8) * ((H + 7) // 8) and table.tobytes() == off["table_%d_%d" % (k, s)].tobytes()
        got = class_counts(table)
        print(v["name"], (W, H), got)
        assert (got["sky"] > 0) == v["sky"], got
        if v["other"]:
            assert got["tiles"] - got["sky"] > 0, got
        for item in ITEMS:
            tag = "%d_%d_%s" % (k, s, item["name"])
            kernel = "k_wavelocal_lean_corun" if item["async"] else "k_wavelocal_lean"
            n = len(item["renders"])
            assert on_l[tag + " wl"][0] == [kernel] * n and off_l[tag + " wl"][0] == [kernel] * n, (tag, on_l[tag + " wl"])
            assert len(on_l[tag + " wl"][1]) == n and not off_l[tag + " wl"][1], tag   # elision on in every pass of one arm, in none of the other
            assert on_l[tag + " mega"][0] == ["k_megakernel"] * n and not on_l[tag + " mega"][1], tag
            x, y, z = on["wl_" + tag], off["wl_" + tag], on["mega_" + tag]
            assert x.tobytes() == y.tobytes(), "%s: differs from MPT_LEAN_SKY_RESOLVE=0 in %d pixels" % (tag, int((x != y).any(-1).sum()))
            assert x.tobytes() == z.tobytes(), "%s: differs from the megakernel in %d pixels" % (tag, int((x != z).any(-1).sum()))
            assert on["counts_wl_" + tag].tolist() == off["counts_wl_" + tag].tolist() == on["counts_mega_" + tag].tolist(), tag
            spp = sum(c for _, c in item["renders"])
            if item["shards"] == 1:
                assert on["counts_wl_" + tag][1] == W * H * spp, tag
            if v["sky"]:   # (a sky path adds 1 to alpha: the sky tiles' pixels got all their samples)
                assert x[..., 3].max() == spp, tag
            if item["moments"]:
                a, b, c = on["m2wl_" + tag], off["m2wl_" + tag], on["m2mega_" + tag]
                assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes(), tag + ": moments differ"
                assert a.max() > 0, tag


@pytest.mark.gpu
def test_frame_protocol_and_generic_kernels_do_not_elide(tmp_path, renders):
    """mpt_draw ends in k_resolve_frame, which reads every slot, and the generic kernels read no class table: neither leaves a tile to the resolve."""
    (on, on_l), (off, _) = renders
    assert on_l["draw wl"][0] == ["k_wavelocal_lean"] and not on_l["draw wl"][1]
    assert on["draw_wl"].tobytes() == off["draw_wl"].tobytes() == on["draw_mega"].tobytes()
    assert np.isfinite(on["draw_wl"]).all() and on["draw_wl"][..., :3].max() > 0
    gen, gen_l = _run(tmp_path, "generic", {"MPT_WL_LEAN": "0"})
    for tag in ("0_0_spp5_d8", "0_0_async3", "0_1_spp17_d8", "1_0_spp3_d8"):
        names, left = gen_l[tag + " wl"]
        assert names and set(names) <= {"k_wavelocal", "k_wavelocal_corun"} and not left, (tag, names, left)
        assert gen["wl_" + tag].tobytes() == on["wl_" + tag].tobytes() and gen["counts_wl_" + tag].tolist() == on["counts_wl_" + tag].tolist(), tag
    assert gen["draw_wl"].tobytes() == on["draw_wl"].tobytes()
