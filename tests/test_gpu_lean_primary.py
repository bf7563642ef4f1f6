"""The camera-relative sphere terms of the lean wave-local kernels (sphere_cam_terms, mpt_device.h / mpt_kernels.h) and the carried
ballot of their box loop (closest_hit_resume<.., LEAN>), against the generic kernels and the megakernel.

A lean kernel stages, once per workgroup, oc = camera - centre and cc = dot3(oc, oc) - r * r into the unused words of every LDS-resident
sphere record; the walk of a primary step reads them instead of computing them per ray.  Every case of tests/lean_primary/cases.py is
rendered three ways — this build, this build with MPT_WL_LEAN=0 in a fresh child process (the knob is read when a context is created),
the megakernel — by mpt_render (k_wavelocal_lean) and by two back-to-back mpt_render_async steps into one sum (k_wavelocal_lean_corun);
HDR sum, ray count and path count must agree bit for bit.  The MPT_DEBUG_LAUNCH line names the kernel that ran.

Cases, 70 x 45 (off the tile grid in both axes), 3 spp, depth 1 (primary rays alone) and 8: scene.xml from its own camera; from the
exact centre of its r = 10 sphere (oc = 0, b = 0: the `!(b >= 0)` rule decides); from inside its r = 40 sphere, off the centre; from
10^6 away; at 1023 x 9 (lanes outside the image in primary steps); with two different cameras in one context — two mpt_render, then the
two mpt_render_async steps with one camera each, running side by side on the context's two lanes: the staged terms belong to a launch;
a soup of 20000 triangles with 20 spheres in it, where primary rays test a sphere whose record is NOT in LDS (asserted below from the
device's own primitive array and the launch's LDS size); bunny20.xml at 1 spp, whose tree does not fit LDS (ALL_LDS = false), so all
four lean kernels run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "lean_primary"))
from cases import CASES, SOUP_SPHERES  # noqa: E402


def _run(tmp_path, tag, env):
    out, err = tmp_path / (tag + ".npz"), tmp_path / (tag + ".err")
    e = dict(os.environ, MPT_DEBUG_LAUNCH="1", **env)
    with open(err, "w") as f:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lean_primary", "render_cases.py"), str(out)], env=e, stderr=f, timeout=300)
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
    d = tmp_path_factory.mktemp("lean_primary")
    return _run(d, "lean", {}), _run(d, "generic", {"MPT_WL_LEAN": "0"})


def _first(name):
    return [k for k, c in enumerate(CASES) if c["name"].startswith(name)][0]


@pytest.mark.gpu
def test_primary_rays_of_the_soup_test_a_sphere_that_is_not_in_lds(renders):
    """A record at index i can be in the LDS image only if 48 (i + 1) bytes fit into the workgroup's LDS allocation, whatever the host's
    rule for the prefix is.  Where the ray from the camera to a sphere's centre lies inside the view (checked below against the
    60-degree vertical field) and mpt_trace_rays answers it with that sphere, the primary rays of the pixels around it test the
    sphere's record."""
    (lean, _, lds), _ = renders
    k = _first("soup")
    rec = lean["soup_prims"].reshape(-1, 12)
    sphere_at = {int(r[11]): i for i, r in enumerate(rec) if (int(r[3]) & 1) == 0}      # caller's id -> index of the record in the device's order
    assert len(sphere_at) == SOUP_SPHERES
    limit = lds[(k, "sync")] // 48
    assert 0 < limit < rec.shape[0]
    assert int(lean["nodes_soup"][0]) * 32 > lds[(k, "sync")]                            # and the tree is not resident either: ALL_LDS = false
    d, prim = lean["soup_ray_dirs"], lean["soup_ray_prim"]
    W, H = CASES[k]["size"]
    half_h = np.tan(np.radians(30.0))
    in_view = (np.abs(d[:, 1] / -d[:, 2]) < half_h) & (np.abs(d[:, 0] / -d[:, 2]) < half_h * W / H) & (d[:, 2] < 0)
    seen_outside = [s for s in range(SOUP_SPHERES) if in_view[s] and prim[s] == s and sphere_at[s] >= limit]
    print("sphere records at", sorted(sphere_at.values()), "LDS can hold at most", limit, "records; seen by the camera and outside:", seen_outside)
    assert seen_outside


@pytest.mark.gpu
def test_bunny20_spills_out_of_lds_and_scene_xml_does_not(renders):
    (lean, _, lds), _ = renders
    assert int(lean["nodes_bunny20.xml"][0]) * 32 > lds[(_first("bunny20"), "sync")] > 0
    assert int(lean["nodes_scene.xml"][0]) * 32 <= lds[(_first("own"), "sync")]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_lean_primary_matches_megakernel_and_generic(renders, k):
    (lean, lean_k, _), (gen, gen_k, _) = renders
    for how in ("sync", "sync_b"):
        assert lean_k[(k, how)] and set(lean_k[(k, how)]) == {"k_wavelocal_lean"}, lean_k[(k, how)]
        assert set(gen_k[(k, how)]) == {"k_wavelocal"}, gen_k[(k, how)]
        assert set(lean_k[(k, "mega_" + how)]) == {"k_megakernel"}
    assert len(lean_k[(k, "async")]) >= 2 and set(lean_k[(k, "async")]) == {"k_wavelocal_lean_corun"}, lean_k[(k, "async")]
    assert set(gen_k[(k, "async")]) == {"k_wavelocal_corun"}, gen_k[(k, "async")]
    for how in ("sync", "sync_b", "async"):
        a, m, g = lean["%s_%d" % (how, k)], lean["mega_%s_%d" % (how, k)], gen["%s_%d" % (how, k)]
        assert a[..., 3].max() > 0, "nothing rendered"
        assert a.tobytes() == m.tobytes(), "%s: differs from the megakernel in %d pixels" % (how, int((a != m).any(-1).sum()))
        assert a.tobytes() == g.tobytes(), "%s: differs from the generic kernel in %d pixels" % (how, int((a != g).any(-1).sum()))
    assert lean["counts_%d" % k].tolist() == lean["mega_counts_%d" % k].tolist() == gen["counts_%d" % k].tolist()
    assert lean["counts_%d" % k][0] > 0
    if CASES[k]["cams"][0] is not CASES[k]["cams"][1]:   # the two cameras really give two images
        assert lean["sync_%d" % k].tobytes() != lean["sync_b_%d" % k].tobytes()
