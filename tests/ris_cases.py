"""The cases tests/test_ris_cpu.py and tests/test_gpu_ris.py share, with their references (tests/ris_ref.py: mpt_set_light_candidates)
computed once per process and never modified.  No new scene: scene.xml 24 x 14, cornell.xml 16 x 16 and handmade 16 x 12 of
tests/direct_cases.py, manylights 16 x 12 and (for mpt_render_nee under MPT_BSDF_SCATTER alone) specular 16 x 12 of tests/nee_cases.py.
The direct pass's references hold samples [0, 10) of every pixel — the ranges the tests use, [0, 1), [0, 3), [7, 8) and [7, 10), are
slices of them — and the render's hold samples [0, 3) per max_depth.  A path's geometry does not depend on the candidates, so the
oracle's closest hits are remembered across the references of a case.  Test code."""
import numpy as np

import anyhit_ref
import denoise_ref
import nee_cases
import ris_ref
from oracle import binding as ob

SEED = (0x0915, 21)
N_MAX = 10
SPP_MAX = 3
DEPTHS = (1, 2, 4)
GAP_CAP = 0.01
AREA, CONE = 0, 1
SAMPLINGS = (AREA, CONE)
DIRECT_CASES = ("scene.xml", "cornell.xml", "handmade", "manylights")
NEE_CASES = DIRECT_CASES + ("specular",)
DIRECT_MS = (2, 5, 32)
SMALL_SIZES = ((1, 1), (7, 3))
SMALL_M = 5

scene_of = nee_cases.scene_of
uniforms_of = nee_cases.uniforms_of
table_of = nee_cases.table_of


def nee_ms(name):
    """The candidate counts the render is checked at: 2 and 5 on every case, 32 on the case with thirteen lights."""
    return (2, 5, 32) if name == "manylights" else (2, 5)


def bsdf_mode(name):
    return nee_cases.CASES[name][4]


_guides = {}
_direct = {}
_nee = {}
_hits = {}


def first_hit(o, d, buffers):
    """oracle.binding.first_hit, remembered by the ray's bits and the scene's buffers."""
    key = (id(buffers), np.asarray(o, np.float32).tobytes(), np.asarray(d, np.float32).tobytes())
    if key not in _hits:
        _hits[key] = ob.first_hit(o, d, buffers)
    return _hits[key]


def guides(name, W=None, H=None):
    """A dict: buf, u, ad, nc (the oracle's first hits), table.  Computed once."""
    key = (name, W, H)
    if key not in _guides:
        _, buf = scene_of(name)
        u = uniforms_of(name, W, H)
        ad, nc, _ = denoise_ref.first_hit_guides(u, buf, ob.first_hit)
        for a in (ad, nc):
            a.setflags(write=False)
        _guides[key] = dict(buf=buf, u=u, ad=ad, nc=nc, table=table_of(name))
    return _guides[key]


def direct_reference(name, M, sampling, W=None, H=None):
    """guides(name, W, H) plus sampled (ris_ref.samples of samples [0, 10)), lower, upper.  Computed once."""
    key = (name, M, sampling, W, H)
    if key not in _direct:
        g = guides(name, W, H)
        sampled = ris_ref.samples(g["ad"], g["nc"], g["u"], g["table"], 0, N_MAX, M, SEED, cone=sampling == CONE)
        lower, upper = ris_ref.occlusion_bounds(sampled, g["buf"], anyhit_ref.bounds)
        for a in (lower, upper) + tuple(sampled):
            a.setflags(write=False)
        _direct[key] = dict(g, sampled=sampled, lower=lower, upper=upper)
    return _direct[key]


def direct_sliced(r, begin, N):
    """The samples [begin, begin + N) of a direct reference: (sampled, lower, upper)."""
    o, wi, tmax, contrib, skipped = r["sampled"]
    s = slice(begin, begin + N)
    return (o, wi[:, :, s], tmax[:, :, s], contrib[:, :, s], skipped[:, :, s]), r["lower"][:, :, s], r["upper"][:, :, s]


def nee_reference(name, max_depth, M, sampling, W=None, H=None):
    """ris_ref.render of a case for samples [0, 3) without a clamp, plus u and buf.  Computed once."""
    key = (name, max_depth, M, sampling, W, H)
    if key not in _nee:
        _, buf = scene_of(name)
        u = uniforms_of(name, W, H)
        out = ris_ref.render(u, buf, table_of(name), first_hit, anyhit_ref.bounds, M, cone=sampling == CONE, bsdf_mode=bsdf_mode(name),
                             max_depth=max_depth, begin=0, count=SPP_MAX, seed=SEED, clamp=np.inf)
        out.update(u=u, buf=buf)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _nee[key] = out
    return _nee[key]
