"""The cases tests/test_restir_cpu.py and tests/test_gpu_restir.py share, with their references (tests/restir_ref.py: mpt_direct_restir)
computed once per process and never modified.  No new scene: the guides, tables and sizes are tests/ris_cases.py's — scene.xml 24 x 14,
cornell.xml 16 x 16, handmade and manylights 16 x 12, sizes that put neighbours across tile and workgroup borders.  Test code."""
import numpy as np

import anyhit_ref
import restir_ref
import ris_cases as rcs

SEED = rcs.SEED
CASES = rcs.DIRECT_CASES
KS = (1, 4)
RS = (2, 8)
MS = (1, 5)
RANGES = ((0, 1), (7, 3))              # rounds [0, 1) and [7, 10) as (begin, N)
SMALL_SIZES = ((1, 1, 8), (7, 3, 64))   # (W, H, R): no neighbour can be inside; the radius exceeds the image
SMALL_K, SMALL_M = 4, 5
TAINT_CAP = 0.10

guides = rcs.guides
scene_of = rcs.scene_of
uniforms_of = rcs.uniforms_of

_refs = {}


def _freeze(x):
    for v in x.values() if isinstance(x, dict) else ():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        else:
            _freeze(v)


def reference(name, M, K, R, begin, N, W=None, H=None, seed=SEED):
    """restir_ref.restir of a case with the default thresholds (both modes), plus the guides' dict under "g".  Computed once."""
    key = (name, M, K, R, begin, N, W, H, seed)
    if key not in _refs:
        g = guides(name, W, H)
        out = restir_ref.restir(g["ad"], g["nc"], g["u"], g["table"], g["buf"], anyhit_ref.bounds, begin, N, M, K, R, seed)
        _freeze(out)
        out["g"] = g
        _refs[key] = out
    return _refs[key]


def grid():
    """Every (K, R, begin, N) of the exactness tests."""
    return [(K, R, begin, N) for K in KS for R in RS for begin, N in RANGES]
