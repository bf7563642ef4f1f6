"""CPU checks of the ambient-occlusion restatement (tests/ao_ref.py) and of the bindings of the shadow-ray entry points; no GPU."""
import ctypes as C

import numpy as np

import ao_ref
from metalpathtracer_amd import capi
from oracle import binding as ob

F = np.float32


def test_philox_restatement_matches_the_known_answers_and_the_oracle():
    # Random123 kat_vectors for philox4x32_10 (the pins of tests/test_oracle_pins.py)
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = ao_ref.philox4x32_10(*[np.uint32(x) for x in ctr], key[0], key[1])
        assert tuple(int(x) for x in got) == want
    # the counter layout of an AO sample, vectorised, against the oracle's own Philox
    rng = np.random.default_rng(7)
    pixel = rng.integers(0, 1 << 21, 64, dtype=np.uint32)
    sample = rng.integers(0, 1 << 32, 64, dtype=np.uint32)
    got = np.stack(ao_ref.philox4x32_10(pixel, sample, np.uint32(ao_ref.WORD2), np.uint32(0), 0x1234567, 0x89ABCDEF), -1)
    for i in range(64):
        c = (C.c_uint32 * 4)(int(pixel[i]), int(sample[i]), ao_ref.WORD2, 0)
        k = (C.c_uint32 * 2)(0x1234567, 0x89ABCDEF)
        o = (C.c_uint32 * 4)()
        ob.lib().orc_philox(c, k, o)
        assert tuple(o) == tuple(int(x) for x in got[i])


def test_sincos_restatement_matches_the_oracle_bit_for_bit():
    u = np.concatenate([np.linspace(0.0, 1.0, 4097, dtype=np.float32)[:-1], ao_ref.u01(np.arange(0, 1 << 32, 16777213, dtype=np.uint64).astype(np.uint32))])
    s, c = ao_ref.sincos_2pi(u)
    so, co = C.c_float(), C.c_float()
    for i in range(u.shape[0]):
        ob.lib().orc_sincos_2pi(float(u[i]), C.byref(so), C.byref(co))
        assert F(so.value).view(np.uint32) == s[i].view(np.uint32) and F(co.value).view(np.uint32) == c[i].view(np.uint32), u[i]
    assert ao_ref.u01(np.uint32(0xFFFFFFFF)) < 1 and ao_ref.u01(np.uint32(0xFF)) == 0


def test_directions_are_unit_length_and_leave_the_surface():
    rng = np.random.default_rng(11)
    H, W, N = 6, 5, 64
    n = rng.normal(size=(H, W, 3)).astype(np.float32)
    n = ao_ref.normalize(n).astype(np.float32)
    nc = np.concatenate([n, np.zeros((H, W, 1), np.float32)], -1)
    ad = np.concatenate([np.full((H, W, 3), 0.5, np.float32), rng.uniform(1, 50, (H, W, 1)).astype(np.float32)], -1)
    u = ob.make_uniforms(W, H, 1)
    surface, o, d = ao_ref.sample_rays(ad, nc, u, 3, N, seed=(5, 9))
    assert surface.all() and d.shape == (H, W, N, 3) and o.shape == (H, W, 3)
    ok = ~np.isnan(d).any(-1)                                   # (n + r = 0 exactly gives a NaN direction: "not occluded")
    assert ok.mean() > 0.999
    length = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
    assert np.abs(length[ok] - 1).max() <= 2 * np.finfo(np.float32).eps           # 2 ulp of 1
    cosine = (d.astype(np.float64) * n[:, :, None, :].astype(np.float64)).sum(-1)   # n and the drawn vector are unit vectors: 1 + cos >= 0
    assert cosine[ok].min() >= 0.0
    # samples are numbered: [3, 3 + N) is [3, 10) followed by [10, 3 + N)
    _, _, d0 = ao_ref.sample_rays(ad, nc, u, 3, 7, seed=(5, 9))
    _, _, d1 = ao_ref.sample_rays(ad, nc, u, 10, N - 7, seed=(5, 9))
    assert np.array_equal(np.concatenate([d0, d1], 2).view(np.uint32), d.view(np.uint32))


def test_occlusion_rule_of_the_restatement():
    d = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], np.float32)
    tstar = np.array([1, 1, 1, np.inf, 1e-3, 1], np.float32)
    tmax = np.array([2, 1, 2, np.inf, 1e-4, np.nan], np.float32)
    assert ao_ref.occluded(tstar, d, tmax).tolist() == [True, False, False, False, False, False]


def test_bindings_list_the_shadow_ray_entry_points():
    for name in ("mpt_trace_occluded", "mpt_ambient_occlusion", "mpt_read_ao", "mpt_ao_buffer", "mpt_ao_image"):
        assert name in capi.SYMBOLS, name
    L = capi.load()
    assert L.mpt_trace_occluded(None, None, None, None, 0, 0, None, None) == 1          # MPT_ERR_INVALID_ARG, no crash
    assert L.mpt_ambient_occlusion(None, None, None) == 1
    assert L.mpt_read_ao(None, None, None) == 1
    assert L.mpt_ao_buffer(None, None, None) == 1
    assert L.mpt_ao_image(None, 1, 1, None, None, None, None, None, None) == 1
    assert C.sizeof(capi.AoParams) == 24 and C.sizeof(capi.AoInfo) == 32
    assert (capi.WALK_REFERENCE, capi.WALK_OWN, capi.WALK_AUTO) == (0, 1, 2) and capi.AO_MAX_SAMPLES == 1024
