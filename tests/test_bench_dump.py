"""bench.py --dump-outputs without a GPU: the files dump_outputs writes for a framebuffer tensor, whole below the size limit and
a fixed, seeded pixel sample above it."""
import numpy as np
import torch

import bench


def _fb(H, W):
    return torch.arange(H * W * 4, dtype=torch.float32).reshape(H, W, 4)


def test_small_sum_is_written_whole(tmp_path):
    fb = _fb(9, 16)
    bench.dump_outputs(str(tmp_path), fb, 1234, 567)
    hdr = np.load(tmp_path / "hdr_sum.npy")
    assert hdr.dtype == np.float32 and np.array_equal(hdr, fb.numpy())
    counts = np.load(tmp_path / "counts.npy")
    assert counts.dtype == np.float64 and counts.tolist() == [1234.0, 567.0]
    assert not (tmp_path / "hdr_sum_pixels.npy").exists()


def test_large_sum_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 24 * 100)
    fb = _fb(30, 40)
    outs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), fb, 1, 1)
        hdr, pix = np.load(d / "hdr_sum.npy"), np.load(d / "hdr_sum_pixels.npy")
        assert hdr.dtype == np.float32 and pix.dtype == np.float64 and hdr.shape == (100, 4) and pix.shape == (100,)
        assert hdr.nbytes + pix.nbytes <= bench.DUMP_LIMIT_BYTES
        assert np.all(np.diff(pix) > 0) and np.array_equal(hdr, fb.numpy().reshape(-1, 4)[pix.astype(np.int64)])
        outs.append(pix)
    assert np.array_equal(outs[0], outs[1])
    # a later run small enough to be written whole removes the index file of the sample
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 48 << 20)
    bench.dump_outputs(str(tmp_path / "0"), fb, 1, 1)
    assert not (tmp_path / "0" / "hdr_sum_pixels.npy").exists()
    assert np.load(tmp_path / "0" / "hdr_sum.npy").shape == (30, 40, 4)
