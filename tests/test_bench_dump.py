"""bench.py --dump-outputs (CPU only): float32 files within the budget, whole when they fit, a fixed seeded sample when not."""
import os

import numpy as np
import torch

import bench


def _total(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_small_output_is_written_whole(tmp_path):
    img = np.random.default_rng(1).integers(0, 256, (64, 48, 4), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"pixels": [img]})
    assert sorted(os.listdir(tmp_path)) == ["pixels.npy"]
    got = np.load(tmp_path / "pixels.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img.reshape(1, -1).astype(np.float32))


def test_dump_large_batch_is_a_seeded_sample_within_budget(tmp_path):
    rows = [torch.randint(0, 256, (3840 * 2160 * 4,), dtype=torch.uint8, generator=torch.Generator().manual_seed(k)) for k in range(40)]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), {"rgba8": rows})
    bench.dump_outputs(str(b), {"rgba8": rows})
    assert _total(a) <= bench.DUMP_BUDGET
    idx = np.load(a / "rgba8_index.npy")
    got = np.load(a / "rgba8.npy")
    assert idx.dtype == np.float64 and got.dtype == np.float32 and got.shape == (len(rows), idx.size)
    assert np.array_equal(idx, np.load(b / "rgba8_index.npy")) and np.array_equal(got, np.load(b / "rgba8.npy"))
    pos = idx.astype(np.int64)
    assert (np.diff(pos) > 0).all() and pos[-1] < rows[0].numel()
    for k in (0, 17, 39):
        assert np.array_equal(got[k], rows[k].numpy()[pos].astype(np.float32))
