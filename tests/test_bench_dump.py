"""CPU: `bench.py --dump-outputs` - the row sample is fixed (seeded, in row order) and the files are float32 `.npy`
within the size limit."""
import os

import numpy as np
import pytest
import torch

import bench


def test_row_sample_is_fixed_and_ordered():
    t = torch.arange(40000 * 8, dtype=torch.float32).view(40000, 8)
    small = t[:100]
    assert bench._row_sample(small) is small                      # fits: the whole array
    a, b = bench._row_sample(t, max_bytes=4096), bench._row_sample(t.clone(), max_bytes=4096)
    assert a.shape == (128, 8) and torch.equal(a, b)
    rows = a[:, 0] / 8
    assert torch.equal(rows, rows.round()) and bool((rows[1:] > rows[:-1]).all())
    assert torch.equal(a, t[rows.long()])


def test_dump_outputs_writes_float32_within_the_limit(tmp_path):
    arrays = {"out": torch.randn(3, 4, dtype=torch.float64), "param.w": torch.ones(5)}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["out.npy", "param.w.npy"]
    out = np.load(tmp_path / "d" / "out.npy")
    assert out.dtype == np.float32 and np.array_equal(out, arrays["out"].float().numpy())
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path / "e"), arrays, limit_bytes=16)
    assert not os.path.exists(tmp_path / "e")
