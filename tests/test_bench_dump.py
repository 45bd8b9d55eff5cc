"""CPU: bench.py --dump-outputs writes a fixed, seeded sample of the last step's outputs as float64 .npy files, within
its byte budget (dump_outputs is device-agnostic, so CPU tensors stand in for the device buffers)."""
import os

import numpy as np
import torch

import bench


def _dump(path, out, status):
    bench.dump_outputs(str(path), out, status)
    return {f: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_is_a_fixed_sample_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 40 * 16 * 64 * 8)             # 40 of the 1000 surfaces fit
    out = torch.arange(1000 * 16 * 64, dtype=torch.float64).reshape(1000, 16, 64)
    status = torch.zeros(1000, dtype=torch.int32)
    status[::7] = 4
    a = _dump(tmp_path / "a", out, status)
    assert sorted(a) == ["status.npy", "surfaces.npy", "surfaces_index.npy"]
    assert all(v.dtype == np.float64 for v in a.values())
    idx = a["surfaces_index.npy"].astype(np.int64)
    assert len(idx) == 40 and len(np.unique(idx)) == 40 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["surfaces.npy"], out.numpy()[idx])
    assert np.array_equal(a["status.npy"], status.numpy()[idx].astype(np.float64))
    b = _dump(tmp_path / "b", out.clone(), status.clone())                   # same arguments -> same files
    assert all(np.array_equal(a[f], b[f]) for f in a)


def test_dump_outputs_small_batch_is_whole(tmp_path):
    a = _dump(tmp_path, torch.ones(3, 16, 64, dtype=torch.float64), torch.zeros(3, dtype=torch.int32))
    assert a["surfaces.npy"].shape == (3, 16, 64) and list(a["surfaces_index.npy"]) == [0.0, 1.0, 2.0]
    assert sum(v.nbytes for v in a.values()) < 64 << 20
