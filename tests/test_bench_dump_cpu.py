"""CPU: `bench.py --dump-outputs` writes the step's arrays as float32 / float64 .npy files under its byte budget, samples the
arrays that do not fit at fixed seeded rows, and writes the same files for the same arrays."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _outputs(n=8, L=300, C=64, m=900):
    g = torch.Generator().manual_seed(3)
    tokens = torch.randn(n, 1 + L, C, generator=g)
    b_ids = torch.randint(0, n, (m,), generator=g)
    return {"conf_matrix": None, "b_ids": b_ids, "i_ids": torch.randint(0, L, (m,), generator=g), "gt_mask": torch.zeros(m, dtype=torch.bool),
            "mkpts0_c": torch.rand(m, 2, generator=g), "mconf": torch.rand(m, generator=g),
            "counts": torch.randint(0, 100, (n,), dtype=torch.int32, generator=g),
            "feat0": tokens[:, 1:], "feat1": 2 * tokens[:, 1:], "cls0": tokens[:, 0]}


def test_dump_outputs_budget_dtypes_and_sampling(tmp_path):
    bench = _bench()
    out = _outputs()
    budget = 400_000   # feat0 / feat1 (8 x 300 x 64 fp32 = 614 KB each) exceed their share, the rest is written whole
    shapes = [bench.dump_outputs(out, str(tmp_path / d), budget=budget) for d in ("a", "b")]
    assert shapes[0] == shapes[1]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "conf_matrix.npy" not in names and "feat0_rows.npy" in names and "cls0_rows.npy" not in names
    total = 0
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
        total += x.nbytes
    assert total <= budget
    assert np.array_equal(np.load(tmp_path / "a" / "i_ids.npy"), out["i_ids"].numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "gt_mask.npy"), np.zeros(900, np.float32))
    rows0, rows1 = (np.load(tmp_path / "a" / f"{k}_rows.npy").astype(np.int64) for k in ("feat0", "feat1"))
    assert np.array_equal(rows0, rows1) and np.all(np.diff(rows0) > 0)   # same rows of same-shaped arrays, ascending
    assert np.array_equal(np.load(tmp_path / "a" / "feat0.npy"), out["feat0"].reshape(-1, 64)[rows0].numpy())
