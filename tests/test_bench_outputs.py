"""bench.py --dump-outputs on the host: what dump_outputs() writes for a batch, within its byte budget, on
tensors that stand in for the last timed step's (the GPU run of the same option is in test_gpu_boundary.py)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _batch(samples, ncode, side, seed=1):
    g = torch.Generator().manual_seed(seed)
    hist = torch.randint(-2 ** 31, 2 ** 31 - 1, (samples, ncode), dtype=torch.int32, generator=g)   # u32 counts, as the engine's int32 tensor holds them
    img = torch.randint(0, 256, (samples, side, side), dtype=torch.uint8, generator=g)
    status = torch.zeros(samples, dtype=torch.int32)
    status[3] = 0x40000001
    return hist, img, status


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_entry_exactly_when_it_fits(tmp_path):
    bench = _bench()
    hist, img, status = _batch(10, 64, 8)
    bench.dump_outputs(str(tmp_path / "d"), hist, img, status)
    got = _load(tmp_path / "d")
    assert sorted(got) == ["histograms", "images", "rows", "status"]
    assert got["images"].dtype == np.float32 and got["histograms"].dtype == np.float64
    assert got["status"].dtype == np.float64 and got["rows"].dtype == np.float64
    assert np.array_equal(got["rows"], np.arange(10))
    assert np.array_equal(got["images"], img.numpy())
    assert np.array_equal(got["histograms"], hist.numpy().view(np.uint32))         # counts above 2^31 stay exact
    assert np.array_equal(got["status"], status.numpy()) and got["status"][3] == 0x40000001


def test_dump_samples_rows_within_the_budget_and_repeats_them(tmp_path):
    bench = _bench()
    bench.DUMP_BYTES = 40_000
    hist, img, status = _batch(50, 256, 16)           # 50 x (256 x 8 + 256 x 4) bytes: more than the budget
    bench.dump_outputs(str(tmp_path / "a"), hist, img, status)
    bench.dump_outputs(str(tmp_path / "b"), hist, img, status)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    rows = a["rows"].astype(np.int64)
    assert 1 <= len(rows) < 50 and np.all(np.diff(rows) > 0) and rows[-1] < 50
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(a["images"], img.numpy()[rows])
    assert np.array_equal(a["histograms"], hist.numpy().view(np.uint32)[rows])
    assert a["status"].shape == (50,)
