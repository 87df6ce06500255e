"""bench.py --dump-outputs, the writer alone (host tensors, no GPU): short
arrays whole, long ones as the fixed seeded sample with its positions beside."""
import numpy as np
import pytest


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets OMP_PROC_BIND for its own process when imported: monkeypatch
    # puts this process's environment back afterwards
    monkeypatch.setenv("OMP_PROC_BIND", "close")
    import bench as B
    return B


def _csr(torch, m, nnz):
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.integers(0, nnz + 1, m - 1))
    rp = np.concatenate([[0], cuts, [nnz]]).astype(np.int32)
    return (torch.from_numpy(rp), torch.from_numpy(rng.integers(0, 77, nnz).astype(np.int32)),
            torch.from_numpy(rng.standard_normal(nnz)))


def test_short_arrays_whole(bench, tmp_path):
    import torch
    rp, ci, vv = _csr(torch, 9, 40)
    bench.dump_outputs(str(tmp_path), 9, 77, rp, ci, vv)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["col.npy", "rowptr.npy", "shape.npy", "val.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "shape.npy"), [9, 77, 40])
    for name, t in (("rowptr", rp), ("col", ci), ("val", vv)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, t.numpy())


def test_long_arrays_sampled_the_same_way_every_time(bench, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_CAP", 64)
    rp, ci, vv = _csr(torch, 50, 1000)  # rowptr (51) whole; col, val (1000) sampled
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), 50, 77, rp, ci, vv)
    bench.dump_outputs(str(b), 50, 77, rp, ci, vv * 2.0)  # other values, same positions
    assert not (a / "rowptr_index.npy").exists()
    np.testing.assert_array_equal(np.load(a / "rowptr.npy"), rp.numpy())
    for name, t in (("col", ci), ("val", vv)):
        idx = np.load(a / (name + "_index.npy"))
        np.testing.assert_array_equal(idx, np.load(b / (name + "_index.npy")))
        assert idx.shape == (64,) and np.all(np.diff(idx) >= 0) and 0 <= idx[0] and idx[-1] < 1000
        np.testing.assert_array_equal(np.load(a / (name + ".npy")), t.numpy()[idx.astype(np.int64)])
    np.testing.assert_array_equal(np.load(b / "val.npy"), 2.0 * np.load(a / "val.npy"))
    # a shorter dump into the same folder leaves no stale sample positions behind
    monkeypatch.setattr(bench, "DUMP_CAP", 4096)
    bench.dump_outputs(str(a), 50, 77, rp, ci, vv)
    assert not (a / "col_index.npy").exists() and np.load(a / "col.npy").shape == (1000,)
