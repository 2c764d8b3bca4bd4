"""bench.py --dump-outputs: the writer of the hand-over arrays (no GPU: made-up parts)."""
import numpy as np

import bench


def _parts(rng):
    return {"refs": rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32),
            "runoff": np.cumsum(rng.integers(0, 1 << 40, 301, dtype=np.uint64), dtype=np.uint64),
            "rundep": rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32),
            "heavy_bits": rng.integers(0, 1 << 63, 40, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
            "members": np.empty(0, np.uint64)}


def _load(path, name):
    a = np.load(path / f"{name}.npy")
    assert a.dtype == np.float64
    return a


def test_dump_is_exact_when_it_fits(tmp_path):
    parts = _parts(np.random.default_rng(5))
    bench.dump_outputs(str(tmp_path), parts, [1, 2, 3])
    for name, a in parts.items():
        got = _load(tmp_path, name)
        if a.dtype == np.uint64:  # (low, high) u32 pairs: every bit of the u64 is kept
            assert got.shape == (a.size, 2)
            back = got[:, 0].astype(np.uint64) | (got[:, 1].astype(np.uint64) << np.uint64(32))
        else:
            back = got.astype(np.uint32)
        assert np.array_equal(back, a), name
    assert _load(tmp_path, "layout").tolist() == [1.0, 2.0, 3.0]


def test_dump_samples_within_budget_and_repeats(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)
    parts = _parts(np.random.default_rng(6))
    bench.dump_outputs(str(tmp_path / "a"), parts, [0])
    bench.dump_outputs(str(tmp_path / "b"), {k: v.copy() for k, v in parts.items()}, [0], suffix=".rank1")
    total = 0
    for name, a in parts.items():
        got = _load(tmp_path / "a", name)
        total += got.nbytes
        assert np.array_equal(got, np.load(tmp_path / "b" / f"{name}.rank1.npy")), name  # the same rows every time
        if name in ("rundep", "heavy_bits", "members"):  # within their share: whole
            assert len(got) == len(a)
    assert total <= 20000
    refs = _load(tmp_path / "a", "refs")
    assert 0 < len(refs) < 5000
    # a sample of rows in row order: refs is a subsequence of the part
    it = iter(parts["refs"].tolist())
    assert all(any(x == y for y in it) for x in refs.astype(np.uint32).tolist())
    # the budget left by the small parts goes to the larger ones
    assert total > 20000 - 2 * 16
