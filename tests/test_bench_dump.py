"""CPU: bench.py --dump-outputs writes float64 .npy files of bounded size, a
small solution whole and a large one as the same seeded sample every time."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_small_solution_is_dumped_whole(tmp_path):
    u = np.arange(257 * 257, dtype=np.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "a"), u, 1.25e-3)
    got = _load(tmp_path / "a")
    assert sorted(got) == ["residual.npy", "u.npy"]
    assert got["u.npy"].dtype == np.float64 and np.array_equal(got["u.npy"], u)
    assert got["residual.npy"].dtype == np.float64
    assert got["residual.npy"].tolist() == [1.25e-3]


def test_large_solution_is_a_fixed_sample(tmp_path):
    keep = bench.DUMP_WHOLE_BYTES // 8
    u = np.arange(keep + 12345, dtype=np.float64)   # value = its own index
    bench.dump_outputs(str(tmp_path / "a"), u, 0.0)
    bench.dump_outputs(str(tmp_path / "b"), u + 1.0, 0.0)
    a, b = _load(tmp_path / "a")["u.npy"], _load(tmp_path / "b")["u.npy"]
    assert a.dtype == np.float64 and a.size == keep
    assert np.array_equal(b, a + 1.0)            # the same points both times
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < u.size
    assert np.unique(a).size > 0.6 * keep        # spread over the grid, not one block
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20


def test_ranks_write_their_own_files_within_the_budget(tmp_path):
    keep = bench.DUMP_WHOLE_BYTES // 8 // 4
    u = np.arange(keep + 7, dtype=np.float64)
    for r in range(4):
        bench.dump_outputs(str(tmp_path), u, 2.0, rank=r, world=4)
    got = _load(tmp_path)
    assert sorted(got) == ["residual.npy"] + [f"u_rank{r}.npy" for r in range(4)]
    assert all(got[f"u_rank{r}.npy"].size == keep for r in range(4))
    assert sum(os.path.getsize(tmp_path / f) for f in got) <= 64 << 20
