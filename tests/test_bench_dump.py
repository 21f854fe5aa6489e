"""bench.py --dump-outputs (CPU): the dumped fields are float64, stay within the size budget over all ranks, and a field too large
for its share is cut down to the same seeded sample of sites in every run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeField:
    def __init__(self, a):
        self.a = a

    def download(self):
        return self.a.copy()


def test_argument_is_parsed():
    assert bench.parse(["--dump-outputs", "out", "--steps", "7"]).dump_outputs == "out"
    assert bench.parse([]).dump_outputs is None


def test_small_fields_whole_large_fields_sampled_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 2 * 1000 * 192)          # share of one field on one of two ranks: 1000 sites
    rng = np.random.default_rng(0)
    small, big = rng.standard_normal((600, 4, 3, 2)), rng.standard_normal((5000, 4, 3, 2))
    fields = (("a", FakeField(small)), ("b", FakeField(big)), ("c", FakeField(big[::-1].copy())))
    total = 0
    for rank in (0, 1):
        rec = bench.dump_outputs(str(tmp_path / ("run%d" % rank)), fields, 2, rank)
        assert sorted(rec) == ["a_rank%d" % rank, "b_rank%d" % rank, "c_rank%d" % rank]
        for name in rec:
            total += os.path.getsize(tmp_path / ("run%d" % rank) / (name + ".npy"))
    assert total <= bench.DUMP_BYTES + 6 * 128                              # 128-byte .npy headers
    a = np.load(tmp_path / "run0" / "a_rank0.npy")
    assert a.dtype == np.float64 and np.array_equal(a, small)
    b0, b1 = np.load(tmp_path / "run0" / "b_rank0.npy"), np.load(tmp_path / "run1" / "b_rank1.npy")
    assert b0.shape == (1000, 4, 3, 2) and np.array_equal(b0, b1)           # same sites in every run
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(5000, size=1000, replace=False))
    assert np.array_equal(b0, big[idx])
    rec = bench.dump_outputs(str(tmp_path / "one"), fields, 1, 0)
    assert rec["b"]["sampled_sites"] == 2000 and rec["a"] == {"sites": 600, "shape": [600, 4, 3, 2]}
