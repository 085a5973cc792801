"""bench.py --dump-outputs (no GPU): the files a run leaves for comparing two builds -- their
names, dtypes and contents, independence of the order the events arrive in, the fixed sample of
an output above the size cap, and the per-rank names at N>1."""
import os

import numpy as np
import pytest

import bench
from txflow_amd import EVENT_DTYPE


def _results(n=5000, n_ev=300, seed=1):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 256, n).astype(np.uint8)
    ev = np.zeros(n_ev, EVENT_DTYPE)
    ev["vote_index"] = rng.choice(n, n_ev, replace=False)
    ev["tx_index"] = rng.permutation(n_ev)
    ev["sum"] = rng.integers(1, 1 << 40, n_ev)
    return st, ev


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_outputs(tmp_path):
    st, ev = _results()
    bench.dump_outputs(str(tmp_path / "a"), st, ev, 0, 1)
    got = _load(tmp_path / "a")
    assert sorted(got) == ["commit_sum.npy", "commit_tx_index.npy", "commit_vote_index.npy", "status.npy"]
    assert got["status.npy"].dtype == np.float32 and np.array_equal(got["status.npy"], st)
    order = np.argsort(ev["vote_index"])
    for f in ("vote_index", "tx_index", "sum"):
        a = got[f"commit_{f}.npy"]
        assert a.dtype == np.float64 and np.array_equal(a, ev[f][order])   # every value exact in float64
    # the same events reported in another order: the same files
    bench.dump_outputs(str(tmp_path / "b"), st, ev[np.random.default_rng(7).permutation(len(ev))], 0, 1)
    other = _load(tmp_path / "b")
    assert all(np.array_equal(got[f], other[f]) for f in got)


def test_dump_sample_above_cap(tmp_path, monkeypatch):
    st, ev = _results()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8192)        # 2048 B per group and rank at N=2
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), st, ev, 1, 2)
    got, again = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(got) == ["commit_sum.rank1.npy", "commit_tx_index.rank1.npy", "commit_vote_index.rank1.npy",
                           "commit_vote_index_rows.rank1.npy", "status.rank1.npy", "status_rows.rank1.npy"]
    assert all(np.array_equal(got[f], again[f]) for f in got)                 # the sample is fixed
    assert sum(a.nbytes for a in got.values()) <= 8192 // 2
    rows = got["status_rows.rank1.npy"].astype(np.int64)
    assert len(rows) == 2048 // 12 and (np.diff(rows) > 0).all() and rows[-1] < len(st)
    assert np.array_equal(got["status.rank1.npy"], st[rows])
    erows = got["commit_vote_index_rows.rank1.npy"].astype(np.int64)
    sev = ev[np.argsort(ev["vote_index"])]
    assert len(erows) == 2048 // 32 and (np.diff(erows) > 0).all()
    for f in ("vote_index", "tx_index", "sum"):
        assert np.array_equal(got[f"commit_{f}.rank1.npy"], sev[f][erows])


def test_steps_must_be_positive(monkeypatch, capsys):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2 and "--steps" in capsys.readouterr().err
