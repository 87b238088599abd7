"""bench.py's command line and --dump-outputs writer (no GPU: the parser and the
writer on a synthetic result array)."""
import os
import sys

import numpy as np

import bench
from minisched_amd import _lib


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere", "--no-cpu-baseline")
    assert a.full is True and a.dump_outputs == "somewhere" and a.no_cpu_baseline is True


def _results(n):
    res = np.zeros(n, dtype=_lib.RESULT)
    res["node"] = np.arange(n) * 3 - 1
    res["code"] = np.arange(n) % 3
    res["score"] = np.arange(n, dtype=np.int64) * 1000003
    res["plugin_mask"] = np.arange(n) % 5
    return res


def test_dump_outputs_whole(tmp_path):
    res = _results(1000)
    bench.dump_outputs(str(tmp_path / "d"), res, 0, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f"{f}.npy" for f in bench.DUMP_FIELDS)
    for f in bench.DUMP_FIELDS:
        got = np.load(tmp_path / "d" / f"{f}.npy")
        assert got.dtype == np.float64 and got.shape == (1000,)
        assert np.array_equal(got, res[f].astype(np.float64))


def test_dump_outputs_sampled_and_per_rank(tmp_path, monkeypatch):
    # a budget of 100 pods per rank at world 2: a fixed sample, the same on every call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 100 * 8 * (len(bench.DUMP_FIELDS) + 1))
    res = _results(1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, 5000, 1, 2)
    idx = np.load(tmp_path / "a" / "pod_index_rank1.npy")
    assert idx.shape == (100,) and np.all(np.diff(idx) > 0) and idx.min() >= 5000 and idx.max() < 6000
    total = 0
    for name in os.listdir(tmp_path / "a"):
        assert name.endswith("_rank1.npy")
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
        total += np.load(tmp_path / "a" / name).nbytes
    assert total <= bench.DUMP_MAX_BYTES // 2
    rows = (idx - 5000).astype(np.int64)
    for f in bench.DUMP_FIELDS:
        assert np.array_equal(np.load(tmp_path / "a" / f"{f}_rank1.npy"), res[f][rows].astype(np.float64))
