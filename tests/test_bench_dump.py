"""bench.py --dump-outputs: the files written for the last timed step's batch (bench.dump_outputs)
hold the downloaded arrays as float32 / float64, long ones as the same fixed sample in every run,
64 MB at most in all. CPU only: the batch and the indel tally are stand-ins that return arrays."""
import os

import numpy as np

import bench
from genomeanonymizer_amd import native


class _Batch:
    def __init__(self, seq, calls, bases, tot):
        self.out = (seq, calls, bases, tot)

    def download(self):
        return self.out


class _Indels:
    def __init__(self, recs):
        self.recs = recs

    def download(self):
        return self.recs


def _outputs(n_seq, n_scopes, n_recs, seed=3):
    rng = np.random.default_rng(seed)
    recs = np.zeros(n_recs, native.INDEL_REC)
    for f in recs.dtype.names:
        recs[f] = rng.integers(0, 1 << 30, n_recs)
    return (_Batch(rng.integers(0, 256, n_seq).astype(np.uint8), rng.integers(0, 9, n_scopes).astype(np.int32),
                   rng.integers(0, 99, n_scopes).astype(np.int32), rng.integers(0, 1 << 40, 8).astype(np.int64)),
            _Indels(recs))


def test_short_outputs_are_written_whole(tmp_path):
    db, ind = _outputs(1001, 77, 13)
    written = bench.dump_outputs(str(tmp_path / "d"), db, ind)
    seq, calls, bases, tot = db.out
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == ["indel_records", "masked_seq_nt16", "scope_masked_bases", "scope_masked_calls", "totals"]
    assert got["masked_seq_nt16"].dtype == np.float32 and np.array_equal(got["masked_seq_nt16"], seq)
    for name, a in (("scope_masked_calls", calls), ("scope_masked_bases", bases), ("totals", tot)):
        assert got[name].dtype == np.float64 and np.array_equal(got[name], a)
    assert got["indel_records"].shape == (13, len(native.INDEL_REC.names))
    assert np.array_equal(got["indel_records"][:, 1], ind.recs["pos"])
    assert written["masked_seq_nt16"] == [1001, 1001] and written["indel_records"] == [13, 13]
    # no tally in the step: no file of it
    assert "indel_records" not in bench.dump_outputs(str(tmp_path / "e"), db, None)
    assert not os.path.exists(tmp_path / "e" / "indel_records.npy")


def test_long_outputs_are_the_same_bounded_sample_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)   # (the rule at a small size: 1024 float32, 512 float64, 64 records)
    db, ind = _outputs(50_000, 3000, 500)
    w1 = bench.dump_outputs(str(tmp_path / "a"), db, ind)
    w2 = bench.dump_outputs(str(tmp_path / "b"), db, ind)
    assert w1 == w2
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.nbytes <= 4096 and np.array_equal(a, b)
    a = np.load(tmp_path / "a" / "masked_seq_nt16.npy")
    idx = np.unique(np.random.default_rng(0).integers(0, 50_000, 1024))
    assert np.array_equal(a, db.out[0][idx]) and len(a) > 900
    # another value at a sampled place shows in the file
    db.out[0][idx[5]] ^= 0xFF
    bench.dump_outputs(str(tmp_path / "c"), db, ind)
    assert not np.array_equal(np.load(tmp_path / "c" / "masked_seq_nt16.npy"), a)


def test_dump_stays_under_64_mb():
    # five arrays at most, each DUMP_BYTES at most (plus the .npy headers)
    assert 5 * (bench.DUMP_BYTES + 1024) <= 64 << 20
