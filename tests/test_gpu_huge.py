"""The huge-scope tile path (scopes wider than 2^20 positions: ganon_huge::plan, k_tile_large<1>,
k_tile_large<4>, k_mask_large, and the huge branches of prep, group and run) against the CPU oracle —
needs an MI355X.

The batches are the hand-built ones of tests/huge_batches.py (pinned without a device by
tests/test_huge_batches.py). Everything is compared bit for bit: the whole output buffer, the per-scope
counts, the totals, and every number of the plan that follows from the batch (huge scopes, tiles,
reads written by huge scopes, rare tiles).
"""
import numpy as np
import pytest

from huge_batches import crowd_batch, rare_stride_batch, threshold_pair, tile_edge_batch

pytestmark = pytest.mark.gpu

DEFAULTS = {"PREP_LONG": -1, "FUSED_FLAT": 1}
CONTEXTS = {"default": {}, "prep_long_1": {"PREP_LONG": 1}, "prep_long_0": {"PREP_LONG": 0},
            "fused_flat_0": {"FUSED_FLAT": 0}}


@pytest.fixture(scope="module")
def masker(hip_built):
    from genomeanonymizer_amd import native
    m = native.HipMasker(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle():
    from pyoracle import OracleEngine
    return OracleEngine()


def _set(masker, **params):
    from genomeanonymizer_amd import native
    for name, value in params.items():
        masker.set_param(getattr(native, "PARAM_" + name), value)


_CACHE = {}


def _batch(oracle, name):
    """(arrays, info, the oracle's result) of a named batch, made once per module and never modified."""
    if name not in _CACHE:
        if name == "ordinary":
            from genomeanonymizer_amd.synth.batch import config2_batch
            arr, _ = config2_batch(n_reads=20_000, genome=4_000_000, n_windows=1_500, n_germline=4_000, seed=5)
            info = {"tiles_per_scope": np.zeros(1, np.int64), "rare_tiles": 0, "huge_written_reads": 0}
        elif name in ("below", "above"):
            arr, info = threshold_pair()[name == "above"]
        else:
            arr, info = {"tile_edge": tile_edge_batch, "rare_stride": rare_stride_batch, "crowd": crowd_batch}[name]()
        want = oracle.mask(arr)
        for a in arr.values():
            a.setflags(write=False)
        _CACHE[name] = (arr, info, want)
    return _CACHE[name]


def _assert_equals_oracle(got, want, info, what):
    """The whole buffer (pass-through reads included), the per-scope counts, the totals the oracle
    computes, and the tile path's own totals."""
    out, calls, bases, tot = got
    assert np.array_equal(calls, want[1]), (what, calls.tolist(), want[1].tolist())
    assert np.array_equal(bases, want[2]), (what, bases.tolist(), want[2].tolist())
    assert np.array_equal(out, want[0]), (what, np.nonzero(out != want[0])[0][:8].tolist())
    assert tot[0] == want[3][0] and tot[1] == want[3][1], (what, tot.tolist())
    assert tot[2:5].tolist() == want[3][2:5].tolist(), (what, tot.tolist())
    assert tot[6] == info["tiles_per_scope"].sum(), (what, tot.tolist())
    assert tot[5] == info["rare_tiles"], (what, tot.tolist())


def _assert_plan(db, info, what):
    got = db.info()
    assert got["huge_scopes"] == int((info["tiles_per_scope"] > 0).sum()), (what, got)
    assert got["huge_tiles"] == info["tiles_per_scope"].sum(), (what, got)
    assert got["huge_written_reads"] == info["huge_written_reads"], (what, got)


def _same(a, b, what):
    for k in range(4):
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("context", list(CONTEXTS))
def test_tile_edges_match_oracle_in_every_prep_mode(masker, oracle, context):
    """The tile-edge batch under each way the ordinary scopes of the same batch are prepared."""
    arr, info, want = _batch(oracle, "tile_edge")
    db = None
    try:
        _set(masker, **CONTEXTS[context])
        db = masker.upload(arr)
        print(context, db.shape(), db.info())
        _assert_plan(db, info, context)
        db.run()
        got = db.download()
    finally:
        _set(masker, **DEFAULTS)
        if db is not None:
            db.free()
    _assert_equals_oracle(got, want, info, context)


def test_repeated_runs_give_the_same_result(masker, oracle):
    """Three runs before one download, then a run and a download again: the per-scope counts are
    cleared by every run and the rare-tile count by every k_finish."""
    arr, info, want = _batch(oracle, "tile_edge")
    db = masker.upload(arr)
    try:
        for _ in range(3):
            db.run()
        first = db.download()
        db.run()
        second = db.download()
    finally:
        db.free()
    _assert_equals_oracle(first, want, info, "after three runs")
    _assert_equals_oracle(second, want, info, "after a fourth run")


def test_span_threshold(masker, oracle):
    """A span of exactly 2^20 stays with the group kernel; one more position takes the tile path."""
    for name, huge in (("below", 0), ("above", 1)):
        arr, info, want = _batch(oracle, name)
        db = masker.upload(arr)
        try:
            assert db.info()["huge_scopes"] == huge
            _assert_plan(db, info, name)
            db.run()
            got = db.download()
        finally:
            db.free()
        _assert_equals_oracle(got, want, info, name)


def test_rare_rerun_grid_stride(masker, oracle):
    """1,030 rare tiles on the re-run's 1,024 workgroups."""
    arr, info, want = _batch(oracle, "rare_stride")
    db = masker.upload(arr)
    try:
        _assert_plan(db, info, "rare_stride")
        db.run()
        got = db.download()
    finally:
        db.free()
    assert got[3][5] == 1030 and got[1].tolist() == [1030]
    _assert_equals_oracle(got, want, info, "rare_stride")


def test_mask_large_wave_stride(masker, oracle):
    """33,000 reads written by one huge scope: more than k_mask_large's 8192 x 4 waves."""
    arr, info, want = _batch(oracle, "crowd")
    db = masker.upload(arr)
    try:
        _assert_plan(db, info, "crowd")
        db.run()
        got = db.download()
    finally:
        db.free()
    _assert_equals_oracle(got, want, info, "crowd")


def _run_twice(db):
    db.run()
    db.run()
    return db.download()


def test_reload_and_replan_lifecycle(masker, oracle):
    """One device batch reloaded between an ordinary batch and huge batches of other table and tile
    counts (the tile plan and the lazily allocated table are released and made again), then replanned
    from its device arrays: every result equals a fresh mask() of that batch."""
    names = ("ordinary", "tile_edge", "ordinary", "rare_stride", "tile_edge")
    fresh = {n: masker.mask(_batch(oracle, n)[0]) for n in set(names)}
    for n in set(names):
        _assert_equals_oracle(fresh[n], _batch(oracle, n)[2], _batch(oracle, n)[1], ("fresh", n))
    db = masker.upload(_batch(oracle, names[0])[0])
    try:
        for step, n in enumerate(names):
            if step:
                db.reload(_batch(oracle, n)[0])
            _assert_plan(db, _batch(oracle, n)[1], (step, n))
            _same(_run_twice(db), fresh[n], (step, n))
        for k in range(3):                      # planned from copies of the device arrays
            db.replan()
        _assert_plan(db, _batch(oracle, "tile_edge")[1], "replanned")
        _same(_run_twice(db), fresh["tile_edge"], "replanned")
        db.replan()
        db.run()
        _same(db.download(), fresh["tile_edge"], "replan, run")
    finally:
        db.free()


def test_lifecycle_with_a_resident_reference(masker, oracle):
    arr, info, want = _batch(oracle, "tile_edge")
    ref = masker.upload_reference(arr["ref_nt16"])
    db = None
    try:
        db = masker.upload({k: v for k, v in arr.items() if k != "ref_nt16"}, ref=ref)
        _assert_plan(db, info, "resident")
        _assert_equals_oracle(_run_twice(db), want, info, "resident")
        for k in range(3):
            db.replan()
        _assert_plan(db, info, "resident, replanned")
        _assert_equals_oracle(_run_twice(db), want, info, "resident, replanned")
    finally:
        if db is not None:
            db.free()
        ref.free()


def test_speculative_plan_falls_back_to_the_tile_path(hip_built, oracle):
    """A reload that speculates on the context's last one-segment shape (GANON_PARAM_SPEC_PLAN 2) meets
    huge scopes: the gate stops the run, the download plans the tiles from the device arrays and runs
    the batch in full."""
    from genomeanonymizer_amd import native
    o_arr, o_info, o_want = _batch(oracle, "ordinary")
    arr, info, want = _batch(oracle, "tile_edge")
    m = native.HipMasker(0)
    db = None
    try:
        m.set_param(native.PARAM_SPEC_PLAN, 2)
        db = m.upload(o_arr)
        db.run()
        _assert_equals_oracle(db.download(), o_want, o_info, "ordinary")
        assert db.shape()["prep_mode"] == "one_segment_fused"
        db.reload(arr)
        db.run()
        assert db.gated_runs() == 1
        _assert_equals_oracle(db.download(), want, info, "gated, planned in full")
        _assert_plan(db, info, "after the fallback")
        db.reload(o_arr)                 # the last plan had huge scopes: a full plan
        db.run()
        assert db.gated_runs() == 0
        _assert_equals_oracle(db.download(), o_want, o_info, "ordinary again")
        _assert_plan(db, o_info, "ordinary again")
    finally:
        if db is not None:
            db.free()
        m.close()
