"""Every compiled k_group instantiation and every tuning knob against the CPU oracle — needs an MI355X.

``ganon_batch_run`` picks one of 18 instantiations of the group kernel: three families (the fused
one, the long-read one, the record pass) times (unroll, observation list) = (1, 2, 4, 8) x 512 and
(1, 2) x 1024. include/ganon.h promises that results never depend on the knobs that pick them, nor
on GANON_PARAM_REF2, NT_COPY, GROUP_TARGET and PREP_UNROLL. Here every one of them runs the
deterministic edge batches of tests/kgroup_batches.py (pinned without a device by
tests/test_kgroup_batches.py) and must give the oracle's bytes and counts, exactly; each family is
asserted through the planned prep mode, each observation-list path through the path counters.
"""
import numpy as np
import pytest

from kgroup_batches import chunk_edge_batch, count_observations, threshold_batch, touched_reads_differ

pytestmark = pytest.mark.gpu

# (unroll, observation list) pairs the dispatch compiles, per family
PAIRS = [(1, 512), (2, 512), (4, 512), (8, 512), (1, 1024), (2, 1024)]
# (unroll, observation list, REF2, NT_COPY)
SETTINGS = ([(u, obs, 1, 1) for u, obs in PAIRS] + [(u, 512, 0, 1) for u in (1, 2, 4, 8)] +
            [(2, 512, 1, 0), (8, 512, 1, 0)])
# family -> for the (one-segment, multi-segment) batch: the parameters read at upload, the prep mode planned
FAMILIES = {
    "fused": (({}, {}), ("one_segment_fused", "multi_segment_fused")),
    "record": (({"FUSED_FLAT": 0}, {"FUSED_FLAT": 0, "PREP_LONG": 0}), ("one_segment", "two_pass")),
    "long": (({"PREP_LONG": 1}, {"PREP_LONG": 1}), ("long_read", "long_read")),
}
DEFAULTS = {"GROUP_UNROLL": 0, "GROUP_OBS": 0, "REF2": 1, "NT_COPY": 1, "GROUP_TARGET": 0, "PREP_LONG": -1,
            "FUSED_FLAT": 1, "PREP_UNROLL": 0}


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


def _restore(masker):
    _set(masker, **DEFAULTS)


_CACHE = {}


def _batch(oracle, key):
    """(arrays, the oracle's result) of a named batch, made once per module and never modified."""
    if key not in _CACHE:
        from genomeanonymizer_amd.synth.batch import config2_batch, longread_batch, random_batch, relayout
        kind = key[0]
        if kind == "edge":
            arr, _ = chunk_edge_batch(key[1], end_on_long=key[2])
        elif kind == "edge_shuffled":
            arr = _batch(oracle, ("edge", key[1], False))[0]
            arr = relayout(arr, np.random.default_rng(77).permutation(len(arr["read_len"])))
        elif kind == "longread":
            # the smallest reads that take the long-read prep on their own (several segments, over
            # 1000 bases) and span more than 16384 positions each
            arr, info = longread_batch(5, n_reads=24, genome=300_000, len_range=(16_500, 17_000))
            assert info["max_span"] > 16384
        elif kind == "random":
            arr = random_batch(key[1], n_scopes=40, **({"wide_scopes": 4} if key[2] else {}))
        elif kind == "config2":
            arr, _ = config2_batch(n_reads=60_000, genome=20_000_000, n_windows=6_000, n_germline=12_000)
        want = oracle.mask(arr)
        assert want[1].sum() > 0 and want[2].sum() > 0
        for a in arr.values():
            a.setflags(write=False)
        _CACHE[key] = (arr, want)
    return _CACHE[key]


def _assert_equals_oracle(arr, got, want, what):
    out, calls, bases, tot = got
    assert touched_reads_differ(arr, out, want[0]) == [], what
    assert np.array_equal(calls, want[1]), what
    assert np.array_equal(bases, want[2]), what
    assert tot[0] == want[3][0] and tot[1] == want[3][1], what


def _run_settings(masker, db, arr, want, settings):
    """Each (unroll, observation list, REF2, NT_COPY) setting on an uploaded batch: the oracle's
    result, and the same bytes from a second run."""
    for u, obs, ref2, ntc in settings:
        _set(masker, GROUP_UNROLL=u, GROUP_OBS=obs, REF2=ref2, NT_COPY=ntc)
        db.run()
        got = db.download()
        _assert_equals_oracle(arr, got, want, (u, obs, ref2, ntc))
        db.run()
        again = db.download()
        for k in range(4):
            assert np.array_equal(got[k], again[k]), (u, obs, ref2, ntc, k)


@pytest.mark.parametrize("long_end", [False, True], ids=["ends_on_1", "ends_on_257"])
@pytest.mark.parametrize("multi", [False, True], ids=["one_segment", "multi_segment"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_instantiation_matches_oracle_on_chunk_edges(masker, oracle, family, multi, long_end):
    arr, want = _batch(oracle, ("edge", multi, long_end))
    upload_params, modes = FAMILIES[family]
    db = None
    try:
        _set(masker, **upload_params[multi])
        db = masker.upload(arr)
        assert db.shape()["prep_mode"] == modes[multi]
        _run_settings(masker, db, arr, want, SETTINGS)
    finally:
        _restore(masker)
        if db is not None:
            db.free()


def test_every_long_instantiation_matches_oracle_on_long_reads(masker, oracle):
    """The long-read family as the plan picks it on its own (no forced prep mode)."""
    arr, want = _batch(oracle, ("longread",))
    db = masker.upload(arr)
    try:
        assert db.shape()["prep_mode"] == "long_read"
        _run_settings(masker, db, arr, want, SETTINGS)
    finally:
        _restore(masker)
        db.free()


@pytest.mark.parametrize("multi", [False, True], ids=["one_segment", "multi_segment"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_wide_unrolls_match_oracle_on_a_shuffled_buffer(masker, oracle, family, multi):
    """The reads' bases in a shuffled buffer order: a group's reads lie all over the buffer, so most
    masks go to the far list and the partitions end anywhere in a read."""
    arr, want = _batch(oracle, ("edge_shuffled", multi))
    upload_params, modes = FAMILIES[family]
    db = None
    try:
        _set(masker, **upload_params[multi])
        db = masker.upload(arr)
        assert db.shape()["prep_mode"] == modes[multi]
        _run_settings(masker, db, arr, want, [(4, 512, 1, 1), (8, 512, 1, 1)])
    finally:
        _restore(masker)
        if db is not None:
            db.free()


def _expected_path(n, obs, cap):
    return None if n <= 256 else "sorted_lists" if n <= obs else "overflowing_lists" if n <= cap else "key_range_splits"


@pytest.mark.parametrize("u", [2, "other"])
@pytest.mark.parametrize("obs", [512, 1024])
@pytest.mark.parametrize("family", ["fused", "record"])
def test_observation_list_thresholds(masker, oracle, family, obs, u):
    """One group with exactly n observations, n at each threshold between the list paths: the
    unsorted match (n <= 256), the sorted LDS list (n <= OBS), the global region (n <= cap, the
    group's region capacity) and the key-range split above it — and, with a region smaller than the
    1024-entry list, the split taken straight from the LDS list."""
    u = u if u == 2 else (1 if obs == 1024 else 8)
    upload_params, modes = FAMILIES[family]
    paths_seen = set()
    try:
        _set(masker, GROUP_UNROLL=u, GROUP_OBS=obs, **upload_params[0])
        cases, cap_of = [(150, 255)], {}
        while cases:
            n_reads, n = cases.pop(0)
            arr, made = threshold_batch(n, n_reads)
            assert made == n == count_observations(arr)
            want = oracle.mask(arr)
            assert want[1][0] > 0 and want[2][0] > 0
            db = masker.upload(arr)
            try:
                assert db.shape()["prep_mode"] == modes[0]
                info = db.info()
                cap = info["overflow_region"]        # one group: its region is the whole region
                if n_reads not in cap_of:
                    cap_of[n_reads] = cap
                    if n_reads == 150:
                        assert cap > 1025
                        cases += [(150, x) for x in (256, 257, obs, obs + 1, cap, cap + 1)] + [(20, 255)]
                    elif obs == 1024:
                        assert cap < 1024
                        cases += [(20, cap + 1), (20, 1025)]
                assert cap == cap_of[n_reads]
                db.run()
                got = db.download()
                paths = db.path_counts()
                assert db.gated_runs() == 0
            finally:
                db.free()
            print(f"{family} U={u} OBS={obs} n_reads={n_reads} n={n} cap={cap}: {paths}")
            _assert_equals_oracle(arr, got, want, (n_reads, n))
            expected = _expected_path(n, obs, cap)
            paths_seen.add(expected)
            if expected is None:
                assert not any(paths.values()), (n, paths)
            elif expected == "key_range_splits":
                assert paths["key_range_splits"] >= 1, (n, paths)
                if cap < obs:                    # straight from the LDS list: the region never filled
                    assert paths["overflowing_lists"] == 0, (n, paths)
            else:
                other = {"sorted_lists", "overflowing_lists", "key_range_splits"} - {expected}
                assert paths[expected] == 1 and not any(paths[k] for k in other), (n, paths)
    finally:
        _restore(masker)
    assert paths_seen == {None, "sorted_lists", "overflowing_lists", "key_range_splits"}


@pytest.mark.parametrize("combo", [(4, 1024), (8, 1024)], ids=["U4_OBS1024", "U8_OBS1024"])
def test_uncompiled_pairs_are_rejected(masker, oracle, combo):
    """No group kernel is compiled for unroll 4 or 8 with the 1024-entry list: the run is an error
    that names both values (never another pair's kernel under that label), and the batch runs as
    before once the parameters are back."""
    from genomeanonymizer_amd import native
    arr, want = _batch(oracle, ("edge", False, False))
    u, obs = combo
    db = masker.upload(arr)
    try:
        db.run()
        before = db.download()
        _set(masker, GROUP_UNROLL=u, GROUP_OBS=obs)
        with pytest.raises(native.GanonError) as e:
            db.run()
        assert str(u) in str(e.value) and str(obs) in str(e.value)
        _restore(masker)
        db.run()
        after = db.download()
    finally:
        _restore(masker)
        db.free()
    _assert_equals_oracle(arr, after, want, combo)
    for k in range(4):
        assert np.array_equal(before[k], after[k]), k


@pytest.mark.parametrize("key", [("random", 2, False), ("random", 4, True), ("config2",)],
                         ids=["random_2", "random_4_wide", "config2"])
def test_group_target_never_changes_results(masker, oracle, key):
    """GANON_PARAM_GROUP_TARGET (read at upload) at its bounds and in between: other groups, the
    same result. (At 16 the largest scopes exceed twice the target: the ordered launch.)"""
    arr, want = _batch(oracle, key)
    groups = {}
    try:
        for target in (16, 64, 65536):
            _set(masker, GROUP_TARGET=target)
            db = masker.upload(arr)
            try:
                groups[target] = db.info()["groups"]
                db.run()
                got = db.download()
            finally:
                db.free()
            _assert_equals_oracle(arr, got, want, target)
    finally:
        _restore(masker)
    assert groups[16] > groups[65536] >= 1, groups


@pytest.mark.parametrize("key", [("edge", False, False), ("config2",)], ids=["chunk_edges", "config2"])
def test_prep_unroll_never_changes_results(masker, oracle, key):
    """GANON_PARAM_PREP_UNROLL: the one-segment record pass's emit at 1, 2 and 4 incidences per trip."""
    arr, want = _batch(oracle, key)
    db = None
    try:
        _set(masker, FUSED_FLAT=0)
        db = masker.upload(arr)
        assert db.shape()["prep_mode"] == "one_segment"
        for pu in (1, 2, 4):
            _set(masker, PREP_UNROLL=pu)
            db.run()
            _assert_equals_oracle(arr, db.download(), want, pu)
    finally:
        _restore(masker)
        if db is not None:
            db.free()
