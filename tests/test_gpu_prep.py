"""The device prep (ganon_prep.hip) on the hand-built batches of tests/prep_batches.py — needs an MI355X.

What the plan reports (ganon_batch_shape, ganon_batch_info) must equal the plain restatement
``plan_reference`` exactly, the planned mode must be the one include/ganon.h's text gives for the
parameters read at upload, the masked bytes and counts must equal the C oracle's, every one of the 14
validation errors must be raised with its kind and index (by the upload, or by the download for the
checks made during the run — also when the batch arrives by a speculative reload), and a speculative
run must be gated for each reason k_prep_reduce gates it, and only then. tests/test_prep_batches.py
pins the batches and the restatement without a device. All integer work: every comparison is exact.
"""
import numpy as np
import pytest

import prep_batches as pb

pytestmark = pytest.mark.gpu

# the parameters read at upload, per family
FAMILIES = {"fused": {}, "record": {"FUSED_FLAT": 0}, "two_pass": {"FUSED_FLAT": 0, "PREP_LONG": 0}, "long": {"PREP_LONG": 1}}
DEFAULTS = {"PREP_LONG": -1, "FUSED_FLAT": 1, "GROUP_TARGET": 0, "SPEC_PLAN": 1, "XREC_INIT": 0}
RUN_KINDS = ("incid_read", "incid_span", "ws_missing")       # found by the run, reported by the download
FLAT_MODES = ("one_segment", "one_segment_fused", "multi_segment_fused")
BORDERS = [(r, s) for r in (1, 255, 256, 257, 1023, 1024, 1025, 2049) for s in (1, 1023, 1024, 1025)]


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


def _valid(oracle, key):
    """(arrays, the oracle's result) of a named valid batch, made once per module and never modified."""
    if key not in _CACHE:
        kind = key[0]
        twin = None
        if kind == "matrix":
            arr = pb.cigar_matrix_batch()[key[1]][0]
        elif kind == "overflow":
            arr, twin, _ = pb.overflow_cigar_batch()[key[1]]
        elif kind == "border":
            arr = pb.block_border_batch(key[1], key[2])[0]
        elif kind == "eight":
            arr = pb.eight_segment_block_batch()[0]
        elif kind == "stripe":
            arr = pb.stripe_batch()[0]
        elif kind == "groups":
            arr = pb.group_table_batch(single=key[1], tail=key[2])[0]
        want = oracle.mask(arr if twin is None else twin)        # (the per-base oracle takes the cut CIGARs)
        for a in arr.values():
            a.setflags(write=False)
        _CACHE[key] = (arr, want)
    return _CACHE[key]


def _assert_equals_oracle(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what
    assert got[3][0] == want[3][0] and got[3][1] == want[3][1] and got[3][3] == want[3][3], what


def _assert_plan(db, arr, params, what):
    ref = pb.plan_reference(arr, params=params)
    shape, info = db.shape(), db.info()
    print(what, shape, {k: info[k] for k in ("groups", "huge_scopes", "written_reads")})
    assert shape == {k: ref[k] for k in ("id_ops", "max_len", "max_seg", "prep_mode")}, what
    assert info["groups"] == ref["planned_groups"], what
    assert info["huge_scopes"] == ref["huge_scopes"] and info["written_reads"] == ref["written_reads"], what
    return ref


def _plan_and_run(masker, oracle, key, family, target=0):
    """Upload in one family: the plan equals the restatement, the result the oracle's, twice."""
    arr, want = _valid(oracle, key)
    params = dict(FAMILIES[family], **({"GROUP_TARGET": target} if target else {}))
    db = None
    try:
        _set(masker, **params)
        db = masker.upload(arr)
        _assert_plan(db, arr, params, (key, family, target))
        db.run()
        got = db.download()
        _assert_equals_oracle(got, want, (key, family, target))
        db.run()
        again = db.download()
        for k in range(4):
            assert np.array_equal(got[k], again[k]), (key, family, k)
    finally:
        _restore(masker)
        if db is not None:
            db.free()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("sub", ["one_segment", "multi_segment", "many_segments", "long_cigar", "long_runs"])
def test_cigar_matrix(masker, oracle, sub, family):
    """Every CIGAR walk edge in every prep family: a family that cannot take a sub-batch (the fused
    mode with a nine-segment read, say) plans the mode the restatement names instead."""
    _plan_and_run(masker, oracle, ("matrix", sub), family)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("sub", ["thread", "wave"])
def test_query_lengths_past_2_31(masker, oracle, sub, family):
    """CIGARs whose query-consuming lengths sum past 2^31: the counting walks stop advancing the
    query offset at the read length as walk_segments does, so the plan counts the segments of the
    CIGAR cut there and the result is the oracle's for that twin."""
    _plan_and_run(masker, oracle, ("overflow", sub), family)


@pytest.mark.parametrize("family", ["fused", "record", "two_pass"])
@pytest.mark.parametrize("n_reads,n_scopes", BORDERS)
def test_scan_block_borders(masker, oracle, n_reads, n_scopes, family):
    """The special reads at the first and last slots of each thread's four reads and of each scan
    block: sums and maxima come out right only if every slot is visited exactly once."""
    _plan_and_run(masker, oracle, ("border", n_reads, n_scopes), family)


@pytest.mark.parametrize("family", ["fused", "two_pass", "long"])
def test_block_of_eight_segment_reads(masker, oracle, family):
    """A scan block whose 1,024 reads all go to the LDS list of multi-segment reads."""
    _plan_and_run(masker, oracle, ("eight",), family)


def test_full_extras_stripe_regrows(masker, oracle):
    """66,000 reads: scan blocks 0 and 64 allocate from the same stripe of the extras list, and with
    this capacity only that stripe overflows: the plan grows the list and scans again — two
    ``prep_scan`` launches for that upload (counted under profiling: the records of uploads add up
    until the next run), one for an upload with the default capacity before and after it."""
    arr, want = _valid(oracle, ("stripe",))
    dbs, scans = [], []
    try:
        masker.set_profiling(True)
        for knob in (0, pb.STRIPE_XREC_INIT, 0):
            _set(masker, XREC_INIT=knob)
            dbs.append(masker.upload(arr))
            dbs[-1].sync()
            scans.append(sum(k[1] for k in dbs[-1].kernel_times() if k[0] == "prep_scan"))
            _assert_plan(dbs[-1], arr, {}, ("stripe", knob))
        print("prep_scan launches after each upload:", scans)
        assert scans[1] - scans[0] == 2 and scans[2] - scans[1] == 1, scans
        masker.set_profiling(False)
        for db in dbs[:2]:
            db.run()
            _assert_equals_oracle(db.download(), want, "stripe")
    finally:
        masker.set_profiling(False)
        _restore(masker)
        for db in dbs:
            db.free()


@pytest.mark.parametrize("family", ["fused", "record", "two_pass", "long"])
@pytest.mark.parametrize("target", [16, 256, 704])
@pytest.mark.parametrize("shape", ["table", "single", "tail"])
def test_group_table(masker, oracle, shape, target, family):
    """Empty scopes at the front, in the middle and at the end, a scope that skips buckets, more than
    256 empty scopes in a row: the group count of the closed form (the launch bound in the
    one-segment modes), and the oracle's result, at each target (256: the only one where the weight is not target / 256
    rounded up)."""
    _plan_and_run(masker, oracle, ("groups", shape == "single", 40 if shape == "tail" else 0), family, target)


def test_kernels_launched_per_family(masker, oracle):
    """The prep kernels each family's plan and run launch (printed; the plan's are timed by the
    replan), with profiling on: each family runs kernels of its own."""
    arr, want = _valid(oracle, ("matrix", "multi_segment"))
    seen = {}
    try:
        masker.set_profiling(True)
        for family, params in FAMILIES.items():
            _set(masker, SPEC_PLAN=0, **params)
            db = masker.upload(arr)
            try:
                db.replan()
                db.run()
                db.sync()
                seen[family] = [k[0] for k in db.kernel_times()]
                print(family, db.shape()["prep_mode"], db.kernel_times())
                _assert_equals_oracle(db.download(), want, family)
            finally:
                db.free()
                _restore(masker)
    finally:
        masker.set_profiling(False)
        _restore(masker)
    assert all("prep_scan" in v for v in seen.values()), seen
    assert "prep_cands" in seen["fused"] and "prep_cands" not in seen["two_pass"], seen
    assert "prep_emit" in seen["two_pass"] and "prep_emit" in seen["long"], seen


# ---- validation -------------------------------------------------------------------------------
def _raises_with(text, fn):
    from genomeanonymizer_amd import native
    with pytest.raises(native.GanonError) as e:
        fn()
    assert text in str(e.value), (text, str(e.value))


def test_invalid_batches_are_named(masker):
    """Each of the 14 error kinds, with its index, at the last slot of a scan block and the first of
    the next: from the upload, or (incidence and write-scope checks) from the download."""
    kinds = set()
    for name, bad, err, good in pb.invalid_batches():
        text = pb.error_text(err)
        kinds.add(err[0])
        if err[0] not in RUN_KINDS:
            _raises_with(text, lambda: masker.upload(bad))
            continue
        db = masker.upload(bad)
        try:
            db.run()
            _raises_with(text, db.download)
        finally:
            db.free()
    assert kinds == set(pb.ERR_TEXT)


def test_invalid_batches_by_speculative_reload(masker, oracle):
    """The same batches arriving by a speculative reload after a plan of the valid neighbour: the
    neighbour runs as speculated, the invalid batch runs nothing (one gated run) and the download
    names the error; then the context masks the neighbour correctly again. (A neighbour that does
    not plan in a one-segment mode cannot be speculated on: its reload plans in full and raises.)"""
    speculated = 0
    try:
        for name, bad, err, good in pb.invalid_batches():
            text = pb.error_text(err)
            want = oracle.mask(good)
            _set(masker, SPEC_PLAN=0)        # a full plan of the neighbour (with 2 the upload may speculate too) ...
            db = masker.upload(good)
            _set(masker, SPEC_PLAN=2)        # ... then reloads of the same sizes speculate after a one-segment plan
            try:
                flat = db.shape()["prep_mode"] in FLAT_MODES
                db.run()
                _assert_equals_oracle(db.download(), want, name)
                if flat:
                    db.reload(good)
                    db.run()
                    _assert_equals_oracle(db.download(), want, name)
                    assert db.gated_runs() == 0, name
                if flat or err[0] in RUN_KINDS:
                    speculated += flat
                    db.reload(bad)
                    db.run()
                    if flat:
                        assert db.gated_runs() == (0 if err[0] in RUN_KINDS else 1), name
                    _raises_with(text, db.download)
                else:
                    _raises_with(text, lambda: db.reload(bad))
                db.reload(good)
                db.run()
                _assert_equals_oracle(db.download(), want, name)
            finally:
                db.free()
    finally:
        _restore(masker)
    assert speculated >= 40


# ---- the gate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("reason", pb.GATE_REASONS)
def test_gate_reasons(masker, oracle, reason):
    """After a full plan of the base batch, a batch of the same sizes on the limit runs as
    speculated (no gated run); one past the limit runs nothing, counts one gated run, and the
    download plans it in full: the oracle's result and the full plan's shape. (The sixth reason, an
    invalid field, is test_invalid_batches_by_speculative_reload.)"""
    base, inside, gated = pb.gate_batches(reason)
    params = {"XREC_INIT": pb.GATE_XREC_INIT} if reason == "extras" else {}
    db = None
    try:
        _set(masker, SPEC_PLAN=0, **params)      # a full plan of the base batch, then speculative reloads
        db = masker.upload(base)
        _set(masker, SPEC_PLAN=2)
        ref = _assert_plan(db, base, {}, (reason, "base"))
        assert ref["prep_mode"] == "one_segment_fused"
        db.run()
        _assert_equals_oracle(db.download(), oracle.mask(base), (reason, "base"))
        db.reload(inside)
        db.run()
        assert db.gated_runs() == 0
        _assert_equals_oracle(db.download(), oracle.mask(inside), (reason, "inside"))
        assert db.gated_runs() == 0
        db.reload(gated)
        db.run()
        assert db.gated_runs() == 1
        _assert_equals_oracle(db.download(), oracle.mask(gated), (reason, "gated"))
        _assert_plan(db, gated, {}, (reason, "gated"))
        assert db.gated_runs() == 1
    finally:
        _restore(masker)
        if db is not None:
            db.free()


# ---- offsets past 2^31 ----------------------------------------------------------------------------
WIDE_FAMILIES = {"fused": ({}, "multi_segment_fused"), "record": ({"FUSED_FLAT": 0}, "two_pass"),
                 "long": ({"PREP_LONG": 1}, "long_read")}


@pytest.fixture(scope="module")
def wide_batch(oracle):
    arr, info = pb.wide_offset_batch()
    want = oracle.mask(arr)
    for a in arr.values():
        a.setflags(write=False)
    return arr, info, want


@pytest.fixture(scope="module", params=list(WIDE_FAMILIES))
def wide_run(request, masker, wide_batch):
    """One upload of the 2 GB batch per family: (family, shape, info, first result, second run's bytes equal)."""
    arr, _, _ = wide_batch
    params, _ = WIDE_FAMILIES[request.param]
    db = None
    try:
        _set(masker, **params)
        db = masker.upload(arr)
        shape, info = db.shape(), db.info()
        db.run()
        got = db.download()
        db.run()
        again = db.download()
        same = all(np.array_equal(got[k], again[k]) for k in range(4))
        del again
    finally:
        _restore(masker)
        if db is not None:
            db.free()
    return request.param, shape, info, got, same


def test_wide_offsets_plan(wide_run, wide_batch):
    """seq_bytes = 2^31 + 4096: the scan's 64-bit instantiation; the plan equals the restatement."""
    family, shape, info, got, same = wide_run
    arr = wide_batch[0]
    assert len(arr["seq_nt16"]) == pb.WIDE_SEQ_BYTES >= (1 << 31) - 1
    ref = pb.plan_reference(arr, params=WIDE_FAMILIES[family][0])
    assert ref["prep_mode"] == WIDE_FAMILIES[family][1]
    assert shape == {k: ref[k] for k in ("id_ops", "max_len", "max_seg", "prep_mode")}, family
    assert info["groups"] == ref["planned_groups"] and info["written_reads"] == ref["written_reads"] == 36
    assert same, "a second run gave other bytes"


def test_wide_offsets_touched_reads(wide_run, wide_batch):
    """Every read (at byte 0, below, across and above byte 2^31, up to the last byte) equals the
    oracle's, and the counts do."""
    family, _, _, got, _ = wide_run
    arr, info, want = wide_batch
    nb = (arr["read_len"].astype(np.int64) + 1) // 2
    bad = [(r, info["regions"][r]) for r in range(len(nb))
           if not np.array_equal(got[0][arr["seq_off"][r]:arr["seq_off"][r] + nb[r]],
                                 want[0][arr["seq_off"][r]:arr["seq_off"][r] + nb[r]])]
    assert bad == [], (family, bad)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), family
    assert got[3][0] == want[3][0] and got[3][1] == want[3][1] == len(info["masked"]) and got[3][3] == want[3][3]


def test_wide_offsets_full_buffer(wide_run, wide_batch):
    family, _, _, got, _ = wide_run
    assert np.array_equal(got[0], wide_batch[2][0]), family
