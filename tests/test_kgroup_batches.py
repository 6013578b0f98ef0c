"""The deterministic batches of tests/kgroup_batches.py hold what the k_group matrix
(tests/test_gpu_kgroup.py) relies on — checked against the CPU oracle, without a device, so that the
GPU tests cannot pass vacuously."""
import numpy as np
import pytest

from kgroup_batches import (LENGTH_CLASSES, alt_offsets, chunk_edge_batch, count_observations, threshold_batch)


@pytest.fixture(scope="module")
def oracle():
    from pyoracle import OracleEngine
    return OracleEngine()


def _codes(arr):
    from genomeanonymizer_amd.synth.batch import unpack_nibbles
    return unpack_nibbles(arr["seq_nt16"], 2 * len(arr["seq_nt16"])), unpack_nibbles(arr["ref_nt16"], 2 * len(arr["ref_nt16"]))


def _ops(arr):
    return arr["cigar"] & 15


@pytest.fixture(scope="module", params=[(False, False), (False, True), (True, False), (True, True)],
                ids=["one_segment", "one_segment_long_end", "multi_segment", "multi_segment_long_end"])
def edge(request, oracle):
    multi, long_end = request.param
    arr, info = chunk_edge_batch(multi, end_on_long=long_end)
    return multi, long_end, arr, info, oracle.mask(arr)


def test_chunk_edge_batch_shape(edge):
    multi, long_end, arr, info, _ = edge
    ops = _ops(arr)
    assert 500 < len(arr["read_len"]) <= 4000
    assert set(np.unique(ops)) <= ({0, 1, 2, 3, 4} if multi else {0, 4})
    if multi:
        assert {1, 2, 3} <= set(np.unique(ops)), "I, D and N ops between the segments"
        assert (np.bincount(info["segments"]["read"]) == 3)[:-2].all()
        assert arr["read_len"].max() <= 1000 and arr["n_cig"].max() <= 9   # short reads, short CIGARs: the fused mode
    else:
        assert (np.bincount(info["segments"]["read"]) == 1).all()
    assert len(arr["scope_span_len"]) == 6 and (np.diff(arr["scope_incid_off"]) > 0).all()
    # both datasets in every scope; the last read of the buffer
    for s in range(6):
        ids = arr["incid_read"][arr["scope_incid_off"][s]:arr["scope_incid_off"][s + 1]]
        assert set(arr["dataset"][ids]) == {0, 1}
    last = int(np.argmax(arr["seq_off"]))
    assert last == len(arr["read_len"]) - 1 and arr["read_len"][last] == (257 if long_end else 1)
    assert arr["seq_off"][last] + (arr["read_len"][last] + 1) // 2 == len(arr["seq_nt16"])
    assert arr["n_cig"][last] == 1 and arr["write_scope"][last] >= 0


def test_chunk_edge_batch_alignments_and_lengths(edge):
    """Every length class at every sequence alignment mod 8 and every reference alignment mod 16, in
    the all-ACGT scopes and in the N scopes alike."""
    multi, _, arr, info, _ = edge
    seg = info["segments"]
    sn = 2 * arr["seq_off"][seg["read"]] + seg["q0"]
    rn = arr["scope_ref_off"][seg["scope"]] + seg["pos"] - arr["scope_span_start"][seg["scope"]]
    assert set(seg["length"]) == set(LENGTH_CLASSES)
    for dirty in (0, 1):
        for c, length in enumerate(LENGTH_CLASSES):
            m = (seg["cls"] == c) & (seg["dirty_set"] == dirty)
            assert (seg["length"][m] == length).all()
            assert set(sn[m] % 8) == set(range(8)), (dirty, length)
            assert set(rn[m] % 16) == set(range(16)), (dirty, length)
    # some segments cross a 4096-base boundary of the reference's block bitmap
    assert ((rn >> 12) != ((rn + seg["length"] - 1) >> 12)).sum() >= 4


def test_chunk_edge_batch_reference_codes(edge):
    """The all-ACGT scopes hold no other code; in the N scopes non-ACGT codes sit in the 64-base block
    just before a segment that starts on a block edge, just after one that ends on an edge (those
    segments stay clean), and inside segments."""
    _, _, arr, info, _ = edge
    _, refc = _codes(arr)
    bad_base = ~np.isin(refc, [1, 2, 4, 8])
    for s in range(3):
        a = int(arr["scope_ref_off"][s])
        assert not bad_base[a - 64:a + int(arr["scope_span_len"][s]) + 64].any()
    n_blk = len(refc) // 64
    bad_blk = bad_base[:n_blk * 64].reshape(n_blk, 64).any(axis=1)
    seg = info["segments"][info["segments"]["dirty_set"] == 1]
    rn = arr["scope_ref_off"][seg["scope"]] + seg["pos"] - arr["scope_span_start"][seg["scope"]]
    k0, k1 = rn >> 6, (rn + seg["length"] - 1) >> 6
    clean = np.array([not bad_blk[a:b + 1].any() for a, b in zip(k0, k1)])
    assert (clean & (rn % 64 == 0) & bad_base[rn - 1]).sum() >= 4, "N in the block before a clean segment"
    end = rn + seg["length"]
    assert (clean & (end % 64 == 0) & bad_base[end]).sum() >= 4, "N in the block after a clean segment"
    inside = np.array([bad_base[a:a + n].any() for a, n in zip(rn, seg["length"])])
    assert inside.sum() >= 50 and clean.sum() >= 50
    assert set(np.unique(refc[bad_base])) - {15}, "IUPAC codes too"


def test_chunk_edge_batch_oracle_masks_the_alts_only(edge):
    """The oracle changes exactly the planted both-dataset alts of written reads: the first and last
    base of segments of every length class among them, and none of the bases that must not be
    observed (clips, inserted bases, read-N, alts over N / IUPAC reference bases, single-dataset alts)."""
    _, _, arr, info, (o_out, o_calls, o_bases, o_tot) = edge
    assert (o_calls > 0).all() and (o_bases > 0).all()
    before, _ = _codes(arr)
    from genomeanonymizer_amd.synth.batch import unpack_nibbles
    after = unpack_nibbles(o_out, 2 * len(o_out))
    changed = np.nonzero(before != after)[0]
    nib = lambda rq: 2 * arr["seq_off"][rq[:, 0]] + rq[:, 1]
    alts, must_not = nib(info["alts"]), nib(info["must_not"])
    assert len(must_not) > 1000 and not np.isin(must_not, changed).any()
    assert np.array_equal(np.sort(alts), changed)
    assert o_tot[1] == len(changed) == o_bases.sum()
    seg = info["segments"]
    first = 2 * arr["seq_off"][seg["read"]] + seg["q0"]
    both = np.isin(first, changed) & np.isin(first + seg["length"] - 1, changed)
    for c in range(len(LENGTH_CLASSES)):
        for dirty in (0, 1):
            assert both[(seg["cls"] == c) & (seg["dirty_set"] == dirty)].sum() >= 8, (c, dirty)
    # the kinds of must-not bases are all there
    ops = _ops(arr)
    assert (ops == 4).sum() > 500                                   # soft clips
    assert (before[must_not] == 15).sum() >= 50                     # read-N at an alt site
    assert alt_offsets(257)[:4] == [0, 15, 16, 31] and alt_offsets(1) == [0]


@pytest.mark.parametrize("n_reads,n_obs", [(150, 255), (150, 256), (150, 257), (150, 512), (150, 513), (150, 1024),
                                           (150, 1025), (150, 1112), (150, 1113), (20, 1025), (2, 4)])
def test_threshold_batch_counts(oracle, n_reads, n_obs):
    arr, made = threshold_batch(n_obs, n_reads)
    assert made == n_obs == count_observations(arr)
    assert len(arr["read_len"]) == n_reads and (arr["read_len"] == 150).all()
    assert (arr["n_cig"] == 1).all() and (arr["cigar"] == (150 << 4)).all()
    o_out, o_calls, o_bases, _ = oracle.mask(arr)
    n_alt = min(n_obs // 2, 5 * n_reads)               # (a site's only carrier is no call)
    assert 0 < o_calls[0] <= 5 and o_bases[0] == n_alt - (n_alt % n_reads == 1)
    assert not np.array_equal(o_out, arr["seq_nt16"])


def test_threshold_batch_rejects_what_does_not_fit():
    with pytest.raises(ValueError):
        threshold_batch(20 * 150, 20)
    with pytest.raises(ValueError):
        threshold_batch(1, 10)
