"""The hand-built FASTQ record sets (tests/fastq_sets.py) on the CPU: the plain per-record formatter,
the restatement of the reference's record code (oracle/fastq_oracle.py) and the host formatter agree
byte for byte on every set, and every set reaches the phases, buffer slots and tile boundaries it is
built for. The coverage conditions are computed from the record arrays and offsets, never from
formatter output. tests/test_gpu_fastq_sets.py runs the same sets through every HIP instance."""
import functools

import numpy as np
import pytest

import fastq_oracle
import fastq_sets as S
from genomeanonymizer_amd import native


def _oracle(recs):
    try:
        return fastq_oracle.format_records(recs)
    except fastq_oracle.BadRecord as e:
        return e.index


def _host(recs):
    try:
        return native.host_format_fastq(recs)
    except native.FastqBadRecord as e:
        return e.index


def _three_agree(recs):
    ref = S.ref_format(recs)
    assert _host(recs) == ref
    assert _oracle(recs) == ref
    return ref


@functools.lru_cache(maxsize=None)
def _lattice(spaced):
    return S.phase_lattice(spaced=spaced)


@functools.lru_cache(maxsize=None)
def _ladder(style):
    return S.boundary_ladder(style)


# ---- the three CPU formatters agree ---------------------------------------------------------

@pytest.mark.parametrize("spaced", [False, True], ids=["plain", "spaced"])
def test_lattice_formatters_agree(spaced):
    ref = _three_agree(_lattice(spaced))
    assert isinstance(ref, bytes) and len(ref) == native.fastq_bytes(_lattice(spaced))


@pytest.mark.parametrize("style", ["sparse", "dense"])
def test_ladder_formatters_agree(style):
    assert isinstance(_three_agree(_ladder(style)), bytes)


def test_aligned_tiles_formatters_agree():
    for name, recs in S.aligned_tiles().items():
        ref = _three_agree(recs)
        assert isinstance(ref, bytes), name
        if name.startswith("total"):
            assert len(ref) == int(name[5:])


def test_long_fields_formatters_agree():
    assert isinstance(_three_agree(S.long_fields()), bytes)


def test_wide_qualities_host_formatter():
    """Every quality byte value, the high ones next to low ones (add33's carries); not for the
    oracle, which prints bytes above 93 as two-byte code points."""
    r = S.wide_qualities()
    used = np.concatenate([r["qual_bufs"][s][o:o + q] for s, o, q in zip(r["qual_sel"], r["qual_off"], r["qual_len"])])
    assert len(np.unique(used)) == 256
    assert len(set(zip((r["qual_off"] % 4).tolist(), r["qual_rev"].tolist(), r["qual_sel"].tolist()))) == 16
    ref = S.ref_format(r)
    assert isinstance(ref, bytes) and native.host_format_fastq(r) == ref


def test_q7_probes_report_the_same_index():
    probes = S.q7_probes()
    assert len(probes) == 2 * 40 + 1 + 2
    for recs, want in probes:
        ref = _three_agree(recs)
        if want is None:
            assert isinstance(ref, bytes)
        else:
            assert ref == want


def test_many_records_host_formatter():
    recs = S.many_records()
    n = len(recs["seq_len"])
    assert n == S.MANY_EMPTY + 50 and (S.MANY_EMPTY + 2047) // 2048 > 1024     # a second k_fq_bscan round
    exp = S.many_expected()
    assert len(exp) == native.fastq_bytes(recs)
    assert native.host_format_fastq(recs) == exp


# ---- what the sets reach ----------------------------------------------------------------------

def _field_starts(recs):
    st = S.record_starts(recs)[:-1]
    NL, L = recs["name_len"].astype(np.int64), recs["seq_len"].astype(np.int64)
    return st + 1, st + NL + 4, st + NL + 7 + L     # name, bases, qualities


@pytest.mark.parametrize("spaced", [False, True], ids=["plain", "spaced"])
def test_lattice_coverage(spaced):
    r = _lattice(spaced)
    n = len(r["seq_len"])
    assert n >= 2 * 2 * 16 * len(S.LATTICE_LENGTHS)
    name0, seq0, qual0 = _field_starts(r)
    seq_lo, qual_lo, name_lo = S.buffer_lows(r)
    # the lowest used byte of every buffer: non-zero, no multiple of 4 (the upload slices there)
    assert len(r["seq_bufs"]) == 4 and len(r["qual_bufs"]) == 4
    for lo in seq_lo + qual_lo + [name_lo]:
        assert lo is not None and lo % 4 != 0
    # zero-length fields with an offset below their buffer's lowest used byte
    assert ((r["seq_len"] == 0) & ((r["seq_nib_off"] >> 1) < np.array(seq_lo)[r["seq_sel"]])).any()
    assert ((r["qual_len"] == 0) & (r["qual_off"] < np.array(qual_lo)[r["qual_sel"]])).any()
    # all 4 x 4 buffer slots
    assert len(set(zip(r["seq_sel"].tolist(), r["qual_sel"].tolist()))) == 16
    # base fields of >= 17 bases: (field start in the output mod 16, first nibble mod 8, reverse), the
    # nibble phase both as the record arrays give it and as the device sees it in the sliced buffer
    m = r["seq_len"] >= 17
    dev_nib = r["seq_nib_off"] - 2 * np.array(seq_lo)[r["seq_sel"]]
    for nib in (r["seq_nib_off"], dev_nib):
        assert len(set(zip((seq0[m] % 16).tolist(), (nib[m] % 8).tolist(), r["reverse"][m].tolist()))) == 256
    assert len(set(zip((r["seq_nib_off"][m] % 16).tolist(), r["reverse"][m].tolist(), r["qual_rev"][m].tolist()))) == 64
    m = r["qual_len"] >= 17
    dev_q = r["qual_off"] - np.array(qual_lo)[r["qual_sel"]]
    for q in (r["qual_off"], dev_q):
        assert len(set(zip((qual0[m] % 16).tolist(), (q[m] % 4).tolist(), r["qual_rev"][m].tolist()))) == 128
    m = r["name_len"] >= 17
    for o in (r["name_off"], r["name_off"] - name_lo):
        assert len(set(zip((name0[m] % 16).tolist(), (o[m] % 4).tolist()))) == 64
    # Q != L on a fifth of the lattice, both zero-length cases among them; qualities 0..93; mates 1, 2
    ne = r["qual_len"] != r["seq_len"]
    assert ne.sum() >= 2 * 2 * 16 * len(S.LATTICE_LENGTHS) // 5
    assert ((r["qual_len"] == 0) & (r["seq_len"] > 0)).any() and ((r["seq_len"] == 0) & (r["qual_len"] > 0)).any()
    used = np.concatenate([r["qual_bufs"][s][o:o + q] for s, o, q in zip(r["qual_sel"], r["qual_off"], r["qual_len"])])
    assert used.min() == 0 and used.max() == 93
    assert set(r["mate"].tolist()) == {1, 2}
    # unmappable nibbles on both sides of every read
    for i in range(n):
        sb, a, L = r["seq_bufs"][r["seq_sel"][i]], int(r["seq_nib_off"][i]), int(r["seq_len"][i])
        if L == 0 and a == 0:
            continue
        for p in (a - 1, a + L):
            assert (sb[p >> 1] & 0xF if p & 1 else sb[p >> 1] >> 4) in (0, 3)
    # which kernel formats the tiles: k_fq_dense (plain) or the selected instance (spaced)
    _, ranged = S.tile_records(r)
    if spaced:
        assert ranged.max() <= S.STAGE
    else:
        assert (ranged[:-1] > S.STAGE).all()


@pytest.mark.parametrize("style", ["sparse", "dense"])
def test_ladder_coverage(style):
    r = _ladder(style)
    meta = r["meta"]
    st = S.record_starts(r)
    NL, L, Q = S.PROBE
    plen = 8 + NL + L + Q
    # the 8 constant bytes and each field's first and last byte, as offsets into the probe
    marks = {"@": 0, "/": NL + 1, "mate": NL + 2, "nl1": NL + 3, "nl2": NL + 4 + L, "+": NL + 5 + L, "nl3": NL + 6 + L,
             "nl4": plen - 1, "name0": 1, "name1": NL, "seq0": NL + 4, "seq1": NL + 3 + L, "qual0": NL + 7 + L,
             "qual1": NL + 6 + L + Q}
    assert len(set(marks.values())) == 14
    for i in meta["probe"]:
        assert (r["name_len"][i], r["seq_len"][i], r["qual_len"][i]) == S.PROBE
    assert sorted(set(meta["d"].tolist())) == list(range(plen + 1))
    last = {k: set() for k in range(4)}
    first = {k: set() for k in range(4)}
    for i, d, kind in zip(meta["probe"], meta["d"], meta["kind"]):
        assert (int(r["reverse"][i]) | int(r["qual_rev"][i]) << 1) == kind
        assert (S.TILE - st[i]) % S.TILE == d
        for name, o in marks.items():
            if (st[i] + o) % S.TILE == S.TILE - 1:
                last[kind].add(name)
            if (st[i] + o) % S.TILE == 0 and st[i] + o > 0:
                first[kind].add(name)
    for kind in range(4):
        assert last[kind] == set(marks) and first[kind] == set(marks)
    # every (d, kind) pair, and the probes' source phases
    assert len(set(zip(meta["d"].tolist(), meta["kind"].tolist()))) == 4 * (plen + 1)
    p = meta["probe"]
    assert set((r["seq_nib_off"][p] % 8).tolist()) == set(range(8))
    assert set((r["qual_off"][p] % 4).tolist()) == set(range(4)) and set((r["name_off"][p] % 4).tolist()) == set(range(4))
    # the tiles on either side of every boundary a probe is placed at
    held, ranged = S.tile_records(r)
    bt = np.unique(np.concatenate([(st[p] + S.TILE - 1) // S.TILE - 1, (st[p] + S.TILE - 1) // S.TILE]))
    bt = bt[(bt >= 0) & (bt < len(held))]
    assert len(bt) >= 4 * (plen + 1)
    if style == "sparse":
        assert held[bt].max() <= S.STAGE and ranged[bt].max() <= S.STAGE
    else:
        assert held[bt].min() >= S.STAGE + 2 and ranged[bt].min() >= S.STAGE + 2
        assert S.record_bytes(r).max() <= 120


def test_aligned_tiles_coverage():
    sets = S.aligned_tiles()
    r = sets["aligned"]
    assert (S.record_bytes(r) == 128).all()
    total = int(S.record_starts(r)[-1])
    assert total % S.TILE == 0 and (total // S.TILE) % 2 == 1
    held, ranged = S.tile_records(r)
    assert (held == 64).all()
    assert (ranged[:-1] == 65).all() and ranged[-1] == 64       # (no record follows the last tile)
    r = sets["shifted"]
    assert S.record_bytes(r)[0] == 129 and (S.record_bytes(r)[1:] == 128).all()
    held, ranged = S.tile_records(r)
    assert held[0] == 64 and (held[1:-1] == 65).all() and held[-1] == 1     # 64 whole records and a partial one
    assert ranged[0] == 64 and (ranged[1:-1] == 65).all() and ranged[-1] == 1
    assert [int(S.record_starts(sets[k])[-1]) for k in ("total8", "total15", "total16", "total17")] == [8, 15, 16, 17]


def test_long_fields_coverage():
    r = S.long_fields()
    L, Q, NL = r["seq_len"], r["qual_len"], r["name_len"]
    big = L > S.TILE
    assert {(int(a), int(b & 1)) for a, b in zip(r["reverse"][big], r["seq_nib_off"][big])} == {(0, 1), (1, 1)}
    assert set(r["qual_rev"][Q > S.TILE].tolist()) == {0, 1}
    assert (NL > S.TILE).any() and (Q != L).any()
