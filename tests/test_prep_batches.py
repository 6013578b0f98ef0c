"""The hand-built batches of tests/prep_batches.py hold what the device-prep tests
(tests/test_gpu_prep.py) rely on, and its plain restatement of the plan agrees with literal values,
with synth.batch's read end and with the C oracle's bytes — checked without a device, so that the GPU
tests cannot pass vacuously. The 32-bit models of the two counting CIGAR walks are compared with
the unbounded walk on every CIGAR of every batch: the walks as they were (``saturate=False``)
diverge exactly on the reads whose query-consuming lengths sum past 2^31."""
import numpy as np
import pytest

import prep_batches as pb


@pytest.fixture(scope="module")
def oracle():
    from pyoracle import OracleEngine
    return OracleEngine()


@pytest.fixture(scope="module")
def matrix():
    return pb.cigar_matrix_batch()


@pytest.fixture(scope="module")
def overflow():
    return pb.overflow_cigar_batch()


def _changed(arr, out):
    """(read, query position) of every base of a read that differs between the batch and ``out``."""
    from genomeanonymizer_amd.synth.batch import unpack_nibbles
    res = []
    for r in range(len(arr["read_len"])):
        L, o = int(arr["read_len"][r]), int(arr["seq_off"][r])
        n = (L + 1) // 2
        a, b = unpack_nibbles(arr["seq_nt16"][o:o + n], L), unpack_nibbles(out[o:o + n], L)
        res += [(r, int(q)) for q in np.nonzero(a != b)[0]]
    return sorted(res)


# (sub-batch, case) -> segments as (q, position - ref_start, n), read_end - ref_start, I/D ops: by hand
LITERALS = {
    ("one_segment", "M"): ([(0, 0, 20)], 20, 0),
    ("one_segment", "S_M_S"): ([(3, 0, 20)], 20, 0),
    ("one_segment", "H_M_H"): ([(0, 0, 20)], 20, 0),
    ("one_segment", "zero_length_ops"): ([(0, 0, 20)], 20, 2),
    ("one_segment", "no_cigar"): ([], 1, 0),
    ("one_segment", "no_cigar_no_bases"): ([], 1, 0),
    ("one_segment", "all_soft_clip"): ([], 1, 0),
    ("one_segment", "query_shorter_than_L"): ([(0, 0, 10)], 10, 0),
    ("one_segment", "clip_mid_op"): ([(0, 0, 12)], 20, 0),
    ("one_segment", "clip_at_border_then_M"): ([(0, 0, 10)], 20, 1),
    ("one_segment", "starts_at_L"): ([], 10, 0),
    ("one_segment", "lead_D16"): ([(0, 16, 20)], 36, 1),
    ("one_segment", "trail_D15"): ([(0, 0, 20)], 35, 1),
    ("one_segment", "clipped_tail_16"): ([(0, 0, 20)], 36, 0),
    ("one_segment", "run_16384_clipped_to_16383"): ([(0, 0, 16383)], 16384, 0),
    ("multi_segment", "two_segments"): ([(0, 0, 10), (12, 10, 10)], 20, 1),
    ("multi_segment", "every_op"): ([(2, 0, 8), (12, 8, 8), (20, 19, 8), (28, 32, 8), (36, 40, 6), (42, 46, 6)], 52, 2),
    ("multi_segment", "clip_at_third"): ([(0, 0, 5), (5, 6, 5)], 17, 2),
    ("long_runs", "run_16384"): ([(0, 0, 16383), (16383, 16383, 1)], 16384, 0),
    ("long_runs", "run_32767_clipped_16384"): ([(0, 0, 16383), (16383, 16383, 1)], 32767, 0),
    ("long_runs", "run_32767"): ([(0, 0, 16383), (16383, 16383, 16383), (32766, 32766, 1)], 32767, 0),
}


def test_literal_cases(matrix):
    seen = 0
    for key, (arr, info) in matrix.items():
        ref = pb.plan_reference(arr)
        for c in info["cases"]:
            want = LITERALS.get((key, c["name"]))
            if want is None:
                continue
            seen += 1
            for r in c["reads"]:
                got = ref["reads"][r]
                assert [(q, p - c["pos"], n) for q, p, n in got["segments"]] == want[0], (key, c["name"])
                assert got["read_end"] - c["pos"] == want[1] and got["id_ops"] == want[2], (key, c["name"])
    assert seen == len(LITERALS)


def test_matrix_shapes_and_modes(matrix):
    """Each sub-batch plans in one mode, for the reason its name gives."""
    want = {"one_segment": ("one_segment_fused", 1, 16383, 0), "multi_segment": ("multi_segment_fused", 8, 80, 0),
            "many_segments": ("two_pass", 48, 150, 0), "long_cigar": ("two_pass", 129, 387, 58),
            "long_runs": ("long_read", 3, 32775, 0)}
    for key, (arr, info) in matrix.items():
        ref = pb.plan_reference(arr)
        assert (ref["prep_mode"], ref["max_seg"], ref["max_len"], ref["long_cigars"]) == want[key], key
        assert ref["written_reads"] == len(arr["read_len"]) and ref["huge_scopes"] == 0
        assert ref["id_ops"] == sum(2 * c["id_ops"] for c in info["cases"])
    n_cig = set(int(x) for x in matrix["long_cigar"][0]["n_cig"]) | set(int(x) for x in matrix["many_segments"][0]["n_cig"])
    assert {48, 49, 64, 65, 128, 129} <= n_cig
    segs = {len(c["segments"]) for k in ("one_segment", "multi_segment", "many_segments") for c in matrix[k][1]["cases"]}
    assert {0, 1, 2, 8, 9} <= segs


def test_expected_mode_rules():
    f = pb.expected_mode
    assert f(1, 150, 0) == "one_segment_fused" and f(0, 0, 0) == "one_segment_fused"
    assert f(8, 1000, 0) == "multi_segment_fused" and f(9, 1000, 0) == "two_pass" and f(2, 1001, 0) == "long_read"
    assert f(1, 100_000, 0) == "one_segment_fused" and f(1, 150, 1) == "one_segment" and f(2, 150, 1) == "two_pass"
    assert f(1, 150, 0, {"FUSED_FLAT": 0}) == "one_segment" and f(2, 150, 0, {"FUSED_FLAT": 0}) == "two_pass"
    assert f(1, 150, 0, {"PREP_LONG": 0}) == "two_pass" and f(1, 150, 0, {"PREP_LONG": 1}) == "long_read"


def test_read_end_equals_synth_ref_end(matrix, overflow):
    from genomeanonymizer_amd.synth.batch import _ref_end
    batches = [a for a, _ in matrix.values()] + [x[0] for x in overflow.values()] + [pb.block_border_batch(2049, 1025)[0]]
    for arr in batches:
        ref = pb.plan_reference(arr)
        for r in range(len(arr["read_len"])):
            assert ref["reads"][r]["read_end"] == _ref_end(int(arr["ref_start"][r]), pb._cig_of(arr, r))


def test_oracle_masks_exactly_the_planted_alts(matrix, oracle):
    """An alt sits on the first and last base of every segment the restatement cuts, in a tumor and
    a normal read; the bases outside the segments differ from the reference too. The oracle, which
    walks the CIGARs on its own, masks exactly the alts: the segments are where it aligns the bases."""
    for key, (arr, info) in matrix.items():
        out, calls, bases, tot = oracle.mask(arr)
        assert _changed(arr, out) == info["masked"], key
        assert bases.sum() == len(info["masked"]) == tot[1]
        for c in info["cases"]:
            assert bases[c["scope"]] == 2 * len(c["alts"]) and (calls[c["scope"]] > 0) == bool(c["alts"]), (key, c["name"])
            assert arr["scope_span_len"][c["scope"]] == c["read_end"] - c["pos"]


def test_overflow_twin(overflow, oracle):
    """The twin is the overflow batch with each CIGAR cut where q >= L: same sizes, ends, I/D ops,
    segments and bases; the oracle (given only the twin) masks what the info dict promises; and the
    query lengths of the overflow batch's reads do pass 2^31."""
    for key, (arr, twin, info) in overflow.items():
        a, t = pb.plan_reference(arr), pb.plan_reference(twin)
        for k in ("id_ops", "max_len", "max_seg", "written_reads", "groups", "prep_mode", "long_cigars"):
            assert a[k] == t[k], (key, k)
        assert a["reads"] == t["reads"]
        for k in arr:
            assert np.array_equal(arr[k], twin[k]) == (k != "cigar"), k
        for r in range(len(arr["read_len"])):
            q = sum(w >> 4 for w in pb._cig_of(arr, r) if (w & 15) in (0, 1, 4, 7, 8))
            assert q >= 1 << 31 and sum(w >> 4 for w in pb._cig_of(twin, r) if (w & 15) in (0, 1, 4, 7, 8)) < 1 << 29
        out, calls, bases, tot = oracle.mask(twin)
        assert _changed(twin, out) == info["masked"] and len(info["masked"]) > 0
    assert overflow["thread"][0]["n_cig"].max() <= 48 < overflow["wave"][0]["n_cig"].min()
    assert pb.plan_reference(overflow["thread"][0])["prep_mode"] == "multi_segment_fused"


def _walks(arr):
    for r in range(len(arr["read_len"])):
        cig, L = pb._cig_of(arr, r), int(arr["read_len"][r])
        segs, rl, nid, _ = pb.walk_unbounded(cig, L, 0)
        yield r, cig, L, segs, rl, nid


def test_int32_walk_models(matrix, overflow):
    """Both counting walks, modelled with 32-bit wrap, count what the unbounded walk counts on every
    CIGAR here; the walks as they were do on every CIGAR except the overflow batch's, where they
    count segments that walk_segments never writes (and describe a first segment at a negative
    query offset)."""
    plain = [a for a, _ in matrix.values()] + [pb.block_border_batch(1025, 1024)[0], pb.eight_segment_block_batch()[0]]
    over = [x[0] for x in overflow.values()]
    diverged = []
    for arr in plain + over:
        for r, cig, L, segs, rl, nid in _walks(arr):
            first = (segs[0][0], segs[0][1], segs[0][2]) if segs else None
            assert pb.scan_walk_i32(cig, L) == (len(segs), nid, rl, first)
            assert pb.wave_walk_i32(cig, L) == (len(segs), nid, rl)
            old = (pb.scan_walk_i32(cig, L, saturate=False), pb.wave_walk_i32(cig, L, saturate=False))
            if old != ((len(segs), nid, rl, first), (len(segs), nid, rl)):
                assert any(arr is o for o in over), "only sums past 2^31 diverge"
                diverged.append((r, old[0][0] - len(segs), old[1][0] - len(segs)))
    n_over = sum(len(a["read_len"]) for a in over)
    assert len(diverged) == n_over, diverged
    # e.g. nine S ops of 2^28 - 1 after an M: the wrapped offset is negative, the last M counts again
    cig = pb.words([("M", 20)] + [("S", (1 << 28) - 1)] * 9 + [("M", 7)])
    assert pb.scan_walk_i32(cig, 20, saturate=False)[0] == 2 and pb.scan_walk_i32(cig, 20)[0] == 1
    # no segment before the wrap: the old walk described one at a negative query offset
    cig = pb.words([("S", 20)] + [("S", (1 << 28) - 1)] * 8 + [("M", 9)])
    assert pb.scan_walk_i32(cig, 20, saturate=False)[3][0] < 0 and pb.scan_walk_i32(cig, 20)[3] is None


def test_invalid_batches_and_their_neighbours(oracle):
    """Every invalid batch is its valid neighbour with one element changed, names one error, and
    the neighbour passes the restated checks and the oracle. All 14 kinds are there."""
    kinds, names = set(), set()
    for name, bad, err, good in pb.invalid_batches():
        assert name not in names
        names.add(name)
        assert pb.differing_elements(bad, good) == 1, name
        assert pb.first_error(good) is None, name
        assert pb.first_error(bad) == err, name
        kinds.add(err[0])
        if len(good["seq_nt16"]) < 1 << 20:
            out, calls, bases, tot = oracle.mask(good)
            assert bases.sum() > 0 and tot[3] == (good["write_scope"] >= 0).sum(), name
    assert kinds == set(pb.ERR_TEXT) and len(names) >= 70
    assert pb.error_text(("write_scope", 1023, -2)) == "read 1023: write_scope -2 out of range"
    assert pb.error_text(("op", 7, 15)) == "read 7: bad cigar op 15"
    for slot in (1023, 1024):
        for n in ("seq_end_even_L", "op_9_at_64_of_130", "keep_code_16", "listed_twice"):
            assert f"{n}@{slot}" in names


def test_block_border_batches():
    for n_reads, n_scopes in [(r, s) for r in (1, 255, 256, 257, 1023, 1024, 1025, 2049) for s in (1, 1023, 1024, 1025)]:
        arr, info = pb.block_border_batch(n_reads, n_scopes)
        sp = info["specials"]
        want = sorted({k + s for k in range(0, n_reads, 1024) for s in (0, 255, 256, 767, 1023) if k + s < n_reads}
                      | {n_reads - 1})
        assert sp == want and len(arr["read_len"]) == n_reads and len(arr["scope_span_len"]) == n_scopes
        ref = pb.plan_reference(arr)
        m = len(sp)
        assert ref["invalid"] is None
        assert ref["written_reads"] == m and ref["id_ops"] == m * (m + 1) // 2
        assert ref["max_len"] == 40 + 3 * m
        assert ref["max_seg"] == min(8, 1 + m)          # (special j has 2 + j % 7 segments)
        others = np.setdiff1d(np.arange(n_reads), sp)
        assert (arr["n_cig"][others] == 1).all() and (arr["read_len"][others] == 12).all()
        assert (arr["write_scope"][others] == -1).all() and not np.isin(others, arr["incid_read"]).any()
        # every special's I/D count and length is its own: a slot visited twice, or one missed for
        # another, changes a sum or a maximum
        assert sorted(int(arr["read_len"][r]) for r in sp) == [40 + 3 * (j + 1) for j in range(m)]
        assert [ref["reads"][r]["id_ops"] for r in sp] == list(range(1, m + 1))


def test_eight_segment_block_and_stripe_batches(oracle):
    arr, info = pb.eight_segment_block_batch()
    ref = pb.plan_reference(arr)
    assert len(arr["read_len"]) == 1030 and all(len(x["segments"]) == 8 for x in ref["reads"])
    # k_prep_scan packs, per thread and summed over the block, the multi-segment reads in bits 16-31
    # and their extras records (a header + the further segments = the segment count) in bits 0-15 of
    # one counter, takes the block's allocation as (sum & 0xFFFF), and keeps (slot in block << 16 |
    # first record) per list entry: reads, records and slots of a block must each stay below 2^16
    nseg = np.array([len(x["segments"]) for x in ref["reads"]])
    multi = (nseg > 1) & (nseg <= pb.FUSED_MAX_SEG)
    blocks = np.arange(0, len(nseg), pb.SCAN_BLOCK)
    reads_per_block = np.add.reduceat(multi.astype(np.int64), blocks)
    records_per_block = np.add.reduceat(np.where(multi, nseg, 0), blocks)
    assert reads_per_block.max() == pb.SCAN_BLOCK and records_per_block.max() == 8 * pb.SCAN_BLOCK
    assert reads_per_block.max() < 1 << 16 and records_per_block.max() < 1 << 16 and pb.SCAN_BLOCK - 1 < 1 << 16
    out = oracle.mask(arr)
    assert _changed(arr, out[0]) == info["masked"] and len(info["masked"]) == 1030 * 16
    arr, info = pb.stripe_batch()
    ref = pb.plan_reference(arr)
    assert len(arr["read_len"]) == 66_000 and ref["prep_mode"] == "multi_segment_fused" and ref["max_seg"] == 2
    multi = np.array([len(x["segments"]) == 2 for x in ref["reads"]])
    per_block = np.add.reduceat(multi, np.arange(0, 66_000, 1024))
    assert len(per_block) == 65 and (per_block == 10).all() and multi.reshape(-1)[:10].all()
    # records per stripe (2 per two-segment read; block b: stripe b mod 64), the capacity per stripe
    stripe = np.zeros(64, int)
    for b, n in enumerate(per_block):
        stripe[b % 64] += 2 * n
    cap = info["xrec_init"] // 64
    assert (stripe > cap).sum() == 1 and stripe[0] == 40 and cap == 30
    assert _changed(arr, oracle.mask(arr)[0]) == info["masked"]


def test_group_table_batch():
    arr, info = pb.group_table_batch()
    counts = info["counts"]
    assert counts[:2] == [0, 0] and counts[-2:] == [0, 0] and 0 in counts[3:-3] and max(counts) == 2000
    run = best = 0
    for c in counts:
        run = run + 1 if c == 0 else 0
        best = max(best, run)
    assert best > 256 and len(counts) == 1013 and sum(counts) == 2022
    # by hand: the last scope's cost prefix is 2022 incidences + weight * 1012 scopes
    assert pb.plan_reference(arr, 704)["groups"] == (2022 + 3 * 1012) // 704 + 1 == 8
    assert pb.plan_reference(arr, 16)["groups"] == (2022 + 1 * 1012) // 16 + 1 == 190
    # (weight = ceil(target / 255), the most scopes of a group less one: 2 at 256, where target / 256 gives 1)
    assert pb.plan_reference(arr, 256)["groups"] == (2022 + 2 * 1012) // 256 + 1 == 16
    # the scope with 2,000 incidences skips buckets (empty groups): its own bucket 0, the next scope's 2
    off = arr["scope_incid_off"]
    assert (off[3] + 3 * 3) // 704 == 0 and (off[4] + 3 * 4) // 704 == 2
    one = pb.group_table_batch(single=True)[0]
    assert len(one["scope_span_len"]) == 1 and pb.plan_reference(one, 16)["groups"] == 1
    tail = pb.plan_reference(pb.group_table_batch(tail=40)[0], 16)
    # (one more scope: 1,014; the bound counts the last scope's 40 incidences too)
    assert tail["groups"] == (2022 + 1013) // 16 + 1 == 190 and tail["group_bound"] == (2062 + 1013) // 16 + 1 == 193
    assert tail["planned_groups"] == tail["group_bound"]
    assert pb.plan_reference(pb.group_table_batch(tail=40)[0], 16, {"PREP_LONG": 0, "FUSED_FLAT": 0})["planned_groups"] == tail["groups"]


def test_wide_offset_batch(oracle):
    """The 2 GB batch: reads at byte 0, below, across and above byte 2^31 and on the last byte, one- and
    three-segment, both datasets; the same reads packed into a small buffer give the oracle the
    masked bases the info dict promises (the GPU test gives the oracle the big buffer)."""
    arr, info = pb.wide_offset_batch()
    small, sinfo = pb.wide_offset_batch(compact=True)
    assert len(arr["seq_nt16"]) == (1 << 31) + 4096 and info["masked"] == sinfo["masked"]
    for k in arr:
        assert np.array_equal(arr[k], small[k]) == (k not in ("seq_nt16", "seq_off")), k
    nb = (arr["read_len"].astype(np.int64) + 1) // 2
    off, end = arr["seq_off"], arr["seq_off"] + nb
    assert off.min() == 0 and end.max() == len(arr["seq_nt16"])
    r = info["straddler"]
    assert len(r) == 1 and arr["write_scope"][r[0]] >= 0
    segs = pb.plan_reference(arr)["reads"][r[0]]["segments"]
    cross = (1 << 32) - 2 * int(off[r[0]])                # the query position whose nibble index is 2^32
    assert len(segs) == 3 and segs[1][0] < cross < segs[1][0] + segs[1][2]
    assert ((off >= 1 << 31) & (arr["write_scope"] >= 0)).sum() >= 16 and (off == 1 << 31).sum() == 0
    written = arr["write_scope"] >= 0
    assert written.sum() == 36 and set(arr["dataset"][written]) == {0, 1} and (~written).sum() == 6
    ref = pb.plan_reference(arr)
    assert ref["prep_mode"] == "multi_segment_fused" and ref["max_seg"] == 3 and ref["max_len"] == 200
    for r0 in range(len(nb)):                             # the same bytes at both places
        assert np.array_equal(arr["seq_nt16"][off[r0]:end[r0]], small["seq_nt16"][small["seq_off"][r0]:small["seq_off"][r0] + nb[r0]])
    out = oracle.mask(small)
    assert _changed(small, out[0]) == info["masked"] and len(info["masked"]) == out[3][1] == 144
