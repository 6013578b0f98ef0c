"""The hand-built indel batches of tests/indel_batches.py, pinned without a device: each batch's
expected records equal the CPU restatement's (oracle/indel_oracle.py), and each batch really has the
shape it is meant to have — the op counts and observation counts at the thresholds, the hash
collision, the runs across k_indel_runs' row and chunk, the cap on the in-place sort — read back
from the arrays with a replica of the decisions ganon_indel_upload makes (``plan_of``).
tests/test_gpu_indels.py runs the same batches on the device.
"""
import numpy as np
import pytest

import indel_batches as ib
from indel_batches import GSORT, HASHED, THREAD_WALK, TSORT

CASES = ib.all_cases()
SILENT = {"nothing_tumor_only", "nothing_single"}


def _bits_for(v: int) -> int:
    return max(1, int(v).bit_length())


def read_ops(a: dict, r: int):
    """(op, length) of read r's CIGAR."""
    c = a["cigar"][int(a["cig_off"][r]):int(a["cig_off"][r]) + int(a["n_cig"][r])]
    return [(int(w) & 0xF, int(w) >> 4) for w in c]


def id_ops(a: dict, r: int):
    """(op index, pos, type) of read r's I/D ops."""
    out, p = [], int(a["ref_start"][r])
    for k, (op, n) in enumerate(read_ops(a, r)):
        if op in (1, 2):
            out.append((k, p, op))
        if op in (0, 2, 3, 7, 8):
            p += n
    return out


def plan_of(a: dict) -> dict:
    """What ganon_indel_upload decides from the batch's shape under default settings."""
    off = a.get("indel_incid_off", a["scope_incid_off"])
    inc = a.get("indel_incid_read", a["incid_read"])
    n_reads = len(a["ref_start"])
    nid = [len(id_ops(a, r)) for r in range(n_reads)]
    max_nc_id = max([int(a["n_cig"][r]) for r in range(n_reads) if nid[r]], default=0)
    seen, n_rcand, per_scope = set(), 0, []
    for s in range(len(off) - 1):
        reads = [int(r) for r in inc[int(off[s]):int(off[s + 1])]]
        per_scope.append(sum(nid[r] for r in reads))
        for r in reads:
            if nid[r] and r not in seen:
                seen.add(r)
                n_rcand += nid[r]
    thread = max_nc_id <= ib.THREAD_WALK_OPS
    tsort = thread and max(per_scope) <= ib.TSORT_MAX
    k = 12
    while (1 << k) < 64 * max(n_rcand, 1):
        k += 1
    hashed = (1 << k) // 16 + 1 < (2 * len(a["ref_nt16"]) + 64) // 16 + 1
    pos_bits = _bits_for(int(a["scope_span_len"].max()))
    return {
        "route": (THREAD_WALK if thread else 0) | (TSORT if tsort else 0) | (GSORT if thread and not tsort else 0) |
                 ((HASHED | k << 8) if hashed else 0),
        "max_nc_id": max_nc_id, "per_scope": per_scope, "observations": sum(per_scope), "pos_bits": pos_bits,
        "key_bits": pos_bits + _bits_for(max(len(off) - 2, 1)),
    }


def filtered_layout(a: dict, e: ib.Expect):
    """Per scope, the relative positions of the filtered observations in the order the expansion
    writes them (incidence order, then op order) — dense map."""
    off = a.get("indel_incid_off", a["scope_incid_off"])
    inc = a.get("indel_incid_read", a["incid_read"])
    base = a["scope_ref_off"] - a["scope_span_start"]
    bits = {}
    for s in range(len(off) - 1):
        for r in inc[int(off[s]):int(off[s + 1])]:
            for _, p, _ in id_ops(a, int(r)):
                g = int(base[s]) + p
                bits[g] = bits.get(g, 0) | 1 << int(a["dataset"][r])
    out = []
    for s in range(len(off) - 1):
        out.append([p - int(a["scope_span_start"][s]) for r in inc[int(off[s]):int(off[s + 1])]
                    for _, p, _ in id_ops(a, int(r)) if bits[int(base[s]) + p] == 3])
    assert sum(map(len, out)) == e.emitted_dense
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_records_equal_the_oracle(name):
    import indel_oracle
    arr, e = CASES[name]
    assert sorted(indel_oracle.indel_records(arr)) == e.records
    assert (len(e.records) == 0) == (name in SILENT)
    assert len(set(e.records)) == len(e.records)


@pytest.mark.parametrize("name", sorted(CASES))
def test_expected_plan_follows_from_the_arrays(name):
    arr, e = CASES[name]
    plan = plan_of(arr)
    assert plan["route"] == e.route
    assert plan["observations"] == e.observations
    assert e.emitted <= e.observations and e.emitted_dense <= e.emitted
    assert (e.emitted == e.emitted_dense) or name == "hash_collision"
    # every read's bases are its CIGAR's M/I/S/=/X total
    for r in range(len(arr["n_cig"])):
        assert int(arr["read_len"][r]) == sum(n for op, n in read_ops(arr, r) if op in (0, 1, 4, 7, 8))
    assert len(arr["cigar"]) <= 10_000


def test_cigar_arith_uses_every_op():
    arr, e = CASES["cigar_arith"]
    assert {int(w) & 0xF for w in arr["cigar"]} == set(range(9))
    assert (0, 235, 1, 3, 0, 1, 18, 45) in e.records and int(arr["read_len"][18]) == 11
    # the double support: CALL at the first offset, SUPPORT at the last
    assert (0, 175, 1, 3, 0, 0, 13, 5) in e.records and (0, 175, 1, 3, 0, 1, 13, 6) in e.records
    assert {r[4] for r in e.records} == {0, 1}


def test_walk_threshold_pair_sits_on_the_threshold():
    (a32, e32), (a33, e33) = CASES["walk_32"], CASES["walk_33"]
    assert (plan_of(a32)["max_nc_id"], plan_of(a33)["max_nc_id"]) == (32, 33)
    assert int(a32["n_cig"].max()) == int(a33["n_cig"].max()) == 40        # the read with no I/D op
    assert e32.route & THREAD_WALK and not e33.route & THREAD_WALK
    # the records differ only by read 0's offsets
    assert [r for r in e32.records if r[6] != 0] == [r for r in e33.records if r[6] != 0]
    assert [r[:7] for r in e32.records] == [r[:7] for r in e33.records] and e32.records != e33.records


def test_block_edge_batch_shape():
    arr, e = CASES["block_edge"]
    assert not e.route & THREAD_WALK
    at = set()
    for r in range(len(arr["n_cig"])):
        ks = [k for k, _, _ in id_ops(arr, r)]
        at.update(ks)
        if ks:
            assert int(arr["n_cig"][r]) in (256, 257, 512, 513)
    assert at == {0, 63, 64, 255, 256, 257, 511, 512}
    blocks = [{k // ib.WALK_BLOCK for k, _, _ in id_ops(arr, r)} for r in range(len(arr["n_cig"]))]
    assert {0, 2} in blocks                                                # block 1 holds none
    assert any([k for k, _, _ in id_ops(arr, r)] == [511] and arr["n_cig"][r] == 512 for r in range(len(blocks)))
    assert len(e.records) == 3 * 22 and {r[4] for r in e.records} == {0, 1}


def test_tsort_threshold_pair_sits_on_the_threshold():
    (a, ea), (b, eb) = CASES["tsort_4096"], CASES["tsort_4097"]
    pa, pb = plan_of(a), plan_of(b)
    assert (pa["per_scope"], pb["per_scope"]) == ([4096], [4097])
    assert ea.route == THREAD_WALK | TSORT and eb.route == THREAD_WALK | GSORT
    assert ea.records == eb.records and len(ea.records) == 24 and ea.emitted == eb.emitted == 16
    assert (pa["pos_bits"], pb["key_bits"]) == (ea.extra["pos_bits"], eb.extra["pos_bits"] + eb.extra["scope_bits"])
    assert pa["pos_bits"] != pb["key_bits"]


def test_tsort_order_batch_shape():
    arr, e = CASES["tsort_order"]
    lay = filtered_layout(arr, e)
    sizes = [len(x) for x in lay]
    assert sizes == [240, 0, 320, 0, 400] and max(sizes) <= 512
    assert plan_of(arr)["per_scope"][1] > 0 and plan_of(arr)["per_scope"][3] > 0     # emptied by the filter
    for x in lay:
        assert all(x[i] >= x[i + 1] for i in range(len(x) // 2 - 1))        # descending, with ties
        assert len(set(x)) * 8 == len(x)
    # scopes 0, 2 and 4 have one segment parity, and each one's last sorted key is the next one's first
    assert max(lay[0]) == min(lay[2]) and max(lay[2]) == min(lay[4])


def test_hash_collision_batch_collides():
    arr, e = CASES["hash_collision"]
    k = e.route >> 8
    assert e.route & HASHED and k == 12 and len(arr["ref_nt16"]) * 2 == 16384
    assert ib.map_cell(214, 12) == ib.map_cell(2798, 12) == 1061
    (p1, p2), (p3, p4) = e.extra["pairs"]
    pos = sorted({p for r in range(len(arr["n_cig"])) for _, p, _ in id_ops(arr, r)})
    assert pos == sorted([p1, p2, p3, p4]) and min(np.diff(pos)) > 100
    assert ib.map_cell(p1, k) == ib.map_cell(p2, k) != ib.map_cell(p3, k) == ib.map_cell(p4, k)
    assert plan_of(arr)["observations"] <= 64
    assert (e.emitted_dense, e.emitted) == (2, 5) and [r[1] for r in e.records] == [p3] * 3


def test_two_contig_batch_shape():
    arr, e = CASES["two_contig"]
    base = (arr["scope_ref_off"] - arr["scope_span_start"]).tolist()
    assert base == [0, 300, 0, 0]
    assert sorted((r[0], r[5], r[6]) for r in e.records if r[1] == 205) == [(2, 0, 8), (2, 1, 8), (3, 0, 8), (3, 1, 9)]
    assert not [r for r in e.records if r[1] == 55]


def test_run_chunk_batch_straddles_row_and_chunk():
    arr, e = CASES["run_chunk"]
    lay = [sorted(x) for x in filtered_layout(arr, e)]
    assert [len(x) for x in lay] == [4201, 1, 5]
    flat = [(s, p) for s, x in enumerate(lay) for p in x]
    for edge in (ib.RUN_ROW, ib.RUN_CHUNK):
        assert flat[edge - 1] == flat[edge] and flat[edge - 2] != flat[edge - 1] != flat[edge + 1]
    assert flat[-1] == flat[-2] != flat[-3]                                  # the last run ends the array
    assert not e.route & THREAD_WALK and len(e.records) == 6306


def test_normal_cover_batch_shape():
    arr, e = CASES["normal_cover"]
    off = arr["scope_incid_off"]
    sizes = np.diff(off)[:15].tolist()
    assert sizes == [n for n in ib.COVER_SIZES for _ in ib.COVER_VARIANTS]
    covered = e.extra["covered"]
    assert {r[0] for r in e.records} == {s for s, c in covered.items() if c}
    for s in range(15):
        last = int(arr["incid_read"][int(off[s + 1]) - 1])
        assert arr["dataset"][last] == 1 and not id_ops(arr, last)
        pos = 40 * s + 20
        end = int(arr["ref_start"][last]) + sum(n for _, n in read_ops(arr, last))
        assert (int(arr["ref_start"][last]) <= pos < end) == covered[s]
        if s % 3 == 0:
            assert end == pos
        # no other normal read of the scope covers pos
        for r in arr["incid_read"][int(off[s]):int(off[s + 1]) - 1]:
            assert arr["dataset"][r] == 0 or int(arr["ref_start"][r]) + \
                sum(n for op, n in read_ops(arr, int(r)) if op != 1) <= pos
    assert not covered[15] and len(e.records) == 3 * 10


def test_rank_and_csr_batches():
    arr, e = CASES["rank"]
    assert sorted({(r[3], r[2], r[4]) for r in e.records}) == [(2, 2, 1), (3, 2, 3)]
    assert len({p for r in range(6) for _, p, _ in id_ops(arr, r)}) == 1
    arr, e = CASES["indel_csr"]
    assert 1 in arr["incid_read"] and 1 not in arr["indel_incid_read"] and id_ops(arr, 1)


def test_key_edge_pair_shape():
    for name, length, bits in (("key_edge_255", 255, 8), ("key_edge_256", 256, 9)):
        arr, e = CASES[name]
        n = len(arr["scope_span_len"])
        assert n == 4 and int(arr["scope_span_len"].argmax()) == n - 1 and int(arr["scope_span_len"][-1]) == length
        plan = plan_of(arr)
        assert plan["pos_bits"] == bits == e.extra["pos_bits"] and plan["key_bits"] == bits + 2
        # the last scope's TN insertion at the span's end: scope and position bits all ones (255)
        rel = [p - 1000 for r in arr["incid_read"][int(arr["scope_incid_off"][3]):] for _, p, _ in id_ops(arr, int(r))]
        assert sorted(rel)[-2:] == [length, length]
        if length == 255:
            assert (3 << bits | length) == (1 << plan["key_bits"]) - 1
        assert e.emitted < e.observations                                    # fillers in the capacity


def test_nothing_left_pair_is_silent():
    (_, a), (_, b) = CASES["nothing_tumor_only"], CASES["nothing_single"]
    assert (a.observations, a.emitted, a.records) == (4, 0, [])
    assert (b.observations, b.emitted, b.records) == (1, 0, [])
