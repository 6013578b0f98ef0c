"""The deterministic batches of tests/huge_batches.py hold what the huge-scope tests
(tests/test_gpu_huge.py) rely on — every listed property is read back from the arrays, and the CPU
oracle must agree with the builders' own bookkeeping — without a device, so that the GPU tests cannot
pass vacuously."""
import numpy as np
import pytest

from huge_batches import HUGE, TILE, crowd_batch, n_tiles, rare_stride_batch, threshold_pair, tile_edge_batch

N0, H1, N2, H3, H4 = range(5)
ACGT = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def oracle():
    from pyoracle import OracleEngine
    return OracleEngine()


@pytest.fixture(scope="module")
def edge():
    arr, info = tile_edge_batch()
    return arr, info, Pile(arr)


def _nibbles(packed):
    from genomeanonymizer_amd.synth.batch import unpack_nibbles
    return unpack_nibbles(packed, 2 * len(packed))


def _ops(arr, r):
    w = arr["cigar"][arr["cig_off"][r]:arr["cig_off"][r] + arr["n_cig"][r]]
    return [(int(x) & 15, int(x) >> 4) for x in w]


def _ref_end(arr, r):
    rl = sum(n for op, n in _ops(arr, r) if op in (0, 2, 3, 7, 8))
    return int(arr["ref_start"][r]) + (rl if rl > 0 else 1)


def _listed(arr, s):
    return arr["incid_read"][arr["scope_incid_off"][s]:arr["scope_incid_off"][s + 1]]


class Pile:
    """The batch decoded again from its arrays: per scope and position, the (dataset, code, read,
    query position) of every aligned base of a listed read that is not the reference's ACGT base."""

    def __init__(self, arr):
        self.arr = arr
        self.seq, self.ref = _nibbles(arr["seq_nt16"]), _nibbles(arr["ref_nt16"])
        self.at = {}
        self.covered = {}       # (scope, position) -> reads aligned there
        for s in range(len(arr["scope_span_len"])):
            for r in _listed(arr, s):
                p, q = int(arr["ref_start"][r]), 0
                for op, n in _ops(arr, r):
                    if op in (0, 7, 8):
                        for i in range(n):
                            c, rc = int(self.seq[2 * arr["seq_off"][r] + q + i]), self.refc(s, p + i)
                            if c != rc or rc not in ACGT:
                                self.at.setdefault((s, p + i), []).append((int(arr["dataset"][r]), c, int(r), q + i))
                    if op in (0, 2, 3, 7, 8):
                        p += n
                    if op in (0, 1, 4, 7, 8):
                        q += n

    def refc(self, s, p):
        a = self.arr
        return int(self.ref[a["scope_ref_off"][s] + p - a["scope_span_start"][s]])

    def codes(self, s, p, ds):
        return {c for d, c, _, _ in self.at.get((s, p), []) if d == ds}

    def calls(self, s, p):
        """Codes both datasets carry at p over an ACGT reference base (read N never counts)."""
        if self.refc(s, p) not in ACGT:
            return set()
        rc = self.refc(s, p)
        return {c for c in self.codes(s, p, 0) & self.codes(s, p, 1) if c != 15 and c != rc}

    def rare_tiles(self, s):
        a = self.arr
        return sorted({(p - int(a["scope_span_start"][s])) // TILE for (sc, p), obs in self.at.items() if sc == s
                       for _, c, _, _ in obs if c not in ACGT + (15,) and self.refc(s, p) in ACGT and c != self.refc(s, p)})

    def tile_calls(self, s, k):
        a0 = int(self.arr["scope_span_start"][s]) + k * TILE
        return sum(len(self.calls(sc, p)) for (sc, p) in self.at if sc == s and a0 <= p < a0 + TILE)


def _check_rules(arr):
    """Each read lies inside every span that lists it; each written read is listed exactly once by its
    write scope; the incidence lists are not sorted by position."""
    n_scopes = len(arr["scope_span_len"])
    for s in range(n_scopes):
        ids = _listed(arr, s)
        ss, se = int(arr["scope_span_start"][s]), int(arr["scope_span_start"][s]) + int(arr["scope_span_len"][s])
        ends = np.array([_ref_end(arr, r) for r in ids[:300]])
        assert (arr["ref_start"][ids] >= ss).all() and (ends <= se).all(), s
        if len(ids) > 3:
            assert (np.diff(arr["ref_start"][ids].astype(np.int64)) < 0).any(), f"scope {s} is listed in position order"
    ws = arr["write_scope"]
    scope_of_incid = np.repeat(np.arange(n_scopes), np.diff(arr["scope_incid_off"]))
    own = ws[arr["incid_read"]] == scope_of_incid
    assert np.array_equal(np.bincount(arr["incid_read"][own], minlength=len(ws)), (ws >= 0).astype(np.int64))


def _check_oracle(oracle, arr, info):
    """The oracle and the builder's bookkeeping agree: every must_mask nibble became the reference
    code, every other nibble is unchanged, the calls and the masked bases per scope."""
    out, calls, bases, tot = oracle.mask(arr)
    before, after = _nibbles(arr["seq_nt16"]), _nibbles(out)
    mm, mn = info["must_mask"], info["must_not"]
    nib = 2 * arr["seq_off"][mm[:, 0]] + mm[:, 1]
    assert len(np.unique(nib)) == len(nib)
    assert (before[nib] != mm[:, 2]).all() and np.array_equal(after[nib], mm[:, 2])
    assert np.array_equal(np.nonzero(before != after)[0], np.sort(nib))
    assert not np.isin(2 * arr["seq_off"][mn[:, 0]] + mn[:, 1], nib).any()
    assert np.array_equal(calls, info["calls_per_scope"])
    assert np.array_equal(bases, np.bincount(arr["write_scope"][mm[:, 0]], minlength=len(calls)))
    assert tot[0] == calls.sum() and tot[1] == len(mm)
    return out, calls, bases


# ---- tile_edge_batch ---------------------------------------------------------------------------

def test_tile_edge_scopes(edge):
    arr, info, pile = edge
    ss, sl, ro = arr["scope_span_start"], arr["scope_span_len"], arr["scope_ref_off"]
    assert len(sl) == 5 and 50 < len(arr["read_len"]) < 400
    assert [int(x) > HUGE for x in sl] == [False, True, False, True, True]
    assert sl[H1] == HUGE + 1 and ss[H1] % 2 == 0 and ro[H1] % 2 == 0
    assert sl[N2] == HUGE
    assert sl[H3] == HUGE + 2 * TILE + 4097 and ss[H3] % 2 == 1 and ro[H3] % 2 == 1
    assert info["tiles_per_scope"].tolist() == [0, 65, 0, 67, n_tiles(sl[H4])]
    assert (int(sl[H3]) - 66 * TILE) % 2 == 1, "H3's last tile has an odd span"
    # the window lies in H1's region and both point into the same bases
    assert ss[H1] < ss[N0] and ss[N0] + sl[N0] < ss[H1] + sl[H1] and sl[N0] < 3000
    assert ro[N0] - ss[N0] == ro[H1] - ss[H1]
    # no scope sees its reference as "nibble = position"
    assert all(ro[s] != ss[s] for s in range(5))
    # reads at both ends of every span (the spans are the reads' extent)
    for s in range(5):
        ids = _listed(arr, s)
        assert arr["ref_start"][ids].min() == ss[s] and max(_ref_end(arr, r) for r in ids) == ss[s] + sl[s], s
        assert set(arr["dataset"][ids]) == {0, 1}
    assert info["huge_written_reads"] == int(np.isin(arr["write_scope"], [H1, H3, H4]).sum()) > 50
    # the ordinary scopes hold no non-ACGTN read base: every rare tile belongs to the tile path
    for s in (N0, N2):
        for r in _listed(arr, s):
            o, n = 2 * int(arr["seq_off"][r]), int(arr["read_len"][r])
            assert np.isin(pile.seq[o:o + n], ACGT + (15,)).all()


def test_tile_edge_follows_the_batch_rules(edge):
    _check_rules(edge[0])


def test_tile_edge_shared_reads(edge):
    arr, info, pile = edge
    ws = arr["write_scope"]
    in0, in1 = set(_listed(arr, N0).tolist()), set(_listed(arr, H1).tolist())
    both = in0 & in1
    assert {int(ws[r]) for r in both} == {N0, H1}, "shared reads written by the window and by H1"
    for w in (N0, H1):      # ... with sites that are calls in both scopes
        assert any(pile.calls(N0, p) and pile.calls(H1, p) for (s, p), obs in pile.at.items() if s == w
                   for _, _, r, _ in obs if r in both and ws[r] == w)
    t = info["tally_only"]
    assert t in in1 and t not in in0 and ws[t] == -1
    u = info["unlisted"]
    assert u not in set(arr["incid_read"].tolist()) and ws[u] == -1
    assert not np.array_equal(pile.seq[2 * arr["seq_off"][u]:2 * arr["seq_off"][u] + 9],
                              pile.ref[arr["scope_ref_off"][H1] + arr["ref_start"][u] - arr["scope_span_start"][H1]:][:9])
    # the window's own site is no site of H1
    own = [p for (s, p) in pile.at if s == N0 and pile.calls(N0, p) and not pile.at.get((H1, p))]
    assert own


def test_tile_edge_borders(edge):
    arr, info, pile = edge
    for s in (H1, H3):
        ss, sl = int(arr["scope_span_start"][s]), int(arr["scope_span_len"][s])
        borders = info["borders"][s]
        last = ss + (n_tiles(sl) - 1) * TILE
        assert len(borders) >= 3 and ss + TILE in borders and last in borders
        ids = _listed(arr, s)
        starts = arr["ref_start"][ids].astype(np.int64)
        ends = np.array([_ref_end(arr, r) for r in ids])
        full = 0
        for b in borders:
            assert (b - ss) % TILE == 0
            sites = [p for p in (b - 2, b - 1, b, b + 1) if p < ss + sl]
            alts = []
            for p in sites:
                t, n = pile.codes(s, p, 0), pile.codes(s, p, 1)
                assert t & n and t | n <= set(ACGT), (s, b, p)
                alts.append(min(t & n))
            assert len(set(alts)) == len(sites) >= 3, "all alt codes differ"
            full += len(sites) == 4
            assert (ends == b).any() and (starts == b).any(), (s, b)
            for ds in (0, 1):
                assert ((starts < b - 2) & (ends > b) & (arr["dataset"][ids] == ds)).any(), (s, b, ds)
        assert full >= 3
    # (H1's last tile is one position wide: its border has no b + 1)
    assert info["borders"][H1][-1] + 1 == arr["scope_span_start"][H1] + arr["scope_span_len"][H1]


def test_tile_edge_classification(edge):
    arr, info, pile = edge
    alleles = set()
    for s in (H1, H3):
        c = info["classify"][s]
        off = (c - int(arr["scope_span_start"][s])) % TILE
        assert off % 4 == 0 and 4 <= off <= TILE - 16, "a whole table word, then the next, away from any border"
        T, N = (lambda k: pile.codes(s, c + k, 0)), (lambda k: pile.codes(s, c + k, 1))
        ref = [pile.refc(s, c + k) for k in range(10)]
        assert all(ref[k] in ACGT for k in (0, 1, 2, 3, 4, 7, 8, 9))
        assert len(T(0)) == 1 and T(0) == N(0)                              # shared alt
        assert len(T(1)) == 1 and not N(1)                                  # tumor only
        assert not T(2) and len(N(2)) == 1                                  # normal only
        assert len(T(3)) == len(N(3)) == 1 and T(3) != N(3)                 # different alts
        assert len(T(4)) == 2 and len(N(4)) == 1 and N(4) < T(4)            # T {X, Y}, N {Y}
        assert ref[5] == 15 and T(5) & N(5) & set(ACGT)                     # over a reference N
        assert ref[6] not in ACGT + (15, 0) and (T(6) & N(6)) - {ref[6]}    # over a reference IUPAC code
        assert T(7) == N(7) == {15}                                         # read N in both
        assert T(8) == N(8) == set(ACGT) - {ref[8]}                         # every alt of one base
        assert [len(pile.calls(s, c + k)) for k in range(10)] == [1, 0, 0, 0, 1, 0, 0, 0, 3, 1]
        for k in range(10):
            alleles |= pile.calls(s, c + k)
        x_reads = [(r, q) for d, code, r, q in pile.at[(s, c + 4)] if code in T(4) - N(4)]
        assert x_reads and all(list(rq) in info["must_not"].tolist() for rq in x_reads)
    assert alleles == set(ACGT), "each of the four 16-bit mask shifts"


def test_tile_edge_rare_tiles(edge):
    arr, info, pile = edge
    rare = {s: pile.rare_tiles(s) for s in range(5)}
    assert rare == {N0: [], N2: [], **info["rare_tile_ids"]}
    assert info["rare_tiles"] == sum(len(v) for v in rare.values()) == 5
    ss = int(arr["scope_span_start"][H1])
    in_tile = lambda k: [(p, obs) for (s, p), obs in pile.at.items() if s == H1 and (p - ss) // TILE == k]
    # '=' in both datasets over an ACGT base: a call
    assert any(pile.calls(H1, p) == {0} for p, _ in in_tile(10))
    # one IUPAC code in both datasets: a call
    assert any(pile.calls(H1, p) - set(ACGT) - {0} for p, _ in in_tile(11))
    # a tumor-only IUPAC code beside ACGT calls of the same tile
    lone = [p for p, _ in in_tile(14) if pile.codes(H1, p, 0) - set(ACGT) - {15} and not pile.codes(H1, p, 1)]
    assert lone and not pile.calls(H1, lone[0])
    assert sum(len(pile.calls(H1, p)) for p, _ in in_tile(14)) >= 2
    # an IUPAC base that equals an IUPAC reference code: nothing, and the tile is not rare
    same = [p for p, obs in in_tile(16) if {c for _, c, _, _ in obs} == {pile.refc(H1, p)}]
    assert same and pile.refc(H1, same[0]) not in ACGT + (15, 0) and 16 not in rare[H1]
    assert {d for d, _, _, _ in pile.at[(H1, same[0])]} == {0, 1}
    # a rare tile directly beside a tile that is not, calls in both
    assert 12 not in rare[H1] and pile.tile_calls(H1, 11) > 0 and pile.tile_calls(H1, 12) > 0
    # H3's rare tile is its odd last tile, with the call on the span's last position
    last = int(arr["scope_span_start"][H3]) + int(arr["scope_span_len"][H3]) - 1
    assert pile.calls(H3, last) - set(ACGT)
    # H4: one tile has tumor reads only
    s, k = info["tumor_only_tile"]
    a0 = int(arr["scope_span_start"][s]) + k * TILE
    ids = [r for r in _listed(arr, s) if arr["ref_start"][r] < a0 + TILE and _ref_end(arr, r) > a0]
    assert len(ids) >= 2 and set(arr["dataset"][ids]) == {0} and pile.tile_calls(s, k) == 0
    assert any(p for (sc, p), obs in pile.at.items() if sc == s and a0 <= p < a0 + TILE and len(obs) >= 2)


def test_tile_edge_keeps(edge):
    arr, info, pile = edge
    kp, kc = arr["keep_pos"], arr["keep_code"]
    assert kp[N0] == -1 and kp[N2] == -1
    # H1: the kept code is a both-dataset alt at a tile's last position; a second one is still a call
    off = (int(kp[H1]) - int(arr["scope_span_start"][H1])) % TILE
    assert off == TILE - 1 and pile.calls(H1, kp[H1]) >= {int(kc[H1])} and len(pile.calls(H1, kp[H1])) == 2
    # H3: another ACGT code than the alt, at a tile's first position
    off = (int(kp[H3]) - int(arr["scope_span_start"][H3])) % TILE
    assert off == 0 and kc[H3] in ACGT and pile.calls(H3, kp[H3]) and int(kc[H3]) not in pile.calls(H3, kp[H3])
    assert kc[H3] != pile.refc(H3, kp[H3])
    # H4: an IUPAC code, kept on a both-dataset site of a rare tile
    assert kc[H4] not in ACGT + (0, 15) and pile.calls(H4, kp[H4]) == {int(kc[H4])}
    assert (int(kp[H4]) - int(arr["scope_span_start"][H4])) // TILE in info["rare_tile_ids"][H4]
    # the kept alleles are nobody's must_mask
    mm = {(int(r), int(q)) for r, q, _ in info["must_mask"]}
    for s in (H1, H4):
        kept = [(r, q) for _, c, r, q in pile.at[(s, int(kp[s]))] if c == kc[s]]
        assert kept and not mm & set(kept) and all(list(x) in info["must_not"].tolist() for x in kept)
    assert {(r, q) for _, c, r, q in pile.at[(H3, int(kp[H3]))] if arr["write_scope"][r] == H3} <= mm


def test_tile_edge_cigars(edge):
    arr, info, pile = edge
    huge_reads = [r for s in (H1, H3, H4) for r in _listed(arr, s)]
    assert {op for r in huge_reads for op, _ in _ops(arr, r)} == set(range(9)), "M I D N S H P = X"
    mm = {(int(r), int(q)) for r, q, _ in info["must_mask"]}
    sites = lambda r: sorted(q for rr, q in mm if rr == r)
    # soft clips at both ends, on written reads with sites
    clipped = [r for r in huge_reads if _ops(arr, r)[:1] and _ops(arr, r)[0][0] == 4 and _ops(arr, r)[-1][0] == 4]
    assert clipped and all(sites(r) for r in clipped)
    # an insertion directly before a site
    r = info["insertion"]
    ops = _ops(arr, r)
    assert [o for o, _ in ops] == [0, 1, 0] and sites(r) == [ops[0][1] + ops[1][1]]
    # a deletion across a tile border, sites either side
    r = info["deletion"]
    ops = _ops(arr, r)
    d0 = int(arr["ref_start"][r]) + ops[0][1] - int(arr["scope_span_start"][H3])
    assert [o for o, _ in ops] == [0, 2, 0] and d0 // TILE != (d0 + ops[1][1] - 1) // TILE
    assert len(sites(r)) == 2 and sites(r)[0] < ops[0][1] <= sites(r)[1]
    # an N skip of more than two whole tiles; sites in the first and the last segment; nothing between
    r = info["long_skip"]
    ops = _ops(arr, r)
    assert [o for o, _ in ops] == [0, 3, 0] and ops[1][1] > 2 * TILE and len(sites(r)) == 2
    a, b = int(arr["ref_start"][r]) + ops[0][1], int(arr["ref_start"][r]) + ops[0][1] + ops[1][1]
    assert not [p for (s, p) in pile.at if s == H3 and a <= p < b]
    assert not [x for x in _listed(arr, H3) if x != r and arr["ref_start"][x] < b and _ref_end(arr, x) > a]
    # H and P ops around and inside a read with a site
    r = info["hard_pad"]
    assert [o for o, _ in _ops(arr, r)] == [5, 4, 0, 6, 0, 5] and len(sites(r)) == 1
    # a read over 129 bases with sites at 63, 64, 127, 128
    r = info["long_read"]
    assert arr["read_len"][r] > 129 and sites(r) == [63, 64, 127, 128]
    # reads of length one and zero
    r = info["one_base"]
    assert arr["read_len"][r] == 1 and sites(r) == [0] and arr["write_scope"][r] == H1
    assert arr["seq_off"][r + 1] == arr["seq_off"][r] + 1 and arr["read_len"][r + 1] > 0, "another read's byte follows"
    z = info["zero_length"]
    assert arr["read_len"][z] == 0 and arr["n_cig"][z] == 0 and arr["write_scope"][z] == H1 and z in _listed(arr, H1)
    # a written read with no site at all
    r = info["plain_written"]
    assert arr["write_scope"][r] == H1 and not [1 for obs in pile.at.values() for _, _, rr, _ in obs if rr == r]


def test_tile_edge_oracle_agrees_with_the_builder(edge, oracle):
    arr, info, pile = edge
    out, calls, bases = _check_oracle(oracle, arr, info)
    assert (calls > 0).all() and (bases > 0).all()
    # the pile-up read back from the arrays says the same
    want = np.zeros(5, np.int64)
    for (s, p) in pile.at:
        want[s] += len(pile.calls(s, p) - ({int(arr["keep_code"][s])} if arr["keep_pos"][s] == p else set()))
    assert np.array_equal(calls, want)
    assert len(info["must_not"]) >= 30
    # N2's calls sit on its first and last position
    ss = int(arr["scope_span_start"][N2])
    assert pile.calls(N2, ss) and pile.calls(N2, ss + HUGE - 1) and calls[N2] == 2


# ---- the sized batches and the threshold pair -----------------------------------------------

def test_rare_stride_batch(oracle):
    arr, info = rare_stride_batch()
    assert arr["scope_span_len"][0] == 1030 * TILE and info["tiles_per_scope"][0] == 1030 > 1024
    assert len(arr["read_len"]) == 2060 and len(arr["ref_nt16"]) < 9_000_000
    _check_rules(arr)
    _check_oracle(oracle, arr, info)
    seq, ref = _nibbles(arr["seq_nt16"]), _nibbles(arr["ref_nt16"])
    tile = (arr["ref_start"].astype(np.int64) - arr["scope_span_start"][0]) // TILE
    assert np.array_equal(tile, np.repeat(np.arange(1030), 2)) and np.array_equal(arr["dataset"], np.tile([0, 1], 1030))
    end_tile = (arr["ref_start"].astype(np.int64) + 3 - arr["scope_span_start"][0]) // TILE
    assert np.array_equal(tile, end_tile)
    codes = seq.reshape(-1, 4)
    rc = ref[(arr["scope_ref_off"][0] + arr["ref_start"].astype(np.int64) - arr["scope_span_start"][0])[:, None] + np.arange(4)]
    assert (codes[:, :2] == rc[:, :2]).all() and (codes[:, 2] != rc[:, 2]).all() and np.isin(codes[:, 2], ACGT).all()
    assert (codes[0::2, 2] == codes[1::2, 2]).all()
    assert (codes[0::2, 3] == 0).all() and (codes[1::2, 3] == rc[1::2, 3]).all(), "a tumor-only '=' in every tile"
    assert info["rare_tiles"] == 1030 and info["calls_per_scope"].tolist() == [1030]


def test_crowd_batch(oracle):
    arr, info = crowd_batch()
    n = len(arr["read_len"])
    assert n == 33000 > 8192 * 4 and (arr["write_scope"] == 0).all() and (arr["read_len"] == 2).all()
    assert info["huge_written_reads"] == n and arr["scope_span_len"][0] > HUGE
    _check_rules(arr)
    _check_oracle(oracle, arr, info)
    seq, ref = _nibbles(arr["seq_nt16"]), _nibbles(arr["ref_nt16"])
    pos = arr["ref_start"].astype(np.int64) - arr["scope_span_start"][0]
    rc = ref[arr["scope_ref_off"][0] + pos]
    alt = seq[0::2] != rc
    assert np.array_equal(~alt, np.arange(n) % 97 == 0), "every 97th read carries no alt"
    assert (seq[1::2] == ref[arr["scope_ref_off"][0] + pos + 1]).all()
    assert np.array_equal(pos[0::2], pos[1::2]) and len(np.unique(pos)) == n // 2
    tiles = set((pos // TILE).tolist())
    last = int(info["tiles_per_scope"][0]) - 1
    assert {0, last} <= tiles and tiles <= {0, 1, last - 2, last - 1, last}   # (the last tile is 3 wide)
    assert pos.min() == 0 and pos.max() + 2 == arr["scope_span_len"][0]
    assert 0 < len(info["must_not"]) < n // 50 < info["calls_per_scope"][0]


def test_threshold_pair(oracle):
    (a, ia), (b, ib) = threshold_pair()
    assert a["scope_span_len"].tolist() == [HUGE] and b["scope_span_len"].tolist() == [HUGE + 1]
    diff = sorted(k for k in a if not np.array_equal(a[k], b[k]))
    assert diff == ["ref_start", "scope_span_len"]
    moved = np.nonzero(a["ref_start"] != b["ref_start"])[0]
    assert moved.tolist() == [ia["mover"]] and b["ref_start"][moved[0]] - a["ref_start"][moved[0]] == 1
    assert ia["tiles_per_scope"].tolist() == [0] and ib["tiles_per_scope"].tolist() == [65]
    for arr, info in ((a, ia), (b, ib)):
        _check_rules(arr)
        _check_oracle(oracle, arr, info)
        assert max(_ref_end(arr, r) for r in range(4)) == arr["scope_span_start"][0] + arr["scope_span_len"][0]
    # the moved read is still masked: on both alts below the threshold, on one above it
    assert (ia["must_mask"][:, 0] == ia["mover"]).sum() == 2 and (ib["must_mask"][:, 0] == ib["mover"]).sum() == 1
    assert ia["calls_per_scope"].tolist() == [3] and ib["calls_per_scope"].tolist() == [2]
