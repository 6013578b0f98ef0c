"""Hand-built FASTQ record sets and a plain per-record formatter (no GPU, no project code).

The sets pin the formatter's phase arithmetic (csrc/ganon_fastq.hip): where a field
starts in its 16-byte output quad, where its source starts in the aligned dword (for bases: at which
nibble), whether it is reversed, which of the four buffer slots it comes from, and where an 8 KiB
output tile boundary cuts it. Every set is the ``native.fastq_records`` dict layout; builders that
need to say more about a set put it under the extra key ``"meta"``, which no formatter reads.

``ref_format`` formats one record at a time from the record arrays alone. It shares nothing with
oracle/fastq_oracle.py or the native formatters; tests/test_fastq_sets.py holds all three equal on
every set here, so a GPU mismatch on one of them is a GPU finding.
"""
from __future__ import annotations

import numpy as np

TILE = 8192                      # output bytes per formatter workgroup (kFqTile)
STAGE = 64                       # records a tile kernel stages; a tile touching more goes to k_fq_dense

_NT16 = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b
ACGTN = np.array([1, 2, 4, 8, 15], np.uint8)
POISON = np.array([0, 3], np.uint8)      # '=' and 'M': codes without a complement


def ref_format(recs: dict):
    """'@name/M\\nSEQ\\n+\\nQUAL\\n' per record; the index of the first reverse record holding a base
    outside ACGTN instead, if there is one."""
    out = bytearray()
    for i in range(len(recs["seq_len"])):
        sb = recs["seq_bufs"][int(recs["seq_sel"][i])]
        nib = int(recs["seq_nib_off"][i]) + np.arange(int(recs["seq_len"][i]), dtype=np.int64)
        byte = sb[nib >> 1]
        seq = _NT16[np.where(nib & 1, byte & 0xF, byte >> 4)]
        if recs["reverse"][i]:
            seq = _COMP[seq][::-1]
            if not seq.all():
                return i
        q0 = int(recs["qual_off"][i])
        qual = recs["qual_bufs"][int(recs["qual_sel"][i])][q0:q0 + int(recs["qual_len"][i])]
        qual = ((qual.astype(np.uint16) + 33) & 0xFF).astype(np.uint8)
        if recs["qual_rev"][i]:
            qual = qual[::-1]
        n0 = int(recs["name_off"][i])
        name = bytes(recs["names"][n0:n0 + int(recs["name_len"][i])])
        mate = (int(recs["mate"][i]) + ord("0")) & 0xFF
        out += b"@" + name + b"/" + bytes([mate]) + b"\n" + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n"
    return bytes(out)


def record_bytes(recs: dict) -> np.ndarray:
    return 8 + recs["name_len"].astype(np.int64) + recs["seq_len"] + recs["qual_len"]


def record_starts(recs: dict) -> np.ndarray:
    """Output offset of every record, and the total as a last entry."""
    return np.concatenate([[0], np.cumsum(record_bytes(recs))]).astype(np.int64)


def tile_records(recs: dict):
    """Per 8 KiB output tile: the records holding at least one of its bytes (as
    test_hip_formatter_staging_threshold counts them), and the records the tile kernels range over
    (k_fq_off's tile_first rule: up to the record holding the next tile's first byte, which has no
    byte in this tile when a record ends on the boundary)."""
    end = record_starts(recs)[1:]
    total = int(end[-1]) if len(end) else 0
    t0 = np.arange(0, total, TILE, dtype=np.int64)
    first = np.searchsorted(end, t0, side="right")
    last = np.searchsorted(end, np.minimum(t0 + TILE, total) - 1, side="right")
    nxt = np.where(t0 + TILE < total, np.searchsorted(end, np.minimum(t0 + TILE, max(total - 1, 0)), side="right"),
                   len(end) - 1)
    return last - first + 1, nxt - first + 1


class SetBuilder:
    """Accumulates records over nibble streams, quality streams and a name blob. A read is placed at
    a wanted nibble phase by padding the stream with codes that have no complement, and one such
    nibble follows every read; qualities are preceded by 1-4 bytes of 0xFF and names by 1-4 bytes of
    0xFF, which also choose their offsets' phase mod 4."""

    def __init__(self, seed: int, n_seq: int = 1, n_qual: int = 1):
        self.rng = np.random.default_rng(seed)
        self.seq = [[] for _ in range(n_seq)]
        self.seq_n = [0] * n_seq
        self.qual = [[] for _ in range(n_qual)]
        self.qual_n = [0] * n_qual
        self.names = []
        self.names_n = 0
        self.rows = []
        self.out = 0            # output bytes so far

    def _bytes_at(self, chunks, count, phase, data):
        pad = 1 + (phase - count - 1) % 4
        chunks.append(np.full(pad, 0xFF, np.uint8))
        chunks.append(data)
        return count + pad, count + pad + len(data)

    def add(self, L, Q, NL, reverse, qual_rev, mate=1, ssel=0, qsel=0, nib_phase=None, nib_mod=16, q_phase=None,
            n_phase=None, bad_at=None, bad_code=0, zero_at=None, qmax=93):
        rng = self.rng
        codes = rng.choice(ACGTN, L) if reverse else rng.integers(0, 16, L).astype(np.uint8)
        if bad_at is not None:
            codes[bad_at] = bad_code
        if L == 0 and zero_at is not None:
            nib_off = zero_at
        else:
            s = self.seq_n[ssel]
            if nib_phase is None:
                nib_phase = int(rng.integers(0, nib_mod))
            pad = (nib_phase - s) % nib_mod
            self.seq[ssel] += [POISON[rng.integers(0, 2, pad)], codes, POISON[rng.integers(0, 2, 1)]]
            nib_off = s + pad
            self.seq_n[ssel] = nib_off + L + 1
        if Q == 0 and zero_at is not None:
            q_off = zero_at
        else:
            if q_phase is None:
                q_phase = int(rng.integers(0, 4))
            q_off, self.qual_n[qsel] = self._bytes_at(self.qual[qsel], self.qual_n[qsel], q_phase,
                                                      rng.integers(0, qmax + 1, Q).astype(np.uint8))
        if NL == 0 and zero_at is not None:
            n_off = zero_at
        else:
            if n_phase is None:
                n_phase = int(rng.integers(0, 4))
            n_off, self.names_n = self._bytes_at(self.names, self.names_n, n_phase,
                                                 rng.integers(33, 127, NL).astype(np.uint8))
        self.rows.append((ssel, nib_off, L, int(bool(reverse)), qsel, q_off, Q, int(bool(qual_rev)), n_off, NL, mate))
        self.out += 8 + NL + L + Q
        return len(self.rows) - 1

    def fill(self, gap: int, dense: bool):
        """Filler records of `gap` output bytes in all: a few of about 2.7 KB, or ones of <= 120 bytes."""
        assert gap >= 8
        k = -(-gap // 100) if dense else max(1, round(gap / 2720))
        k = min(k, gap // 8)
        for i in range(k):
            z = gap // k + (1 if i < gap % k else 0)
            NL = int(self.rng.integers(0, min(12, z - 8) + 1))
            L = (z - 8 - NL) // 2
            self.add(L, z - 8 - NL - L, NL, self.rng.random() < 0.5, self.rng.random() < 0.5, 1 + i % 2)

    def recs(self, meta=None) -> dict:
        def packed(chunks):
            c = np.concatenate(chunks + [POISON[[0, 1, 0, 1]]]) if chunks else POISON[[0, 1, 0, 1]]
            c = c[: len(c) & ~1].astype(np.uint8)
            return ((c[0::2] << 4) | c[1::2]).astype(np.uint8)

        def joined(chunks):
            return np.concatenate(chunks + [np.full(1, 0xFF, np.uint8)]).astype(np.uint8)

        cols = list(zip(*self.rows)) if self.rows else [[]] * 11
        A = lambda j, dt: np.ascontiguousarray(np.array(cols[j], dtype=dt))
        r = {"seq_bufs": [packed(c) for c in self.seq], "seq_sel": A(0, np.uint8), "seq_nib_off": A(1, np.int64),
             "seq_len": A(2, np.int32), "reverse": A(3, np.uint8),
             "qual_bufs": [joined(c) for c in self.qual], "qual_sel": A(4, np.uint8), "qual_off": A(5, np.int64),
             "qual_len": A(6, np.int32), "qual_rev": A(7, np.uint8),
             "names": joined(self.names), "name_off": A(8, np.int64), "name_len": A(9, np.int32), "mate": A(10, np.uint8)}
        if meta is not None:
            r["meta"] = meta
        return r


LATTICE_LENGTHS = tuple(range(41)) + (63, 64, 65, 127, 129)


def buffer_lows(recs: dict):
    """Lowest used byte of every sequence and quality buffer and of the name blob (fields of length
    zero use nothing) — where the upload slices each buffer."""
    def lows(sel, off, length, n):
        return [int(off[(sel == s) & (length > 0)].min()) if ((sel == s) & (length > 0)).any() else None
                for s in range(n)]
    sl = lows(recs["seq_sel"], recs["seq_nib_off"] >> 1, recs["seq_len"], len(recs["seq_bufs"]))
    ql = lows(recs["qual_sel"], recs["qual_off"], recs["qual_len"], len(recs["qual_bufs"]))
    nl = lows(np.zeros(len(recs["name_len"]), np.uint8), recs["name_off"], recs["name_len"], 1)[0]
    return sl, ql, nl


def _lattice_records(b: SetBuilder, lengths, spaced: bool, lows_seq):
    """reverse x qual_rev x first-nibble phase 0..15 x L, in permuted order, over 4 x 4 buffer slots.
    The name length of a read of >= 17 bases is chosen so that its base field starts at the next
    output phase mod 16 its (nibble phase mod 8 as the device sees it, reverse) class has not had."""
    rng = b.rng
    grid = [(rev, qrev, ph, L) for rev in (0, 1) for qrev in (0, 1) for ph in range(16) for L in lengths]
    turn = {}
    for i, g in enumerate(rng.permutation(len(grid))):
        rev, qrev, ph, L = grid[g]
        ssel, qsel = i % 4, (i // 4) % 4
        Q = L
        if i % 5 == 0:      # Q != L, both zero-length cases among them
            Q = [0 if L else 9, L + 1 + L % 7, (L + 1) // 3][(i // 5) % 3]
            if Q == L:
                Q = L + 4
        NL = int(rng.integers(0, 24))
        if L >= 17:
            # the nibble offset this read will get, relative to its buffer's lowest used byte
            nib_off = b.seq_n[ssel] + (ph - b.seq_n[ssel]) % 16
            key = ((nib_off - 2 * lows_seq[ssel]) % 8, rev)
            want = turn.get(key, int(rng.integers(0, 16)))
            turn[key] = (want + 1) % 16
            NL = (want - b.out - 4) % 16
            if NL + 16 < 24 and rng.random() < 0.5:
                NL += 16
        b.add(L, Q, NL, rev, qrev, 1 + int(rng.integers(0, 2)), ssel, qsel, nib_phase=ph)
        if spaced and i % 8 == 7:   # ballast: keeps every tile at <= 64 records, on the instance's own kernel
            b.add(700, 700, 20, 0, i % 16 == 7, 1, ssel, qsel)


def phase_lattice(seed: int = 11, spaced: bool = False, lengths=LATTICE_LENGTHS) -> dict:
    """The phase lattice. Plain, its records average ~75 bytes, so its tiles hold more than 64 of
    them and k_fq_dense formats them; ``spaced`` puts a 1.4 KB forward read after every eighth record,
    which keeps every tile on the selected instance's own kernel.

    The first records pin the upload's slicing: every buffer's lowest used byte is non-zero and no
    multiple of 4, and records 0 and 1 have a zero-length field whose offset (0) lies below it."""
    b = SetBuilder(seed, 4, 4)
    b.add(0, 9, 0, 0, 0, 2, 0, 0, q_phase=1, zero_at=0)              # no bases, no name: offsets 0
    b.add(7, 0, 0, 1, 0, 2, 0, 0, nib_phase=11, zero_at=0)           # no qualities: offset 0
    for k, (nph, qph) in enumerate(((13, 2), (15, 3), (3, 1)), start=1):
        b.add(6, 6, 3, 0, 0, 1, k, k, nib_phase=nph, q_phase=qph, n_phase=1)
    lows_seq = [5, 6, 7, 1]
    _lattice_records(b, lengths, spaced, lows_seq)
    r = b.recs()
    assert buffer_lows(r)[0] == lows_seq
    return r


PROBE = (5, 21, 21)     # name, bases, qualities: 55 bytes


def boundary_ladder(style: str, seed: int = 21) -> dict:
    """A 55-byte probe record starting d bytes before an 8 KiB boundary for every d in 0..55, four
    times over so that each of the four (reverse, qual_rev) kinds meets every d; between placements,
    filler up to the next boundary minus d. ``meta``: the probes' record indices, d and kind."""
    assert style in ("sparse", "dense")
    NL, L, Q = PROBE
    plen = 8 + NL + L + Q
    b = SetBuilder(seed)
    idx, ds, kinds = [], [], []
    j = 0
    for rnd in range(4):
        for d in range(plen + 1):
            bound = (b.out + 8 + d + TILE - 1) // TILE * TILE      # room for at least one filler record
            bound = max(bound, TILE)
            b.fill(bound - d - b.out, style == "dense")
            kind = (d + rnd) % 4
            idx.append(b.add(L, Q, NL, kind & 1, kind >> 1, 1 + j % 2, nib_phase=(5 * j + rnd) % 8, nib_mod=8,
                             q_phase=(3 * j + j // 7) % 4, n_phase=(j + j // 5) % 4))
            assert (b.out - plen) % TILE == (TILE - d) % TILE
            ds.append(d)
            kinds.append(kind)
            j += 1
    b.fill(TILE, style == "dense")      # the tile after the last boundary, filled like the others
    return b.recs({"probe": np.array(idx), "d": np.array(ds), "kind": np.array(kinds)})


def _fixed_records(b: SetBuilder, sizes):
    for i, z in enumerate(sizes):
        NL = min(i % 9, z - 8)
        L = (z - 8 - NL) // 2
        b.add(L, z - 8 - NL - L, NL, i % 2, (i // 2) % 2, 1 + i % 2)


def aligned_tiles(seed: int = 31) -> dict:
    """name -> set. "aligned": 320 records of exactly 128 bytes, five whole tiles (an odd number, for
    the two-tile instance), every record boundary on a 128-byte grid and every 64th on a tile boundary:
    a tile's record range is its own 64 records plus the neighbour that has no byte in it. "shifted":
    the first record is 129 bytes. "total8" .. "total17": outputs shorter than, equal to and just
    over one 16-byte quad."""
    sets = {}
    b = SetBuilder(seed)
    _fixed_records(b, [128] * 320)
    sets["aligned"] = b.recs()
    b = SetBuilder(seed + 1)
    _fixed_records(b, [129] + [128] * 319)
    sets["shifted"] = b.recs()
    for k, (NL, L, Q, rev) in enumerate(((0, 0, 0, 0), (7, 0, 0, 0), (0, 4, 4, 1), (1, 4, 4, 1))):
        b = SetBuilder(seed + 2 + k)
        b.add(L, Q, NL, rev, rev, 2, nib_phase=2 * k + 1)
        sets[f"total{8 + NL + L + Q}"] = b.recs()
    return sets


def long_fields(seed: int = 41) -> dict:
    """Fields longer than a tile: 20,000 bases from an odd nibble (forward, reverse), 20,000
    qualities (stored order, reversed), a 20,000-byte name, and Q != L."""
    b = SetBuilder(seed, 2, 2)
    N = 20000
    b.add(N, N, 9, 0, 0, 1, 0, 1, nib_phase=5)
    b.add(N, N, 0, 1, 1, 2, 1, 0, nib_phase=11)
    b.add(30, 30, N, 1, 0, 1, 0, 0, n_phase=3)
    b.add(N, 10, 4, 1, 1, 2, 1, 1, nib_phase=7)
    b.add(5, N, 4, 0, 1, 1, 0, 0, nib_phase=1, q_phase=1)
    b.add(33, 33, 6, 1, 0, 2, 1, 1, nib_phase=15)
    return b.recs()


def wide_qualities(seed: int = 45) -> dict:
    """Quality bytes 0..255 at every source phase, stored order and reversed: the formatters print
    (q + 33) & 0xFF, and add33's SWAR add must keep every byte's carry to itself. (Above 93 the
    oracle, like the reference, prints a code point of two bytes: this set is not for it.)"""
    b = SetBuilder(seed, 1, 2)
    for i in range(96 + 320):      # 96 records of ~250 bytes (the instance's own kernel), then 320 of ~40 (k_fq_dense)
        Q = 100 + (5 * i) % 50 if i < 96 else 16 + (5 * i) % 24
        b.add(Q if i < 96 and i % 3 else 4, Q, i % 7, i % 2, (i // 2) % 2, 1 + i % 2, 0, i % 2, q_phase=(i // 4) % 4,
              qmax=255)
    return b.recs()


def q7_probes(seed: int = 51):
    """[(set, expected)]: expected is the index the formatters must report, or None for clean sets.
    Per filler style and per j in 0..39: a reverse read of 40 bases cut by the first tile boundary
    at base 20, with one base without a complement at stored position j (codes 0 and 3 in turn);
    two bad records in different tiles; sets (tiles of <= 64 records, and dense ones) whose only
    such nibbles are the neighbours and pad nibbles of clean reverse reads and bases of forward reads."""
    out = []
    for dense in (False, True):
        for j in range(40):
            b = SetBuilder(seed + j, 2, 2)
            b.fill(TILE - 20 - 4 - 5, dense)
            p = b.add(40, 40, 5, 1, j % 2, 1, 1, 1, nib_phase=j % 16, bad_at=j, bad_code=(0, 3)[j % 2])
            assert b.out - (40 + 3 + 40 + 1) + 20 == TILE      # the base field starts 20 bytes before the boundary
            b.add(30, 30, 3, 1, 0, 2, 1, 1)
            b.add(30, 30, 3, 1, 1, 1)
            out.append((b.recs(), p))
    b = SetBuilder(seed + 100)
    b.fill(TILE + 100, False)
    p = b.add(50, 50, 4, 1, 0, 1, nib_phase=3, bad_at=49, bad_code=3)
    b.fill(2 * TILE, False)
    b.add(50, 50, 4, 1, 0, 1, nib_phase=6, bad_at=0, bad_code=0)
    b.fill(500, False)
    out.append((b.recs(), p))
    for dense in (False, True):
        b = SetBuilder(seed + 200 + dense, 3, 2)
        for i in range(640):
            rev = i % 3 != 2
            L = 1 + (7 * i) % 40 if rev else 40
            b.add(L, 12 if dense else 100, 4 if dense else 60, rev, i % 2, 1 + i % 2, i % 3, i % 2, nib_phase=i % 16)
        out.append((b.recs(), None))
    return out


MANY_EMPTY = 2 * 1024 * 1024 + 2048 + 5     # more than two rounds of k_fq_bscan's 1024 block sums of 2048 records


def _many_tail(seed: int) -> dict:
    b = SetBuilder(seed, 2, 2)
    for i in range(50):
        L = (0, 1, 17, 40, 65, 129)[i % 6]
        b.add(L, L if i % 5 else L + 3, i % 24, i % 2, (i // 2) % 2, 1 + i % 2, i % 2, (i // 2) % 2, nib_phase=i % 16)
    return b.recs()


def many_records(seed: int = 61) -> dict:
    """MANY_EMPTY records of 8 bytes (no name, no bases, no qualities; mates 1, 2 in turn), then 50
    lattice-style records: the offset scan's carry between rounds of 1024 block sums."""
    t = _many_tail(seed)
    n = MANY_EMPTY
    z = lambda k: np.concatenate([np.zeros(n, t[k].dtype), t[k]])
    r = {k: (z(k) if isinstance(v, np.ndarray) and len(v) == 50 and k != "names" else v) for k, v in t.items()}
    r["mate"][:n] = 1 + np.arange(n) % 2
    return r


def many_expected(seed: int = 61) -> bytes:
    pair = np.frombuffer(b"@/1\n\n+\n\n@/2\n\n+\n\n", np.uint8)
    head = np.tile(pair, (MANY_EMPTY + 1) // 2)[: 8 * MANY_EMPTY]
    return head.tobytes() + ref_format(_many_tail(seed))
