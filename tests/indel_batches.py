"""Deterministic batches for the germline indel tally (ganon_indel.hip), for tests/test_gpu_indels.py
and the CPU test that pins them (tests/test_indel_batches.py). Each one sits on a path or a threshold
that the upload chooses from the batch's shape, or on a boundary inside a kernel:

* ``cigar_arith_batch``: all nine CIGAR ops around I/D ops; leading / trailing I and D; ``1I1I``; an I
  followed by a D at one position; 40H on an 11-base read; a clipped DEL allele; nibble parity.
* ``walk_threshold_pair``: a read with an I/D op has 32 CIGAR ops, or 33 (thread walk / wave walk).
* ``block_edge_batch``: wave walk, I/D ops at op indices 0, 63, 64, 255, 256, 257, 511, 512.
* ``tsort_threshold_pair``: one scope of 4096 unfiltered observations, or 4097 (tsort / gsort).
* ``tsort_order_batch``: scopes whose filtered observations arrive in descending position order, with
  emptied scopes between scopes of equal keys.
* ``hash_collision_batch``: a hashed candidate map of 2^12 cells with two planted collisions.
* ``two_contig_batch``: the same contig positions on two contigs; a read of two overlapping scopes.
* ``run_chunk_batch``: wave walk, 4,207 filtered observations, runs across k_indel_runs' 256 | 4096.
* ``normal_cover_batch``: scopes of 7, 8, 9, 16 and 17 incidences whose covering normal read is last.
* ``rank_batch``: four calls at one position, registered in an order the slots do not follow.
* ``indel_csr_batch``: the tally's own incidence CSR leaves a normal read out.
* ``key_edge_pair``: the last of 2^k scopes has the widest span, 2^k - 1 or 2^k positions long, and a
  TN insertion at its end (the all-ones 64-bit key).
* ``nothing_left_pair``: tumor-only ops (nothing passes the filter); exactly one observation.

Every builder returns ``(arrays, expect)`` (the ``*_pair`` builders two of them). ``expect`` is the
builder's own answer: the records ``(scope, pos, length, type, rank, kind, read, in_read_pos)``
written out as literals or from the closed form of the generated CIGARs, the observations, the
observations that pass the candidate filter under the default map (``emitted``) and under the dense
map (``emitted_dense``), and the route bits of ``ganon_indel_info`` under default settings. Nothing in
here calls the oracle or the device; every base of every read is given (``A`` where not stated), the
reference is all ``A``: the tally never reads it.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from genomeanonymizer_amd.synth.batch import _cigar_word, pack_nibbles

NT = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
DEL, INS = 2, 3
CALL, SUPPORT = 0, 1
# ganon_indel_info's route slot (include/ganon.h GANON_INDEL_ROUTE_*)
THREAD_WALK, TSORT, GSORT, HASHED = 1, 2, 4, 8
THREAD_WALK_OPS = 32      # kThreadWalkOps
TSORT_MAX = 4096          # kTsortMax
WALK_BLOCK = 256          # kWalkOps
RUN_ROW, RUN_CHUNK = 256, 4096   # k_indel_runs: threads of a workgroup, elements of a workgroup
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
_HASH = 0x9E3779B97F4A7C15


def map_cell(g: int, log2_cells: int) -> int:
    """Cell of genome nibble g in a hashed candidate map of 2^log2_cells cells (0: dense)."""
    return ((g * _HASH) & (2 ** 64 - 1)) >> (64 - log2_cells) if log2_cells else g


@dataclass
class Expect:
    records: List[tuple]
    observations: int
    emitted: int              # filtered run, default map
    emitted_dense: int        # filtered run, dense map (GANON_INDEL_DENSE_MAP=1)
    route: int                # THREAD_WALK | TSORT | GSORT | HASHED | log2 cells << 8, default settings
    extra: dict = field(default_factory=dict)


def _ops(cigar) -> List[Tuple[str, int]]:
    return [(o, int(n)) for n, o in _CIGAR.findall(cigar)] if isinstance(cigar, str) else list(cigar)


class _Builder:
    def __init__(self, contig_lens: List[int]):
        self.contig_base = [0]
        for n in contig_lens:
            self.contig_base.append(self.contig_base[-1] + n)
        self.scopes = []      # [contig, span_start or None, span_len or None]
        self.reads = []       # dict per read

    def scope(self, contig: int = 0, start: int = None, length: int = None) -> int:
        self.scopes.append([contig, start, length])
        return len(self.scopes) - 1

    def read(self, listed, ws: int, ds: int, pos: int, cigar, seq: str = None, tally=None) -> int:
        """A read listed by the scopes ``listed`` (tallied by ``tally``, default the same), written by
        ``ws``. ``seq``: its bases (default all A); its length must be the CIGAR's M/I/S/=/X total."""
        ops = _ops(cigar)
        qlen = sum(n for o, n in ops if o in "MIS=X")
        seq = "A" * qlen if seq is None else seq
        assert len(seq) == qlen, (cigar if isinstance(cigar, str) else len(ops), len(seq), qlen)
        rl = sum(n for o, n in ops if o in "MDN=X")
        # the I/D ops as the reference's arithmetic places them: (pos, in_read_pos, type, length)
        id_ops, p, q = [], pos, 0
        for o, n in ops:
            if o in "ID":
                id_ops.append((p, q, INS if o == "I" else DEL, n))
            if o in "MDN=X":
                p += n
            if o in "MINSH=X":
                q += n
        listed = list(listed)
        self.reads.append(dict(pos=pos, ops=ops, seq=seq, ds=ds, ws=ws, listed=listed,
                               tally=listed if tally is None else list(tally), end=pos + (rl if rl > 0 else 1),
                               id_ops=id_ops, contig=self.scopes[listed[0]][0]))
        return len(self.reads) - 1

    def _csr(self, key: str):
        incid, offs = [], [0]
        for s in range(len(self.scopes)):
            ids = [i for i, r in enumerate(self.reads) if s in r[key]]
            incid += sorted(ids, key=lambda i: (self.reads[i]["ds"], i))    # tumor, then normal; file order
            offs.append(len(incid))
        return np.array(offs, np.int64), np.array(incid, np.int32)

    def counts(self, log2_cells: int) -> Tuple[int, int]:
        """(observations, observations at map cells that a tumor and a normal tallied read both mark)."""
        bits: Dict[int, int] = {}
        for r in self.reads:
            if r["tally"]:
                for p, _, _, _ in r["id_ops"]:
                    c = map_cell(self.contig_base[r["contig"]] + p, log2_cells)
                    bits[c] = bits.get(c, 0) | (1 << r["ds"])
        n_obs = n_emit = 0
        for r in self.reads:
            for p, _, _, _ in r["id_ops"]:
                n_obs += len(r["tally"])
                if bits.get(map_cell(self.contig_base[r["contig"]] + p, log2_cells), 0) == 3:
                    n_emit += len(r["tally"])
        return n_obs, n_emit

    def finish(self, records, route: int, **extra) -> Tuple[Dict[str, np.ndarray], Expect]:
        n_scopes = len(self.scopes)
        ss, sl, ro = [], [], []
        for s, (c, start, length) in enumerate(self.scopes):
            mine = [r for r in self.reads if s in r["listed"]]
            a = min(r["pos"] for r in mine) if start is None else start
            n = max(r["end"] for r in mine) - a if length is None else length
            assert all(a <= r["pos"] and r["end"] <= a + n and r["contig"] == c for r in mine), s
            assert a + n <= self.contig_base[c + 1] - self.contig_base[c], s
            ss.append(a)
            sl.append(n)
            ro.append(self.contig_base[c] + a)
        packed = [pack_nibbles(np.array([NT[ch] for ch in r["seq"]], np.uint8)) for r in self.reads]
        nb = np.array([len(x) for x in packed], np.int64)
        cig = [np.array([_cigar_word(o, n) for o, n in r["ops"]], np.uint32) for r in self.reads]
        nc = np.array([len(x) for x in cig], np.int64)
        off, incid = self._csr("listed")
        arr = {
            "ref_start": np.array([r["pos"] for r in self.reads], np.int32),
            "read_len": np.array([len(r["seq"]) for r in self.reads], np.int32),
            "seq_off": np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64),
            "seq_nt16": np.concatenate(packed),
            "cig_off": np.concatenate([[0], np.cumsum(nc)[:-1]]).astype(np.int64),
            "n_cig": nc.astype(np.int32),
            "cigar": np.concatenate(cig),
            "dataset": np.array([r["ds"] for r in self.reads], np.uint8),
            "write_scope": np.array([r["ws"] for r in self.reads], np.int32),
            "scope_incid_off": off,
            "incid_read": incid,
            "scope_span_start": np.array(ss, np.int32),
            "scope_span_len": np.array(sl, np.int32),
            "scope_ref_off": np.array(ro, np.int64),
            "ref_nt16": np.full((self.contig_base[-1] + 1) // 2, 0x11, np.uint8),
            "keep_pos": np.full(n_scopes, -1, np.int32),
            "keep_code": np.zeros(n_scopes, np.uint8),
        }
        if any(r["tally"] != r["listed"] for r in self.reads):
            arr["indel_incid_off"], arr["indel_incid_read"] = self._csr("tally")
        n_obs, dense = self.counts(0)
        k = (route >> 8) & 0xFF
        return arr, Expect(sorted(records), n_obs, self.counts(k)[1] if k else dense, dense, route, extra)


def _tn(s: int, pos: int, length: int, vt: int, rank: int, first: Tuple[int, int], supports) -> List[tuple]:
    """The records of one masked call: CALL by (read, in_read_pos) ``first``, SUPPORT by each of
    ``supports`` (read, in_read_pos)."""
    return [(s, pos, length, vt, rank, CALL, first[0], first[1])] + \
           [(s, pos, length, vt, rank, SUPPORT, r, q) for r, q in supports]


# ---- literals ------------------------------------------------------------------------------------

def cigar_arith_batch():
    b = _Builder([400])
    s = b.scope()
    c = "C"
    # S and H before and after: H counts toward in_read_pos (2 + 3 + 5 = 10), the allele is read at
    # seq[10:12] although the inserted bases are seq[8:10]
    r0 = b.read([s], s, 0, 10, "2H3S5M2I5M4S1H", "ACGTACGTACGTACGTACG")          # seq[10:12] = GT
    r1 = b.read([s], s, 1, 10, "5S5M2I5M", c * 10 + "GT" + c * 5)
    # N, =, X between count, P does not: pos 40 + 4 + 3 + 2 + 2, in_read_pos 4 + 3 + 2 + 2
    r2 = b.read([s], s, 0, 40, "4M3N2=1P2X1D6M", c * 11 + "TT" + c)
    r3 = b.read([s], s, 1, 40, "11M1D6M", c * 11 + "TT" + c * 4)
    # leading I at op 0, leading D
    r4 = b.read([s], s, 0, 70, "2I8M", "GG" + c * 8)
    r5 = b.read([s], s, 1, 70, "2I8M", "GG" + c * 8)
    r6 = b.read([s], s, 0, 90, "2D8M", c * 8)
    r7 = b.read([s], s, 1, 90, "2D8M", c * 8)
    # trailing I at reference_end 118 (a plain normal read covers it), trailing D (allele '')
    r8 = b.read([s], s, 0, 110, "8M1I", c * 8 + "T")
    r9 = b.read([s], s, 1, 110, "8M1I", c * 8 + "T")
    b.read([s], s, 1, 115, "10M", c * 10)                                         # r10
    r11 = b.read([s], s, 0, 140, "8M2D", c * 8)
    r12 = b.read([s], s, 1, 140, "8M2D", c * 8)
    # 1I1I: one call supported twice by r13 (CALL: first offset 5; SUPPORT: last offset 6); the
    # normal's second base differs: its own call, normal only, rank 1
    r13 = b.read([s], s, 0, 170, "5M1I1I5M", c * 5 + "AA" + c * 5)
    r14 = b.read([s], s, 1, 170, "5M1I1I5M", c * 5 + "AG" + c * 5)
    # I directly followed by D at 205: two calls, ranks 0 and 1
    r15 = b.read([s], s, 0, 200, "5M2I3D5M", c * 5 + "GGTT" + c * 3)
    r16 = b.read([s], s, 1, 200, "5M2I3D5M", c * 5 + "GGTT" + c * 3)
    # 40H on an 11-base read: in_read_pos 45 is past the read, the allele is ''
    r17 = b.read([s], s, 0, 230, "40H5M1I5M", c * 5 + "G" + c * 5)
    r18 = b.read([s], s, 1, 230, "40H5M1I5M", c * 5 + "T" + c * 5)
    # DEL allele seq[9:11]: clipped to T by r19's end, TC in r21 and r20: two calls, the second TN
    b.read([s], s, 0, 260, "9M2D1M", c * 9 + "T")                                 # r19
    r20 = b.read([s], s, 1, 260, "9M2D3M", c * 9 + "TC" + c)
    r21 = b.read([s], s, 0, 260, "9M2D3M", c * 9 + "TC" + c)
    # one insertion at even (4) and odd (5) in_read_pos; r24's allele is the nibbles swapped. r23
    # (ref_start 289, normal) registers the call first
    r22 = b.read([s], s, 0, 290, "4M2I6M", c * 4 + "GT" + c * 6)
    r23 = b.read([s], s, 1, 289, "5M2I6M", c * 5 + "GT" + c * 6)
    b.read([s], s, 1, 289, "5M2I6M", c * 5 + "TG" + c * 6)                        # r24
    assert (r0, r9, r18, r23) == (0, 9, 18, 23)
    records = (
        _tn(0, 15, 2, INS, 0, (r0, 10), [(r0, 10), (r1, 10)]) +
        _tn(0, 51, 1, DEL, 0, (r2, 11), [(r2, 11), (r3, 11)]) +
        _tn(0, 70, 2, INS, 0, (r4, 0), [(r4, 0), (r5, 0)]) +
        _tn(0, 90, 2, DEL, 0, (r6, 0), [(r6, 0), (r7, 0)]) +
        _tn(0, 118, 1, INS, 0, (r8, 8), [(r8, 8), (r9, 8)]) +
        _tn(0, 148, 2, DEL, 0, (r11, 8), [(r11, 8), (r12, 8)]) +
        _tn(0, 175, 1, INS, 0, (r13, 5), [(r13, 6), (r14, 5)]) +
        _tn(0, 205, 2, INS, 0, (r15, 5), [(r15, 5), (r16, 5)]) +
        _tn(0, 205, 3, DEL, 1, (r15, 7), [(r15, 7), (r16, 7)]) +
        _tn(0, 235, 1, INS, 0, (r17, 45), [(r17, 45), (r18, 45)]) +
        _tn(0, 269, 2, DEL, 1, (r21, 9), [(r21, 9), (r20, 9)]) +
        _tn(0, 294, 2, INS, 0, (r23, 5), [(r22, 4), (r23, 5)]))
    arr, e = b.finish(records, THREAD_WALK | TSORT)
    assert (e.observations, e.emitted) == (28, 28)
    return arr, e


def walk_threshold_pair():
    """(32-op batch, 33-op batch): r0 is 1M1I x16, with a leading 1S in the second batch (every
    in_read_pos of r0 moves by one); r3 has 40 ops and no I/D op in both."""
    out = []
    for lead in ("", "1S"):
        b = _Builder([400])
        s = b.scope()
        r0 = b.read([s], s, 0, 10, lead + "1M1I" * 16)
        r1 = b.read([s], s, 1, 10, "1M1I" * 16)
        b.read([s], s, 1, 5, "40M")
        b.read([s], s, 0, 100, "1M1X" * 20)
        q0 = len(lead) // 2
        records = []
        for k in range(16):     # op 2k + 1: pos 10 + k + 1, in_read_pos 2k + 1
            records += _tn(0, 11 + k, 1, INS, 0, (r0, 2 * k + 1 + q0), [(r0, 2 * k + 1 + q0), (r1, 2 * k + 1)])
        out.append(b.finish(records, 0 if lead else THREAD_WALK | TSORT, id_read_ops=33 if lead else 32))
    return tuple(out)


def rank_batch():
    b = _Builder([200])
    s = b.scope()
    t = "T"
    r0 = b.read([s], s, 0, 45, "5M1I5M", t * 5 + "C" + t * 5)       # INS C: tumor only
    r1 = b.read([s], s, 0, 45, "5M2I5M", t * 5 + "AG" + t * 5)      # INS AG
    r2 = b.read([s], s, 0, 46, "4M2D5M", t * 9)                     # DEL, allele TT
    r3 = b.read([s], s, 1, 40, "10M1I5M", t * 10 + "A" + t * 5)     # INS A: normal only, ref_start 40: rank 0
    r4 = b.read([s], s, 1, 44, "6M2D5M", t * 11)                    # DEL, ref_start 44: rank 1
    r5 = b.read([s], s, 1, 45, "5M2I5M", t * 5 + "AG" + t * 5)      # INS AG after r0's INS C (rank 2): rank 3
    assert (r0, r3) == (0, 3)
    records = _tn(0, 50, 2, DEL, 1, (r4, 6), [(r2, 4), (r4, 6)]) + _tn(0, 50, 2, INS, 3, (r1, 5), [(r1, 5), (r5, 5)])
    arr, e = b.finish(records, THREAD_WALK | TSORT)
    assert (e.observations, e.emitted) == (6, 6)
    return arr, e


def two_contig_batch():
    b = _Builder([300, 300])
    s0, s1, s2, s3 = b.scope(0), b.scope(1), b.scope(0), b.scope(0)
    b.read([s0], s0, 0, 50, "5M1I5M")          # r0: tumor I at 55 of contig A
    b.read([s0], s0, 1, 45, "20M")             # r1
    b.read([s1], s1, 1, 50, "5M1I5M")          # r2: normal I at 55 of contig B: never TN with r0
    b.read([s1], s1, 0, 45, "20M")             # r3
    b.read([s0], s0, 0, 95, "5M2D5M")          # r4, r5: TN at 100 of A
    b.read([s0], s0, 1, 95, "5M2D5M")
    b.read([s1], s1, 0, 95, "5M2D5M")          # r6, r7: TN at 100 of B
    b.read([s1], s1, 1, 95, "5M2D5M")
    b.read([s2, s3], s2, 0, 200, "5M1I5M")     # r8: written by scope 2 only
    b.read([s2, s3], s3, 1, 200, "5M1I5M")     # r9: written by scope 3 only
    records = (_tn(0, 100, 2, DEL, 0, (4, 5), [(4, 5), (5, 5)]) + _tn(1, 100, 2, DEL, 0, (6, 5), [(6, 5), (7, 5)]) +
               _tn(2, 205, 1, INS, 0, (8, 5), [(8, 5)]) + _tn(3, 205, 1, INS, 0, (8, 5), [(9, 5)]))
    arr, e = b.finish(records, THREAD_WALK | TSORT)
    assert (e.observations, e.emitted) == (10, 8)
    return arr, e


def indel_csr_batch():
    b = _Builder([200])
    s = b.scope()
    b.read([s], s, 0, 10, "5M1I5M")                    # r0: I at 15
    b.read([s], s, 1, 10, "5M1I40M", tally=[])         # r1: the same I, left out of the tally; covers 45
    b.read([s], s, 0, 40, "5M1I")                      # r2, r3: TN trailing I at 45, covered by r1 only
    b.read([s], s, 1, 40, "5M1I")
    arr, e = b.finish(_tn(0, 45, 1, INS, 0, (2, 5), [(2, 5), (3, 5)]), THREAD_WALK | TSORT)
    assert (e.observations, e.emitted) == (3, 2)
    return arr, e


def key_edge_pair():
    """(span 2^8 - 1, span 2^8) of the last of four scopes. The TN insertion at the span's end has no
    normal pileup column (no read reaches past the span), so it is classified and makes no record."""
    out = []
    for length in (255, 256):
        b = _Builder([2000])
        records = []
        for s in range(3):
            base = 100 + 300 * s
            b.scope()
            t = b.read([s], s, 0, base, "5M2D5M")
            n = b.read([s], s, 1, base, "5M2D5M")
            b.read([s], s, 0, base + 30, "5M1I5M")     # tumor only: the 64-bit sort's capacity has fillers
            records += _tn(s, base + 5, 2, DEL, 0, (t, 5), [(t, 5), (n, 5)])
        s = b.scope(0, 1000, length)
        b.read([s], s, 1, 1000, "10M")
        t = b.read([s], s, 0, 1100, "5M2D5M")
        n = b.read([s], s, 1, 1100, "5M2D5M")
        records += _tn(s, 1105, 2, DEL, 0, (t, 5), [(t, 5), (n, 5)])
        b.read([s], s, 0, 1150, "5M1I5M")
        b.read([s], s, 0, 1000 + length - 5, "5M1I")   # TN at pos - span_start = length
        b.read([s], s, 1, 1000 + length - 5, "5M1I")
        arr, e = b.finish(records, THREAD_WALK | TSORT, pos_bits=8 if length == 255 else 9, last_rel=length)
        assert (e.observations, e.emitted) == (14, 10)
        out.append((arr, e))
    return tuple(out)


def nothing_left_pair():
    """(I/D ops in tumor reads only, exactly one observation): both silent."""
    b = _Builder([300])
    s0, s1 = b.scope(), b.scope()
    b.read([s0], s0, 0, 10, "5M1I5M2D5M")
    b.read([s0], s0, 0, 12, "3M1I5M")
    b.read([s0], s0, 1, 5, "40M")
    b.read([s1], s1, 0, 110, "5M2D5M")
    b.read([s1], s1, 1, 100, "40M")
    first = b.finish([], THREAD_WALK | TSORT)
    assert (first[1].observations, first[1].emitted) == (4, 0)
    b = _Builder([100])
    s = b.scope()
    b.read([s], s, 0, 10, "5M1I5M")
    b.read([s], s, 1, 5, "40M")
    second = b.finish([], THREAD_WALK | TSORT)
    assert (second[1].observations, second[1].emitted) == (1, 0)
    return first, second


# ---- generated, closed form ----------------------------------------------------------------------

def _edge_cigar(n_ops: int, at) -> List[Tuple[str, int]]:
    """n_ops ops of length 1: I at the odd and D at the even indices of ``at``, M / = / X elsewhere."""
    return [(("I" if k & 1 else "D") if k in at else "M=X"[k % 3], 1) for k in range(n_ops)]


BLOCK_EDGE_PAIRS = ((256, (0, 63, 64, 255)), (257, (0, 63, 64, 255, 256)), (512, (255, 256, 257, 511)),
                    (513, (0, 63, 512)),      # blocks 0 and 2 hold I/D ops, block 1 none
                    (512, (511,)),            # the only I/D op is the last op of the last block
                    (513, (64, 256, 257, 511, 512)))


def block_edge_batch():
    b = _Builder([3700])
    s = b.scope()
    records = []
    for i, (n_ops, at) in enumerate(BLOCK_EDGE_PAIRS):
        start = 20 + 600 * i
        ops = _edge_cigar(n_ops, at)
        t = b.read([s], s, 0, start, ops)
        n = b.read([s], s, 1, start, ops)
        b.read([s], s, 1, start - 2, [("M", n_ops + 6)])      # covers every position of the pair
        for j, k in enumerate(at):
            # before op k: k - j ops of M / = / X (pos and in_read_pos + 1 each), and the I/D ops
            # before it: an I adds to in_read_pos, a D to pos
            n_i = sum(1 for x in at[:j] if x & 1)
            pos, irp = start + (k - j) + (j - n_i), (k - j) + n_i
            # a D right after an I sits at the I's position: the second call there
            rank = 1 if not k & 1 and k - 1 in at else 0
            records += _tn(0, pos, 1, INS if k & 1 else DEL, rank, (t, irp), [(t, irp), (n, irp)])
    return b.finish(records, 0)


def tsort_threshold_pair():
    """(4096, 4097) unfiltered observations in the one scope."""
    out = []
    for extra in (0, 1):
        b = _Builder([200])
        s = b.scope()
        for _ in range(255):
            b.read([s], s, 0, 10, "1M1I" * 16)               # I at 11..26: tumor only
        t = b.read([s], s, 0, 100, "2M1D" * 8 + "2M")
        n = b.read([s], s, 1, 100, "2M1D" * 8 + "2M")
        if extra:
            b.read([s], s, 0, 50, "3M1I3M")
        records = []
        for k in range(8):      # D k: pos 100 + 3k + 2, in_read_pos 2(k + 1)
            records += _tn(0, 102 + 3 * k, 1, DEL, 0, (t, 2 * k + 2), [(t, 2 * k + 2), (n, 2 * k + 2)])
        arr, e = b.finish(records, THREAD_WALK | (GSORT if extra else TSORT), pos_bits=7, scope_bits=1)
        assert (e.observations, e.emitted, len(e.records)) == (4096 + extra, 16, 24)
        out.append((arr, e))
    return tuple(out)


TSORT_ORDER_GROUPS = (30, None, 40, None, 50)     # None: a scope whose observations the filter removes
TSORT_ORDER_M = 4


def tsort_order_batch():
    """Scopes 0, 2, 4: G positions 4 apart, each with an insertion by M tumor and M normal reads
    (``aM1I3M`` at pos - a, a = 1..M), all listed in descending ref_start; the first position of a scope
    has the offset in its span that the last position of the scope before has. Scopes 1 and 3: tumor
    only."""
    b = _Builder([5000])
    records, m, rel = [], TSORT_ORDER_M, 20
    for s, groups in enumerate(TSORT_ORDER_GROUPS):
        base = 1000 * s
        if groups is None:
            b.scope(0, base, 600)
            b.read([s], s, 0, base + 10, "5M1I5M")
            b.read([s], s, 1, base + 5, "30M")
            continue
        b.scope(0, base, 600)
        ids = {}
        for ds in (0, 1):
            for g in reversed(range(groups)):
                for a in range(1, m + 1):
                    ids[ds, g, a] = b.read([s], s, ds, base + rel + 4 * g - a, [("M", a), ("I", 1), ("M", 3)])
        for g in range(groups):
            # first registered: the lowest ref_start (a = M), tumor before normal
            records += _tn(s, base + rel + 4 * g, 1, INS, 0, (ids[0, g, m], m),
                           [(ids[ds, g, a], a) for ds in (0, 1) for a in range(1, m + 1)])
        rel += 4 * (groups - 1)
    return b.finish(records, THREAD_WALK | TSORT)


def collision_positions(log2_cells: int = 12, lo: int = 200, hi: int = 16000, apart: int = 100):
    """((p1, p2), (p3, p4)): the first two pairs of positions of one cell each, every position more
    than ``apart`` from the others, the two cells different."""
    first: Dict[int, int] = {}
    pairs: List[Tuple[int, int]] = []
    for p in range(lo, hi):
        c = map_cell(p, log2_cells)
        taken = [x for pr in pairs for x in pr]
        if any(abs(p - x) <= apart or map_cell(x, log2_cells) == c for x in taken):
            continue
        q = first.setdefault(c, p)
        if p - q > apart and all(abs(q - x) > apart for x in taken):
            pairs.append((q, p))
            if len(pairs) == 2:
                return pairs[0], pairs[1]
    raise AssertionError("no colliding positions")


def hash_collision_batch():
    (p1, p2), (p3, p4) = collision_positions()
    b = _Builder([16384])
    s = b.scope()
    b.read([s], s, 0, p1 - 5, "5M2D5M")        # r0: tumor only at p1
    b.read([s], s, 1, p2 - 5, "5M2D5M")        # r1: normal only at p2, p1's cell
    t = b.read([s], s, 0, p3 - 5, "5M2D5M")    # r2, r3: the real call
    n = b.read([s], s, 1, p3 - 5, "5M2D5M")
    b.read([s], s, 0, p4 - 5, "5M2D5M")        # r4: tumor only at p4, p3's cell
    b.read([s], s, 1, 2, "16000M")
    arr, e = b.finish(_tn(0, p3, 2, DEL, 0, (t, 5), [(t, 5), (n, 5)]), THREAD_WALK | TSORT | HASHED | 12 << 8,
                      pairs=((p1, p2), (p3, p4)))
    # dense: the real call's two; hashed: + the colliding pair + the third position
    assert (e.observations, e.emitted_dense, e.emitted) == (5, 2, 2 + 2 + 1)
    return arr, e


RUN_CHUNK_OPS = 2100


def run_chunk_batch():
    b = _Builder([7100])
    s0, s1, s2 = b.scope(), b.scope(), b.scope()
    t = b.read([s0], s0, 0, 10, "3M1I" * RUN_CHUNK_OPS)
    n = b.read([s0], s0, 1, 10, "3M1I" * RUN_CHUNK_OPS)
    # a third observation at the first position: every later run of two starts at an odd element. It
    # also covers the last insertion, at the pair's reference_end
    b.read([s0], -1, 1, 10, "3M1I6310M")
    records = []
    for i in range(RUN_CHUNK_OPS):      # I i: pos 10 + 3(i + 1), in_read_pos 4i + 3
        records += _tn(0, 13 + 3 * i, 1, INS, 0, (t, 4 * i + 3), [(t, 4 * i + 3), (n, 4 * i + 3)])
    b.read([s1], s1, 0, 7000, "5M1I5M")         # scope 1: one filtered observation (scope 2's r4 marks 7005)
    b.read([s2], s2, 1, 7000, "5M1I5M")         # scope 2: one, two and two observations at 7005, 7025, 7030
    t2 = b.read([s2], s2, 0, 7020, "5M1I5M1I5M")
    n2 = b.read([s2], s2, 1, 7020, "5M1I5M1I5M")
    records += _tn(2, 7025, 1, INS, 0, (t2, 5), [(t2, 5), (n2, 5)]) + _tn(2, 7030, 1, INS, 0, (t2, 11), [(t2, 11), (n2, 11)])
    arr, e = b.finish(records, 0)
    assert (e.observations, e.emitted, len(e.records)) == (4207, 4207, 6306)
    return arr, e


COVER_SIZES = (7, 8, 9, 16, 17)
COVER_VARIANTS = ("ends_at_pos", "ends_past_pos", "starts_at_pos")


def normal_cover_batch():
    """Per size and variant a scope: a tumor and a normal read with a trailing insertion at pos (their
    own reference_end), filler reads that do not cover pos, and last the plain normal read that may.
    Then a scope whose only covering normal read is listed by another scope."""
    b = _Builder([40 * (len(COVER_SIZES) * len(COVER_VARIANTS) + 1) + 40])
    records, covered = [], {}
    for size in COVER_SIZES:
        for v, variant in enumerate(COVER_VARIANTS):
            s = b.scope()
            pos = 40 * s + 20
            t = b.read([s], s, 0, pos - 5, "5M1I")
            n = b.read([s], s, 1, pos - 5, "5M1I")
            for i in range(size - 3):
                b.read([s], s, i & 1, pos - 8, "8M")          # ends at pos
            b.read([s], s, 1, *((pos - 4, "4M"), (pos - 4, "5M"), (pos, "3M"))[v])
            covered[s] = v > 0
            if v:
                records += _tn(s, pos, 1, INS, 0, (t, 5), [(t, 5), (n, 5)])
    s = b.scope()
    other = b.scope()
    pos = 40 * s + 20
    b.read([s], s, 0, pos - 5, "5M1I")
    b.read([s], s, 1, pos - 5, "5M1I")
    b.read([other], other, 1, pos - 4, "8M")
    covered[s] = False
    return b.finish(records, THREAD_WALK | TSORT, covered=covered)


_CASES = None


def all_cases() -> Dict[str, Tuple[Dict[str, np.ndarray], Expect]]:
    """Every batch by name, built once; the arrays are read-only."""
    global _CASES
    if _CASES is None:
        w32, w33 = walk_threshold_pair()
        t4096, t4097 = tsort_threshold_pair()
        k255, k256 = key_edge_pair()
        tumor_only, single = nothing_left_pair()
        _CASES = {
            "cigar_arith": cigar_arith_batch(), "walk_32": w32, "walk_33": w33, "block_edge": block_edge_batch(),
            "tsort_4096": t4096, "tsort_4097": t4097, "tsort_order": tsort_order_batch(),
            "hash_collision": hash_collision_batch(), "two_contig": two_contig_batch(), "run_chunk": run_chunk_batch(),
            "normal_cover": normal_cover_batch(), "rank": rank_batch(), "indel_csr": indel_csr_batch(),
            "key_edge_255": k255, "key_edge_256": k256, "nothing_tumor_only": tumor_only, "nothing_single": single,
        }
        for arr, _ in _CASES.values():
            for a in arr.values():
                a.setflags(write=False)
    return _CASES
