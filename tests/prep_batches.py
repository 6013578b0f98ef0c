"""Hand-built batches for the device prep (genomeanonymizer_amd/csrc/ganon_prep.hip), a plain
restatement of what its plan must find, and 32-bit models of its two counting CIGAR walks.

Used by tests/test_prep_batches.py (CPU: pins the batches and the restatement to the C oracle and
to literal values) and tests/test_gpu_prep.py (the device plan, its validation and its results).

``plan_reference`` is written from the text of include/ganon.h and DESIGN §4a with Python's
unbounded ints; nothing here calls the package except for the array layout (nt16 codes, nibble
packing). Every builder returns the array dict of ``genomeanonymizer_amd.synth.batch`` plus an info
dict; reference nibble = contig position in all of them.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np

from genomeanonymizer_amd.synth.batch import ACGT, pack_nibbles

OPS = "MIDNSHP=X"
SEG_MAX = (1 << 14) - 1        # longer aligned runs are cut
FUSED_MAX_SEG = 8              # most aligned segments of a read in the fused mode
LONG_CIGAR = 48                # reads with more CIGAR ops are walked by a wave
HUGE_SPAN = 1 << 20            # wider scopes take the tile path
LONG_READ_LEN = 1000           # auto prep: long-read mode above this read length (with several segments)
MAX_READ_LEN = 1 << 24
INT32_MAX = (1 << 31) - 1
SCAN_BLOCK = 1024              # reads, and scopes, per block of the scan
STRIPES = 64                   # allocation counters of the extras list
STRIPE_XREC_INIT = 64 * 30     # extras capacity at which exactly one stripe of stripe_batch() overflows

ERR_TEXT = {
    "seq": "read {i}: sequence out of range",
    "cigar": "read {i}: cigar out of range",
    "dataset": "read {i}: dataset must be 0 or 1",
    "write_scope": "read {i}: write_scope {a} out of range",
    "long": "read {i} longer than 16 Mb",
    "op": "read {i}: bad cigar op {a}",
    "pos": "read {i}: bad position",
    "scope_off": "scope {i}: incidence offsets decreasing or out of range",
    "scope_span": "scope {i}: bad span",
    "scope_ref": "scope {i}: reference slice out of range",
    "scope_keep": "scope {i}: keep_code > 15",
    "incid_read": "incidence {i}: read {a} out of range",
    "incid_span": "scope {i}: read ",
    "ws_missing": "read {i}: write_scope {a} does not list it exactly once",
}


def cw(op: str, n: int) -> int:
    return (n << 4) | OPS.index(op)


def words(ops) -> List[int]:
    return [cw(o, n) for o, n in ops]


# ---- the walks -------------------------------------------------------------------------------
def walk_unbounded(cig, L: int, ref_start: int):
    """One read's CIGAR with unbounded ints: (segments [(q, pos, n)] cut at SEG_MAX and clipped to
    the read length L, reference length, I/D ops, first bad op as (index, code) or None)."""
    q, p, rl, nid, segs = 0, ref_start, 0, 0, []
    for k, w in enumerate(cig):
        op, n = int(w) & 15, int(w) >> 4
        if op > 8:
            return segs, rl, nid, (k, op)
        if op in (0, 7, 8):
            if q < L:
                m = min(n, L - q)
                for o in range(0, m, SEG_MAX):
                    segs.append((q + o, p + o, min(SEG_MAX, m - o)))
            q += n
            p += n
            rl += n
        elif op in (1, 4):
            q += n
        elif op in (2, 3):
            p += n
            rl += n
        nid += op in (1, 2)
    return segs, rl, nid, None


def _i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _cdiv(a: int, b: int) -> int:
    """C's integer division (truncation toward zero)."""
    s = -1 if (a < 0) != (b < 0) else 1
    return s * (abs(a) // abs(b))


def scan_walk_i32(cig, L: int, saturate: bool = True):
    """k_prep_scan's per-thread walk (reads of at most LONG_CIGAR ops) with its 32-bit ``int q``:
    (segments counted, I/D ops, reference length, first segment (q, reference offset, n) or None).
    ``saturate`` False: the walk as it was, the offset advancing past the read length and wrapping."""
    q = ns = nid = rl = 0
    first = None
    for w in cig:
        op, n = int(w) & 15, int(w) >> 4
        if op > 8:
            return None
        if op in (0, 7, 8):
            if q < L:
                m = min(n, _i32(L - q))
                if ns == 0:
                    first = (q, rl, min(m, SEG_MAX))
                ns = _i32(ns + _cdiv(_i32(m + SEG_MAX - 1), SEG_MAX))
                if saturate:
                    q = _i32(q + n)
            if not saturate:
                q = _i32(q + n)
            rl += n
        elif op in (1, 4):
            if not saturate or q < L:
                q = _i32(q + n)
        elif op in (2, 3):
            rl += n
        nid += op in (1, 2)
    return ns, nid, rl, (first if ns else None)


def wave_walk_i32(cig, L: int, saturate: bool = True):
    """wave_cigar_walk (reads of more than LONG_CIGAR ops): 64 ops per trip, the query offsets from a
    32-bit prefix sum over the lanes: (segments counted, I/D ops, reference length), or None after
    an op code above 8. ``saturate`` False: the walk as it was (uncapped deltas, wrapping carry)."""
    q = seg = nid = rl = 0
    cig = [int(w) for w in cig]
    for base in range(0, len(cig), 64):
        chunk = cig[base:base + 64]
        if any((w & 15) > 8 for w in chunk):
            return None
        incl = 0
        for w in chunk:
            op, n = w & 15, w >> 4
            al = op in (0, 7, 8)
            dq = (min(n, L) if saturate else n) if (al or op in (1, 4)) else 0
            incl = _i32(incl + dq)
            q0 = _i32(q + incl - dq)
            if al and q0 < L:
                seg = _i32(seg + _cdiv(_i32(min(n, _i32(L - q0)) + SEG_MAX - 1), SEG_MAX))
            nid += op in (1, 2)
            rl += n if (al or op in (2, 3)) else 0
        q = min(_i32(q + incl), L) if saturate else _i32(q + incl)
    return seg, nid, rl


# ---- the plan, restated -------------------------------------------------------------------------
def _cig_of(arr, r):
    o, n = int(arr["cig_off"][r]), int(arr["n_cig"][r])
    return [int(w) for w in arr["cigar"][o:o + n]]


def first_error(arr: Dict[str, np.ndarray]) -> Optional[Tuple[str, int, int]]:
    """The batch's validation error as (kind, index, detail), or None: the per-read checks, the CIGAR
    walks, the per-scope checks (all made by the plan), then the incidence checks and the write-scope
    check (made by the run, reported by the download). Each hand-built invalid batch has one."""
    n_reads, n_scopes = len(arr["read_len"]), len(arr["scope_span_len"])
    seq_bytes, n_ops, n_incid = len(arr["seq_nt16"]), len(arr["cigar"]), len(arr["incid_read"])
    ref_nibs = 2 * len(arr["ref_nt16"])
    for r in range(n_reads):
        L, so = int(arr["read_len"][r]), int(arr["seq_off"][r])
        nc, co = int(arr["n_cig"][r]), int(arr["cig_off"][r])
        ws = int(arr["write_scope"][r])
        if L < 0 or so < 0 or so + (L + 1) // 2 > seq_bytes:
            return "seq", r, 0
        if nc < 0 or co < 0 or co + nc > n_ops:
            return "cigar", r, 0
        if int(arr["dataset"][r]) > 1:
            return "dataset", r, 0
        if ws < -1 or ws >= n_scopes:
            return "write_scope", r, ws
        if L >= MAX_READ_LEN:
            return "long", r, 0
    ends = []
    for r in range(n_reads):
        rs = int(arr["ref_start"][r])
        _, rl, _, bad = walk_unbounded(_cig_of(arr, r), int(arr["read_len"][r]), rs)
        if bad:
            return "op", r, bad[1]
        if rs < 0 or rs + rl > INT32_MAX:
            return "pos", r, 0
        ends.append(rs + (rl if rl > 0 else 1))
    off = [int(x) for x in arr["scope_incid_off"]]
    for s in range(n_scopes):
        i0, i1 = off[s], off[s + 1]
        if i0 < 0 or i1 < i0 or i1 > n_incid:
            return "scope_off", s, 0
        ss, sl = int(arr["scope_span_start"][s]), int(arr["scope_span_len"][s])
        if ss < 0 or sl < 0:
            return "scope_span", s, 0
        ro = int(arr["scope_ref_off"][s])
        if ro < 0 or ro + sl > ref_nibs:
            return "scope_ref", s, 0
        if int(arr["keep_code"][s]) > 15:
            return "scope_keep", s, 0
    listed = [0] * n_reads
    for s in range(n_scopes):
        ss = int(arr["scope_span_start"][s])
        se = ss + int(arr["scope_span_len"][s])
        for i in range(off[s], off[s + 1]):
            r = int(arr["incid_read"][i])
            if r < 0 or r >= n_reads:
                return "incid_read", i, r
            if int(arr["ref_start"][r]) < ss or ends[r] > se:
                return "incid_span", s, 0       # (which of the scope's reads is named is not fixed)
            listed[r] += int(arr["write_scope"][r]) == s
    for r in range(n_reads):
        if int(arr["write_scope"][r]) >= 0 and listed[r] != 1:
            return "ws_missing", r, int(arr["write_scope"][r])
    return None


def error_text(err: Tuple[str, int, int]) -> str:
    """What the raised error's message must contain."""
    return ERR_TEXT[err[0]].format(i=err[1], a=err[2])


def expected_mode(max_seg: int, max_len: int, n_long_cigar: int, params: Optional[dict] = None) -> str:
    """The prep mode ganon_batch_shape must report for a full plan. From include/ganon.h:
    GANON_PARAM_PREP_LONG 1 is always the long-read prep; -1 (auto) takes it when a read has more
    than one segment and reads are longer than 1000 bases. Otherwise, with PREP_LONG -1 or 2, the
    one-segment prep applies when no read has more than one segment — and, GANON_PARAM_FUSED_FLAT 1,
    the fused mode when no read has more than 8 segments nor more than 48 CIGAR ops (mode 4 when a
    read has 2-8 segments, 3 else). Everything else is the two-pass emit."""
    p = {"PREP_LONG": -1, "FUSED_FLAT": 1}
    p.update(params or {})
    if p["PREP_LONG"] == 1 or (p["PREP_LONG"] == -1 and max_seg > 1 and max_len > LONG_READ_LEN):
        return "long_read"
    if p["PREP_LONG"] in (-1, 2):
        if p["FUSED_FLAT"] and n_long_cigar == 0 and max_seg <= FUSED_MAX_SEG:
            return "multi_segment_fused" if max_seg > 1 else "one_segment_fused"
        if max_seg <= 1:
            return "one_segment"
    return "two_pass"


def plan_reference(arr: Dict[str, np.ndarray], group_target: int = 704, params: Optional[dict] = None) -> dict:
    """What the device plan must find (see the module docstring). ``group_target``: cost units per
    short-read group (the long-read prep's default is 2816 unless params sets GROUP_TARGET).
    An invalid batch: {"invalid": (kind, index, detail)} only."""
    err = first_error(arr)
    if err:
        return {"invalid": err}
    params = dict(params or {})
    n_reads, n_scopes = len(arr["read_len"]), len(arr["scope_span_len"])
    reads = []
    for r in range(n_reads):
        rs = int(arr["ref_start"][r])
        segs, rl, nid, _ = walk_unbounded(_cig_of(arr, r), int(arr["read_len"][r]), rs)
        reads.append({"read_end": rs + (rl if rl > 0 else 1), "segments": segs, "id_ops": nid})
    max_len = max([int(x) for x in arr["read_len"]], default=0)
    max_seg = max([len(x["segments"]) for x in reads], default=0)
    n_long = sum(int(x) > LONG_CIGAR for x in arr["n_cig"])
    mode = expected_mode(max_seg, max_len, n_long, params)
    off = [int(x) for x in arr["scope_incid_off"]]
    n_incid = off[-1]
    # short-read groups (ganon.h): the scopes whose cost prefix, incidences before the
    # scope + weight per scope before it, falls in one bucket of `target` units; the weight keeps a
    # group to 256 scopes
    target = params.get("GROUP_TARGET") or group_target
    weight = -(-target // 255)
    groups = bound = 0
    if n_scopes:
        groups = (off[n_scopes - 1] + weight * (n_scopes - 1)) // target + 1
        bound = (n_incid + weight * (n_scopes - 1)) // target + 1
    if mode == "long_read" and n_scopes:
        # long-read groups: cut on the prefix of (aligned segments of the scope's incidences + weight)
        lt = params.get("GROUP_TARGET") or 2816
        lw = -(-lt // 255)
        prefix = 0
        for s in range(n_scopes - 1):
            prefix += lw + sum(len(reads[int(arr["incid_read"][i])]["segments"]) for i in range(off[s], off[s + 1]))
        planned = prefix // lt + 1
    elif mode == "two_pass":
        planned = groups
    else:
        planned = bound        # one-segment modes launch for the bound (ganon_batch_info's text)
    return {
        "invalid": None, "reads": reads,
        "id_ops": sum(x["id_ops"] for x in reads), "max_len": max_len, "max_seg": max_seg,
        "written_reads": int((arr["write_scope"] >= 0).sum()),
        "huge_scopes": sum(int(x) > HUGE_SPAN for x in arr["scope_span_len"]),
        "groups": groups, "group_bound": bound, "planned_groups": planned, "long_cigars": n_long, "prep_mode": mode,
    }


# ---- assembling arrays -------------------------------------------------------------------------
def _other(code: int, k: int = 1) -> int:
    code = int(code)
    return int(ACGT[((code.bit_length() - 1) + k) % 4]) if code in (1, 2, 4, 8) else int(ACGT[k % 4])


class Batch:
    """Reads (position, CIGAR words, nt16 codes, dataset, write scope) and scopes (read list, span)
    gathered into the array dict; the buffers follow the order of ``storage`` (default: read order)."""

    def __init__(self, ref: np.ndarray):
        self.ref = ref
        self.reads: List[dict] = []
        self.scopes: List[dict] = []

    def read(self, pos, cig, codes, ds, ws=-1) -> int:
        self.reads.append({"pos": pos, "cig": [int(w) for w in cig], "codes": np.asarray(codes, np.uint8), "ds": ds, "ws": ws})
        return len(self.reads) - 1

    def scope(self, reads, start, length, keep=None) -> int:
        self.scopes.append({"reads": list(reads), "start": start, "len": length, "keep": keep})
        return len(self.scopes) - 1

    def arrays(self, storage=None, seq_pad: int = 0) -> Dict[str, np.ndarray]:
        n = len(self.reads)
        order = list(range(n)) if storage is None else list(storage)
        seq_off, cig_off = np.zeros(n, np.int64), np.zeros(n, np.int64)
        seq, cig = [], []
        sb = cb = 0
        for r in order:
            x = self.reads[r]
            seq_off[r], cig_off[r] = sb, cb
            pk = pack_nibbles(x["codes"]) if len(x["codes"]) else np.zeros(0, np.uint8)
            seq.append(pk)
            cig.append(np.array(x["cig"], np.uint32))
            sb += len(pk)
            cb += len(x["cig"])
        if seq_pad:
            seq.append(np.zeros(seq_pad, np.uint8))
        offs, incid = [0], []
        for s in self.scopes:
            incid += s["reads"]
            offs.append(len(incid))
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        return {
            "ref_start": np.array([x["pos"] for x in self.reads], np.int32),
            "read_len": np.array([len(x["codes"]) for x in self.reads], np.int32),
            "seq_off": seq_off, "seq_nt16": cat(seq, np.uint8),
            "cig_off": cig_off, "n_cig": np.array([len(x["cig"]) for x in self.reads], np.int32),
            "cigar": cat(cig, np.uint32),
            "dataset": np.array([x["ds"] for x in self.reads], np.uint8),
            "write_scope": np.array([x["ws"] for x in self.reads], np.int32),
            "scope_incid_off": np.array(offs, np.int64), "incid_read": np.array(incid, np.int32),
            "scope_span_start": np.array([s["start"] for s in self.scopes], np.int32),
            "scope_span_len": np.array([s["len"] for s in self.scopes], np.int32),
            "scope_ref_off": np.array([s["start"] for s in self.scopes], np.int64),
            "ref_nt16": pack_nibbles(self.ref),
            "keep_pos": np.array([s["keep"][0] if s["keep"] else -1 for s in self.scopes], np.int32),
            "keep_code": np.array([s["keep"][1] if s["keep"] else 0 for s in self.scopes], np.uint8),
        }


def case_codes(ref: np.ndarray, pos: int, cig, L: int):
    """Bases of a read that equals the reference along its aligned segments except for an alt at
    the first and the last base of every segment; bases outside the segments (clips, insertions,
    bases past the CIGAR) differ from the reference base they would meet if they were aligned at
    pos + q. Returns (codes, segments, alt query positions)."""
    segs, _, _, _ = walk_unbounded(cig, L, pos)
    codes = np.array([_other(ref[(pos + q) % len(ref)], 2) for q in range(L)], np.uint8)
    alts = []
    for q, p, n in segs:
        codes[q:q + n] = ref[p:p + n]
        for o in {0, n - 1}:
            codes[q + o] = _other(ref[p + o], 1)
            alts.append(q + o)
    return codes, segs, sorted(alts)


def add_case(b: Batch, cases: list, name: str, ops, L: Optional[int] = None, pos: Optional[int] = None) -> int:
    """A tumor and a normal read with the same CIGAR and bases in a scope of their own that fits
    them exactly (span = [ref_start, read_end)): every alt is in both datasets, so the oracle masks
    it in both reads iff the segment under it is where the CIGAR puts it."""
    cig = words(ops)
    qlen = sum(n for o, n in ops if o in "MIS=X")
    L = qlen if L is None else L
    pos = b.cursor if pos is None else pos
    segs, rl, nid, _ = walk_unbounded(cig, L, pos)
    end = pos + (rl if rl > 0 else 1)
    codes, segs, alts = case_codes(b.ref, pos, cig, L)
    s = len(b.scopes)
    r0 = b.read(pos, cig, codes, 0, s)
    r1 = b.read(pos, cig, codes, 1, s)
    b.scope([r0, r1], pos, end - pos)
    b.cursor = end + 32 + (-end) % 16 + len(cases) % 16
    cases.append({"name": name, "reads": (r0, r1), "scope": s, "ops": list(ops), "L": L, "pos": pos,
                  "segments": segs, "read_end": end, "id_ops": nid, "alts": alts})
    return s


def _new_batch(ref_len: int, seed: int) -> Batch:
    rng = np.random.default_rng(seed)
    b = Batch(ACGT[rng.integers(0, 4, ref_len)])
    b.cursor = 64
    return b


def _finish(b: Batch, cases: list, **kw):
    assert b.cursor + 64 <= len(b.ref), (b.cursor, len(b.ref))
    arr = b.arrays(**kw)
    masked = sorted((r, q) for c in cases for r in c["reads"] for q in c["alts"])
    return arr, {"cases": cases, "masked": masked}


def many_ops(n: int, id_lanes=(), bad=None) -> list:
    """An ``n``-op CIGAR of 3-base M ops, with a 2-base I (even lane) or D (odd lane) at ``id_lanes``."""
    ops = [("M", 3)] * n
    for k in id_lanes:
        ops[k] = ("D", 2) if k % 2 else ("I", 2)
    return ops


def query_before(ops, lane: int) -> int:
    return sum(n for o, n in ops[:lane] if o in "MIS=X")


def cigar_matrix_batch() -> Dict[str, Tuple[Dict[str, np.ndarray], dict]]:
    """The CIGAR walk edges, one case (a tumor/normal pair in its own scope) each, in sub-batches by
    the mode a default plan gives them:
    ``one_segment`` (one_segment_fused), ``multi_segment`` (multi_segment_fused: 2..8 segments, at
    most 48 ops, short), ``many_segments`` (two_pass: 9 and more segments, 48 ops), ``long_cigar``
    (two_pass: 49..129 ops, the wave walk) and ``long_runs`` (long_read: aligned runs around the
    16,383 cut). info: ``cases`` and ``masked``, the (read, query position) pairs the oracle must mask."""
    out = {}
    # -- at most one aligned segment
    b, cs = _new_batch(80_000, 1), []
    for name, ops, L in [
        ("M", [("M", 20)], None), ("eq", [("=", 12)], None), ("X", [("X", 12)], None),
        ("S_M_S", [("S", 3), ("M", 20), ("S", 4)], None), ("H_M_H", [("H", 5), ("M", 20), ("H", 5)], None),
        ("zero_length_ops", [("M", 0), ("S", 0), ("I", 0), ("M", 20), ("D", 0), ("P", 0), ("N", 0)], None),
        ("no_cigar", [], 5), ("no_cigar_no_bases", [], 0), ("all_soft_clip", [("S", 12)], None),
        ("query_shorter_than_L", [("M", 10)], 15), ("query_equals_L", [("M", 10), ("S", 5)], 15),
        ("clip_mid_op", [("M", 20)], 12), ("clip_at_border", [("M", 10), ("S", 5)], 10),
        ("clip_at_border_then_M", [("M", 10), ("I", 2), ("M", 10)], 12), ("clip_after_insert", [("M", 10), ("I", 2), ("M", 10)], 10),
        ("starts_at_L", [("S", 8), ("M", 10)], 8), ("starts_past_L", [("S", 8), ("M", 10)], 5),
        ("lead_D15", [("D", 15), ("M", 20)], None), ("lead_D16", [("D", 16), ("M", 20)], None),
        ("lead_N15", [("N", 15), ("M", 20)], None), ("lead_N16", [("N", 16), ("M", 20)], None),
        ("trail_D15", [("M", 20), ("D", 15)], None), ("trail_D16", [("M", 20), ("D", 16)], None),
        ("clipped_tail_15", [("M", 35)], 20), ("clipped_tail_16", [("M", 36)], 20),
        ("M_I", [("M", 20), ("I", 3)], None), ("M_D_S", [("M", 20), ("D", 3), ("S", 2)], None),
        ("one_base", [("M", 1)], None), ("run_16382", [("M", 16382)], None), ("run_16383", [("M", 16383)], None),
        ("run_16384_clipped_to_16383", [("M", 16384)], 16383),
    ]:
        add_case(b, cs, name, ops, L)
    out["one_segment"] = _finish(b, cs)
    # -- 2..8 segments, short reads, at most 48 ops
    b, cs = _new_batch(8_000, 2), []
    eight = [("M", 10), ("D", 1)] * 7 + [("M", 10)]
    for name, ops, L in [
        ("every_op", [("S", 2), ("M", 8), ("I", 2), ("M", 8), ("D", 3), ("M", 8), ("N", 5), ("M", 8), ("H", 3),
                      ("=", 6), ("P", 2), ("X", 6), ("S", 1)], None),
        ("two_segments", [("M", 10), ("I", 2), ("M", 10)], None),
        ("two_segments_P", [("M", 10), ("P", 4), ("M", 10)], None),
        ("adjacent_eq_X", [("=", 10), ("X", 5)], None),
        ("clip_mid_second", [("M", 10), ("I", 2), ("M", 10)], 15),
        ("clip_at_third", [("M", 5), ("D", 1), ("M", 5), ("D", 1), ("M", 5)], 10),
        ("eight_segments", eight, None),
        ("eight_segments_48_ops", eight + [("P", 1)] * 33, None),
        ("eight_segments_clipped", eight + [("I", 1), ("M", 10)], 80),
        ("lead_D16_two", [("D", 16), ("M", 10), ("N", 20), ("M", 10)], None),
        ("trail_D16_two", [("M", 10), ("I", 1), ("M", 10), ("D", 16)], None),
    ]:
        add_case(b, cs, name, ops, L)
    out["multi_segment"] = _finish(b, cs)
    # -- more than 8 segments, at most 48 ops: the thread walk, no fused mode
    b, cs = _new_batch(8_000, 3), []
    m48 = many_ops(48, id_lanes=(0, 47))
    for name, ops, L in [
        ("nine_segments", [("M", 16), ("I", 1)] * 8 + [("M", 14)], None),
        ("ops_48", many_ops(48), None), ("ops_48_id_0_47", m48, None),
        ("ops_48_clip_47", many_ops(48), query_before(many_ops(48), 47) + 1),
        ("ops_48_clip_0", many_ops(48), 1),
    ]:
        add_case(b, cs, name, ops, L)
    out["many_segments"] = _finish(b, cs)
    # -- more than 48 ops: the wave walk, 64 ops per trip
    b, cs = _new_batch(40_000, 4), []
    for n in (49, 64, 65, 128, 129):
        lanes = [k for k in (0, 63, 64, 127, 128) if k < n]
        add_case(b, cs, f"ops_{n}", many_ops(n), None)
        add_case(b, cs, f"ops_{n}_id", many_ops(n, id_lanes=lanes), None)
        for k in lanes[:3]:
            ops = many_ops(n)
            add_case(b, cs, f"ops_{n}_clip_mid_{k}", ops, query_before(ops, k) + 1)
            if k:
                add_case(b, cs, f"ops_{n}_clip_at_{k}", ops, query_before(ops, k))
    out["long_cigar"] = _finish(b, cs)
    # -- aligned runs around the 16,383 cut
    b, cs = _new_batch(300_000, 5), []
    for name, ops, L in [
        ("run_16382", [("M", 16382)], None), ("run_16383", [("M", 16383)], None), ("run_16384", [("M", 16384)], None),
        ("run_32766", [("M", 32766)], None), ("run_32767", [("M", 32767)], None),
        ("run_32767_clipped_16384", [("M", 32767)], 16384),
        ("S_run_16384_I_run_16383", [("S", 5), ("M", 16384), ("I", 3), ("M", 16383)], None),
    ]:
        add_case(b, cs, name, ops, L)
    out["long_runs"] = _finish(b, cs)
    return out


def overflow_cigar_batch() -> Dict[str, tuple]:
    """Short reads whose query-consuming op lengths sum past 2^31 (each op holds up to 2^28 - 1), in
    two sub-batches: ``thread`` (at most 48 ops: the scan's per-thread walk, the fused mode) and
    ``wave`` (more: the wave walk). Each is (arrays, twin arrays, info): the twin holds the same
    reads with each CIGAR cut where q >= L, which is where walk_segments stops — later ops that
    consume the query only keep their code with length 0, later aligned ops become N ops of the same
    length — so both batches have the same sizes, ends, I/D ops and expected result. Only the twin
    is for the per-base C oracle."""
    big = (1 << 28) - 1
    specs = {"thread": [
        ("nine_S_then_M", [("M", 20)] + [("S", big)] * 9 + [("M", 7)], 20),
        ("M_after_the_wrap", [("S", 4), ("M", 16)] + [("I", big)] * 8 + [("S", 40)] + [("M", 9)], 20),
        ("two_segments_then_wrap_to_4", [("M", 10), ("D", 2), ("M", 10)] + [("S", big)] * 16 + [("M", 5)], 20),
        ("aligned_ops_after_the_wrap", [("M", 20)] + [("S", big)] * 8 + [("S", 8), ("M", 30), ("M", 30)], 20),
        ("no_segment_before_the_wrap", [("S", 20)] + [("S", big)] * 8 + [("M", 9)], 20),
    ], "wave": [
        ("wave_49_ops", [("M", 12), ("I", 1), ("M", 7)] + [("S", big)] * 9 + [("P", 1)] * 36 + [("M", 4)], 20),
        ("wave_wrap_within_one_trip", many_ops(6) + [("I", big)] * 16 + [("M", 3)] * 30, 18),
        ("wave_carry_wraps", many_ops(6) + [("S", 1 << 26)] * 63 + [("S", (1 << 26) - 10)] + [("M", 3)] * 50, 18),
    ]}
    out = {}
    for key, sp in specs.items():
        pair = []
        for cut in (False, True):
            b, cs = _new_batch(4_000, 6), []
            for name, ops, L in sp:
                if cut:
                    q, kept = 0, []
                    for o, n in ops:
                        kept.append((o, n) if q < L else (o, 0) if o in "IS" else ("N", n) if o in "M=X" else (o, n))
                        q += n if o in "MIS=X" else 0
                    ops = kept
                add_case(b, cs, name, ops, L)
            pair.append(_finish(b, cs))
        (arr, info), (twin, tinfo) = pair
        assert info["masked"] == tinfo["masked"]
        out[key] = (arr, twin, info)
    return out


def block_border_batch(n_reads: int, n_scopes: int, eight: bool = False):
    """``n_reads`` reads of which only the ones at block-relative slots 0, 255, 256, 767, 1023 of each
    scan block and the batch's last read are in scopes, written, have I/D ops, several segments
    and more than 12 bases: special j has 2 + j % 7 segments, j + 1 I/D ops and 40 + 3 (j + 1)
    bases — the sums and maxima come out right only if every slot is visited exactly once.
    The others are 12M reads outside every scope. All ``n_scopes`` scopes share one span."""
    rng = np.random.default_rng(n_reads * 7 + n_scopes)
    ref = ACGT[rng.integers(0, 4, 1024)]
    b = Batch(ref)
    pos, span = 64, 256
    slots = sorted({k + s for k in range(0, n_reads, SCAN_BLOCK) for s in (0, 255, 256, 767, 1023) if k + s < n_reads}
                   | {n_reads - 1})
    plain = np.array(ref[pos:pos + 12], np.uint8)
    by_scope = [[] for _ in range(n_scopes)]
    specials = []
    for r in range(n_reads):
        if r not in slots:
            b.read(pos, [cw("M", 12)], plain, r & 1)
            continue
        j = len(specials)
        nseg, nid = 2 + j % 7, j + 1
        ops = []
        for k in range(nseg - 1):        # the joins: I / D ops while the read has some left, then N
            ops += [("M", 4), (("D" if k % 2 else "I") if k < nid else "N", 1)]
        ops += [("M", 4)] + [("I", 1)] * max(0, nid - (nseg - 1))
        L = 40 + 3 * (j + 1)
        ops += [("S", L - sum(n for o, n in ops if o in "MIS=X"))]
        codes, _, _ = case_codes(ref, pos, words(ops), L)
        s = (j * 37) % n_scopes
        b.read(pos, words(ops), codes, j & 1, s)
        by_scope[s].append(r)
        specials.append(r)
    for s in range(n_scopes):
        b.scope(by_scope[s], pos, span)
    return b.arrays(), {"specials": specials}


def eight_segment_block_batch():
    """1,030 reads (a full scan block and six more), every one of 8 aligned segments, as tumor /
    normal pairs with alts at every segment end: the block's LDS list of multi-segment reads is full
    (1,024 entries, 8,192 records: both below the packed 16-bit counters' 65,535)."""
    b, cs = _new_batch(120_000, 8), []
    for k in range(515):
        add_case(b, cs, f"pair_{k}", [("M", 4), ("I", 1)] * 7 + [("M", 4)], None)
    return _finish(b, cs)


def stripe_batch(n_reads: int = 66_000, per_block: int = 10):
    """``n_reads`` reads in 65 scan blocks: blocks 0 and 64 share stripe 0 of the extras list. The
    first ``per_block`` reads of every block are two-segment tumor / normal pairs with alts (2
    extras records each); the others are 12M reads outside every scope. With an extras capacity of
    64 * 3 * per_block records exactly stripe 0 (4 * per_block records) overflows."""
    b, cs = _new_batch(40_000, 9), []
    plain = np.array(b.ref[64:76], np.uint8)
    for r0 in range(0, n_reads, SCAN_BLOCK):
        for k in range(per_block // 2):
            add_case(b, cs, f"block_{r0 // SCAN_BLOCK}_{k}", [("M", 10), ("D", 2), ("M", 10)], None)
        for r in range(r0 + per_block, min(r0 + SCAN_BLOCK, n_reads)):
            b.read(64, [cw("M", 12)], plain, r & 1)
    arr, info = _finish(b, cs)
    info["xrec_init"] = STRIPES * 3 * per_block      # (STRIPE_XREC_INIT for the default per_block)
    return arr, info


def group_table_batch(single: bool = False, tail: int = 0):
    """Scopes by incidence count: none at the front, in the middle and at the end; one with 2,000
    (several buckets of any target up to 704 skipped: empty groups); more than 256 empty scopes in a
    row (only the weight cuts them). ``single``: one scope. Every scope spans the same 64 positions;
    two reads of each listed scope carry a both-dataset alt and are written. ``tail``: one more scope
    with that many incidences at the end (the group bound then exceeds the group count)."""
    counts = [5] if single else [0, 0, 3, 2000, 0, 5, 2] + [0] * 300 + [4, 0, 6] + [0] * 700 + [2, 0, 0]
    counts += [tail] if tail else []
    rng = np.random.default_rng(10)
    ref = ACGT[rng.integers(0, 4, 512)]
    b = Batch(ref)
    pos = 64
    plain = np.array(ref[pos:pos + 20], np.uint8)
    alt = plain.copy()
    alt[7] = _other(ref[pos + 7], 1)
    for s, c in enumerate(counts):
        ids = []
        for k in range(c):
            ids.append(b.read(pos, [cw("M", 20)], alt if k < 2 else plain, k & 1, s if k < 2 else -1))
        b.scope(ids, pos, 64)
    return b.arrays(), {"counts": counts}


# ---- the gate of a speculative run ------------------------------------------------------------------
GATE_REASONS = ("segments", "read_length", "huge_scope", "long_cigar", "extras")
GATE_XREC_INIT = 64 * 8      # extras capacity of the gate batches: 8 records per stripe


def _add_pair(b: Batch, name: str, ops_t, ops_n, span_len: Optional[int] = None) -> None:
    """A tumor and a normal read (their own CIGARs, alts at every segment end) in a scope of their own."""
    pos, s, ids, end = b.cursor, len(b.scopes), [], b.cursor + 1
    for d, ops in ((0, ops_t), (1, ops_n)):
        cig = words(ops)
        L = sum(n for o, n in ops if o in "MIS=X")
        codes, _, _ = case_codes(b.ref, pos, cig, L)
        _, rl, _, _ = walk_unbounded(cig, L, pos)
        end = max(end, pos + rl)
        ids.append(b.read(pos, cig, codes, d, s))
    b.scope(ids, pos, span_len if span_len is not None else end - pos)
    b.cursor = end + 40


def gate_batches(reason: str):
    """(base, inside, gated) for one reason of the speculative run's gate: three batches of the same
    read, scope and incidence counts — 40 pairs of 20M reads, a pair of 144M reads (so that every
    plan cuts the overflow regions for ceil(144 / 48) = 3 observations per incidence) and two probe
    pairs. ``base`` is plain (probes of 20M); ``inside`` sits on the limit and must run as
    speculated; ``gated`` is one past it. For "extras" upload with GATE_XREC_INIT: the two probe
    pairs' records fill a stripe exactly (8), or need 9."""
    m20 = [("M", 20)]
    two = [("M", 10), ("D", 2), ("M", 10)]
    probes = {
        "segments": ((([("M", 4), ("I", 1)] * 7 + [("M", 4)],) * 2, (m20, m20), None),
                     (([("M", 4), ("I", 1)] * 8 + [("M", 4)],) * 2, (m20, m20), None)),
        "read_length": ((([("M", 144)],) * 2, (m20, m20), None), (([("M", 145)],) * 2, (m20, m20), None)),
        "huge_scope": (((m20, m20), (m20, m20), HUGE_SPAN), ((m20, m20), (m20, m20), HUGE_SPAN + 1)),
        "long_cigar": (((m20 + [("P", 1)] * 47,) * 2, (m20, m20), None), ((m20 + [("P", 1)] * 48,) * 2, (m20, m20), None)),
        "extras": (((two, two), (two, two), None), ((two, two), (two, [("M", 10), ("D", 2), ("M", 5), ("I", 1), ("M", 4)]), None)),
    }[reason]
    out = []
    for a, bb, span in (((m20, m20), (m20, m20), None),) + probes:
        b = _new_batch(HUGE_SPAN + 8_192, 13)
        for k in range(40):
            _add_pair(b, f"plain_{k}", m20, m20)
        _add_pair(b, "longest", [("M", 144)], [("M", 144)])
        _add_pair(b, "probe_b", *bb)
        _add_pair(b, "probe_a", *a, span_len=span)       # (last: a huge span runs on to the reference's end)
        assert b.reads[-1]["pos"] + (span or 0) <= len(b.ref)
        out.append(b.arrays())
    return tuple(out)


# ---- invalid batches ---------------------------------------------------------------------------
def _base(slot: int, n_scopes: int = 1100, last_ops=None, last_L=None, last_pos=None):
    """``n_scopes`` scopes of a tumor and a normal 20M read with one alt, spans fitting exactly.
    The reads' slots are in scope order except that the LAST scope's normal read — the last in the
    sequence and CIGAR buffers — sits at read slot ``slot`` (and that slot's read at the end).
    ``last_ops`` / ``last_L`` / ``last_pos``: that read's CIGAR, length, and both reads' position."""
    rng = np.random.default_rng(11)
    ref = ACGT[rng.integers(0, 4, 64 + 160 * n_scopes + 256)]
    n = 2 * n_scopes
    slot_of = list(range(n))
    slot_of[n - 1], slot_of[slot] = slot, n - 1
    logical = [None] * n
    b = Batch(ref)
    scopes = []
    plain = _plain_codes(n_scopes)
    for s in range(n_scopes):
        pos = 64 + 160 * s
        p = last_pos if (s == n_scopes - 1 and last_pos is not None) else pos
        ids, length = [], 0
        for d in (0, 1):
            j = 2 * s + d
            cig, codes, rl = [cw("M", 20)], plain[s], 20
            if j == n - 1 and last_ops is not None:
                cig = words(last_ops)
                codes, _, _ = case_codes(ref, pos, cig, 20 if last_L is None else last_L)   # (the scope's reference slice)
                _, rl, _, _ = walk_unbounded(cig, len(codes), p)
            length = max(length, rl if rl > 0 else 1)
            logical[j] = {"pos": p, "cig": cig, "codes": codes, "ds": d, "ws": s}
            ids.append(slot_of[j])
        scopes.append((ids, p, length))
    by_slot = [None] * n
    for j in range(n):
        by_slot[slot_of[j]] = logical[j]
    for x in by_slot:
        b.read(x["pos"], x["cig"], x["codes"], x["ds"], x["ws"])
    for s, (ids, start, length) in enumerate(scopes):
        b.scope(ids, start, length)
    storage = [slot_of[j] for j in range(n)]
    arr = b.arrays(storage=storage)
    if last_pos is not None:      # the reference slice stays where the scope's bases came from
        arr["scope_ref_off"][n_scopes - 1] = 64 + 160 * (n_scopes - 1)
    return arr


_PLAIN = {}


def _plain_codes(n_scopes: int):
    """The 20M reads' bases of _base, per scope (made once)."""
    if n_scopes not in _PLAIN:
        rng = np.random.default_rng(11)
        ref = ACGT[rng.integers(0, 4, 64 + 160 * n_scopes + 256)]
        _PLAIN[n_scopes] = [case_codes(ref, 64 + 160 * s, [cw("M", 20)], 20)[0] for s in range(n_scopes)]
    return _PLAIN[n_scopes]


def _with(arr, **changes):
    """A copy with single elements changed: name=(index, value)."""
    out = dict(arr)
    for name, (i, v) in changes.items():
        a = arr[name].copy()
        a[i] = v
        out[name] = a
    return out


def invalid_batches() -> Iterator[Tuple[str, dict, Tuple[str, int, int], dict]]:
    """(name, invalid arrays, (kind, index, detail), valid neighbour arrays): the invalid batch is
    its neighbour with ONE element changed, the neighbour sits on the limit. The changed element is
    at the last slot of a scan block (1023) and at the first of the next (1024)."""
    for slot in (SCAN_BLOCK - 1, SCAN_BLOCK):
        t = f"@{slot}"
        base = _base(slot)
        ns, n = len(base["scope_span_len"]), len(base["read_len"])
        sb, nops = len(base["seq_nt16"]), len(base["cigar"])
        r = slot
        assert base["seq_off"][r] + 10 == sb and base["cig_off"][r] + 1 == nops and base["write_scope"][r] == ns - 1
        yield "seq_end_even_L" + t, _with(base, seq_off=(r, sb - 9)), ("seq", r, 0), base
        odd = _with(base, read_len=(r, 19))
        yield "seq_end_odd_L" + t, _with(odd, seq_off=(r, sb - 9)), ("seq", r, 0), odd
        yield "cig_end" + t, _with(base, cig_off=(r, nops)), ("cigar", r, 0), base
        zero = _with(base, read_len=(r, 0))
        yield "negative_L" + t, _with(base, read_len=(r, -1)), ("seq", r, 0), zero
        zero_so = _with(base, read_len=(r, 0), seq_off=(r, 0))
        yield "negative_seq_off" + t, _with(zero_so, seq_off=(r, -1)), ("seq", r, 0), zero_so
        nocig = _with(base, n_cig=(r, 0))
        yield "negative_n_cig" + t, _with(base, n_cig=(r, -1)), ("cigar", r, 0), nocig
        nocig0 = _with(base, n_cig=(r, 0), cig_off=(r, 0))
        yield "negative_cig_off" + t, _with(nocig0, cig_off=(r, -1)), ("cigar", r, 0), nocig0
        yield "dataset_2" + t, _with(base, dataset=(r, 2)), ("dataset", r, 0), base
        unwritten = _with(base, write_scope=(r, -1))
        yield "write_scope_minus_2" + t, _with(base, write_scope=(r, -2)), ("write_scope", r, -2), unwritten
        yield "write_scope_n_scopes" + t, _with(base, write_scope=(r, ns)), ("write_scope", r, ns), base
        yield "ref_start_minus_1" + t, _with(base, ref_start=(r, -1)), ("pos", r, 0), base
        edge = _base(slot, last_pos=INT32_MAX - 20)
        yield "end_past_int32" + t, _with(edge, ref_start=(r, INT32_MAX - 19)), ("pos", r, 0), edge
        for nops_r, places in ((1, (0,)), (48, (0, 47)), (130, (0, 63, 64, 129))):
            for k in places:
                for code in (9, 15):
                    ops = [("M", 1)] * nops_r if nops_r > 1 else [("M", 20)]
                    ops[k] = ("X", ops[k][1])
                    good = _base(slot, last_ops=ops)
                    at = int(good["cig_off"][r]) + k
                    w = (int(good["cigar"][at]) & ~15) | code
                    yield f"op_{code}_at_{k}_of_{nops_r}" + t, _with(good, cigar=(at, w)), ("op", r, code), good
        # per scope
        s = slot
        merged = dict(base)      # scope s - 1 empty, scope s lists (and writes) both scopes' reads
        for name in ("scope_incid_off", "scope_span_start", "scope_span_len", "scope_ref_off", "write_scope"):
            merged[name] = base[name].copy()
        merged["scope_incid_off"][s] = base["scope_incid_off"][s - 1]
        merged["scope_span_start"][s] = merged["scope_ref_off"][s] = base["scope_span_start"][s - 1]
        merged["scope_span_len"][s] = 180
        merged["write_scope"][base["incid_read"][base["scope_incid_off"][s - 1]:base["scope_incid_off"][s]]] = s
        yield ("incid_off_decreasing" + t, _with(merged, scope_incid_off=(s, int(merged["scope_incid_off"][s]) - 1)),
               ("scope_off", s - 1, 0), merged)
        yield "span_start_minus_1" + t, _with(base, scope_span_start=(s, -1)), ("scope_span", s, 0), base
        yield "span_len_minus_1" + t, _with(base, scope_span_len=(s, -1)), ("scope_span", s, 0), base
        rn = 2 * len(base["ref_nt16"])
        tail = _with(base, scope_ref_off=(s, rn - 20))
        yield "ref_slice_end" + t, _with(base, scope_ref_off=(s, rn - 19)), ("scope_ref", s, 0), tail
        yield "ref_off_minus_1" + t, _with(base, scope_ref_off=(s, -1)), ("scope_ref", s, 0), base
        k15 = _with(base, keep_code=(s, 15))
        yield "keep_code_16" + t, _with(base, keep_code=(s, 16)), ("scope_keep", s, 0), k15
        # found by the run
        i = int(base["scope_incid_off"][s])
        yield "incid_read_minus_1" + t, _with(base, incid_read=(i, -1)), ("incid_read", i, -1), base
        yield "incid_read_n_reads" + t, _with(base, incid_read=(i + 1, n)), ("incid_read", i + 1, n), base
        yield "span_one_short" + t, _with(base, scope_span_len=(s, 19)), ("incid_span", s, 0), base
        yield "span_starts_one_late" + t, _with(base, scope_span_start=(s, int(base["scope_span_start"][s]) + 1)), ("incid_span", s, 0), base
        a, bb = (int(x) for x in base["incid_read"][i:i + 2])
        nb_unwritten = _with(base, write_scope=(bb, -1))
        yield "listed_twice" + t, _with(nb_unwritten, incid_read=(i + 1, a)), ("ws_missing", a, s), nb_unwritten
        other = int(base["incid_read"][0])
        yield "listed_zero_times" + t, _with(base, write_scope=(other, s)), ("ws_missing", other, s), base
    # read_end observed through the span check: a read of no reference length, one that ends on a D
    for name, ops, L in (("zero_reference_length", [("S", 20)], 20), ("ends_on_D", [("M", 20), ("D", 5)], 20)):
        good = _base(SCAN_BLOCK - 1, n_scopes=600, last_ops=ops, last_L=L)
        s = len(good["scope_span_len"]) - 1
        if name == "zero_reference_length":      # both reads of the scope: the span is one position
            partner = int(good["incid_read"][good["scope_incid_off"][s]])
            at = int(good["cig_off"][partner])
            good = _with(good, cigar=(at, cw("S", 20)), scope_span_len=(s, 1))
        yield "span_one_short_" + name, _with(good, scope_span_len=(s, int(good["scope_span_len"][s]) - 1)), ("incid_span", s, 0), good
    # a read of 2^24 - 1 bases against 2^24: one all-soft-clip read in an 8 MB buffer
    rng = np.random.default_rng(12)
    b = Batch(ACGT[rng.integers(0, 4, 256)])
    r0 = b.read(64, [cw("S", MAX_READ_LEN - 1)], np.zeros(0, np.uint8), 0, 0)
    codes, _, _ = case_codes(b.ref, 64, [cw("M", 20)], 20)
    r1 = b.read(64, [cw("M", 20)], codes, 1, 0)
    r2 = b.read(64, [cw("M", 20)], codes, 0, 0)
    b.scope([r0, r1, r2], 64, 20)
    good = b.arrays(storage=[r1, r2, r0], seq_pad=MAX_READ_LEN // 2)    # the long read's zero bytes last
    good = _with(good, read_len=(r0, MAX_READ_LEN - 1))
    assert good["seq_off"][r0] + MAX_READ_LEN // 2 == len(good["seq_nt16"])
    yield "read_len_2^24", _with(good, read_len=(r0, MAX_READ_LEN)), ("long", r0, 0), good


def differing_elements(a: dict, b: dict) -> int:
    return sum(int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else 10**9 for k in a)


# ---- offsets past 2^31 ----------------------------------------------------------------------------
WIDE_SEQ_BYTES = (1 << 31) + 4096


def wide_offset_batch(compact: bool = False):
    """``seq_bytes`` = 2^31 + 4096, the smallest shape that takes k_prep_scan's wide instantiation
    (64-bit offsets; bits 32-39 of every query-nibble field non-zero above byte 2^31). The buffer is
    zero-filled (sparse on the host); 36 written reads, tumor / normal pairs with alts at every
    segment end, half of them 40M and half of three segments (200 bases), sit at byte 0, just below
    2^31, across it (a three-segment read whose nibble index passes 2^32 inside its second segment;
    its partner just above), just above it, and up to the last byte; six unwritten reads outside
    every scope lie in between. ``compact``: the same reads packed into a small buffer in the same
    order (for the per-base oracle on a machine without the memory). info: ``masked``, ``regions``
    (read -> region name), ``straddler``."""
    rng = np.random.default_rng(14)
    ref = ACGT[rng.integers(0, 4, 16_384)]
    one = [("M", 40)]
    three = [("M", 60), ("D", 2), ("M", 60), ("I", 3), ("M", 77)]
    half, end = 1 << 31, WIDE_SEQ_BYTES
    # (region, byte offsets of the tumor and the normal read, CIGAR); None: an unwritten 12M read
    layout = [("straddle", (half - 50, half + 50), three), ("above", (half + 150, half + 170), one)]
    for k in range(2):
        b, a, e = half - 2000 + 400 * k, half + 200 + 400 * k, end - 400 * k
        layout += [("start", (400 * k, 20 + 400 * k), one), ("start", (40 + 400 * k, 140 + 400 * k), three),
                   ("below", (b, b + 20), one), ("below", (b + 100, b + 200), three),
                   ("above", (a, a + 20), one), ("above", (a + 60, a + 160), three),
                   ("end", (e - 20, e - 40), one), ("end", (e - 140, e - 240), three)]
    plain = [half - 2400, half - 150, 900, half + 1500, half + 2000, end - 1200]
    reads, scopes, regions, masked = [], [], {}, []
    pos = 64
    for region, offs, ops in layout:
        cig = words(ops)
        L = sum(n for o, n in ops if o in "MIS=X")
        codes, segs, alts = case_codes(ref, pos, cig, L)
        _, rl, _, _ = walk_unbounded(cig, L, pos)
        s = len(scopes)
        ids = []
        for d, off in enumerate(offs):
            regions[len(reads)] = region
            masked += [(len(reads), q) for q in alts]
            ids.append(len(reads))
            reads.append({"pos": pos, "cig": cig, "codes": codes, "ds": d, "ws": s, "off": off})
        scopes.append((ids, pos, rl))
        pos += rl + 40
    for k, off in enumerate(plain):
        regions[len(reads)] = "unwritten"
        reads.append({"pos": 64, "cig": [cw("M", 12)], "codes": np.array(ref[64:76], np.uint8), "ds": k & 1, "ws": -1, "off": off})
    order = sorted(range(len(reads)), key=lambda r: reads[r]["off"])
    if compact:
        at = 0
        for r in order:
            reads[r]["off"] = at
            at += (len(reads[r]["codes"]) + 1) // 2
    seq = np.zeros(at if compact else WIDE_SEQ_BYTES, np.uint8)
    spans = []
    for r in order:
        pk = pack_nibbles(reads[r]["codes"])
        o = reads[r]["off"]
        spans.append((o, o + len(pk)))
        seq[o:o + len(pk)] = pk
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "reads overlap"
    cig_off = np.cumsum([0] + [len(x["cig"]) for x in reads])
    offs, incid = [0], []
    for ids, _, _ in scopes:
        incid += ids
        offs.append(len(incid))
    arr = {
        "ref_start": np.array([x["pos"] for x in reads], np.int32),
        "read_len": np.array([len(x["codes"]) for x in reads], np.int32),
        "seq_off": np.array([x["off"] for x in reads], np.int64), "seq_nt16": seq,
        "cig_off": cig_off[:-1].astype(np.int64), "n_cig": np.array([len(x["cig"]) for x in reads], np.int32),
        "cigar": np.concatenate([np.array(x["cig"], np.uint32) for x in reads]),
        "dataset": np.array([x["ds"] for x in reads], np.uint8),
        "write_scope": np.array([x["ws"] for x in reads], np.int32),
        "scope_incid_off": np.array(offs, np.int64), "incid_read": np.array(incid, np.int32),
        "scope_span_start": np.array([s[1] for s in scopes], np.int32),
        "scope_span_len": np.array([s[2] for s in scopes], np.int32),
        "scope_ref_off": np.array([s[1] for s in scopes], np.int64),
        "ref_nt16": pack_nibbles(ref),
        "keep_pos": np.full(len(scopes), -1, np.int32), "keep_code": np.zeros(len(scopes), np.uint8),
    }
    straddler = [r for r in range(len(reads)) if reads[r]["off"] < half < reads[r]["off"] + (len(reads[r]["codes"]) + 1) // 2]
    return arr, {"masked": sorted(masked), "regions": regions, "straddler": straddler}
