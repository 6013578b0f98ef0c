"""Deterministic batches for the k_group instantiation matrix (tests/test_gpu_kgroup.py) and the
CPU test that pins them (tests/test_kgroup_batches.py).

* ``chunk_edge_batch``: every aligned-segment length around the multiples of 16 * U (U up to 8) at
  every nibble alignment of the read (mod 8) and of the reference (mod 16), with both-dataset alts
  at the ends of the segment and either side of every 16-base window border, and with bases that
  must never be observed right where a chunk's loads and masks end.
* ``threshold_batch``: one scope, one group, an exact number of observations, for the thresholds
  between the group kernel's observation-list paths.

Both return the dict of arrays of ``genomeanonymizer_amd.synth.batch`` plus an info dict.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from genomeanonymizer_amd.synth.batch import ACGT, _cigar_word, pack_nibbles

# every multiple of 16 * U for U up to 8, minus one, exact, plus one
LENGTH_CLASSES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SEGMENT = np.dtype([("read", np.int32), ("q0", np.int32), ("pos", np.int32), ("length", np.int32),
                    ("cls", np.int32), ("scope", np.int32), ("dirty_set", np.int8)])
_IUPAC = (3, 5, 6, 7, 9, 10, 11, 12, 13, 14)
_GAP = 160            # reference bases between two sites: a site's N never shares a 64-base block with a neighbour
_SITES_PER_SCOPE = 86


def _other(code: int, k: int) -> int:
    """An ACGT code that differs from ``code`` (k = 1..3); for a non-ACGT ``code`` any ACGT code."""
    code = int(code)
    if code in (1, 2, 4, 8):
        return int(ACGT[((code.bit_length() - 1) + k) % 4])
    return int(ACGT[k % 4])


def alt_offsets(length: int) -> List[int]:
    """Where a segment of ``length`` bases carries a both-dataset alt: its first and last base, the
    first and last base of an interior 16-base window, and the base either side of every 16 * U
    border (U = 1, 2, 4, 8) inside it."""
    offs = {0, length - 1}
    if length >= 48:
        offs |= {16, 31}
    for u in (1, 2, 4, 8):
        for b in range(16 * u, length, 16 * u):
            offs |= {b - 1, b}
    return sorted(offs)


def _free_offset(length: int) -> int:
    """An offset of the segment that carries no alt (-1: none)."""
    alts = set(alt_offsets(length))
    for o in range(length // 2, 0, -1):
        if o not in alts:
            return o
    return -1


class _Builder:
    def __init__(self, ref: np.ndarray):
        self.ref = ref
        self.reads = []            # (pos, ops, codes, dataset, scope)
        self.segments = []
        self.alts = []             # (read, qpos, pos): a both-dataset alt over an ACGT reference base
        self.must_not = []         # (read, qpos): bases no kernel may observe or change
        self.seq_bytes = 0

    def add_read(self, pos: int, lead_target: int, segs, joins, trail: int, ds: int, scope: int, dirty_set: int,
                 special: dict) -> None:
        """segs: [(length, class index)]; joins[j]: (insert target alignment or -1, 'D'/'N'/None, ref gap)
        between segment j and j + 1. special: {(segment, offset): code} bases other than the reference's
        (alts, read-N); offsets not listed copy the reference."""
        ref = self.ref
        r = len(self.reads)
        ops, codes = [], []
        lead = (lead_target - 2 * self.seq_bytes) % 8
        if lead:
            ops.append(("S", lead))
            codes += [_other(ref[pos - lead + j], 2) for j in range(lead)]
            self.must_not += [(r, j) for j in range(lead)]
        p = pos
        for j, (length, cls) in enumerate(segs):
            q0 = len(codes)
            self.segments.append((r, q0, p, length, cls, scope, dirty_set))
            for o in range(length):
                codes.append(special.get((j, o), (int(ref[p + o]),))[0])
            ops.append(("M", length))
            p += length
            if j + 1 < len(segs):
                a_s, gap_op, gap = joins[j]
                if a_s >= 0:
                    ins = (a_s - (2 * self.seq_bytes + len(codes))) % 8 or 8
                    q = len(codes)
                    codes += [_other(ref[p + i], 2) for i in range(ins)]   # differ from the bases past the end
                    self.must_not += [(r, q + i) for i in range(ins)]
                    ops.append(("I", ins))
                if gap_op:
                    ops.append((gap_op, gap))
                    p += gap
        if trail:
            q = len(codes)
            codes += [_other(ref[p + i], 2) for i in range(trail)]
            self.must_not += [(r, q + i) for i in range(trail)]
            ops.append(("S", trail))
        for (j, o), v in special.items():
            seg = self.segments[len(self.segments) - len(segs) + j]
            if v[1] == "alt":
                self.alts.append((r, seg[1] + o, seg[2] + o))
            else:
                self.must_not.append((r, seg[1] + o))
        self.reads.append((pos, [_cigar_word(o, n) for o, n in ops], np.array(codes, np.uint8), ds, scope))
        self.seq_bytes += (len(codes) + 1) // 2


def chunk_edge_batch(multi_segment: bool, end_on_long: bool = False) -> Tuple[Dict[str, np.ndarray], dict]:
    """See the module docstring. Six scopes on private regions of one contig (reference nibble =
    position): scopes 0-2 over an all-ACGT reference (the 2-bit reference path), scopes 3-5 with N and
    IUPAC codes placed where they decide a segment's clean flag. Every site holds a tumor and a normal
    read over the same reference bases. ``multi_segment``: three segments per read, joined by I, D and
    N ops. The buffer ends on a 1-base read, or with ``end_on_long`` on a 257-base read.

    info: ``segments`` (SEGMENT records), ``alts`` (read, query position) of every base the masking
    must change, ``must_not`` (read, query position) of the bases that must never be observed."""
    rng = np.random.default_rng(20240917)
    n_cls = len(LENGTH_CLASSES)
    per_site = 3 if multi_segment else 1
    n_sites = 2 * n_cls * 16 + 1
    ref = ACGT[rng.integers(0, 4, 256 + n_sites * (per_site * (257 + 16) + 2 * _GAP + 64) + 4096)]
    b = _Builder(ref)
    cursor = 256
    keep = {}
    for dirty_set in (0, 1):
        for c in range(n_cls):
            for k in range(16):
                scope = 3 * dirty_set + min(2, (c * 16 + k) // _SITES_PER_SCOPE)
                cls = [(c + 5 * j) % n_cls for j in range(per_site)]
                lens = [LENGTH_CLASSES[x] for x in cls]
                a_r = [(k + 7 * j) % 16 for j in range(per_site)]
                # the first segment's position: its reference alignment; in the N scopes a segment that
                # starts (k = 0) or ends (k = -length mod 16) on a 64-base block edge
                base = cursor + _GAP
                n_before = n_after = False
                if dirty_set and k == (-lens[0]) % 16 and (k or c % 2 == 0):
                    pos = base + ((-lens[0]) - base) % 64
                    n_after = True
                elif dirty_set and k == 0:
                    pos = base + (-base) % 64
                    n_before = True
                else:
                    pos = base + (a_r[0] - base) % 16
                # reference gaps between the segments (shared by both reads), then the site's extent
                joins_ref, p = [], pos + lens[0]
                for j in range(1, per_site):
                    d = (a_r[j] - p) % 16
                    if d == 0 and k % 2 == 0:
                        joins_ref.append((None, 0))          # insertion only
                    else:
                        joins_ref.append(("D" if (k + j) % 2 else "N", d or 16))
                    p += joins_ref[-1][1] + lens[j]
                end = p
                # N / IUPAC codes of the N scopes
                deco = (c + k) % 4 if dirty_set else -1
                free = _free_offset(lens[0])
                if deco == 0 and free >= 0:
                    ref[pos + free] = 15
                elif deco == 1 and free >= 0:
                    ref[pos + free] = _IUPAC[(c + k) % len(_IUPAC)]
                elif deco == 2:
                    n_before = n_after = True
                if n_before:
                    ref[pos - 1] = 15
                if n_after:
                    ref[end if per_site == 1 else pos + lens[0]] = 15
                # the reads' bases that are not the reference's
                t_sp, n_sp = {}, {}
                for j, length in enumerate(lens):
                    seg_pos = pos + sum(lens[:j]) + sum(g for _, g in joins_ref[:j])
                    for o in alt_offsets(length):
                        rc = int(ref[seg_pos + o])
                        kind = "alt" if rc in (1, 2, 4, 8) else "refn"
                        t_sp[(j, o)] = n_sp[(j, o)] = (_other(rc, 1), kind)
                if free >= 0:
                    rc = int(ref[pos + free])
                    if deco in (0, 1):          # an alt over an N / IUPAC reference base: never a call
                        t_sp[(0, free)] = n_sp[(0, free)] = (_other(rc, 1), "refn")
                    elif (c + k) % 4 == 3 or (not dirty_set and (c + k) % 4 == 1):
                        # a read-N at an alt site: N in the tumor read, the alt (k even: N too) in the normal read
                        t_sp[(0, free)] = (15, "readn")
                        n_sp[(0, free)] = (15, "readn") if k % 2 else (_other(rc, 1), "single")
                trail = (3 * k + c) % 19
                for ds, sp, a_s0, mul in ((0, t_sp, 3 * k + c, 3), (1, n_sp, 5 * k + c + 1, 5)):
                    joins = [((a_s0 + mul * j) % 8 if (op is None or (k + j + ds) % 3) else -1, op, g)
                             for j, (op, g) in enumerate(joins_ref, 1)]
                    b.add_read(pos, a_s0 % 8, list(zip(lens, cls)), joins, trail, ds, scope, dirty_set, sp)
                if not keep and scope == 1:
                    keep[scope] = (pos, _other(ref[pos], 1))
                cursor = end
    # the buffer's last site: one segment, no clips; a 1-base read last, or a 257-base read
    length = 257 if end_on_long else 1
    cls = LENGTH_CLASSES.index(length)
    pos = cursor + _GAP
    sp = {(0, o): (_other(ref[pos + o], 1), "alt") for o in alt_offsets(length)}
    for ds in (1, 0):
        lead_target = (2 * b.seq_bytes) % 8          # no leading clip
        b.add_read(pos, lead_target, [(length, cls)], [], 0, ds, 5, 1, sp)

    n = len(b.reads)
    n_scopes = 6
    starts = np.array([r[0] for r in b.reads], np.int64)
    cig = [np.array(r[1], np.uint32) for r in b.reads]
    ends = np.array([r[0] + sum(int(w) >> 4 for w in r[1] if (int(w) & 15) in (0, 2, 3)) for r in b.reads], np.int64)
    packed = [pack_nibbles(r[2]) for r in b.reads]
    nb = np.array([len(x) for x in packed], np.int64)
    scope_of = np.array([r[4] for r in b.reads], np.int32)
    incid, offs, span_start, span_len = [], [0], [], []
    for s in range(n_scopes):
        ids = np.nonzero(scope_of == s)[0]
        incid += rng.permutation(ids).tolist()
        offs.append(len(incid))
        span_start.append(int(starts[ids].min()))
        span_len.append(int(ends[ids].max()) - span_start[-1])
    ws = scope_of.copy()
    ws[np.arange(n) % 7 == 3] = -1                   # some pass-through reads
    ws[-2:] = 5
    keep_pos = np.full(n_scopes, -1, np.int32)
    keep_code = np.zeros(n_scopes, np.uint8)
    for s, (kp, kc) in keep.items():
        keep_pos[s], keep_code[s] = kp, kc
    arr = {
        "ref_start": starts.astype(np.int32),
        "read_len": np.array([len(r[2]) for r in b.reads], np.int32),
        "seq_off": np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64),
        "seq_nt16": np.concatenate(packed),
        "cig_off": np.concatenate([[0], np.cumsum([len(x) for x in cig])[:-1]]).astype(np.int64),
        "n_cig": np.array([len(x) for x in cig], np.int32),
        "cigar": np.concatenate(cig),
        "dataset": np.array([r[3] for r in b.reads], np.uint8),
        "write_scope": ws,
        "scope_incid_off": np.array(offs, np.int64),
        "incid_read": np.array(incid, np.int32),
        "scope_span_start": np.array(span_start, np.int32),
        "scope_span_len": np.array(span_len, np.int32),
        "scope_ref_off": np.array(span_start, np.int64),
        "ref_nt16": pack_nibbles(ref),
        "keep_pos": keep_pos,
        "keep_code": keep_code,
    }
    alts = np.array([(r, q) for r, q, p in b.alts
                     if ws[r] >= 0 and not (keep_pos[scope_of[r]] == p)], np.int64).reshape(-1, 2)
    info = {"segments": np.array(b.segments, SEGMENT), "alts": alts,
            "must_not": np.array(sorted(set(b.must_not)), np.int64).reshape(-1, 2)}
    return arr, info


def threshold_batch(n_obs: int, n_reads: int) -> Tuple[Dict[str, np.ndarray], int]:
    """One scope (one group) of ``n_reads`` 150M reads, tumor and normal alternating, that equal the
    reference except for exactly ``n_obs`` observations: alts at five sites every read covers, carried
    by as many reads as half the budget allows (both datasets: calls), then single-dataset errors in
    tumor reads only (never a call). Returns (arrays, the observations made)."""
    read_len, alt_sites = 150, (100, 110, 120, 130, 140)
    if n_reads < 2:
        raise ValueError("threshold_batch needs a tumor and a normal read")
    rng = np.random.default_rng(4242)
    base = 64
    ref = ACGT[rng.integers(0, 4, base + 100 + read_len + 64)]
    starts = base + (np.arange(n_reads) * 7) % 100
    ds = (np.arange(n_reads) % 2).astype(np.uint8)
    codes = np.stack([ref[s:s + read_len] for s in starts]).astype(np.uint8)
    n_alt = min(n_obs // 2, len(alt_sites) * n_reads)
    if n_alt < 2:
        raise ValueError("too few observations for a call in both datasets")
    made = 0
    for p in alt_sites:                              # site by site: the first reads of each, tumor and normal
        for r in range(n_reads):
            if made < n_alt:
                codes[r, base + p - starts[r]] = _other(ref[base + p], 1)
                made += 1
    free = [o for o in range(read_len)]
    for r in range(0, n_reads, 2):                   # tumor reads
        for o in free:
            if made >= n_obs:
                break
            if starts[r] + o - base in alt_sites:
                continue
            codes[r, o] = _other(ref[starts[r] + o], 1 + (r // 2 + o) % 3)
            made += 1
    if made != n_obs:
        raise ValueError(f"{n_reads} reads cannot carry {n_obs} observations")
    h = read_len // 2
    arr = {
        "ref_start": starts.astype(np.int32),
        "read_len": np.full(n_reads, read_len, np.int32),
        "seq_off": np.arange(n_reads, dtype=np.int64) * h,
        "seq_nt16": ((codes[:, 0::2] << 4) | codes[:, 1::2]).reshape(-1).astype(np.uint8),
        "cig_off": np.arange(n_reads, dtype=np.int64),
        "n_cig": np.ones(n_reads, np.int32),
        "cigar": np.full(n_reads, _cigar_word("M", read_len), np.uint32),
        "dataset": ds,
        "write_scope": np.zeros(n_reads, np.int32),
        "scope_incid_off": np.array([0, n_reads], np.int64),
        "incid_read": np.arange(n_reads, dtype=np.int32),
        "scope_span_start": np.array([int(starts.min())], np.int32),
        "scope_span_len": np.array([int(starts.max()) + read_len - int(starts.min())], np.int32),
        "scope_ref_off": np.array([int(starts.min())], np.int64),
        "ref_nt16": pack_nibbles(ref),
        "keep_pos": np.full(1, -1, np.int32),
        "keep_code": np.zeros(1, np.uint8),
    }
    return arr, made


def count_observations(arr: Dict[str, np.ndarray]) -> int:
    """Observations of a batch of one-op ``M`` reads in one scope, recounted from the arrays: read
    bases that are not N, differ from the reference and sit over an ACGT reference base."""
    from genomeanonymizer_amd.synth.batch import unpack_nibbles
    assert len(arr["scope_span_len"]) == 1 and (arr["n_cig"] == 1).all() and (arr["cigar"] & 15 == 0).all()
    refc = unpack_nibbles(arr["ref_nt16"], 2 * len(arr["ref_nt16"]))
    n = 0
    for r in arr["incid_read"]:
        L = int(arr["read_len"][r])
        c = unpack_nibbles(arr["seq_nt16"][arr["seq_off"][r]:arr["seq_off"][r] + (L + 1) // 2], L)
        p = int(arr["scope_ref_off"][0]) + int(arr["ref_start"][r]) - int(arr["scope_span_start"][0])
        rc = refc[p:p + L]
        n += int(((c != 15) & (c != rc) & np.isin(rc, ACGT)).sum())
    return n


def touched_reads_differ(arr: Dict[str, np.ndarray], a: np.ndarray, b: np.ndarray) -> List[int]:
    """Reads in an incidence list or written whose packed bytes differ between two outputs (the read
    filter of test_hip_matches_oracle_edge_batches)."""
    touched = arr["write_scope"] >= 0
    touched[arr["incid_read"]] = True
    nbytes = (arr["read_len"].astype(np.int64) + 1) // 2
    bad = []
    for r in np.nonzero(touched)[0]:
        o, n = int(arr["seq_off"][r]), int(nbytes[r])
        if not np.array_equal(a[o:o + n], b[o:o + n]):
            bad.append(int(r))
    return bad
