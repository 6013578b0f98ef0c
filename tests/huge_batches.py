"""Deterministic batches for the huge-scope tile path (scopes wider than kGrpMaxSpan = 2^20
positions: k_tile_large / k_mask_large, ganon_huge.hip), for tests/test_gpu_huge.py and the CPU test
that pins them (tests/test_huge_batches.py).

* ``tile_edge_batch``: five scopes (ordinary window N0, huge H1 of 2^20 + 1 positions, ordinary N2
  of exactly 2^20, huge H3 with an odd start and an odd last tile, huge H4) with sites either side of
  tile borders, every classification of a site inside one table word, rare (non-ACGTN) tiles, kept
  variants, the CIGAR corner cases, and reads that H1 shares with the window N0.
* ``rare_stride_batch``: one huge scope of 1,030 tiles, every one rare (the re-run's grid-stride loop).
* ``crowd_batch``: one huge scope that writes 33,000 reads (k_mask_large's wave-stride loop).
* ``threshold_pair``: one scope of span 2^20, and of 2^20 + 1 after one read moved by one base.

Every builder returns the dict of arrays of ``genomeanonymizer_amd.synth.batch`` plus an info dict
with the builder's own bookkeeping: ``must_mask`` (read, query position, reference code) of every base
that has to become the reference base, ``must_not`` (read, query position) of the bases on a site that
must stay, ``calls_per_scope``, ``tiles_per_scope``, ``rare_tiles``, ``huge_written_reads``. The only
randomness is a seeded generator for the filler reference bases.
"""
from __future__ import annotations

import re
from math import gcd
from typing import Dict, List, Tuple

import numpy as np

from genomeanonymizer_amd.synth.batch import ACGT, _cigar_word, pack_nibbles

TILE = 16384          # kTile
HUGE = 1 << 20        # kGrpMaxSpan: the widest scope of the group kernels
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")


def _rot(code: int, k: int = 1) -> int:
    """The ACGT code k steps after the ACGT code ``code``."""
    return int(ACGT[(int(code).bit_length() - 1 + k) % 4])


def _permute(ids: List[int]) -> List[int]:
    """A fixed permutation of a list (a stride coprime with its length): not sorted by position."""
    n = len(ids)
    if n < 3:
        return list(reversed(ids))
    k = n // 2 + 1
    while gcd(k, n) != 1:
        k += 1
    return [ids[n - 1 - (i * k + 1) % n] for i in range(n)]


def n_tiles(span_len: int) -> int:
    return (int(span_len) + TILE - 1) // TILE if span_len > HUGE else 0


class _Builder:
    """Reads, their planted bases and the calls the builder means them to make."""

    def __init__(self, scopes: List[Tuple[int, int, int]], seed: int, ref_len: int = 0):
        self.scopes = scopes                     # (span_start, span_len, scope_ref_off)
        total = ref_len or max(ro + sl for _, sl, ro in scopes) + 64
        self.ref = ACGT[np.random.default_rng(seed).integers(0, 4, total + (total & 1))]
        self.reads = []                          # [pos, cigar ops, codes, dataset, write scope, scopes]
        self.obs = []                            # (read, query position, position, code): planted bases
        self.expect = {}                         # (scope, position) -> codes of the calls meant there
        self.keep = {}                           # scope -> (keep_pos, keep_code)
        self.named = {}

    def nib(self, s: int, p: int) -> int:
        ss, _, ro = self.scopes[s]
        return ro + p - ss

    def refc(self, s: int, p: int) -> int:
        return int(self.ref[self.nib(s, p)])

    def set_ref(self, s: int, p: int, codes) -> None:
        a = self.nib(s, p)
        self.ref[a:a + len(codes)] = codes

    def call(self, s: int, p: int, *codes: int) -> None:
        self.expect.setdefault((s, p), set()).update(codes)

    def read(self, scopes, ws: int, ds: int, pos: int, cigar: str, subs=None, home: int = None) -> int:
        """A read listed by ``scopes``, written by ``ws``; its aligned bases copy the reference (as
        scope ``home`` or the first listing scope sees it) except at the positions of ``subs``."""
        subs = subs or {}
        home = scopes[0] if home is None else home
        ops = [(o, int(n)) for n, o in _CIGAR.findall(cigar)]
        r, codes, p, used = len(self.reads), [], pos, set()
        for op, n in ops:
            if op in "M=X":
                for i in range(n):
                    if p + i in subs:
                        self.obs.append((r, len(codes), p + i, int(subs[p + i])))
                        used.add(p + i)
                        codes.append(int(subs[p + i]))
                    else:
                        codes.append(self.refc(home, p + i))
                p += n
            elif op in "IS":
                codes += [int(ACGT[(len(codes) + i) % 4]) for i in range(n)]
            elif op in "DN":
                p += n
        assert used == set(subs), (cigar, pos, sorted(set(subs) - used))
        self.reads.append([pos, [_cigar_word(o, n) for o, n in ops], np.array(codes, np.uint8), ds, ws, list(scopes)])
        return r

    def pair(self, s: int, p: int, t_code=None, n_code=None, ws=None, scopes=None) -> Tuple[int, int]:
        """A tumor 5M read and a normal 7M read over position p that carry the given codes there
        (None: no read of that dataset)."""
        ws = s if ws is None else ws
        scopes = [s] if scopes is None else scopes
        rt = self.read(scopes, ws, 0, p - 2, "5M", {p: t_code}) if t_code is not None else -1
        rn = self.read(scopes, ws, 1, p - 3, "7M", {p: n_code}) if n_code is not None else -1
        return rt, rn

    def finish(self) -> Tuple[Dict[str, np.ndarray], dict]:
        n, n_scopes = len(self.reads), len(self.scopes)
        ws = np.array([r[4] for r in self.reads], np.int32)
        must_mask, must_not = [], []
        for r, q, p, code in self.obs:
            w = int(ws[r])
            if w >= 0 and code in self.expect.get((w, p), ()):
                must_mask.append((r, q, self.refc(w, p)))
            else:
                must_not.append((r, q))
        incid, offs = [], [0]
        for s in range(n_scopes):
            incid += _permute([i for i, r in enumerate(self.reads) if s in r[5]])
            offs.append(len(incid))
        packed = [pack_nibbles(r[2]) for r in self.reads]
        nb = np.array([len(x) for x in packed], np.int64)
        cig = [np.array(r[1], np.uint32) for r in self.reads]
        nc = np.array([len(x) for x in cig], np.int64)
        keep_pos = np.full(n_scopes, -1, np.int32)
        keep_code = np.zeros(n_scopes, np.uint8)
        for s, (kp, kc) in self.keep.items():
            keep_pos[s], keep_code[s] = kp, kc
        span_len = np.array([sl for _, sl, _ in self.scopes], np.int32)
        arr = {
            "ref_start": np.array([r[0] for r in self.reads], np.int32),
            "read_len": np.array([len(r[2]) for r in self.reads], np.int32),
            "seq_off": np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64),
            "seq_nt16": np.concatenate(packed),
            "cig_off": np.concatenate([[0], np.cumsum(nc)[:-1]]).astype(np.int64),
            "n_cig": nc.astype(np.int32),
            "cigar": np.concatenate(cig),
            "dataset": np.array([r[3] for r in self.reads], np.uint8),
            "write_scope": ws,
            "scope_incid_off": np.array(offs, np.int64),
            "incid_read": np.array(incid, np.int32),
            "scope_span_start": np.array([ss for ss, _, _ in self.scopes], np.int32),
            "scope_span_len": span_len,
            "scope_ref_off": np.array([ro for _, _, ro in self.scopes], np.int64),
            "ref_nt16": pack_nibbles(self.ref),
            "keep_pos": keep_pos,
            "keep_code": keep_code,
        }
        calls = np.zeros(n_scopes, np.int32)
        for (s, _), codes in self.expect.items():
            calls[s] += len(codes)
        huge = span_len > HUGE
        info = {
            "must_mask": np.array(must_mask, np.int64).reshape(-1, 3),
            "must_not": np.array(must_not, np.int64).reshape(-1, 2),
            "calls_per_scope": calls,
            "tiles_per_scope": np.array([n_tiles(sl) for sl in span_len], np.int64),
            "huge_written_reads": int((huge[np.maximum(ws, 0)] & (ws >= 0)).sum()),
        }
        info.update(self.named)
        return arr, info


def _border_cluster(b: _Builder, s: int, bp: int, right: bool = True, straddle=None, edge=None) -> None:
    """Both-dataset alts at bp-2, bp-1, bp, bp+1 (all four codes differ; ``right`` False: the span ends
    at bp + 1, no site at bp + 1), carried by a tumor and a normal read that straddle bp (soft clips;
    = and X ops), a tumor read whose reference end is bp and a normal read that starts at bp.
    ``straddle`` / ``edge``: (listing scopes, write scope) of those reads."""
    n = 4 if right else 3
    b.set_ref(s, bp - 2, [1, 2, 4, 8][:n])
    alt = {bp - 2 + i: a for i, a in enumerate([2, 4, 8, 1][:n])}
    sc, ws = straddle or ([s], s)
    b.read(sc, ws, 0, bp - 10, f"3S{18 if right else 11}M2S", alt)
    b.read(sc, ws, 1, bp - 7, f"5=3X{4}M" if right else "5=3X", alt)
    sc, ws = edge or ([s], s)
    b.read(sc, ws, 0, bp - 6, "6M", {p: a for p, a in alt.items() if p < bp})
    b.read(sc, ws, 1, bp, "6M" if right else "1M", {p: a for p, a in alt.items() if p >= bp})
    for listing in {tuple(straddle[0]) if straddle else (s,)} | {tuple(edge[0]) if edge else (s,)}:
        for x in listing:
            for p, a in alt.items():
                b.call(x, p, a)


def _classify_block(b: _Builder, s: int, c: int) -> None:
    """Ten adjacent positions from c (a table word's first position): every way a site classifies."""
    b.set_ref(s, c, [1, 2, 4, 8, 1, 15, 5, 2, 1, 2])
    t = [{}, {}, {}]
    n = [{}, {}, {}]
    t[0][c], n[0][c] = 2, 2                          # T and N share the alt: call
    t[0][c + 1] = 4                                  # tumor only
    n[0][c + 2] = 8                                  # normal only
    t[0][c + 3], n[0][c + 3] = 1, 2                  # T one alt, N another
    t[0][c + 4], t[1][c + 4], n[0][c + 4] = 2, 4, 4  # T {X, Y}, N {Y}: call Y only
    t[0][c + 5], n[0][c + 5] = 1, 1                  # both over a reference N
    t[0][c + 6], n[0][c + 6] = 2, 2                  # both over a reference IUPAC code
    t[0][c + 7], n[0][c + 7] = 15, 15                # read N over ACGT in both
    for k, code in enumerate((2, 4, 8)):             # all three alts of one reference base, both datasets
        t[k][c + 8] = n[k][c + 8] = code
    t[0][c + 9], n[0][c + 9] = 1, 1                  # the fourth ACGT code as a call
    for k in range(3):
        b.read([s], s, 0, c - 3, "16M", t[k])
        b.read([s], s, 1, c - 3 - k, "19M", n[k])
    b.call(s, c, 2)
    b.call(s, c + 4, 4)
    b.call(s, c + 8, 2, 4, 8)
    b.call(s, c + 9, 1)


def tile_edge_batch() -> Tuple[Dict[str, np.ndarray], dict]:
    """See the module docstring. Scopes in order: N0 (a window inside H1's region, sharing its
    reference bases and some reads), H1, N2, H3, H4."""
    ss1, sl1, ro1 = 4096, HUGE + 1, 2000
    b5 = ss1 + 5 * TILE                                  # the border the window N0 sits on
    ss0, sl0 = b5 - 300, 700
    ss2, sl2 = 1_200_000, HUGE
    ro2 = ro1 + sl1 + 999
    ss3, sl3 = 2_400_001, HUGE + 2 * TILE + 4097
    ro3 = ro2 + sl2 + 1000 + ((ro2 + sl2 + 1000) % 2 == 0)   # odd
    ss4, sl4 = ss3 + sl3 + 1000, HUGE + 3 * TILE + 7
    ro4 = ro3 + sl3 + 501
    N0, H1, N2, H3, H4 = range(5)
    b = _Builder([(ss0, sl0, ro1 + ss0 - ss1), (ss1, sl1, ro1), (ss2, sl2, ro2), (ss3, sl3, ro3), (ss4, sl4, ro4)], 20250611)
    t1 = lambda k: ss1 + k * TILE
    t3 = lambda k: ss3 + k * TILE
    t4 = lambda k: ss4 + k * TILE

    # ---- H1 and the window N0 ---------------------------------------------------------------
    named = b.named
    named["plain_written"] = b.read([H1], H1, 0, ss1, "9M")          # a written read with no site; the span's start
    named["zero_length"] = b.read([H1], H1, 1, t1(31) + 5, "")
    _border_cluster(b, H1, t1(1))
    # the shared border: the straddling reads are written by the window, the edge reads by H1
    _border_cluster(b, H1, b5, straddle=([N0, H1], N0), edge=([H1, N0], H1))
    alt5 = {b5 - 2: 2, b5 - 1: 4, b5: 8, b5 + 1: 1}
    named["tally_only"] = b.read([H1], -1, 0, b5 - 4, "8M", alt5)    # tallied by H1, written by nobody
    named["unlisted"] = b.read([], -1, 1, b5 - 5, "9M", alt5, home=H1)
    b.set_ref(N0, ss0 + 50, [4])
    b.pair(N0, ss0 + 50, 1, 1)                                       # the window's own site: H1 does not list it
    b.call(N0, ss0 + 50, 1)
    b.read([N0], N0, 0, ss0, "6M")
    b.read([N0], N0, 1, ss0 + sl0 - 6, "6M")
    _border_cluster(b, H1, t1(12))                                   # tile 11 is rare, tile 12 is not
    _border_cluster(b, H1, t1(63))
    # keep: the alt at the last position of tile 62 is kept; a second both-dataset alt there is masked
    b.keep[H1] = (t1(63) - 1, 4)
    b.expect[(H1, t1(63) - 1)] = {8}
    b.read([H1], H1, 0, t1(63) - 2, "3M", {t1(63) - 1: 8})
    b.read([H1], H1, 1, t1(63) - 3, "4M", {t1(63) - 1: 8})
    _border_cluster(b, H1, t1(64), right=False)                      # the last tile: one position
    _classify_block(b, H1, t1(2) + 64)
    # rare tiles
    p = t1(10) + 100
    b.set_ref(H1, p, [1])
    b.pair(H1, p, 0, 0)                                              # '=' in both datasets over A: a call, masked
    b.call(H1, p, 0)
    p = t1(11) + 101
    b.set_ref(H1, p, [2])
    b.pair(H1, p, 6, 6)                                              # one IUPAC code in both datasets: a call
    b.call(H1, p, 6)
    p = t1(14) + 50
    b.set_ref(H1, p, [4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 2])
    b.pair(H1, p, 9, None)                                           # tumor-only IUPAC: rare tile, no call
    b.pair(H1, p + 10, 1, 1)
    b.pair(H1, p + 11, 4, 4)                                         # ... whose ACGT calls count once
    b.call(H1, p + 10, 1)
    b.call(H1, p + 11, 4)
    p = t1(16) + 77
    b.set_ref(H1, p, [10])
    b.pair(H1, p, 10, 10)                                            # IUPAC base equal to an IUPAC reference code
    named["rare_tile_ids"] = {H1: [10, 11, 14], H3: [66], H4: [5]}
    # a read over 129 bases with sites at query positions 63, 64, 127, 128
    p = t1(30) + 1000
    long_subs = {p + q: _rot(b.refc(H1, p + q)) for q in (63, 64, 127, 128)}
    named["long_read"] = b.read([H1], H1, 0, p, "140M", long_subs)
    b.read([H1], H1, 1, p, "140M", long_subs)
    for pp, a in long_subs.items():
        b.call(H1, pp, a)
    # reads of one base: odd-length written reads followed in the buffer by another read
    p = t1(31) + 40
    b.set_ref(H1, p, [8])
    named["one_base"] = b.read([H1], H1, 0, p, "1M", {p: 2})
    b.read([H1], H1, 1, p, "1M", {p: 2})
    b.call(H1, p, 2)

    # ---- N2: exactly 2^20 positions, sites on its first and last position -------------------------
    for p, pos in ((ss2, ss2), (ss2 + HUGE - 1, ss2 + HUGE - 10)):
        a = _rot(b.refc(N2, p), 2)
        b.read([N2], N2, 0, pos, "10M", {p: a})
        b.read([N2], N2, 1, pos, "10M", {p: a})
        b.call(N2, p, a)

    # ---- H3: odd span start, odd reference nibble, odd last tile ----------------------------
    b.read([H3], H3, 1, ss3, "9M")
    _border_cluster(b, H3, t3(1))
    _border_cluster(b, H3, t3(33))
    b.keep[H3] = (t3(33), 1)                                         # another ACGT code than the alt: masked, counted
    _border_cluster(b, H3, t3(66))
    _classify_block(b, H3, t3(3) + 128)
    p = ss3 + sl3 - 1                                                # the span's last position, in a rare odd tile
    b.set_ref(H3, p, [4])
    b.read([H3], H3, 0, p - 4, "5M", {p: 3})
    b.read([H3], H3, 1, p - 6, "7M", {p: 3})
    b.call(H3, p, 3)
    # an insertion directly before a site
    p = t3(8) + 200
    a = _rot(b.refc(H3, p))
    named["insertion"] = b.read([H3], H3, 0, p - 10, "10M2I10M", {p: a})
    b.read([H3], H3, 1, p - 10, "20M", {p: a})
    b.call(H3, p, a)
    # H and P ops
    p = t3(9) + 300
    a = _rot(b.refc(H3, p), 2)
    named["hard_pad"] = b.read([H3], H3, 0, p - 10, "2H3S10M1P10M2H", {p: a})
    b.read([H3], H3, 1, p - 10, "20M", {p: a})
    b.call(H3, p, a)
    # a deletion across a tile border, sites either side
    bp = t3(20)
    subs = {bp - 5: _rot(b.refc(H3, bp - 5)), bp + 4: _rot(b.refc(H3, bp + 4), 3)}
    named["deletion"] = b.read([H3], H3, 0, bp - 11, "8M6D8M", subs)
    b.read([H3], H3, 1, bp - 11, "22M", subs)
    for pp, a in subs.items():
        b.call(H3, pp, a)
    # an N skip longer than two whole tiles, sites in the first and the last segment only
    p0 = t3(40) + 300
    skip = 2 * TILE + 500
    p1 = p0 + 10 + skip
    subs = {p0 + 5: _rot(b.refc(H3, p0 + 5)), p1 + 5: _rot(b.refc(H3, p1 + 5), 2)}
    named["long_skip"] = b.read([H3], H3, 0, p0, f"10M{skip}N10M", subs)
    for pp, a in subs.items():
        b.read([H3], H3, 1, pp - 2, "5M", {pp: a})
        b.call(H3, pp, a)

    # ---- H4: the last scope --------------------------------------------------------------------------
    b.read([H4], H4, 0, ss4, "9M")
    b.read([H4], H4, 1, ss4 + sl4 - 9, "9M")
    p = t4(2) + 700                                                  # a tile with tumor reads only: no call
    for k in range(3):
        b.read([H4], H4, 0, p - k, "12M", {p + 3: _rot(b.refc(H4, p + 3)), p + 4 + k: _rot(b.refc(H4, p + 4 + k), 2)})
    named["tumor_only_tile"] = (H4, 2)
    p = t4(5) + 9                                                    # a rare tile: the kept variant is an IUPAC code
    b.set_ref(H4, p, [1, 2, 4, 8, 1])
    b.pair(H4, p, 12, 12)
    b.keep[H4] = (p, 12)
    b.pair(H4, p + 1, 12, 12)                                        # the same code one position on is a call
    b.call(H4, p + 1, 12)
    b.pair(H4, p + 4, 8, 8)
    b.call(H4, p + 4, 8)

    named["borders"] = {H1: [t1(1), b5, t1(12), t1(63), t1(64)], H3: [t3(1), t3(33), t3(66)]}
    named["classify"] = {H1: t1(2) + 64, H3: t3(3) + 128}
    named["rare_tiles"] = 5
    return b.finish()


def _flat(starts, codes, ds, span_start, span_len, ref, cigar_len) -> Dict[str, np.ndarray]:
    """One scope that lists and writes every read; all reads ``cigar_len`` M; incidences permuted."""
    n = len(starts)
    half = (cigar_len + 1) // 2
    if cigar_len & 1:
        codes = np.concatenate([codes, np.zeros((n, 1), np.uint8)], axis=1)
    k = n // 2 + 1
    while gcd(k, n) != 1:
        k += 1
    return {
        "ref_start": starts.astype(np.int32),
        "read_len": np.full(n, cigar_len, np.int32),
        "seq_off": np.arange(n, dtype=np.int64) * half,
        "seq_nt16": ((codes[:, 0::2] << 4) | codes[:, 1::2]).reshape(-1).astype(np.uint8),
        "cig_off": np.arange(n, dtype=np.int64),
        "n_cig": np.ones(n, np.int32),
        "cigar": np.full(n, _cigar_word("M", cigar_len), np.uint32),
        "dataset": ds.astype(np.uint8),
        "write_scope": np.zeros(n, np.int32),
        "scope_incid_off": np.array([0, n], np.int64),
        "incid_read": ((np.arange(n, dtype=np.int64) * k + 1) % n).astype(np.int32),
        "scope_span_start": np.array([span_start], np.int32),
        "scope_span_len": np.array([span_len], np.int32),
        "scope_ref_off": np.array([3], np.int64),
        "ref_nt16": pack_nibbles(ref),
        "keep_pos": np.full(1, -1, np.int32),
        "keep_code": np.zeros(1, np.uint8),
    }


_ROT = np.zeros(16, np.uint8)
_ROT[[1, 2, 4, 8]] = [2, 4, 8, 1]


def rare_stride_batch(tiles: int = 1030) -> Tuple[Dict[str, np.ndarray], dict]:
    """One huge scope of ``tiles`` tiles. Each tile holds a tumor and a normal 4M read over the same
    four positions: a both-dataset ACGT alt on the third base, a tumor-only '=' on the fourth. Every
    tile is rare and makes one call; more tiles than the re-run's 1,024 workgroups."""
    ss, sl = 1001, tiles * TILE
    ref = ACGT[np.random.default_rng(1030).integers(0, 4, sl + 68)]
    k = np.arange(tiles, dtype=np.int64)
    off = (k * 37) % (TILE - 8)
    off[-1] = TILE - 4                                   # the last read ends on the span's end
    pos = ss + k * TILE + off
    starts = np.repeat(pos, 2)
    ds = np.tile([0, 1], tiles)
    codes = ref[(starts - ss + 3)[:, None] + np.arange(4)[None, :]].copy()
    rc = codes[:, 2].copy()
    codes[:, 2] = _ROT[rc]
    codes[0::2, 3] = 0
    arr = _flat(starts, codes, ds, ss, sl, ref, 4)
    r = np.arange(2 * tiles, dtype=np.int64)
    info = {"must_mask": np.stack([r, np.full_like(r, 2), rc.astype(np.int64)], axis=1),
            "must_not": np.stack([r[0::2], np.full(tiles, 3, np.int64)], axis=1),
            "calls_per_scope": np.array([tiles], np.int32), "tiles_per_scope": np.array([tiles], np.int64),
            "rare_tiles": tiles, "huge_written_reads": 2 * tiles}
    return arr, info


def crowd_batch(n_reads: int = 33000) -> Tuple[Dict[str, np.ndarray], dict]:
    """One huge scope that writes ``n_reads`` 2M reads (more than 8192 workgroups of four waves): pairs
    of a tumor and a normal read on a position of their own, an alt on the first base, half of the pairs
    from the span's start (the first tiles), half up to its end (the last tiles). Every 97th read
    carries no alt, so its pair makes no call and its partner's alt stays."""
    ss, sl = 501, HUGE + 5 * TILE + 3
    ref = ACGT[np.random.default_rng(33000).integers(0, 4, sl + 68)]
    pairs = n_reads // 2
    j = np.arange(pairs, dtype=np.int64)
    pos = np.where(j < pairs // 2, ss + 2 * j, ss + sl - 2 - 2 * (j - pairs // 2))
    starts = np.repeat(pos, 2)
    ds = np.tile([0, 1], pairs)
    codes = ref[(starts - ss + 3)[:, None] + np.arange(2)[None, :]].copy()
    rc = codes[:, 0].copy()
    r = np.arange(2 * pairs, dtype=np.int64)
    plain = r % 97 == 0
    codes[~plain, 0] = _ROT[rc[~plain]]
    arr = _flat(starts, codes, ds, ss, sl, ref, 2)
    call = ~(plain[0::2] | plain[1::2])
    masked = np.repeat(call, 2)
    info = {"must_mask": np.stack([r[masked], np.zeros(int(masked.sum()), np.int64), rc[masked].astype(np.int64)], axis=1),
            "must_not": np.stack([r[~masked & ~plain], np.zeros(int((~masked & ~plain).sum()), np.int64)], axis=1),
            "calls_per_scope": np.array([int(call.sum())], np.int32),
            "tiles_per_scope": np.array([n_tiles(sl)], np.int64), "rare_tiles": 0, "huge_written_reads": 2 * pairs}
    return arr, info


def threshold_pair():
    """((arrays, info), (arrays, info)): one scope whose span is 2^20 positions, then 2^20 + 1 after
    its last tumor read moved one base on (nothing else differs). The reference under the span's end is
    a run of A, so the moved read still equals it except for its two alts."""
    res = []
    for shift in (0, 1):
        ss = 777
        e = ss + HUGE
        b = _Builder([(ss, HUGE + shift, ss + 11)], 2020, ref_len=ss + 11 + HUGE + 66)
        b.set_ref(0, e - 12, [1] * 14)
        a = _rot(b.refc(0, ss))
        b.read([0], 0, 0, ss, "10M", {ss: a})
        b.read([0], 0, 1, ss, "10M", {ss: a})
        b.call(0, ss, a)
        b.read([0], 0, 1, e - 10, "10M", {e - 2: 2, e - 1: 2})
        mover = b.read([0], 0, 0, e - 10 + shift, "10M", {e - 2 + shift: 2, e - 1 + shift: 2})
        b.call(0, e - 1, 2)
        if not shift:
            b.call(0, e - 2, 2)
        b.named["mover"] = mover
        b.named["rare_tiles"] = 0
        res.append(b.finish())
    return tuple(res)
