"""Helpers of the tests of --discover_sites' evidence filters and rule (--discover_min_base_quality,
--discover_min_mapq, --discover_exclude_flags, --discover_rule). The filtered tally and both modes are
restated here in plain Python, independently of the C++, over decoded tables and over hand-built records;
no expectation ever comes from the code under test. ``hand_built`` is a record set of the filters'
corners on discover_helpers' short contigs, with literal expectations under the rule FULL in both modes;
``scenario_sites`` is D(X; rule) of a golden scenario."""
from __future__ import annotations

import os
import struct
from collections import namedtuple

import numpy as np

import discover_helpers as D
import known_sites_helpers as K

TILE = D.TILE
CODE = K.CODE
NT16 = K.NT16
HAND_CONTIGS = D.HAND_CONTIGS

Rule = namedtuple("Rule", "q m f mode")
ZERO = Rule(0, 0, 0, "both")
Q, MQ, F = 20, 30, 0x700                 # the thresholds the hand-built set is laid around
FULL = Rule(Q, MQ, F, "both")
FULL_NORMAL = Rule(Q, MQ, F, "normal")
RULES = (ZERO, Rule(Q, 0, 0, "both"), Rule(0, MQ, 0, "both"), Rule(0, 0, F, "both"), FULL, Rule(0, 0, 0, "normal"),
         Rule(Q, 0, 0, "normal"), FULL_NORMAL, Rule(Q + 1, MQ + 1, 0x400, "normal"))
ENVS = ("GANON_DISCOVER_MIN_BASE_QUALITY", "GANON_DISCOVER_MIN_MAPQ", "GANON_DISCOVER_EXCLUDE_FLAGS", "GANON_DISCOVER_RULE")


def site_rule(rule: Rule):
    from genomeanonymizer_amd.native import SiteRule
    return SiteRule(rule.q, rule.m, rule.f, rule.mode)


def set_rule(monkeypatch, rule) -> None:
    """The four environment defaults of ``rule`` (None: all unset)."""
    for env, v in zip(ENVS, rule if rule is not None else (None,) * 4):
        if v is None:
            monkeypatch.delenv(env, raising=False)
        else:
            monkeypatch.setenv(env, str(v))


# ---- the rule --------------------------------------------------------------------------------------------

def tally_record(ev: dict, contig, ref, flag: int, mapq: int, pos: int, cigar, nib, qual, ds: int, rule: Rule) -> None:
    """One record's evidence under ``rule``'s filters into ``ev``: (contig, position) -> [tumor allele mask,
    normal allele mask]. ``cigar``: (op letter, length) pairs; ``nib``: the l_seq base codes; ``qual``: the
    l_seq quality bytes (0..255); ``ref``: the contig's FASTA text or None; ``contig`` None: no such tid."""
    if (flag & 4) or contig is None or ref is None or not cigar or not len(nib):
        return
    if mapq < rule.m or (flag & rule.f):
        return
    r, x = pos, 0
    for op, n in cigar:
        if op in "M=X":
            for _ in range(n):
                if x < len(nib) and 0 <= r < len(ref):
                    b, f = nib[x], CODE.get(ref[r].upper(), 0)
                    if b in (1, 2, 4, 8) and f and b != f and int(qual[x]) >= rule.q:
                        ev.setdefault((contig, r), [0, 0])[ds] |= b
                r += 1
                x += 1
        elif op in "IS":
            x += n
        elif op in "DN":
            r += n


def tally_records(ev: dict, recs, fa: dict, ds: int, rule: Rule) -> None:
    for r in recs:
        contig = HAND_CONTIGS[r["tid"]][0] if 0 <= r["tid"] < len(HAND_CONTIGS) else None
        tally_record(ev, contig, fa.get(contig) if contig is not None else None, r["flag"], r["mapq"], r["pos"], r["cigar"],
                     r["nib"], r["qual"], ds, rule)


def tally_table(ev: dict, t, fa: dict, ds: int, rule: Rule) -> None:
    """The evidence of every record of a decoded table (io.bam.ReadTable)."""
    names = list(t.ref_names)
    qual = np.asarray(t.qual)
    for i in range(t.n):
        tid = int(t.tid[i])
        contig = names[tid] if 0 <= tid < len(names) and names.index(names[tid]) == tid else None
        cig = [(K.OPS[w & 15] if (w & 15) < 9 else "?", int(w >> 4)) for w in t.cigar_of(i).tolist()]
        qo = int(t.qual_off[i])
        tally_record(ev, contig, fa.get(contig) if contig is not None else None, int(t.flag[i]), int(t.mapq[i]),
                     int(t.pos[i]), cig, K.table_nibbles(t, i), qual[qo:qo + int(t.l_seq[i])].tolist(), ds, rule)


def sites_of(ev: dict, fa: dict, mode: str) -> dict:
    """contig -> {position: (ref_nt16, alt mask)}: mode "both" the alleles both datasets show, "normal"
    the alleles the normal shows."""
    out: dict = {}
    for (contig, p), (t, n) in ev.items():
        alt = n if mode == "normal" else t & n
        if alt:
            out.setdefault(contig, {})[p] = (CODE[fa[contig][p].upper()], alt)
    return out


# ---- D(X; rule) of a golden scenario ---------------------------------------------------------------------

_SCEN: dict = {}


def scenario_sites(name: str, rule: Rule) -> dict:
    """{"sites": D(X; rule), "less_own": less the scenario's own SNV positions, as known_sites_helpers.Sites,
    "plain": D(X) of discover_helpers} for golden scenario ``name``, once per rule."""
    if (name, rule) in _SCEN:
        return _SCEN[(name, rule)]
    from genomeanonymizer_amd.io.bam import ReadTable
    base = D.scenario_sites(name)
    tables = _SCEN.get(name)
    if tables is None:
        tables = _SCEN[name] = [ReadTable(base["paths"][s], threads=2) for s in ("T", "N")]
    ev: dict = {}
    for ds, t in enumerate(tables):
        tally_table(ev, t, base["fa"], ds, rule)
    sites = sites_of(ev, base["fa"], rule.mode)
    out = _SCEN[(name, rule)] = {"sites": sites, "less_own": K.Sites(D.less_own(sites, base["own"])), "plain": base["sites"]}
    return out


# ---- records and streams with a mapq ---------------------------------------------------------------------

def bam_record(tid, pos, flag, mapq, cigar, nib, qual, name=b"r\x00") -> bytes:
    """One BAM record from (op letter, length) pairs, base codes and l_seq quality bytes."""
    L = len(nib)
    full = list(nib) + ([0] if L & 1 else [])
    packed = bytes((full[k] << 4) | full[k + 1] for k in range(0, len(full), 2))
    cig = b"".join(struct.pack("<I", (n << 4) | K.OPS.index(op)) for op, n in cigar)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, 4680, len(cigar), flag, L, -1, -1, 0)
    body += name + cig + packed + bytes(qual)
    return struct.pack("<i", len(body)) + body


def stream_of(recs):
    """(inflated BAM stream, offset of its first record) of hand-built records, in the order given."""
    from test_bam_device import _header
    head = _header(HAND_CONTIGS)
    body = b"".join(bam_record(r["tid"], r["pos"], r["flag"], r["mapq"], r["cigar"], r["nib"], r["qual"],
                               name=f"r{k}".encode() + b"\x00") for k, r in enumerate(recs))
    return np.frombuffer(head + body, np.uint8), len(head)


# ---- the hand-built set ----------------------------------------------------------------------------------

def hand_built():
    """(tumor records, normal records, FASTA dict, literal expectations). Records are dicts (tid, pos, flag,
    mapq, cigar, nib, qual), in coordinate order, those no index can list marked ``"no_index": True``. The
    literal expectations hold under FULL (Q 20, mapq 30, flags 0x700): {"both" / "normal": {"site": {(contig,
    pos): alt mask}, "none": [(contig, pos), ...]}}, and "zero_none": positions without a site under the zero
    rule too. A base under test has the stated quality; its neighbours in the read have a quality on the
    other side of Q, so that a quality read at a wrong index gives the wrong outcome."""
    fa = D.hand_fasta()
    T = TILE
    recs = ([], [])
    lit = {"both": {"site": {}, "none": []}, "normal": {"site": {}, "none": []}, "zero_none": []}

    def alts(contig, p):
        return [CODE[b] for b in "ACGT" if b != fa[contig][p].upper()]

    def expect(contig, p, alt, both, normal):
        for mode, on in (("both", both), ("normal", normal)):
            if on:
                lit[mode]["site"][(contig, p)] = on if on is not True else alt
            else:
                lit[mode]["none"].append((contig, p))

    def read(ds, tid, pos, cigar, edits=None, flag=0, mapq=60, L=None, fill=None, **kw):
        """A read that shows the reference under M / = / X and A under I and S, then ``edits`` {query index:
        (code, quality)}; the other bases get quality ``fill`` (default: 40 when any edited base fails Q,
        else 0 — the other side)."""
        contig = HAND_CONTIGS[tid][0]
        ref = fa.get(contig, "")
        nib, r = [], pos
        for op, n in cigar:
            if op in "M=X":
                nib += [NT16.index(ref[p].upper()) if 0 <= p < len(ref) else 1 for p in range(r, r + n)]
                r += n
            elif op in "IS":
                nib += [1] * n
            elif op in "DN":
                r += n
        if L is not None:
            nib = (nib + [1] * L)[:L]
        edits = edits or {}
        if fill is None:
            fill = 40 if any(q < Q for _, q in edits.values()) else 0
        qual = [fill] * len(nib)
        for x, (b, q) in edits.items():
            nib[x], qual[x] = b, q
        recs[ds].append(dict(tid=tid, pos=pos, flag=flag, mapq=mapq, cigar=cigar, nib=nib, qual=qual, **kw))

    def both(tid, pos, cigar, edits=None, **kw):
        for ds in (0, 1):
            read(ds, tid, pos, cigar, edits, **kw)

    # ---- qualities Q-1, Q, Q+1, 0, 93, 0xFF on the first base, the last base (odd index) of an even read, the
    # last base (even index) and an odd index of an odd-length read
    at = 300
    for qv in (Q - 1, Q, Q + 1, 0, 93, 0xFF):
        for L, x in ((8, 0), (8, 7), (7, 6), (7, 3)):
            a = alts("h3", at + x)[0]
            both(2, at, [("M", L)], {x: (a, qv)})
            expect("h3", at + x, a, qv >= Q, qv >= Q)
            at += 10
    assert at == 540
    # ---- a mismatch at each offset of the eight-base steps of a 21-base read (8, 8 and a tail of 5)
    for j in range(21):
        p0 = 600 + 25 * j
        a, qv = alts("h3", p0 + j)[1], (Q if j % 2 == 0 else Q - 1)
        both(2, p0, [("M", 21)], {j: (a, qv)})
        expect("h3", p0 + j, a, qv >= Q, qv >= Q)
    # ... and every base of one read a mismatch, every third one passing
    both(2, 1150, [("M", 21)], {j: (alts("h3", 1150 + j)[2], Q + 5 if j % 3 == 0 else Q - 5) for j in range(21)}, fill=0)
    for j in range(21):
        expect("h3", 1150 + j, alts("h3", 1150 + j)[2], j % 3 == 0, j % 3 == 0)
    # ---- a passing and a failing read showing one allele at one position
    a = alts("h3", 1202)[0]
    for ds in (0, 1):
        read(ds, 2, 1200, [("M", 5)], {2: (a, Q - 1)})
        read(ds, 2, 1201, [("M", 5)], {1: (a, Q)})
    expect("h3", 1202, a, True, True)
    a = alts("h3", 1212)[0]
    read(0, 2, 1210, [("M", 5)], {2: (a, Q)})                 # the normal's reads both fail: no evidence of it
    read(1, 2, 1210, [("M", 5)], {2: (a, Q - 1)})
    read(1, 2, 1211, [("M", 5)], {1: (a, 0)})
    expect("h3", 1212, a, False, False)
    a = alts("h3", 1222)[0]
    read(0, 2, 1220, [("M", 5)], {2: (a, Q - 1)})             # the tumor's fails, the normal's passes
    read(1, 2, 1220, [("M", 5)], {2: (a, Q)})
    expect("h3", 1222, a, False, True)
    # ---- query index ahead of and behind the reference: H S M I D M N M P M = X S H (as discover_helpers):
    # aligned [100,104) [106,109) [209,213) [213,216) [216,218), first / last base of each op
    ops = [("H", 3), ("S", 2), ("M", 4), ("I", 2), ("D", 2), ("M", 3), ("N", 100), ("M", 4), ("P", 1), ("=", 3),
           ("X", 2), ("S", 3), ("H", 2)]
    qidx = {100: 2, 103: 5, 106: 8, 108: 10, 209: 11, 212: 14, 213: 15, 215: 17, 216: 18, 217: 19}
    edits = {}
    for k, (p, x) in enumerate(sorted(qidx.items())):
        qv = Q if k % 2 == 0 else Q - 1
        edits[x] = (alts("h3", p)[0], qv)
        expect("h3", p, alts("h3", p)[0], qv >= Q, qv >= Q)
    # (the fill, 40, is the quality of the clipped and inserted bases at the query indexes of a walk that
    # forgot an op)
    both(2, 100, ops, edits)
    # ---- a CIGAR longer than l_seq
    both(2, 1300, [("M", 10)], {1: (alts("h3", 1301)[0], Q), 4: (alts("h3", 1304)[0], Q - 1)}, L=5, fill=Q)
    expect("h3", 1301, alts("h3", 1301)[0], True, True)
    expect("h3", 1304, alts("h3", 1304)[0], False, False)
    both(2, 1310, [("M", 10)], {4: (alts("h3", 1314)[1], Q)}, L=5)
    expect("h3", 1314, alts("h3", 1314)[1], True, True)
    # ---- records placed before the sequence's start (stream form only): the walk's clip moves the quality
    # index with the query index. pos -1: query 1 is position 0. pos -3: query 4 is position 1, query 5 position 2
    both(2, -1, [("M", 4)], {1: (alts("h3", 0)[0], Q), 0: (2, 0)}, fill=0, no_index=True)
    expect("h3", 0, alts("h3", 0)[0], True, True)
    q3 = {4: (alts("h3", 1)[0], Q - 1), 5: (alts("h3", 2)[0], Q), 1: (fa_code(fa, "h3", 1), 40), 2: (fa_code(fa, "h3", 2), 0),
          0: (2, 40), 3: (fa_code(fa, "h3", 0), 40)}
    both(2, -3, [("M", 6)], q3, no_index=True)
    expect("h3", 1, alts("h3", 1)[0], False, False)
    expect("h3", 2, alts("h3", 2)[0], True, True)
    # ---- mapq M-1, M, 0, 255 (qualities pass)
    for k, mq in enumerate((MQ - 1, MQ, 0, 255)):
        p = 1400 + 10 * k
        both(2, p, [("M", 5)], {2: (alts("h3", p + 2)[0], 40)}, mapq=mq)
        expect("h3", p + 2, alts("h3", p + 2)[0], mq >= MQ, mq >= MQ)
    # ---- each bit of F alone, a set bit outside F, two bits of F, flag & 4 (which no rule lets in)
    for k, fl in enumerate((0x100, 0x200, 0x400, 0x800, 0x600, 0x800 | 1 | 16, 4 | 1)):
        p = 1500 + 10 * k
        both(2, p, [("M", 5)], {2: (alts("h3", p + 2)[0], 40)}, flag=fl)
        expect("h3", p + 2, alts("h3", p + 2)[0], not (fl & (F | 4)), not (fl & (F | 4)))
        if fl & 4:
            lit["zero_none"].append(("h3", p + 2))
    # ---- the modes
    a = alts("h3", 1602)
    read(1, 2, 1600, [("M", 5)], {2: (a[0], 40)})             # normal-only: a site under normal
    read(0, 2, 1600, [("M", 5)])
    expect("h3", 1602, a[0], False, True)
    a = alts("h3", 1612)
    read(0, 2, 1610, [("M", 5)], {2: (a[0], 40)})             # tumor-only: none
    read(1, 2, 1610, [("M", 5)])
    expect("h3", 1612, a[0], False, False)
    lit["zero_none"].append(("h3", 1612))
    a = alts("h3", 1622)
    read(0, 2, 1620, [("M", 5)], {2: (a[0], 40)})             # tumor a0, normal a1: ALT a1 alone under normal
    read(1, 2, 1620, [("M", 5)], {2: (a[1], 40)})
    expect("h3", 1622, a[1], False, True)
    a = alts("h3", 1632)
    read(1, 2, 1630, [("M", 5)], {2: (a[0], 40)})             # normal {a0, a2}: both ALTs under normal
    read(1, 2, 1631, [("M", 5)], {1: (a[2], 40)})
    read(0, 2, 1630, [("M", 5)], {2: (a[1], 40)})             # (the tumor's a1 is no ALT)
    expect("h3", 1632, a[0] | a[2], False, a[0] | a[2])
    # reference N (h2 12) and an ambiguity code (16): none; h2 10 (G): the normal's A is a site under normal
    read(1, 1, 10, [("M", 8)], {0: (1, 40), 2: (2, 40), 6: (2, 40)}, fill=40)
    read(0, 1, 10, [("M", 8)])
    expect("h2", 10, 1, False, True)
    expect("h2", 12, 2, False, False)
    expect("h2", 16, 2, False, False)
    # sites at T - 1, T, T + 1 and 2 T from the normal alone; at T + 10, 2 T - 1 and the last position from both
    for p in (T - 1, T, T + 1, 2 * T):
        read(1, 2, p - 2, [("M", 5)], {2: (alts("h3", p)[0], Q)})
        expect("h3", p, alts("h3", p)[0], False, True)
    for p in (T + 10, 2 * T - 1, 3 * T):
        both(2, p - 2, [("M", 5)], {2: (alts("h3", p)[0], Q)})
        expect("h3", p, alts("h3", p)[0], True, True)
    # ---- 300 one-base records a dataset (more than one workgroup; four positions share a tally word)
    for p in range(4200, 4500):
        qv = Q - 1 + p % 3
        both(2, p, [("M", 1)], {0: (alts("h3", p)[p % 3], qv)})
        expect("h3", p, alts("h3", p)[p % 3], qv >= Q, qv >= Q)
    # ---- long CIGARs (the wave path): 48, 49, 64, 65 and 129 ops, random bases, random qualities 3..39
    for ds, seeds in ((0, (9,)), (1, (9, 11))):
        for seed in seeds:
            for r in K.long_cigar_records((48, 49, 64, 65, 129), seed=seed):
                assert min(r["qual"]) < Q <= max(r["qual"])
                recs[ds].append(dict(r, tid=2, pos=r["pos"] + 3000, mapq=60))
    # ... one of them below the mapq threshold and one with an excluded flag
    for ds in (0, 1):
        for k, r in enumerate(K.long_cigar_records((65, 129), seed=13)):
            recs[ds].append(dict(r, tid=2, pos=r["pos"] + 3500, mapq=MQ - 1 if k == 0 else 60, flag=0 if k == 0 else 0x400))
    # h4 is not in the FASTA
    both(3, 10, [("M", 6)], {k: (2, 40) for k in range(6)})
    for ds in (0, 1):
        recs[ds].sort(key=lambda r: (r["tid"], max(r["pos"], -1)))
    return recs[0], recs[1], fa, lit


def fa_code(fa: dict, contig: str, p: int) -> int:
    return CODE[fa[contig][p].upper()]


_EXP: dict = {}


def expected_hand(rule: Rule) -> dict:
    """The hand-built set's sites under ``rule`` by the restatement; under FULL and FULL_NORMAL (and, for what
    no rule lets in, ZERO) checked against the literal expectations."""
    if rule in _EXP:
        return _EXP[rule]
    t, n, fa, lit = hand_built()
    ev: dict = {}
    tally_records(ev, t, fa, 0, rule)
    tally_records(ev, n, fa, 1, rule)
    sites = sites_of(ev, fa, rule.mode)
    if rule in (FULL, FULL_NORMAL):
        for (c, p), alt in lit[rule.mode]["site"].items():
            assert sites.get(c, {}).get(p) == (CODE[fa[c][p].upper()], alt), (rule, c, p, sites.get(c, {}).get(p))
        for c, p in lit[rule.mode]["none"]:
            assert p not in sites.get(c, {}), (rule, c, p)
    if rule == ZERO:
        for c, p in lit["zero_none"]:
            assert p not in sites.get(c, {}), (c, p)
    assert "h1" not in sites and "h4" not in sites
    _EXP[rule] = sites
    return sites


def write_hand_files(d: str, indexed: bool = True) -> dict:
    """The hand-built set as files: a FASTA and the tumor and normal BAMs, through the generator's writer
    (coordinate order, with an index; the records no index can list left out) or as plain BGZF streams
    of every record. The expectations of the indexed files are ``expected_hand`` only where the records left
    out change nothing: ``expected_indexed``."""
    from genomeanonymizer_amd.synth import bamwriter as W
    os.makedirs(d, exist_ok=True)
    t, n, fa, _ = hand_built()
    ref = os.path.join(d, "rules.fa")
    W.write_fasta(ref, [(c, fa[c]) for c, _ in HAND_CONTIGS if c in fa])
    out = {"ref": ref, "fa": fa}
    for tag, recs in (("T", t), ("N", n)):
        path = os.path.join(d, f"rules_{tag}{'_idx' if indexed else ''}.bam")
        if indexed:
            brs = [W.BamRecord(f"r{k}", r["flag"], r["tid"], r["pos"], r["mapq"], r["cigar"], -1, -1, 0,
                               "".join(NT16[b] for b in r["nib"]), r["qual"])
                   for k, r in enumerate(recs) if not r.get("no_index")]
            W.write_bam(path, HAND_CONTIGS, brs, index=True)
        else:
            W.write_bgzf(path, stream_of(recs)[0].tobytes())
        out[tag] = path
    return out


def expected_indexed(rule: Rule) -> dict:
    """The sites of the indexed files: the hand-built set without the records no index can list."""
    t, n, fa, _ = hand_built()
    ev: dict = {}
    tally_records(ev, [r for r in t if not r.get("no_index")], fa, 0, rule)
    tally_records(ev, [r for r in n if not r.get("no_index")], fa, 1, rule)
    return sites_of(ev, fa, rule.mode)
