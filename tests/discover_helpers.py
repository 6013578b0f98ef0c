"""Helpers of the --discover_sites tests. The tally rule is restated here in plain Python — over decoded
tables (``table_nibbles``, ``cigar_of`` and a FASTA dict) and over hand-built records — and no expectation
ever comes from the code under test. ``hand_built`` is a record set of the rule's corners on three short
contigs (and a header sequence the FASTA lacks); ``scenario_sites`` is D(X) of a golden scenario."""
from __future__ import annotations

import os

import numpy as np

import known_sites_helpers as K

TILE = 2048     # positions per workgroup of k_site_compact (native.site_compact_tile(); the GPU tests check it)
CODE = K.CODE
NT16 = K.NT16


# ---- the rule --------------------------------------------------------------------------------------------

def tally_record(ev: dict, contig, ref, flag: int, pos: int, cigar, nib, ds: int) -> None:
    """One record's evidence into ``ev``: (contig, position) -> [tumor allele mask, normal allele mask].
    ``cigar``: (op letter, length) pairs; ``nib``: the l_seq base codes; ``ref``: the contig's FASTA text or
    None when the FASTA lacks it; ``contig`` None: tid outside the header."""
    if (flag & 4) or contig is None or ref is None or not cigar or not len(nib):
        return
    L = len(nib)
    r, q = pos, 0
    for op, n in cigar:
        if op in "M=X":
            for k in range(n):
                x, p = q + k, r + k
                if x < L and 0 <= p < len(ref):
                    b, f = nib[x], CODE.get(ref[p].upper(), 0)
                    if b in (1, 2, 4, 8) and f and b != f:
                        ev.setdefault((contig, p), [0, 0])[ds] |= b
            r += n
            q += n
        elif op in "IS":
            q += n
        elif op in "DN":
            r += n


def tally_table(ev: dict, t, fa: dict, ds: int) -> None:
    """The evidence of every record of a decoded table (io.bam.ReadTable)."""
    names = list(t.ref_names)
    for i in range(t.n):
        tid = int(t.tid[i])
        contig = names[tid] if 0 <= tid < len(names) and names.index(names[tid]) == tid else None
        cig = [(K.OPS[w & 15] if (w & 15) < 9 else "?", int(w >> 4)) for w in t.cigar_of(i).tolist()]
        tally_record(ev, contig, fa.get(contig) if contig is not None else None, int(t.flag[i]), int(t.pos[i]), cig,
                     K.table_nibbles(t, i), ds)


def tally_records(ev: dict, recs, contigs, fa: dict, ds: int) -> None:
    """The evidence of hand-built records (dicts of known_sites_helpers.bam_record's arguments)."""
    for r in recs:
        contig = contigs[r["tid"]][0] if 0 <= r["tid"] < len(contigs) else None
        tally_record(ev, contig, fa.get(contig) if contig is not None else None, r["flag"], r["pos"], r["cigar"],
                     r["nib"], ds)


def sites_of(ev: dict, fa: dict) -> dict:
    """contig -> {position: (ref_nt16, alt mask)} of the positions both datasets show one allele at."""
    out: dict = {}
    for (contig, p), (t, n) in ev.items():
        if t & n:
            out.setdefault(contig, {})[p] = (CODE[fa[contig][p].upper()], t & n)
    return out


def panel_as_dict(panel) -> dict:
    """A known_sites.Panel in the shape of ``sites_of`` (contigs without sites left out)."""
    return {c: {int(p): (int(v) >> 4, int(v) & 15) for p, v in zip(pos.tolist(), code.tolist())}
            for c, (pos, code) in panel.contigs.items() if len(pos)}


def lists_as_dict(names, lists) -> dict:
    """[(positions, codes) or None per sequence] in the shape of ``sites_of``; the lists must be sorted."""
    out = {}
    for name, pc in zip(names, lists):
        if pc is None or not len(pc[0]):
            continue
        pos, code = np.asarray(pc[0]), np.asarray(pc[1])
        assert (np.diff(pos) > 0).all(), name
        out[name] = {int(p): (int(v) >> 4, int(v) & 15) for p, v in zip(pos.tolist(), code.tolist())}
    return out


def less_own(sites: dict, own: dict) -> dict:
    return {c: {p: v for p, v in d.items() if p not in own.get(c, ())} for c, d in sites.items()}


# ---- D(X) of a golden scenario -----------------------------------------------------------------------------

_SCEN: dict = {}


def scenario_sites(name: str) -> dict:
    """{"sites": D(X) as ``sites_of``, "less_own": D(X) less the scenario's own SNV positions as
    known_sites_helpers.Sites, "own": those positions, "paths": X} for golden scenario ``name``, once."""
    if name in _SCEN:
        return _SCEN[name]
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth import generate as G
    paths = G.make_inputs(name, os.path.join(K._tmpdir(), "discover_" + name), False)
    fa = K._fasta(paths["ref"])
    ev: dict = {}
    for ds, s in enumerate(("T", "N")):
        tally_table(ev, ReadTable(paths[s], threads=2), fa, ds)
    sites = sites_of(ev, fa)
    own = K.own_vcf_snv_positions(paths["vcf"])
    out = _SCEN[name] = {"sites": sites, "own": own, "less_own": K.Sites(less_own(sites, own)), "paths": paths, "fa": fa}
    return out


# ---- a hand-built record set -------------------------------------------------------------------------------

HAND_CONTIGS = [("h1", 1), ("h2", 40), ("h3", 3 * TILE + 1), ("h4", 500)]     # h4 is not in the FASTA
H2 = "ACGTACGTACGTNACGRTACgtacgtACGTACGTACGTAC"                               # N at 12, R at 16, lower case 20..25


def hand_fasta() -> dict:
    rng = np.random.default_rng(41)
    return {"h1": "A", "h2": H2, "h3": "".join("ACGT"[int(x)] for x in rng.integers(0, 4, 3 * TILE + 1))}


def hand_built():
    """(tumor records, normal records, FASTA dict, literal expectations). Records are dicts of
    known_sites_helpers.bam_record's arguments, in coordinate order, the records no index can list (a tid
    past the header) marked ``"no_index": True``. The literal expectations: {"site": {(contig, pos): alt mask},
    "none": [(contig, pos), ...]} for the cases whose outcome is stated by hand."""
    fa = hand_fasta()
    h3 = fa["h3"]
    T = TILE
    recs = ([], [])
    lit = {"site": {}, "none": []}

    def alts(contig, p):
        """The three bases other than the reference's at p, as codes, in A C G T order."""
        return [CODE[b] for b in "ACGT" if b != fa[contig][p].upper()]

    def read(ds, tid, pos, cigar, edits=None, flag=0, L=None, clip=1, **kw):
        """A read that shows the reference under its M / = / X ops (ambiguity codes as they are, N as 15),
        ``clip`` under I and S, then ``edits`` {query index: code}."""
        contig = HAND_CONTIGS[tid][0] if 0 <= tid < len(HAND_CONTIGS) else None
        ref = fa.get(contig, "")
        nib, r = [], pos
        for op, n in cigar:
            if op in "M=X":
                nib += [NT16.index(ref[p].upper()) if 0 <= p < len(ref) else 1 for p in range(r, r + n)]
                r += n
            elif op in "IS":
                nib += [clip] * n
            elif op in "DN":
                r += n
        if L is not None:
            nib = (nib + [1] * L)[:L]
        for x, b in (edits or {}).items():
            nib[x] = b
        recs[ds].append(dict(tid=tid, pos=pos, flag=flag, cigar=cigar, nib=nib, qual=[30] * len(nib), **kw))

    def both(tid, pos, cigar, edits=None, **kw):
        for ds in (0, 1):
            read(ds, tid, pos, cigar, edits, **kw)

    # h1, one base: tumor evidence alone at its only position: a touched contig without sites
    read(0, 0, 0, [("M", 1)], {0: 2})
    read(1, 0, 0, [("M", 1)])
    lit["none"].append(("h1", 0))
    # h2: reference N (12), an ambiguity code (16), lower case (20..25); read codes 15, 3 and 5
    both(1, 10, [("M", 8)], {2: 2, 6: 2})                     # against N and against R: no evidence
    lit["none"] += [("h2", 12), ("h2", 16)]
    both(1, 20, [("M", 6)], {0: 8, 5: 1})                     # g -> T at 20, t -> A at 25: lower case is folded
    lit["site"][("h2", 20)] = 8
    lit["site"][("h2", 25)] = 1
    both(1, 26, [("M", 4)], {0: 15, 1: 3, 2: 5})              # N, M (A|C) and R (A|G) in the read: no evidence
    lit["none"] += [("h2", 26), ("h2", 27), ("h2", 28)]
    both(1, 36, [("M", 8)], {3: 1, 4: 2, 7: 2})               # runs past the end: 39 is the last position (C -> A)
    lit["site"][("h2", 39)] = 1
    both(1, 30, [("M", 10)], {1: 8, 4: 4}, L=5)               # a CIGAR longer than l_seq: 31 C -> T, 34 A -> G
    lit["site"][("h2", 31)] = 8
    lit["site"][("h2", 34)] = 4
    both(1, 0, [("S", 3), ("M", 2)], {0: 8, 1: 8, 2: 8, 3: 8, 4: 8})   # clipped bases are none; 0 A -> T, 1 C -> T
    lit["site"][("h2", 0)] = 8
    lit["site"][("h2", 1)] = 8
    # h3: every op: H S M I D M N M P M = X S H; aligned [100,104) [106,109) [209,213) [213,216) [216,218)
    ops = [("H", 3), ("S", 2), ("M", 4), ("I", 2), ("D", 2), ("M", 3), ("N", 100), ("M", 4), ("P", 1), ("=", 3),
           ("X", 2), ("S", 3), ("H", 2)]
    qidx = {100: 2, 103: 5, 106: 8, 108: 10, 209: 11, 212: 14, 213: 15, 215: 17, 216: 18, 217: 19}   # first / last of each op
    both(2, 100, ops, {x: alts("h3", p)[0] for p, x in qidx.items()}, clip=15)
    for p in qidx:
        lit["site"][("h3", p)] = alts("h3", p)[0]
    lit["none"] += [("h3", p) for p in (98, 99, 104, 105, 109, 150, 208, 218, 219)]
    # even / odd query index on even / odd reference position
    for pos, x in ((300, 0), (300, 1), (311, 0), (311, 1), (320, 2), (331, 3)):
        both(2, pos, [("M", 5)], {x: alts("h3", pos + x)[1]})
        lit["site"][("h3", pos + x)] = alts("h3", pos + x)[1]
    # position 0 (a read placed at -1 as well) and the last position, a CIGAR that runs past it
    both(2, 0, [("M", 4)], {0: alts("h3", 0)[0]})
    both(2, -1, [("M", 3)], {1: alts("h3", 0)[0], 0: 2}, no_index=True)
    lit["site"][("h3", 0)] = alts("h3", 0)[0]
    both(2, 3 * T - 3, [("M", 10)], {3: alts("h3", 3 * T)[2], 4: 2, 9: 4})
    lit["site"][("h3", 3 * T)] = alts("h3", 3 * T)[2]
    # the allele combinations
    a = alts("h3", 400)
    read(0, 2, 398, [("M", 5)], {2: a[0]})                    # tumor-only, two reads
    read(0, 2, 400, [("M", 5)], {0: a[0]})
    read(1, 2, 398, [("M", 5)])
    lit["none"].append(("h3", 400))
    read(1, 2, 408, [("M", 5)], {2: alts("h3", 410)[0]})      # normal-only
    read(0, 2, 408, [("M", 5)])
    lit["none"].append(("h3", 410))
    a = alts("h3", 420)
    read(0, 2, 418, [("M", 5)], {2: a[0]})                    # tumor one allele, normal another
    read(1, 2, 418, [("M", 5)], {2: a[1]})
    lit["none"].append(("h3", 420))
    a = alts("h3", 430)
    read(0, 2, 428, [("M", 5)], {2: a[0]})                    # tumor {a0, a1}, normal {a1, a2}: ALT a1 alone
    read(0, 2, 429, [("M", 5)], {1: a[1]})
    read(1, 2, 430, [("M", 5)], {0: a[1]})
    read(1, 2, 426, [("M", 5)], {4: a[2]})
    lit["site"][("h3", 430)] = a[1]
    a = alts("h3", 440)
    for ds in (0, 1):                                         # two alleles, both shared
        read(ds, 2, 438, [("M", 5)], {2: a[0]})
        read(ds, 2, 440 - ds, [("M", 5)], {ds: a[2]})
    lit["site"][("h3", 440)] = a[0] | a[2]
    # skipped records: their bases would make sites at 500..503 with the tumor's valid read
    a = [alts("h3", p)[0] for p in range(500, 504)]
    bad = {k: a[k] for k in range(4)}
    read(0, 2, 500, [("M", 4)], bad)
    read(1, 2, 500, [("M", 4)], bad, flag=4 | 1)              # unmapped but placed
    read(1, 2, 500, [], bad, L=4)                             # no CIGAR
    read(1, 2, 500, [("M", 4)], L=0)                          # no bases
    lit["none"] += [("h3", p) for p in range(500, 504)]
    # sites at T - 1, T, T + 1 and 2 T
    for p in (T - 1, T, T + 1, 2 * T):
        both(2, p - 2, [("M", 5)], {2: alts("h3", p)[0]})
        lit["site"][("h3", p)] = alts("h3", p)[0]
    # 300 one-base records a dataset: the four bytes of a tally word get their bits from eight records
    for p in range(1000, 1300):
        both(2, p, [("M", 1)], {0: alts("h3", p)[p % 3]})
        lit["site"][("h3", p)] = alts("h3", p)[p % 3]
    # long CIGARs (M 1 alternating with I 1 / D 1: op borders inside a byte), random bases
    for ds, seeds in ((0, (9,)), (1, (9, 11))):
        for seed in seeds:
            for r in K.long_cigar_records(seed=seed):
                recs[ds].append(dict(r, tid=2, pos=r["pos"] + 3000))
    # h4 is not in the FASTA; records past the header and without a sequence
    both(3, 10, [("M", 6)], {k: 2 for k in range(6)})
    for ds in (0, 1):
        recs[ds].sort(key=lambda r: (r["tid"] if r["tid"] >= 0 else 1 << 30, r["pos"]))
    tail = dict(tid=len(HAND_CONTIGS), pos=500, flag=0, cigar=[("M", 4)], nib=[2, 2, 2, 2], qual=[9] * 4, no_index=True)
    recs[1].append(tail)                                      # tid >= n_ref
    recs[1].append(dict(tid=-1, pos=-1, flag=4, cigar=[], nib=[2, 4], qual=[7, 7]))
    recs[0].append(dict(tid=-1, pos=500, flag=0, cigar=[("M", 2)], nib=[2, 4], qual=[7, 7]))    # tid -1
    return recs[0], recs[1], fa, lit


def expected_hand() -> dict:
    """The hand-built set's sites by the restatement, checked against the literal expectations."""
    t, n, fa, lit = hand_built()
    ev: dict = {}
    tally_records(ev, t, HAND_CONTIGS, fa, 0)
    tally_records(ev, n, HAND_CONTIGS, fa, 1)
    sites = sites_of(ev, fa)
    for (c, p), alt in lit["site"].items():
        assert sites.get(c, {}).get(p) == (CODE[fa[c][p].upper()], alt), (c, p, sites.get(c, {}).get(p))
    for c, p in lit["none"]:
        assert p not in sites.get(c, {}), (c, p)
    assert "h1" not in sites and "h4" not in sites and max(sites["h3"]) == 3 * TILE
    return sites


def write_hand_files(d: str, indexed: bool = True) -> dict:
    """The hand-built set as files: a FASTA and the tumor and normal BAMs, through the generator's writer
    (coordinate order, with an index; the records no index can list left out) or as plain BGZF streams
    of every record."""
    from genomeanonymizer_amd.synth import bamwriter as W
    os.makedirs(d, exist_ok=True)
    t, n, fa, _ = hand_built()
    ref = os.path.join(d, "hand.fa")
    W.write_fasta(ref, [(c, fa[c]) for c, _ in HAND_CONTIGS if c in fa])
    out = {"ref": ref, "fa": fa}
    for tag, recs in (("T", t), ("N", n)):
        path = os.path.join(d, f"hand_{tag}{'_idx' if indexed else ''}.bam")
        if indexed:
            brs = [W.BamRecord(f"r{k}", r["flag"], r["tid"], r["pos"], 30, r["cigar"], -1, -1, 0,
                               "".join(NT16[b] for b in r["nib"]), r["qual"])
                   for k, r in enumerate(recs) if not r.get("no_index")]
            W.write_bam(path, HAND_CONTIGS, brs, index=True)
        else:
            stream, _ = stream_of(recs)
            W.write_bgzf(path, stream.tobytes())
        out[tag] = path
    return out


def stream_of(recs):
    """(inflated BAM stream, offset of its first record) of hand-built records."""
    return K.stream_of([{k: v for k, v in r.items() if k != "no_index"} for r in recs], contigs=HAND_CONTIGS)
