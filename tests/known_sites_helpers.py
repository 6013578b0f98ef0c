"""Helpers of the --known_sites tests. The rule is restated here in plain Python — on the synthetic
generator's ``BamRecord`` objects, on decoded tables and on a hand-built stream — and no expectation
ever comes from the code under test. ``scenario_panel`` builds a panel for a golden scenario from what
its reads show, ``make_inputs`` with a panel writes X' (the scenario's inputs with the rule applied to
every record, through the generator's own BAM writer, so that the .bai of job mode is valid too),
``run_files`` runs the product pipeline on either."""
from __future__ import annotations

import bisect
import copy
import gzip
import os
import shutil
import struct
import tempfile

import numpy as np

NT16 = "=ACMGRSVTWYHKDBN"
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}
OPS = "MIDNSHP=X"
I32 = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len", "aux_len")
I64 = ("name_off", "cig_off", "seq_off", "qual_off", "aux_off")
BLOBS = ("names_blob", "cigar", "aux")


class Sites:
    """contig name -> sorted positions with (ref_nt16, alt_mask): the panel as the tests understand it."""

    def __init__(self, by_contig: dict):
        self.pos = {c: sorted(d) for c, d in by_contig.items()}
        self.val = {c: [d[p] for p in self.pos[c]] for c, d in by_contig.items()}

    def n(self) -> int:
        return sum(len(v) for v in self.pos.values())


def apply_rule(sites: Sites, contig, flag: int, pos: int, cigar, nib: list, qual, quality=None) -> int:
    """The rule on one record: ``cigar`` a list of (op letter, length), ``nib`` its l_seq base codes and
    ``qual`` its quality bytes (both changed in place). Returns the bases rewritten."""
    if (flag & 4) or contig is None or not cigar or not nib:
        return 0
    sp, sv = sites.pos.get(contig, []), sites.val.get(contig, [])
    q_on = quality is not None and len(qual) and qual[0] != 0xFF
    r, q, cnt = pos, 0, 0
    for op, n in cigar:
        if op in "M=X":
            i = bisect.bisect_left(sp, r)
            while i < len(sp) and sp[i] < r + n:
                x = q + sp[i] - r
                ref, alt = sv[i]
                if x < len(nib) and nib[x] in (1, 2, 4, 8) and (nib[x] & alt):
                    nib[x] = ref
                    if q_on:
                        qual[x] = quality
                    cnt += 1
                i += 1
            r += n
            q += n
        elif op in "IS":
            q += n
        elif op in "DN":
            r += n
    return cnt


def rule_on_record(sites: Sites, contigs, rec, quality=None):
    """A copy of a generator BamRecord with the rule applied (and how many bases it rewrote)."""
    r2 = copy.copy(rec)
    nib = [NT16.index(c) for c in rec.seq]
    qual = list(rec.qual)
    contig = contigs[rec.tid][0] if 0 <= rec.tid < len(contigs) else None
    cnt = apply_rule(sites, contig, rec.flag, rec.pos, rec.cigar, nib, qual, quality)
    r2.seq = "".join(NT16[b] for b in nib)
    r2.qual = type(rec.qual)(qual) if not isinstance(rec.qual, np.ndarray) else np.array(qual, rec.qual.dtype)
    return r2, cnt


def table_nibbles(t, i: int) -> list:
    o, L = int(t.seq_off[i]), int(t.l_seq[i])
    b = np.asarray(t.seq[o:o + (L + 1) // 2])
    return np.stack([b >> 4, b & 15], axis=1).reshape(-1)[:L].tolist()


def rule_on_table(sites: Sites, t, quality=None):
    """(expected seq blob, expected qual blob, bases rewritten) of a table decoded without the option."""
    seq, qual = np.array(t.seq, np.uint8), np.array(t.qual, np.uint8)
    total = 0
    for i in range(t.n):
        tid, L = int(t.tid[i]), int(t.l_seq[i])
        nib = table_nibbles(t, i)
        qo = int(t.qual_off[i])
        q = qual[qo:qo + L].tolist()
        cig = [(OPS[w & 15] if (w & 15) < 9 else "?", int(w >> 4)) for w in t.cigar_of(i).tolist()]
        contig = t.ref_names[tid] if 0 <= tid < len(t.ref_names) else None
        cnt = apply_rule(sites, contig, int(t.flag[i]), int(t.pos[i]), cig, nib, q, quality)
        if cnt:
            total += cnt
            so = int(t.seq_off[i])
            pad = int(seq[so + L // 2]) & 15 if L & 1 else 0     # (an odd read's pad nibble stays)
            full = nib + ([pad] if L & 1 else [])
            seq[so:so + (L + 1) // 2] = [(full[k] << 4) | full[k + 1] for k in range(0, len(full), 2)]
            qual[qo:qo + L] = q
    return seq, qual, total


def assert_masked_table(got, plain, sites: Sites, quality=None, what="") -> int:
    """``got`` is ``plain`` with the rule applied to seq (and qual), everything else equal, and its
    count is the rule's. Returns the count."""
    assert got.n == plain.n, what
    seq, qual, total = rule_on_table(sites, plain, quality)
    assert np.array_equal(np.asarray(got.seq), seq), (what, "seq")
    assert np.array_equal(np.asarray(got.qual), qual), (what, "qual")
    for f in I32 + I64 + BLOBS:
        assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(plain, f))), (what, f)
    return total


def table_of(sites: Sites, ref_names, quality=None):
    """The decoders' table (known_sites.SitesTable) built from the tests' own panel by sequence id."""
    from genomeanonymizer_amd.known_sites import SitesTable
    off, pos, code = [0], [], []
    for name in ref_names:
        for p, (ref, alt) in zip(sites.pos.get(name, []), sites.val.get(name, [])):
            pos.append(p)
            code.append((ref << 4) | alt)
        off.append(len(pos))
    return SitesTable(np.array(off, np.int64), np.array(pos, np.int32), np.array(code, np.uint8),
                      -1 if quality is None else quality)


# ---- a panel for a golden scenario -------------------------------------------------------------------

_PANELS: dict = {}
_TMP = []


def _tmpdir() -> str:
    if not _TMP:
        import atexit
        _TMP.append(tempfile.mkdtemp(prefix="known_sites_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    return _TMP[0]


def _fasta(path: str) -> dict:
    out, name = {}, None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            out[name] = []
        elif line:
            out[name].append(line)
    return {k: "".join(v) for k, v in out.items()}


def own_vcf_snv_positions(vcf: str) -> dict:
    """contig -> the 0-based positions of the scenario's own VCF lines with equal-length REF and ALT."""
    out: dict = {}
    for line in open(vcf):
        if line.startswith("#") or not line.strip():
            continue
        f = line.rstrip("\n").split("\t")
        for a in f[4].split(","):
            if len(a) == len(f[3]) and not a.startswith(("<", ".", "*")) and "[" not in a and "]" not in a:
                out.setdefault(f[0], set()).update(range(int(f[1]) - 1, int(f[1]) - 1 + len(f[3])))
    return out


def scenario_panel(name: str) -> dict:
    """{"vcf": panel path (.vcf.gz for every second scenario name length, else plain), "sites": Sites — the
    panel the product must end up using, own SNV positions already left out —, "own": the position left
    out} for golden scenario ``name``, built once per session from the aligned bases of X that differ
    from the FASTA: (a) about half of them with the ALT seen, (b) some with another ALT only, (c) a
    multi-allelic line (and a second line at one position), (d) positions no read differs at, (e) an
    indel, an MNV, a symbolic ALT and a contig the BAMs do not have, (f) one of the scenario's own SNVs."""
    if name in _PANELS:
        return _PANELS[name]
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth import generate as G
    d = os.path.join(_tmpdir(), name)
    paths = G.make_inputs(name, os.path.join(d, "x"), False)
    fa = _fasta(paths["ref"])
    seen: dict = {}        # (contig, pos) -> set of ALT letters seen in aligned bases
    for s in ("T", "N"):
        t = ReadTable(paths[s], threads=2)
        for i in range(t.n):
            if (int(t.flag[i]) & 4) or int(t.tid[i]) < 0 or not int(t.n_cigar[i]):
                continue
            contig = t.ref_names[int(t.tid[i])]
            ref = fa[contig]
            nib = np.array(table_nibbles(t, i), np.int64)
            r, q = int(t.pos[i]), 0
            for w in t.cigar_of(i).tolist():
                op, n = OPS[w & 15], int(w >> 4)
                if op in "M=X":
                    m = min(n, len(nib) - q, len(ref) - r)
                    if m > 0:
                        rb = np.array([CODE.get(c, 0) for c in ref[r:r + m].upper()], np.int64)
                        qb = nib[q:q + m]
                        for k in np.nonzero((qb != rb) & (rb != 0) & np.isin(qb, (1, 2, 4, 8)))[0].tolist():
                            seen.setdefault((contig, r + k), set()).add(NT16[int(qb[k])])
                    r += n
                    q += n
                elif op in "IS":
                    q += n
                elif op in "DN":
                    r += n
    own = own_vcf_snv_positions(paths["vcf"])
    rng = np.random.default_rng(len(name) * 7919 + sum(map(ord, name)))
    keys = sorted(seen)
    lines, by_contig = [], {}

    def add(contig, pos, ref, alts, used=True):
        lines.append((contig, pos, ref, ",".join(alts)))
        ref = ref.upper()
        if used and pos not in own.get(contig, ()):
            d_ = by_contig.setdefault(contig, {})
            m = 0
            for a in alts:
                if a in CODE and a != ref:
                    m |= CODE[a]
            if m:
                d_[pos] = (CODE[ref], m | d_.get(pos, (0, 0))[1])
    for k, (contig, pos) in enumerate(keys):
        ref = fa[contig][pos].upper()
        alts = sorted(seen[(contig, pos)])
        other = [b for b in "ACGT" if b != ref and b not in alts]
        if k % 2 == 0:
            add(contig, pos, ref if k % 4 else ref.lower(), alts[:1])                  # (a), lower case folded
        elif k % 8 == 1 and other:
            add(contig, pos, ref, other[:1])                                            # (b)
        elif k % 8 == 3:
            add(contig, pos, ref, [other[0] if other else alts[0], "<DEL>", alts[0] + "A", alts[0], "*"])   # (c)
            add(contig, pos, ref, alts[-1:])                                            # a second line, OR-ed
    # (f) one of the pair's own SNV positions that a read shows an ALT at, if any, else any of them
    own_pick = None
    for contig, pos in keys:
        if pos in own.get(contig, ()):
            own_pick = (contig, pos)
            break
    if own_pick is None:
        for contig, ps in sorted(own.items()):
            for pos in sorted(ps):
                if contig in fa and fa[contig][pos].upper() in CODE:
                    own_pick = (contig, pos)
                    break
            if own_pick:
                break
    if own_pick is not None:
        contig, pos = own_pick
        ref = fa[contig][pos].upper()
        add(contig, pos, ref, [b for b in "ACGT" if b != ref])
    names = sorted(fa)
    for _ in range(40):                                                                 # (d)
        contig = names[int(rng.integers(0, len(names)))]
        pos = int(rng.integers(0, len(fa[contig])))
        ref = fa[contig][pos].upper()
        if ref in CODE and (contig, pos) not in seen:
            add(contig, pos, ref, [b for b in "ACGT" if b != ref][:1 + int(rng.integers(0, 3))])
    c0 = names[0]
    p0 = next(p for p in range(50, len(fa[c0])) if all(c in "ACGT" for c in fa[c0][p:p + 3].upper()))
    r3 = fa[c0][p0:p0 + 3].upper()
    add(c0, p0, r3[:2], [r3[0]], used=False)                                            # (e) a deletion
    add(c0, p0, r3, ["TTT" if r3 != "TTT" else "AAA"], used=False)                      # an MNV
    add(c0, p0 + 1, r3[1], [r3[1] + "GG", "<INS>", "."], used=False)                    # no one-base ALT
    add("chrNotInTheBam", 12, "A", ["C"], used=False)                                   # another contig
    lines.sort(key=lambda x: (names.index(x[0]) if x[0] in names else len(names), x[1]))
    text = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join(
        f"{c}\t{p + 1}\t.\t{r}\t{a}\t.\tPASS\t.\n" for c, p, r, a in lines)
    gz = len(name) % 2 == 0
    vcf = os.path.join(d, "panel.vcf" + (".gz" if gz else ""))
    with (gzip.open(vcf, "wt") if gz else open(vcf, "w")) as fh:
        fh.write(text)
    out = _PANELS[name] = {"vcf": vcf, "sites": Sites(by_contig), "own": own_pick, "plain_inputs": paths}
    return out


def set_option(monkeypatch, panel) -> None:
    """The option on with panel file ``panel``, or off (None)."""
    if panel is None:
        monkeypatch.delenv("GANON_KNOWN_SITES", raising=False)
    else:
        monkeypatch.setenv("GANON_KNOWN_SITES", panel)


MIN_CHANGED = 20


def make_inputs(name: str, outdir: str, bam_index: bool, sites: Sites = None, monkeypatch=None, quality=None) -> dict:
    """A golden scenario's inputs X, or with ``sites`` X': the generator's write_bam wrapped so that
    each record is written with the rule applied; X' must differ from X in at least MIN_CHANGED bases."""
    from genomeanonymizer_amd.synth import generate as G
    if sites is None:
        return G.make_inputs(name, outdir, bam_index)
    real = G.write_bam
    changed = [0]

    def masked(path, contigs, records, **kw):
        out = []
        for r in records:
            r2, cnt = rule_on_record(sites, contigs, r, quality)
            changed[0] += cnt
            out.append(r2)
        return real(path, contigs, out, **kw)
    monkeypatch.setattr(G, "write_bam", masked)
    try:
        paths = G.make_inputs(name, outdir, bam_index)
    finally:
        monkeypatch.setattr(G, "write_bam", real)
    assert changed[0] >= MIN_CHANGED, (name, changed[0])
    paths["_changed"] = changed[0]
    return paths


def run_files(name: str, workdir: str, anonymizer, bam_index: bool = False, sites: Sites = None, monkeypatch=None,
              gz: bool = False, quality=None) -> dict:
    """The product pipeline on scenario ``name`` (X, or X' with ``sites``) under the environment the
    caller set; file tag -> bytes."""
    import namehash_helpers as H
    from genomeanonymizer_amd import short_read_tumor_normal_anonymizer as sr
    from genomeanonymizer_amd import writer
    shutil.rmtree(workdir, ignore_errors=True)
    paths = make_inputs(name, os.path.join(workdir, "in"), bam_index, sites, monkeypatch, quality)
    t_out, n_out = sr.name_output(paths["T"]), sr.name_output(paths["N"])
    orig = writer.io_block_size
    writer.io_block_size = lambda d: 4096
    try:
        sr.run_short_read_tumor_normal_anonymizer([paths["vcf"]], [(paths["T"], paths["N"])], paths["ref"],
                                                  anonymizer, [(t_out, n_out)], True, 4)
    finally:
        writer.io_block_size = orig
    return H.collect(paths, gz)


def assert_option_equals_plain_on_rewritten(name, tmp_path, monkeypatch, anonymizer_of, index=False, quality=None,
                                            gz=False, plain_anonymizer_of=None, base=None) -> dict:
    """The defining property on scenario ``name`` under the mode the caller set: the option on X writes
    the files the plain run writes on X', byte for byte, and not the files the plain run writes on X
    (``base``: those files where the caller has them, the scenario's goldens; else X is run too)."""
    sp = scenario_panel(name)
    set_option(monkeypatch, sp["vcf"])
    got = run_files(name, str(tmp_path / "x"), anonymizer_of(), index, gz=gz)
    set_option(monkeypatch, None)
    plain_of = plain_anonymizer_of or anonymizer_of
    exp = run_files(name, str(tmp_path / "xp"), plain_of(), index, sp["sites"], monkeypatch, gz=gz, quality=quality)
    if base is None:
        base = run_files(name, str(tmp_path / "x0"), plain_of(), index, gz=gz)
    assert sorted(got) == sorted(exp)
    for f in exp:
        assert got[f] == exp[f], f
    assert any(base.get(f) != exp[f] for f in exp), "the plain runs on X and X' wrote the same files"
    return got


# ---- a hand-built stream -------------------------------------------------------------------------------

def bam_record(tid, pos, flag, cigar, nib, qual, name=b"r\x00", mate=(-1, -1), aux=b"") -> bytes:
    """One BAM record from (op letter, length) pairs and base codes; ``qual`` a list of l_seq bytes."""
    L = len(nib)
    full = list(nib) + ([0] if L & 1 else [])
    packed = bytes((full[k] << 4) | full[k + 1] for k in range(0, len(full), 2))
    cig = b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for op, n in cigar)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), 30, 4680, len(cigar), flag, L, mate[0], mate[1], 0)
    body += name + cig + packed + bytes(qual) + aux
    return struct.pack("<i", len(body)) + body


HAND_CONTIGS = [("c1", 5000), ("c2", 3000), ("c3", 1000)]


def hand_built(seed: int = 5):
    """(records as dicts, Sites) covering the rule's corners on HAND_CONTIGS (c3 has no sites): every CIGAR op
    with leading H + S, I next to D, N, P, = and X; sites on the first and last aligned base, inside a D
    and an N, under a soft clip, on both nibbles, on the last base of odd reads and next to each other;
    l_seq 0, no CIGAR, a placed unmapped record, tid -1; a CIGAR longer than the read; ambiguity codes
    and N at sites; qualities 0xFF. Every base at a site is an ALT of it unless a case says otherwise."""
    rng = np.random.default_rng(seed)
    recs, by = [], {"c1": {}, "c2": {}}

    def site(c, p, ref=1, alt=2 | 4 | 8):
        by[c][p] = (ref, alt)

    def rec(tid, pos, cigar, flag=0, qual=None, nib=None, L=None):
        L = sum(n for op, n in cigar if op in "MIS=X") if L is None else L
        nib = [int(x) for x in rng.choice([2, 4, 8], L)] if nib is None else nib    # (never the REF A)
        qual = [int(x) for x in rng.integers(5, 40, L)] if qual is None else qual
        recs.append(dict(tid=tid, pos=pos, flag=flag, cigar=cigar, nib=nib, qual=qual))
    # every op: H S M I D M N M P M = X S H; aligned: [100,104) [106,109) [209,213) [213,216) [216,218)
    rec(0, 100, [("H", 3), ("S", 2), ("M", 4), ("I", 2), ("D", 2), ("M", 3), ("N", 100), ("M", 4), ("P", 1),
                 ("=", 3), ("X", 2), ("S", 3), ("H", 2)])
    for p in (98, 99, 100, 103, 104, 105, 106, 108, 109, 150, 208, 209, 212, 213, 215, 216, 217, 218, 219):
        site("c1", p)    # 98, 99: under the soft clip; 104, 105: in the D; 109..208: in the N; 218, 219: past the end
    # even and odd reads, a site on the high nibble, the low nibble and the last base of an odd read
    rec(0, 300, [("M", 7)])
    for p in (300, 301, 306):
        site("c1", p)
    rec(0, 320, [("M", 8)])
    for p in (320, 323, 327):
        site("c1", p)
    rec(0, 340, [("M", 1)])
    site("c1", 340)
    # adjacent sites, one with an ALT mask the base is not in, one where the base is the REF
    rec(0, 400, [("M", 6)], nib=[2, 2, 4, 1, 8, 2])
    site("c1", 400)
    site("c1", 401, 1, 4 | 8)      # base C is no ALT here
    site("c1", 402)
    site("c1", 403)                # base A = REF
    site("c1", 404, 2, 8)          # T -> C
    # ambiguity codes, N and '=' at sites
    rec(0, 420, [("M", 6)], nib=[15, 3, 5, 0, 12, 8])
    for p in range(420, 426):
        site("c1", p)
    # skipped records: l_seq 0, no CIGAR, unmapped but placed, tid -1 (their positions hold sites)
    rec(0, 500, [("M", 4)], L=0, nib=[], qual=[])
    rec(0, 500, [], nib=[2, 4, 8, 2], qual=[9, 9, 9, 9])
    rec(0, 500, [("M", 4)], flag=4 | 1)
    rec(-1, 500, [("M", 4)])
    rec(-1, -1, [], flag=4, nib=[2, 4], qual=[7, 7])
    for p in range(498, 506):
        site("c1", p)
    # a CIGAR longer than the read: sites past l_seq are not bases of it
    rec(0, 600, [("M", 10)], L=5)
    for p in (600, 604, 605, 609):
        site("c1", p)
    # qualities 0xFF (none stored), and a read whose first quality alone is 0xFF
    rec(0, 700, [("M", 5)], qual=[0xFF] * 5)
    rec(0, 710, [("M", 5)], qual=[0xFF, 20, 20, 20, 20])
    rec(0, 720, [("M", 5)], qual=[20, 0xFF, 20, 20, 20])
    for p in list(range(700, 705)) + list(range(710, 715)) + list(range(720, 725)):
        site("c1", p)
    # I next to D at a site, lower and upper case do not matter here; a second sequence; one without sites
    rec(1, 50, [("M", 3), ("D", 1), ("I", 2), ("M", 3)])
    for p in (49, 50, 52, 53, 54, 56, 57):
        site("c2", p, 8, 1 | 2 | 4)
    rec(1, 50, [("S", 4), ("M", 2)], nib=[1, 1, 1, 1, 1, 2])
    rec(2, 10, [("M", 20)])
    # pos -1 with a tid (no site can be at -1; the walk starts there)
    rec(0, -1, [("M", 3)], nib=[2, 2, 2], qual=[1, 2, 3])
    site("c1", 0)
    site("c1", 1)
    return recs, Sites(by)


def stream_of(recs, contigs=HAND_CONTIGS) -> tuple:
    """(inflated BAM stream, offset of its first record) of hand-built records, in the order given."""
    from test_bam_device import _header
    head = _header(contigs)
    body = b"".join(bam_record(r["tid"], r["pos"], r["flag"], r["cigar"], r["nib"], r["qual"],
                               name=f"r{k}".encode() + b"\x00", aux=b"XAZq\x00" if k % 3 == 0 else b"")
                    for k, r in enumerate(recs))
    return np.frombuffer(head + body, np.uint8), len(head)


def expected_of(recs, sites: Sites, contigs=HAND_CONTIGS, quality=None):
    """Per record (nib, qual) after the rule, and the total count."""
    out, total = [], 0
    for r in recs:
        nib, qual = list(r["nib"]), list(r["qual"])
        contig = contigs[r["tid"]][0] if 0 <= r["tid"] < len(contigs) else None
        total += apply_rule(sites, contig, r["flag"], r["pos"], r["cigar"], nib, qual, quality)
        out.append((nib, qual))
    return out, total


def long_cigar_records(n_ops_list=(48, 49, 63, 64, 65, 128, 129), seed: int = 9):
    """Records whose CIGARs have exactly these many ops, M of length 1 alternating with I 1 / D 1 (so that
    op boundaries fall inside a byte), on c2 from position 100 on; and the sites: every position of c2."""
    rng = np.random.default_rng(seed)
    recs = []
    for k, n_ops in enumerate(n_ops_list):
        cigar = [("M", 1) if j % 2 == 0 else (("I", 1) if (j // 2) % 2 == 0 else ("D", 1)) for j in range(n_ops)]
        L = sum(n for op, n in cigar if op in "MI")
        recs.append(dict(tid=1, pos=100 + 7 * k, flag=0, cigar=cigar, nib=[int(x) for x in rng.choice([1, 2, 4, 8], L)],
                         qual=[int(x) for x in rng.integers(3, 40, L)]))
    return recs
