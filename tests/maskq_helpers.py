"""Helpers of the --masked_base_quality tests: pipeline runs against the fixtures the hooked reference
wrote (tests/golden/maskq2, tools/make_maskq_golden.py), the invariants for the scenarios the hooked
reference cannot finish, and the crafted record set of the formatter tests with its numpy
restatement."""
from __future__ import annotations

import gzip
import json
import os
import shutil

import numpy as np

import helpers

MASKQ_Q = 2
MASKQ_GOLDEN = os.path.join(helpers.GOLDEN, "maskq%d" % MASKQ_Q)
FILES = [f"{tag}{suf}" for tag in ("tumor", "normal") for suf in (".1.fastq", ".2.fastq", ".single_end.fastq")]
MODES = ("streamed", "whole", "jobs")


def set_mode(monkeypatch, mode: str, quality=MASKQ_Q) -> bool:
    """Environment of one pipeline mode with the option on (``quality`` None: off). Returns whether
    the inputs need BAM indexes."""
    monkeypatch.setenv("GANON_WHOLE_SAMPLE", "1" if mode == "whole" else "0")
    if mode == "jobs":
        monkeypatch.setenv("GANON_JOB_BP", "2500")
    else:
        monkeypatch.delenv("GANON_JOB_BP", raising=False)
    if quality is None:
        monkeypatch.delenv("GANON_MASKED_BASE_QUALITY", raising=False)
    else:
        monkeypatch.setenv("GANON_MASKED_BASE_QUALITY", str(quality))
    return mode == "jobs"


def run_vs_maskq_golden(name: str, workdir: str, anonymizer, bam_index: bool = False) -> dict:
    """helpers.run_pipeline_vs_golden with the golden root swapped for the hooked reference's."""
    root = helpers.GOLDEN
    helpers.GOLDEN = MASKQ_GOLDEN
    try:
        return helpers.run_pipeline_vs_golden(name, workdir, anonymizer, bam_index=bam_index)
    finally:
        helpers.GOLDEN = root


def golden_files(name: str, root: str = helpers.GOLDEN) -> dict:
    """file tag -> plain bytes of a scenario's golden FASTQ files (absent files left out)."""
    out = {}
    for f in FILES:
        p = os.path.join(root, name, f + ".gz")
        if os.path.exists(p):
            out[f] = gzip.open(p).read()
    out["statistics"] = open(os.path.join(root, name, "normal.statistics.txt"), "rb").read()
    return out


def run_pipeline_files(name: str, workdir: str, anonymizer, bam_index: bool = False, block_size: int = 4096) -> dict:
    """Run the product pipeline on a scenario; file tag -> bytes written (as golden_files)."""
    from genomeanonymizer_amd.synth.generate import make_inputs
    from genomeanonymizer_amd import short_read_tumor_normal_anonymizer as sr
    from genomeanonymizer_amd import writer
    meta = json.load(open(os.path.join(helpers.GOLDEN, name, "meta.json")))
    shutil.rmtree(workdir, ignore_errors=True)
    paths = make_inputs(name, os.path.join(workdir, "in"), bam_index)
    assert helpers.input_digests(paths) == meta["inputs_sha256"], "synthetic generator drifted from the fixtures"
    t_out, n_out = sr.name_output(paths["T"]), sr.name_output(paths["N"])
    orig = writer.io_block_size
    writer.io_block_size = lambda d: block_size
    try:
        sr.run_short_read_tumor_normal_anonymizer([paths["vcf"]], [(paths["T"], paths["N"])], paths["ref"],
                                                  anonymizer, [(t_out, n_out)], True, 4)
    finally:
        writer.io_block_size = orig
    out = {}
    for tag, pre in (("tumor", t_out), ("normal", n_out)):
        for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
            if os.path.exists(pre + suf):
                out[tag + suf] = open(pre + suf, "rb").read()
    out["statistics"] = open(paths["N"] + ".statistics.txt", "rb").read()
    return out


def quality_diff(plain: dict, got: dict, qc: bytes = b"#") -> int:
    """Asserts that ``got`` equals ``plain`` outside the quality lines (same files, same lines, same
    line lengths, same statistics) and, with ``qc``, that every changed quality character is ``qc``
    (None: any — a deletion's inserted bases take int(mean) of the patched qualities); returns how
    many characters changed."""
    assert sorted(plain) == sorted(got)
    assert plain["statistics"] == got["statistics"]
    changed = 0
    for f in plain:
        if f == "statistics":
            continue
        a, b = plain[f].split(b"\n"), got[f].split(b"\n")
        assert len(a) == len(b), f
        for i, (x, y) in enumerate(zip(a, b)):
            if x == y:
                continue
            assert i % 4 == 3, (f, i)
            assert len(x) == len(y), (f, i)
            xa, ya = np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)
            d = xa != ya
            if qc is not None:
                other = np.nonzero(d & (ya != qc[0]))[0]
                if len(other):
                    # the one exception the definition itself makes: the bases a deletion left-over
                    # inserted take int(mean) of the record's patched qualities (one run of one value,
                    # the mean of the line without it), so a patched read's run can move with its mean
                    assert other[-1] - other[0] + 1 == len(other) and len(set(ya[other].tolist())) == 1, (f, i)
                    run = np.zeros(len(ya), bool)
                    run[other[0]:other[-1] + 1] = True
                    rest = ya[~run].astype(np.int64) - 33
                    assert int(ya[other[0]]) - 33 == int(np.mean(rest)), (f, i)
            changed += int(d.sum())
    return changed


# ---- crafted records ---------------------------------------------------------------------------

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 4097, 70001)


def crafted_records(quality: int, seed: int = 7) -> dict:
    """A ``fastq_records`` dict with masked copies in buffer 0 and originals in buffers 1 and 2 (at
    other offsets than the copies, reads starting on odd bytes too): every length of LENGTHS forward
    and reverse with masks at the first base, the last base, both nibbles of a byte, every base and
    nowhere; a record without an original; two records sharing one quality range with different
    masks; names of 1 and 255 characters."""
    from genomeanonymizer_amd.synth.batch import pack_nibbles
    rng = np.random.default_rng(seed)
    acgt = np.array([1, 2, 4, 8], np.uint8)
    cases = []   # (length, reverse, mask kind, has original, name length, shared quality slot)
    for L in LENGTHS:
        for rev in (0, 1):
            for kind in ("first", "last", "byte", "all", "none"):
                cases.append([L, rev, kind, True, 1 + (len(cases) * 37) % 40, -1])
    cases.append([150, 0, "all", False, 9, -1])
    cases.append([150, 1, "first", True, 1, -1])
    cases.append([151, 0, "last", True, 255, -1])
    cases.append([70001, 1, "byte", True, 255, -1])
    cases.append([150, 0, "first", True, 12, 0])     # one quality range, two records, two masks
    cases.append([150, 1, "last", True, 12, 0])
    n = len(cases)
    masked, orig = [bytearray(3)], [bytearray(5), bytearray(2)]    # buffers 0 | 1, 2 (uneven starts)
    quals, names = bytearray(1), bytearray()
    shared = {}
    rec = {k: [] for k in ("seq_nib_off", "seq_len", "reverse", "qual_off", "name_off", "name_len", "mate",
                           "orig_sel", "orig_nib_off", "qual_sel")}
    truth = []      # per record: masked query positions
    for i, (L, rev, kind, has, nl, slot) in enumerate(cases):
        o = acgt[rng.integers(0, 4, L)]
        pos = {"first": [0], "last": [L - 1], "byte": [2 * ((L - 1) // 4), 2 * ((L - 1) // 4) + 1],
               "all": list(range(L)), "none": []}[kind]
        pos = sorted({p for p in pos if 0 <= p < L})
        m = o.copy()
        for p in pos:
            m[p] = acgt[(int(np.nonzero(acgt == o[p])[0][0]) + 1 + p % 3) % 4]
        pack = lambda a: pack_nibbles(a).tobytes()
        ob = orig[i % 2]
        rec["seq_nib_off"].append(2 * len(masked[0]))
        masked[0] += pack(m) + bytes(i % 3)               # copies start on any byte
        rec["orig_sel"].append(1 + i % 2 if has else 255)
        rec["orig_nib_off"].append(2 * len(ob) if has else 0)
        if has:
            ob += pack(o) + bytes((i + 1) % 4)
        rec["seq_len"].append(L)
        rec["reverse"].append(rev)
        if slot >= 0 and slot in shared:
            rec["qual_off"].append(shared[slot])
        else:
            rec["qual_off"].append(len(quals))
            if slot >= 0:
                shared[slot] = len(quals)
            quals += bytes(rng.integers(3, 42, L, dtype=np.uint8).tobytes())
        rec["qual_sel"].append(0)
        rec["name_off"].append(len(names))
        rec["name_len"].append(nl)
        names += bytes(rng.integers(65, 91, nl, dtype=np.uint8).tobytes())
        rec["mate"].append(1 + i % 2)
        truth.append(pos if has else [])
    dt = {"seq_nib_off": np.int64, "seq_len": np.int32, "reverse": np.uint8, "qual_off": np.int64,
          "name_off": np.int64, "name_len": np.int32, "mate": np.uint8, "orig_sel": np.uint8,
          "orig_nib_off": np.int64, "qual_sel": np.uint8}
    out = {k: np.array(v, dt[k]) for k, v in rec.items()}
    out["seq_sel"] = np.zeros(n, np.uint8)
    out["qual_len"] = out["seq_len"].copy()
    out["qual_rev"] = np.zeros(n, np.uint8)
    pad = lambda b: np.frombuffer(bytes(b) + bytes(8), np.uint8).copy()
    out["seq_bufs"] = [pad(masked[0]), pad(orig[0]), pad(orig[1])]
    out["qual_bufs"] = [pad(quals)]
    out["names"] = bytes(names)
    out["maskq"] = quality
    out["_truth"] = truth
    return out


def plain_of(recs: dict) -> dict:
    """The same records with the option off."""
    return {k: v for k, v in recs.items() if k not in ("maskq", "orig_sel", "orig_nib_off", "_truth")}


def restate(recs: dict, plain: bytes) -> bytes:
    """The definition, independently: the plain formatter's output with the quality character at the
    text index of every base whose nibble differs between the record's copy and its original set to
    chr(33 + Q). Nibbles are compared through numpy, not through the masks the records were built with."""
    out = bytearray(plain)
    nib = [np.stack([b >> 4, b & 15], axis=1).reshape(-1) for b in recs["seq_bufs"]]
    o = 0
    for i in range(len(recs["seq_len"])):
        L, Q, nl = int(recs["seq_len"][i]), int(recs["qual_len"][i]), int(recs["name_len"][i])
        if recs["orig_sel"][i] != 255 and L == Q:
            a = nib[int(recs["seq_sel"][i])][int(recs["seq_nib_off"][i]):][:L]
            b = nib[int(recs["orig_sel"][i])][int(recs["orig_nib_off"][i]):][:L]
            p = np.nonzero(a != b)[0]
            assert p.tolist() == recs["_truth"][i]
            k = L - 1 - p if recs["reverse"][i] else p
            q0 = o + nl + L + 7
            for x in k.tolist():
                out[q0 + x] = 33 + recs["maskq"]
        o += 8 + nl + L + Q
    assert o == len(plain)
    return bytes(out)
