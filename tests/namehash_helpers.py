"""Helpers of the --hash_read_names tests. Expected names always come from ``hashlib.blake2s``, never
from the code under test: ``hashed`` is the definition, ``make_inputs`` with a key writes X' (a scenario's
inputs with every QNAME replaced by its hash, through the synthetic generator's own BAM writer, so
that the .bai of job mode is valid too), ``run_files`` runs the product pipeline on either."""
from __future__ import annotations

import collections
import copy
import hashlib
import os
import shutil

import numpy as np

KEY = bytes(range(7, 39))            # 32 bytes
KEY16 = bytes(range(200, 216))
KEYS = (b"\x5a", KEY16, KEY)         # 1, 16 and 32 bytes
I32 = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "aux_len")
I64 = ("cig_off", "seq_off", "qual_off", "aux_off")
BLOBS = ("cigar", "seq", "qual", "aux")


def hashed(name: bytes, key: bytes = KEY) -> bytes:
    return hashlib.blake2s(name, key=key, digest_size=16).hexdigest().encode()


def set_option(monkeypatch, key=KEY) -> None:
    """The option on with ``key`` (bytes; None: on without a key), or off (``key`` False)."""
    if key is False:
        monkeypatch.delenv("GANON_HASH_READ_NAMES", raising=False)
        monkeypatch.delenv("GANON_READ_NAME_KEY", raising=False)
        return
    monkeypatch.setenv("GANON_HASH_READ_NAMES", "1")
    if key is None:
        monkeypatch.delenv("GANON_READ_NAME_KEY", raising=False)
    else:
        monkeypatch.setenv("GANON_READ_NAME_KEY", key.hex())


def table_names(t) -> list:
    """The names a table reports: names_blob[name_off : name_off + name_len] per record."""
    nb = np.asarray(t.names_blob).tobytes()
    return [nb[o:o + l] for o, l in zip(np.asarray(t.name_off).tolist(), np.asarray(t.name_len).tolist())]


def assert_keyed_table(keyed, plain, key: bytes, what="") -> None:
    """``keyed`` is ``plain`` with hashlib's names in the fixed-width layout, everything else equal."""
    n = plain.n
    assert keyed.n == n, what
    assert np.array_equal(keyed.name_len, np.full(n, 32, np.int32)), what
    assert np.array_equal(keyed.name_off, 33 * np.arange(n, dtype=np.int64)), what
    exp = b"".join(hashed(x, key) + b"\x00" for x in table_names(plain))
    assert np.asarray(keyed.names_blob).tobytes() == exp, what
    for f in I32 + I64 + BLOBS:
        assert np.array_equal(np.asarray(getattr(keyed, f)), np.asarray(getattr(plain, f))), (what, f)


def make_inputs(name: str, outdir: str, bam_index: bool, hash_key=None, monkeypatch=None) -> dict:
    """A golden scenario's inputs X, or with ``hash_key`` X': the generator's write_bam wrapped so that
    each record is written under hashlib's name (copies: a duplicated record is one object twice)."""
    from genomeanonymizer_amd.synth import generate as G
    if hash_key is None:
        return G.make_inputs(name, outdir, bam_index)
    real = G.write_bam

    def renamed(path, contigs, records, **kw):
        out = []
        for r in records:
            r2 = copy.copy(r)
            r2.name = hashed(r.name.encode(), hash_key).decode()
            out.append(r2)
        return real(path, contigs, out, **kw)
    monkeypatch.setattr(G, "write_bam", renamed)
    try:
        return G.make_inputs(name, outdir, bam_index)
    finally:
        monkeypatch.setattr(G, "write_bam", real)


def collect(paths: dict, gz: bool = False) -> dict:
    """file tag -> bytes the pipeline wrote for the pair of ``paths`` (absent files left out)."""
    import gzip
    from genomeanonymizer_amd import short_read_tumor_normal_anonymizer as sr
    out = {}
    for tag, pre in (("tumor", sr.name_output(paths["T"])), ("normal", sr.name_output(paths["N"]))):
        for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
            p = pre + suf + (".gz" if gz else "")
            if os.path.exists(p):
                out[tag + suf] = gzip.open(p).read() if gz else open(p, "rb").read()
    out["statistics"] = open(paths["N"] + ".statistics.txt", "rb").read()
    return out


def run_files(name: str, workdir: str, anonymizer, bam_index: bool = False, hash_key=None, monkeypatch=None,
              gz: bool = False) -> dict:
    """The product pipeline on scenario ``name`` (X, or X' with ``hash_key``) under the environment the
    caller set; file tag -> bytes."""
    from genomeanonymizer_amd import short_read_tumor_normal_anonymizer as sr
    from genomeanonymizer_amd import writer
    shutil.rmtree(workdir, ignore_errors=True)
    paths = make_inputs(name, os.path.join(workdir, "in"), bam_index, hash_key, monkeypatch)
    t_out, n_out = sr.name_output(paths["T"]), sr.name_output(paths["N"])
    orig = writer.io_block_size
    writer.io_block_size = lambda d: 4096
    try:
        sr.run_short_read_tumor_normal_anonymizer([paths["vcf"]], [(paths["T"], paths["N"])], paths["ref"],
                                                  anonymizer, [(t_out, n_out)], True, 4)
    finally:
        writer.io_block_size = orig
    return collect(paths, gz)


def fastq_records(data: bytes) -> list:
    """(name without its /1 or /2, suffix, sequence, quality) per record."""
    lines = data.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    out = []
    for i in range(0, len(lines) - 1, 4):
        h = lines[i]
        assert h[:1] == b"@" and lines[i + 2] == b"+"
        h = h[1:]
        suf = h[-2:] if h[-2:] in (b"/1", b"/2") else b""
        out.append((h[:len(h) - len(suf)], suf, lines[i + 1], lines[i + 3]))
    return out


def record_multiset(data: bytes, key=None) -> collections.Counter:
    """The records of a FASTQ file as a multiset, their names hashed by hashlib with ``key``."""
    return collections.Counter((hashed(n, key) if key is not None else n, s, q1, q2)
                               for n, s, q1, q2 in fastq_records(data))


def helpers_repo() -> str:
    """The repository root (for a child process's PYTHONPATH)."""
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_anonymizer():
    from pyoracle import OracleEngine
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(engine=OracleEngine())


# ---- crafted names and streams ---------------------------------------------------------------------

NAME_LENGTHS = (0, 1, 31, 32, 55, 56, 63, 64, 65, 127, 128, 129, 254)


def crafted_names(seed: int = 3) -> list:
    """Names of every length of NAME_LENGTHS, random bytes 1..255, and three more that together hold
    every byte value 1..255."""
    rng = np.random.default_rng(seed)
    names = [bytes(rng.integers(1, 256, L, dtype=np.uint8).tolist()) for L in NAME_LENGTHS]
    allb = bytes(range(1, 256))
    names += [allb[:254], allb[254:], allb[100:229]]
    assert set(b"".join(names)) == set(range(1, 256))
    return names


CHUNK = 2048      # the device walk's chunk (csrc/ganon_bam.hip kChunk)
TAIL_STARTS = (1, 2, 3, 4, 5, 8, 35, 36, 37)    # bytes before a chunk's end at which a record starts


def _bam_record(rng, name: bytes, l_seq: int, aux: bytes = b"", n_ops: int = 2) -> bytes:
    """One BAM record; ``name`` is written as given (the caller adds the NUL, or leaves it out)."""
    import struct
    ops = [(int(rng.integers(1, 80)) << 4) | int(rng.choice([0, 1, 2, 4, 7, 8])) for _ in range(n_ops)]
    body = struct.pack("<iiBBHHHiiii", int(rng.integers(0, 2)), int(rng.integers(0, 10**6)), len(name),
                       int(rng.integers(0, 61)), 4680, len(ops), int(rng.choice([0, 1 | 2 | 64, 1 | 16 | 128])), l_seq,
                       int(rng.integers(-1, 2)), int(rng.integers(-1, 10**6)), int(rng.integers(-500, 500)))
    body += name + struct.pack(f"<{len(ops)}I", *ops)
    body += rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
    body += rng.integers(0, 60, l_seq, dtype=np.uint8).tobytes() + aux
    return struct.pack("<i", len(body)) + body


def crafted_stream(seed: int = 11):
    """(inflated BAM stream, offset of its first record) for the device decoder, under 1 MB: every name
    length 0..254 twice (random bytes 1..255, NUL-terminated) in records of varied sizes; records that
    start 1..37 bytes before the end of a 2,048-byte chunk of the walk (counted from the first
    record); 40 records with 2,000-base sequences back to back (a scatter group of 32 exceeds the
    16 KiB LDS stage); one record whose name lacks its NUL and one with l_read_name 0."""
    from test_bam_device import _header
    rng = np.random.default_rng(seed)
    head = _header([("c1", 10**6), ("c2", 2 * 10**6)])
    out = bytearray()

    def rname(L):
        return bytes(rng.integers(1, 256, L, dtype=np.uint8).tolist())
    lengths = list(range(255)) * 2
    rng.shuffle(lengths)
    tails = list(TAIL_STARTS)
    for k, L in enumerate(lengths):
        if k % 50 == 25 and tails:
            # a filler whose aux ends d bytes before a chunk's end: the next record starts there
            d = tails.pop()
            base = len(_bam_record(np.random.default_rng(0), b"f\x00", 10))
            target = ((len(out) + base + 64) // CHUNK + 1) * CHUNK - d
            out += _bam_record(rng, b"f\x00", 10, aux=bytes(target - len(out) - base))
            assert len(out) % CHUNK == CHUNK - d
        out += _bam_record(rng, rname(L) + b"\x00", int(rng.integers(0, 300)), aux=b"XAZ" + rname(int(rng.integers(0, 30))) + b"\x00")
        if k == 100:
            out += _bam_record(rng, b"no-nul-name", 75)          # l_read_name 11, no terminator
            out += _bam_record(rng, b"", 40)                      # l_read_name 0
        if k == 300:
            for j in range(40):
                out += _bam_record(rng, f"long{j}".encode() + b"\x00", 2000, n_ops=3)
    assert not tails and len(head) + len(out) < 1 << 20
    return np.frombuffer(head + bytes(out), np.uint8), len(head)
