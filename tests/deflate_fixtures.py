"""Blocks and checks shared by the deflate tests (tests/test_deflate_host.py on the CPU,
tests/test_gpu_deflate.py on the device): the fixture blocks, a BGZF member walk, and the host
check program (tools/deflate_host_check.cpp: the kernel's encoder source run on the host)."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_IN = 0xFF00
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


def de_bruijn(k: int, n: int) -> bytes:
    """B(k, n) over the letters 'a'..: every n-gram of the cyclic sequence occurs once."""
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(97 + c for c in seq)


def golden_text(name: str, which: str = "normal.1") -> bytes:
    return gzip.open(os.path.join(REPO, "tests", "golden", name, which + ".fastq.gz")).read()


_BLOCKS = None


def fixture_blocks():
    """[(name, bytes)], every block 1..0xFF00 bytes: the eight texts of test_inflate._zlib_streams
    (the empty one gives no block; the 64 KiB ones are cut at 0xFF00) and the encoder's edge cases."""
    global _BLOCKS
    if _BLOCKS is not None:
        return _BLOCKS
    import test_inflate
    rng = np.random.default_rng(11)
    texts = [t for _, t in test_inflate._zlib_streams()[0:64:8]]
    assert len(texts) == 8 and len(set(texts)) == 8
    out = []
    for k, t in enumerate(texts):
        for j in range(0, len(t), MAX_IN):
            out.append((f"text{k}_{j // MAX_IN}", t[j:j + MAX_IN]))
    nb = de_bruijn(6, 3)                       # 216 bytes of 6 letters, no 3 bytes twice (not cyclically closed)
    assert len({nb[i:i + 3] for i in range(len(nb) - 2)}) == len(nb) - 2
    half = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    out += [
        ("one_byte", b"Q"),
        ("two_bytes", b"QR"),
        ("noise_full", bytes(rng.integers(0, 256, MAX_IN, dtype=np.uint8))),
        ("zeros_full", b"\x00" * MAX_IN),
        ("run259", b"x" * 259),
        ("three", b"aaa"),
        ("no_repeat", nb),
        ("one_distance", nb * 3),
        ("window_edge", (half + half)[:MAX_IN]),
        ("config1", golden_text("config1")[:MAX_IN]),
        ("longpair", golden_text("longpair")[:MAX_IN]),
    ]
    assert all(1 <= len(b) <= MAX_IN for _, b in out)
    _BLOCKS = out
    return out


def walk_members(stream: bytes):
    """[(payload, crc, isize, member size)] of a BGZF stream; asserts the header of every member."""
    out, off = [], 0
    while off < len(stream):
        assert stream[off:off + 4] == b"\x1f\x8b\x08\x04", off
        assert stream[off + 10:off + 16] == b"\x06\x00BC\x02\x00", off
        size = struct.unpack_from("<H", stream, off + 16)[0] + 1
        assert 26 <= size <= 65536 and off + size <= len(stream), (off, size)
        crc, isize = struct.unpack_from("<II", stream, off + size - 8)
        assert isize <= MAX_IN
        out.append((stream[off + 18:off + size - 8], crc, isize, size))
        off += size
    return out


def check_members(stream: bytes, blocks):
    """Every member inflates (zlib, raw) to its block; CRC32 and ISIZE are zlib's; no member is larger
    than its stored form. Returns the first DEFLATE block type of every member."""
    members = walk_members(stream)
    assert len(members) == len(blocks)
    types = []
    for (payload, crc, isize, size), b in zip(members, blocks):
        d = zlib.decompressobj(-15)
        got = d.decompress(payload)
        assert d.eof and not d.unused_data
        assert got == b
        assert crc == zlib.crc32(b) and isize == len(b)
        assert size <= len(b) + 31
        types.append((payload[0] >> 1) & 3)
    return types


def build_host_check(dirpath, sanitize: bool = False) -> str:
    exe = os.path.join(str(dirpath), "deflate_host_check" + ("_san" if sanitize else ""))
    flags = SAN if sanitize else ["-O2"]
    r = subprocess.run(["g++", *flags, "-std=c++17", "-o", exe, os.path.join(REPO, "tools", "deflate_host_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run_blocks(exe: str, dirpath, blocks):
    """The members the host check program makes of `blocks`: (stream, sizes)."""
    d = str(dirpath)
    meta = struct.pack("<q", len(blocks))
    off = 0
    for b in blocks:
        meta += struct.pack("<qq", off, len(b))
        off += len(b)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(b"".join(blocks))
    with open(os.path.join(d, "meta.bin"), "wb") as f:
        f.write(meta)
    r = subprocess.run([exe, "blocks", os.path.join(d, "in.bin"), os.path.join(d, "meta.bin"),
                        os.path.join(d, "out.bin")], capture_output=True, text=True, env=_env(), timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    sizes = [int(x) for x in r.stdout.split()]
    stream = open(os.path.join(d, "out.bin"), "rb").read()
    assert sum(sizes) == len(stream) and len(sizes) == len(blocks)
    return stream, sizes


def run_lengths(exe: str, limit: int, counts):
    r = subprocess.run([exe, "lengths", str(limit), str(len(counts)), *[str(int(c)) for c in counts]],
                       capture_output=True, text=True, env=_env(), timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    return [int(x) for x in r.stdout.split()]


def run_compressed(name: str, workdir: str, anonymizer, bam_index: bool = False, block_size: int = 4096):
    """The scenario through the product pipeline (GANON_COMPRESS_OUTPUT is the caller's to set):
    (paths, tumor prefix, normal prefix)."""
    import shutil
    from genomeanonymizer_amd import short_read_tumor_normal_anonymizer as sr
    from genomeanonymizer_amd import writer
    from genomeanonymizer_amd.synth.generate import make_inputs
    shutil.rmtree(workdir, ignore_errors=True)
    paths = make_inputs(name, os.path.join(workdir, "in"), bam_index)
    t_out, n_out = sr.name_output(paths["T"]), sr.name_output(paths["N"])
    orig = writer.io_block_size
    writer.io_block_size = lambda d: block_size   # the block size the fixtures were written with
    try:
        sr.run_short_read_tumor_normal_anonymizer([paths["vcf"]], [(paths["T"], paths["N"])], paths["ref"],
                                                  anonymizer, [(t_out, n_out)], True, 4)
    finally:
        writer.io_block_size = orig
    return paths, t_out, n_out


def check_compressed_outputs(name: str, paths, t_out: str, n_out: str) -> int:
    """Every output of a compressed run of scenario ``name``: gzip reads it back equal to the golden
    plain file; no plain .fastq and no spool exist; it ends with the EOF member; every member has the
    BC subfield, BSIZE <= 65536, ISIZE <= 0xFF00. The statistics file is the plain run's. Returns the
    number of members seen (EOF members not counted)."""
    golden = os.path.join(REPO, "tests", "golden", name)
    n_members = 0
    for tag, pre in (("tumor", t_out), ("normal", n_out)):
        for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
            gp = os.path.join(golden, f"{tag}{suf}.gz")
            assert not os.path.exists(pre + suf), f"plain {tag}{suf} exists"
            if not os.path.exists(gp):
                assert not os.path.exists(pre + suf + ".gz"), f"unexpected {tag}{suf}.gz"
                continue
            raw = open(pre + suf + ".gz", "rb").read()
            assert gzip.open(pre + suf + ".gz").read() == gzip.open(gp).read(), tag + suf
            assert raw[-28:] == EOF_MEMBER
            members = walk_members(raw)
            assert members[-1][2] == 0
            assert all(m[2] > 0 for m in members[:-1])      # the only empty member is the last
            n_members += len(members) - 1
    d = os.path.dirname(t_out)
    assert [f for f in os.listdir(d) if "spool" in f] == []
    assert open(paths["N"] + ".statistics.txt").read() == open(os.path.join(golden, "normal.statistics.txt")).read()
    return n_members
