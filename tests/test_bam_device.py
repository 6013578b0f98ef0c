"""Device BAM record walk (``ganon_bam_columns``, include/ganon.h; SURVEY §8(f)4, the record walk
after the inflate): the records of an inflated BAM stream decoded to columns on the GPU.

Parity: the host decoder of libganon_host.so (``io.bam.ReadTable`` → ``records_to_columns``,
csrc/ganon_host.cpp), which the product reads its BAMs with and whose columns are pinned against
pysam/htslib semantics by the file-to-file goldens — column for column and byte for byte on the
same file: synthetic scenarios (short and long reads), the stream left on the device by the GPU
inflate, and hand-made streams built to defeat the chunk guesses (records longer than a chunk,
copies of whole record chains inside aux bytes, names without their NUL, unmapped records), plus
the host decoder's errors.

The walk's edges — the chunk grid, the stream's last bytes, the scatter's LDS stage, the per-record
arithmetic, decoys, `fixes` by equality — are pinned by the hand-built streams of tests/bam_streams.py
against the specification's restatement: tests/test_bam_streams.py (CPU) and
tests/test_gpu_bam_streams.py (device).
"""
import gzip
import struct

import numpy as np
import pytest

COLS = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len", "aux_len",
        "name_off", "cig_off", "seq_off", "qual_off", "aux_off")
BLOBS = ("names_blob", "cigar", "seq", "qual", "aux")


def first_record(d: bytes) -> int:
    from genomeanonymizer_amd.synth.bamwriter import first_record_offset
    return first_record_offset(d)


def inflated(path: str):
    d = gzip.decompress(open(path, "rb").read())   # BGZF is multi-member gzip
    return np.frombuffer(d, np.uint8), first_record(d)


def assert_same(cols, t):
    assert len(cols["pos"]) == t.n
    for f in COLS:
        assert np.array_equal(cols[f], getattr(t, f)), f
    for f in BLOBS:
        assert np.array_equal(cols[f], getattr(t, f)), f


from bam_streams import _header, _record  # noqa: E402,F401  (the builders' home; namehash_helpers imports them from here)


def adversarial_stream(seed: int = 5, n: int = 3000) -> bytes:
    """Header + records that defeat the chunk guesses: long reads and long random aux (records over
    a 4 KiB chunk, chunks with no record start), aux holding byte copies of the last few records (a
    chain of plausible records inside a record), names without a NUL, unmapped records."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        kind = i % 7
        if kind == 0 and len(recs) >= 4:
            aux = b"".join(recs[-4:])                                      # a plausible chain inside aux
        elif kind == 3:
            aux = rng.integers(0, 256, int(rng.integers(0, 12000)), dtype=np.uint8).tobytes()
        else:
            aux = b"XAZ" + bytes(rng.integers(65, 90, int(rng.integers(0, 40)), dtype=np.uint8)) + b"\x00"
        l_seq = int(rng.integers(3000, 20000)) if kind == 5 else None
        recs.append(_record(rng, i, aux=aux, l_seq=l_seq, nul=(i % 11 != 0)))
    return _header([("c1", 10**6), ("c2", 2 * 10**6), ("c3", 500)]) + b"".join(recs)


def write_raw_bam(path: str, stream: bytes, level: int = 1) -> None:
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    write_bgzf(path, stream, level)


def test_first_record_offset_and_adversarial_stream_decode_on_host(tmp_path):
    """The hand-made stream is a valid BAM for the host decoder (the parity side of the GPU tests)."""
    from genomeanonymizer_amd.io.bam import ReadTable
    s = adversarial_stream(n=400)
    path = str(tmp_path / "adv.bam")
    write_raw_bam(path, s)
    t = ReadTable(path, threads=2)
    assert t.n == 400
    d, p = inflated(path)
    assert d.tobytes() == s
    assert p == len(_header([("c1", 10**6), ("c2", 2 * 10**6), ("c3", 500)]))


@pytest.fixture(scope="module")
def ctx(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["config1", "edge", "long1", "fuzz1001"])
def test_device_columns_match_host_decoder(ctx, tmp_path, name):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.generate import generate, scenario
    paths = generate(scenario(name), str(tmp_path / "in"))
    for key in ("T", "N"):
        d, p = inflated(paths[key])
        cols, fixes = native.bam_columns_device(ctx.handle, d, p, len(d), on_host=True)
        assert_same(cols, ReadTable(paths[key], threads=2))
        if name == "config1":
            assert fixes == 0   # (short reads: every chunk's first guess is right)
        assert (np.diff(cols["rec_off"]) > 0).all() and (len(cols["rec_off"]) == 0 or cols["rec_off"][0] == p)


@pytest.mark.gpu
def test_device_columns_on_the_gpu_inflate_output(ctx, tmp_path):
    """Inflate on the device, then the record walk on the bytes the inflate left there."""
    import zlib
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.generate import generate, scenario
    paths = generate(scenario("config1"), str(tmp_path / "in"))
    raw = open(paths["N"], "rb").read()
    pay, isz, off = [], [], 0
    while off < len(raw):
        xlen = raw[off + 10] | (raw[off + 11] << 8)
        bsize = raw[off + 16] | (raw[off + 17] << 8)   # (our writer: the BC subfield is the only one)
        blen = bsize + 1
        n = int.from_bytes(raw[off + blen - 4:off + blen], "little")
        if n:
            pay.append(raw[off + 12 + xlen:off + blen - 8])
            isz.append(n)
        off += blen
    comp = np.frombuffer(b"".join(pay), np.uint8)
    in_len = np.array([len(x) for x in pay], np.int32)
    in_off = np.concatenate([[0], np.cumsum(in_len[:-1])]).astype(np.int64)
    out = ctx.inflate(comp, in_off, in_len, np.array(isz, np.int32))
    assert out.tobytes() == b"".join(zlib.decompress(x, -15) for x in pay)
    p = first_record(out.tobytes())
    cols, fixes = ctx.bam_columns(p, len(out))
    assert_same(cols, ReadTable(paths["N"], threads=2))


@pytest.mark.gpu
def test_device_columns_adversarial_stream(ctx, tmp_path):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    s = adversarial_stream()
    path = str(tmp_path / "adv.bam")
    write_raw_bam(path, s)
    d, p = inflated(path)
    cols, fixes = native.bam_columns_device(ctx.handle, d, p, len(d), on_host=True)
    assert_same(cols, ReadTable(path, threads=2))
    assert fixes >= 1   # (the aux copies and the long random aux make wrong guesses: proven and fixed)
    # the same records from a later start (the first chunk's own guess path) and as a suffix
    k = int(cols["rec_off"][1234])
    sub, _ = native.bam_columns_device(ctx.handle, d, k, len(d), on_host=True)
    assert np.array_equal(sub["pos"], cols["pos"][1234:]) and np.array_equal(sub["rec_off"], cols["rec_off"][1234:])
    # no records at all
    empty, _ = native.bam_columns_device(ctx.handle, d, len(d), len(d), on_host=True)
    assert len(empty["pos"]) == 0 and len(empty["names_blob"]) == 0


@pytest.mark.gpu
def test_device_columns_errors_match_host(ctx, tmp_path):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    rng = np.random.default_rng(9)
    hdr = _header([("c1", 1000)])
    good = [_record(rng, i) for i in range(50)]
    # a stream cut inside its last record: "bad record size" from both decoders
    s = hdr + b"".join(good)
    path = str(tmp_path / "cut.bam")
    write_raw_bam(path, s[:-7])
    with pytest.raises(native.GanonError, match="record size"):
        ReadTable(path, threads=1)
    d = np.frombuffer(s[:-7], np.uint8)
    with pytest.raises(native.GanonError, match="record size"):
        native.bam_columns_device(ctx.handle, d, len(hdr), len(d), on_host=True)
    # a record whose sequence runs past its block: "fields exceed block size" from both
    bad = bytearray(good[20])
    bad[4 + 16:4 + 20] = struct.pack("<i", 10**5)
    s = hdr + b"".join(good[:20]) + bytes(bad) + b"".join(good[21:])
    path = str(tmp_path / "bad.bam")
    write_raw_bam(path, s)
    with pytest.raises(native.GanonError, match="exceed block size"):
        ReadTable(path, threads=1)
    d = np.frombuffer(s, np.uint8)
    with pytest.raises(native.GanonError, match="exceed block size"):
        native.bam_columns_device(ctx.handle, d, len(hdr), len(d), on_host=True)
    # the context still works
    d = np.frombuffer(hdr + b"".join(good), np.uint8)
    cols, _ = native.bam_columns_device(ctx.handle, d, len(hdr), len(d), on_host=True)
    assert len(cols["pos"]) == 50


def _walk_chunks(d: bytes, p: int, chunk: int, probe: int = 4, span: int = None):
    """Host restatement of ganon_bam_columns' boundary proof (csrc/ganon_bam.hip: k_bam_guess,
    k_bam_check, k_bam_fix) at a small chunk size: guesses, exact-by-induction check, run fixes.
    Returns (record offsets, failing chunks met)."""
    n = len(d)
    span = span or 2 * chunk
    i32 = lambda o: int.from_bytes(d[o:o + 4], "little", signed=True)

    def plausible(o):
        if o + 36 > n:
            return None
        bs = i32(o)
        if bs < 32 or o + 4 + bs > n:
            return None
        tid, pos, l_rn = i32(o + 4), i32(o + 8), d[o + 12]
        ncig = d[o + 16] | (d[o + 17] << 8)
        lseq, mtid, mpos = i32(o + 20), i32(o + 24), i32(o + 28)
        if min(tid, pos, mtid, mpos) < -1 or l_rn < 1 or lseq < 0:
            return None
        if 32 + l_rn + 4 * ncig + (lseq + 1) // 2 + lseq > bs or d[o + 4 + 32 + l_rn - 1] != 0:
            return None
        return o + 4 + bs

    def chain(o):
        for _ in range(probe):
            if o >= n:
                return True
            o = plausible(o)
            if o is None:
                return False
        return True

    nc = (n - p + chunk - 1) // chunk
    entry, exitp = [0] * nc, [0] * nc

    def walk(c, e):
        ce = min(n, p + (c + 1) * chunk)
        s = e
        while 0 <= s < ce:
            bs = i32(s) if s + 4 <= n else -1
            if bs < 32 or s + 4 + bs > n:   # (the device walk stops on a bad size: exit -2)
                s = -2
                break
            s += 4 + bs
        entry[c], exitp[c] = e, (s if e >= 0 else -1)

    for c in range(nc):
        if c == 0:
            e = p
        else:
            cs = p + c * chunk
            lim = min(n, cs + span)
            e = next((o for o in range(cs, lim) if chain(o)), n if lim == n else -1)
        walk(c, e)
    fixes = 0
    while True:
        flag = [c > 0 and (entry[c] < 0 or entry[c] != exitp[c - 1]) for c in range(nc)]
        if not any(flag):
            break
        fixes += sum(flag)
        for c in range(1, nc):
            if flag[c] and not flag[c - 1]:
                cc = c
                while cc < nc and (cc == c or flag[cc]):
                    walk(cc, exitp[cc - 1])
                    cc += 1
    recs = []
    for c in range(nc):
        ce = min(n, p + (c + 1) * chunk)
        s = entry[c]
        while 0 <= s < ce:
            recs.append(s)
            s += 4 + i32(s)
    return recs, fixes


def test_chunk_proof_restatement_finds_every_record():
    """The boundary algorithm itself, on the host: wrong guesses (aux holding record chains, long
    records, chunks without a record start) are all caught and fixed, and the records found are the
    sequential walk's, for several chunk sizes."""
    s = adversarial_stream(seed=11, n=250)
    p = len(_header([("c1", 10**6), ("c2", 2 * 10**6), ("c3", 500)]))
    seq, o = [], p
    while o < len(s):
        seq.append(o)
        o += 4 + int.from_bytes(s[o:o + 4], "little", signed=True)
    assert o == len(s)
    total_fixes = 0
    for chunk in (97, 256, 1024, 2048):
        recs, fixes = _walk_chunks(s, p, chunk)
        assert recs == seq, chunk
        total_fixes += fixes
    assert total_fixes > 0
