"""Region reads against an independent reference (tests/bam_reference.py: gzip, struct and numpy —
a restatement of AlignmentFile.fetch(contig, beg, end)), on a hand-built indexed BAM whose kept
records are not a suffix of the walked ones: long and short records mixed in one 16 kb window,
records without reference length (no CIGAR, all S/I, the unmapped flag over a CIGAR), l_seq == 0,
Z tags of some kB, unplaced records at the end. Both readers — the host walk (scan_region,
csrc/ganon_host.cpp) and the device path (ganon_region_decode, csrc/ganon_bam.hip: cut-mode walk,
k_region_keep, rocprim::select, k_bam_scatter over records that are not back to back) — must equal
the reference column for column and blob for blob. Malformed records (fields past their block) are
an error whenever the walk passes them, kept or not, and never one when it does not; an index that
points before its sequence is an error. Everything is compared for exact equality."""
import os
import shutil
import struct

import numpy as np
import pytest

import bam_reference as ref
from test_region_device import COLS, _regions

CONTIGS = [("c0", 200_000), ("c1", 50_000), ("c2", 1_000)]
N_KINDS = 12


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def build_mixed(path, n, long_lo, long_hi, tag_max, seed):
    """n records at sorted random positions on c0 and on c1, each of one of twelve equally likely
    kinds, none on c2, 40 unplaced records at the end; indexed."""
    from genomeanonymizer_amd.synth.bamwriter import BamRecord, write_bam
    rng = np.random.default_rng(seed)
    recs = []
    for tid in (0, 1):
        L = CONTIGS[tid][1]
        for pos in np.sort(rng.integers(0, L, n)).tolist():
            kind = int(rng.integers(0, N_KINDS))
            flag, tags, l_seq = 0, None, None
            if kind == 0:
                cigar = [("M", int(rng.integers(long_lo, long_hi + 1)))]
            elif kind == 1:
                cigar, flag, l_seq = [], 4 | 1 | 8, 75                       # placed unmapped, no CIGAR
            elif kind == 2:
                cigar = [("S", 30), ("I", 20)]                               # no reference length
            elif kind == 3:
                cigar = [("M", 40), ("D", 7), ("M", 30), ("N", 500), ("M", 31)]
            elif kind == 4:
                cigar, flag = [("M", 100)], 4                                # unmapped flag over a CIGAR
            elif kind == 5:
                cigar = [("M", 101)]
                tags = [("XZ", "Z", "".join(chr(c) for c in rng.integers(33, 127, int(rng.integers(1, tag_max + 1)))))]
            elif kind == 6:
                cigar, l_seq = [("=", 50), ("X", 1), ("=", 49)], 0           # l_seq == 0
            else:
                cigar = [("S", 3), ("M", 97)]
            if l_seq is None:
                l_seq = sum(k for op, k in cigar if op in "MIS=X")
            recs.append(BamRecord(f"r{len(recs)}", flag, tid, pos, int(rng.integers(0, 61)), cigar, tid,
                                  int(rng.integers(0, L)), 0, _seq(rng, l_seq), bytes(rng.integers(0, 42, l_seq, np.uint8)),
                                  tags))
    for _ in range(40):
        recs.append(BamRecord(f"u{len(recs)}", 4, -1, -1, 0, [], -1, -1, 0, _seq(rng, 60),
                              bytes(rng.integers(0, 42, 60, np.uint8))))
    write_bam(path, CONTIGS, recs, level=1, index=True)
    return path


def mixed_regions(records, seed):
    """Per contig: the edge set of test_region_device, regions that begin on, and one before, about
    every 40th distinct record end (and one that ends there), and 60 random ones."""
    rng = np.random.default_rng(seed)
    out = []
    for tid, (_, L) in enumerate(CONTIGS):
        regs = _regions(L, rng, 0)
        ends = sorted({r["end"] for r in records if r["tid"] == tid})
        for e in ends[::40]:
            regs += [(e, e + 10), (e - 1, e + 10), (max(0, e - 50), e)]
        for _ in range(60):
            a = int(rng.integers(0, L))
            regs.append((a, a + int(rng.integers(1, L // 3 + 1))))
        out += [(tid, a, b) for a, b in regs]
    return out


def _interleaved(records, tid, beg, end):
    """Are the kept flags over the walked records (tid, pos < end; file order) no step function: is
    some kept record followed by one that is not kept?"""
    if beg >= end:
        return False
    kept = [r["end"] > beg for r in records if r["tid"] == tid and r["pos"] < end]
    return any(a and not b for a, b in zip(kept, kept[1:]))


def _assert_equal(got, exp, where):
    n = len(exp["tid"])
    assert got.n == n, (where, got.n, n)
    for f in COLS:
        g = np.asarray(getattr(got, f))
        assert g.dtype == exp[f].dtype and np.array_equal(g, exp[f]), (where, f)


def _compare_all(reader, records, regions, where):
    for tid, a, b in regions:
        _assert_equal(reader.region(tid, a, b), ref.table(ref.fetch(records, tid, a, b)), (where, tid, a, b))


class Mixed:
    def __init__(self, path, seed):
        self.path = path
        self.records = ref.parse(path)
        self.regions = mixed_regions(self.records, seed)
        with_records = {r["tid"] for r in self.records}
        # the regions that read a window: not empty, on a sequence that has records
        self.n_reading = sum(1 for t, a, b in self.regions if a < b and t in with_records)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    p = build_mixed(str(tmp_path_factory.mktemp("mixed_small") / "small.bam"), 400, 2_100, 9_000, 5_000, seed=45)
    # under 1 MiB a region read's first window covers the sequence's whole remaining span
    assert os.path.getsize(p) < (1 << 20)
    return Mixed(p, seed=145)


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    p = build_mixed(str(tmp_path_factory.mktemp("mixed_large") / "large.bam"), 1_500, 5_000, 40_000, 9_000, seed=23)
    return Mixed(p, seed=24)


# ---- malformed records: 3000 records of 100M, 10 bp apart, record k's fields past its block ----
N_PLAIN = 3000
PLAIN_LAST_END = 10 * (N_PLAIN - 1) + 100
PATCHES = {"n_cigar": (16, struct.pack("<H", 60000)), "l_seq": (20, struct.pack("<i", 10**5))}


def build_plain(path, bad_k=None, patch="n_cigar", seed=31):
    """(offsets into the encoded record: block_size 0, tid 4, pos 8, l_read_name 12, mapq 13, bin 14,
    n_cigar 16, flag 18, l_seq 20). The index spans come from the good CIGAR."""
    from genomeanonymizer_amd.synth.bamwriter import BamRecord, write_bam

    class Bad(BamRecord):
        __slots__ = ()

        def encode(self):
            b = bytearray(super().encode())
            at, val = PATCHES[patch]
            b[at:at + len(val)] = val
            return bytes(b)

    rng = np.random.default_rng(seed)
    recs = []
    for i in range(N_PLAIN):
        cls = Bad if i == bad_k else BamRecord
        recs.append(cls(f"p{i}", 0, 0, 10 * i, 30, [("M", 100)], 0, 10 * i + 200, 300, _seq(rng, 100),
                        bytes(rng.integers(0, 42, 100, np.uint8))))
    write_bam(path, [("c0", 40_000)], recs, level=1, index=True)
    return path


def walk_passes(k, beg, end):
    """Does a region read's walk pass record k? It runs from the linear-index entry of beg's 16 kb
    window — the first record that ends inside or after that window — to the first record with
    pos >= end."""
    if beg >= end:
        return False
    w = min(beg >> 14, (PLAIN_LAST_END - 1) >> 14)
    first = next(i for i in range(N_PLAIN) if 10 * i + 100 > (w << 14))
    return first <= k and 10 * k < end


# (k, regions): the first two of each raise; (30140, 30390) with k the file's last record read 240 KB
# past the inflated data and returned no record and no error before scan_region checked the fields
MALFORMED = {
    2999: [(30140, 30390), (29940, 29995), (0, 5000), (16000, 29990), (29000, 29000)],
    1500: [(15150, 15400), (0, 100000), (0, 5000), (20000, 21000), (0, 15000), (14990, 15001)],
}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("plain")
    good = build_plain(str(d / "good.bam"))
    files = {(k, patch): build_plain(str(d / f"bad_{patch}_{k}.bam"), k, patch)
             for k in MALFORMED for patch in PATCHES}
    assert all(os.path.getsize(p) < (1 << 20) for p in files.values())
    return ref.parse(good), files


def _check_malformed(open_reader, plain, on_region=None):
    from genomeanonymizer_amd import native
    records, files = plain
    for (k, patch), path in files.items():
        r = open_reader(path)
        for a, b in MALFORMED[k]:
            raises = walk_passes(k, a, b)
            if raises:
                with pytest.raises(native.GanonError, match="exceed block size"):
                    r.region(0, a, b)
            else:
                _assert_equal(r.region(0, a, b), ref.table(ref.fetch(records, 0, a, b)), (path, a, b))
            if on_region:
                on_region(path, a, b, raises)
        r.close()


def make_stale(src, dst):
    """A copy of src whose index sends every read of contig 1 to contig 0's first record: every chunk
    begin and every linear offset of contig 1 (the pseudo-bin's count pair left alone)."""
    shutil.copy(src, dst)
    b = bytearray(open(src + ".bai", "rb").read())
    assert b[:4] == b"BAI\x01"
    n_ref, = struct.unpack_from("<i", b, 4)
    p, first0 = 8, None
    for t in range(n_ref):
        n_bin, = struct.unpack_from("<i", b, p)
        p += 4
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<Ii", b, p)
            p += 8
            for c in range(n_chunk):
                if t == 0 and bin_ == 37450 and c == 0:
                    first0, = struct.unpack_from("<Q", b, p)
                if t == 1 and not (bin_ == 37450 and c == 1):
                    struct.pack_into("<Q", b, p, first0)
                p += 16
        n_intv, = struct.unpack_from("<i", b, p)
        p += 4
        if t == 1:
            struct.pack_into(f"<{n_intv}Q", b, p, *([first0] * n_intv))
        p += 8 * n_intv
    with open(dst + ".bai", "wb") as fh:
        fh.write(bytes(b))
    return dst


def _check_stale(open_reader, small, path):
    from genomeanonymizer_amd import native
    r = open_reader(path)
    for tid, a, b in small.regions:
        if tid == 1 and a < b:
            with pytest.raises(native.GanonError, match="BAM index points before its sequence"):
                r.region(tid, a, b)
        else:
            _assert_equal(r.region(tid, a, b), ref.table(ref.fetch(small.records, tid, a, b)), (path, tid, a, b))
    r.close()


def _host(path):
    from genomeanonymizer_amd.io.bam import BamReader
    r = BamReader(path, 4)
    assert r.has_index
    return r


# ---- CPU ----
@pytest.mark.parametrize("which", ["small", "large"])
def test_host_regions_equal_reference(which, request):
    m = request.getfixturevalue(which)
    assert len(m.records) == 2 * (400 if which == "small" else 1_500) + 40
    r = _host(m.path)
    _compare_all(r, m.records, m.regions, which)
    r.close()


@pytest.mark.parametrize("which", ["small", "large"])
def test_kept_records_interleave_in_half_of_the_regions(which, request):
    m = request.getfixturevalue(which)
    n = sum(_interleaved(m.records, t, a, b) for t, a, b in m.regions)
    assert 2 * n >= len(m.regions), (n, len(m.regions))


def test_host_malformed_record_is_an_error_when_walked(plain):
    assert walk_passes(2999, 30140, 30390) and walk_passes(2999, 29940, 29995)
    assert walk_passes(1500, 15150, 15400) and walk_passes(1500, 0, 100000)
    assert not walk_passes(2999, 0, 5000) and not walk_passes(1500, 0, 5000) and not walk_passes(1500, 20000, 21000)
    assert len(ref.fetch(plain[0], 0, 0, 5000)) == 500
    _check_malformed(_host, plain)


def test_host_stale_index_is_an_error(small, tmp_path):
    _check_stale(_host, small, make_stale(small.path, str(tmp_path / "stale.bam")))


# ---- GPU ----
@pytest.fixture(scope="module")
def inflater(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.close()


def _device(inflater, window=0):
    def open_reader(path):
        from genomeanonymizer_amd.io.bam import BamReader
        r = BamReader(path, 4, window, inflater=inflater)
        assert r.has_index
        return r
    return open_reader


@pytest.mark.gpu
def test_device_regions_equal_reference_small(inflater, small):
    """Every region that reads a window is decoded on the device: the file is under 1 MiB, so the
    first window (dev_step, ganon_bam_reader_region) covers the sequence's remaining span and two
    blocks more, and every region ends inside it."""
    from genomeanonymizer_amd import native
    r = _device(inflater)(small.path)
    native.decode_phase_times(reset=True)
    _compare_all(r, small.records, small.regions, "small")
    ph = native.decode_phase_times(reset=True)
    r.close()
    print("small: regions", len(small.regions), "reading", small.n_reading, "device_regions", ph["device_regions"],
          "device_fallbacks", ph["device_fallbacks"])
    assert ph["device_regions"] == small.n_reading and ph["device_fallbacks"] == 0, (ph, small.n_reading)


@pytest.mark.gpu
def test_device_regions_equal_reference_large_through_fallback(inflater, large):
    """A reader window of 128 KiB: the decoder's first window is at most 16 of them, the larger
    regions go on past it and the host walk takes over from the bytes it inflated. (Measured: 16 s,
    11.5 s of it the 124 fallbacks' further 128 KiB windows, each a round trip through the GPU
    inflater; 234 regions decoded on the device.)"""
    from genomeanonymizer_amd import native
    r = _device(inflater, 1 << 17)(large.path)
    native.decode_phase_times(reset=True)
    _compare_all(r, large.records, large.regions, "large")
    ph = native.decode_phase_times(reset=True)
    r.close()
    print("large: regions", len(large.regions), "reading", large.n_reading, "device_regions", ph["device_regions"],
          "device_fallbacks", ph["device_fallbacks"])
    assert ph["device_fallbacks"] > 0 and ph["device_regions"] > 0, ph


@pytest.mark.gpu
def test_device_malformed_record_declines_only_when_walked(inflater, plain):
    """The host's errors on the host's regions (the device declines, the host walk reports) — also
    where the region walks the bad record without keeping it, as (15150, 15400) with a bad l_seq,
    which the round-6 kernel decoded to an empty table; a region that ends before the bad record is
    decoded on the device although its window — the whole file — holds the record."""
    from genomeanonymizer_amd import native

    def on_region(path, a, b, raises):
        ph = native.decode_phase_times(reset=True)
        want = (0, 0) if a >= b else (0, 1) if raises else (1, 0)
        assert (ph["device_regions"], ph["device_fallbacks"]) == want, (path, a, b, ph)

    native.decode_phase_times(reset=True)
    _check_malformed(_device(inflater), plain, on_region)


@pytest.mark.gpu
def test_device_stale_index_is_the_hosts_error(inflater, small, tmp_path):
    _check_stale(_device(inflater), small, make_stale(small.path, str(tmp_path / "stale.bam")))
