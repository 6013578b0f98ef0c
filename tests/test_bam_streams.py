"""The hand-built streams of tests/bam_streams.py, checked without a device: every property a builder
claims is read back from its bytes (so a stream that stopped sitting on its edge fails here, not
silently on the GPU), the host decoder (``io.bam.ReadTable`` on the stream written as a BAM file)
equals the specification's restatement column for column, the boundary proof's restatement
(``test_bam_device._walk_chunks``) at the device's constants finds the sequential record offsets and
exactly the literal ``fixes``, and the host decoder refuses the malformed streams with its messages.
tests/test_gpu_bam_streams.py runs the same streams through the kernels."""
import struct

import numpy as np
import pytest

import bam_streams as S
from test_bam_device import _walk_chunks, write_raw_bam

C, SPAN, STAGE, RECS = S.CHUNK, S.GUESS_SPAN, S.SCAT_STAGE, S.SCAT_RECS


@pytest.fixture(scope="module")
def streams():
    return {b.name: b for b in S.all_streams()}


NAMES = [b.name for b in S.all_streams()]


def first_start_in_chunk(b, c):
    """The first record start in chunk c relative to the chunk's start, None if it holds none."""
    rel = [o - c * C for o in b.rel() if c * C <= o < (c + 1) * C]
    return rel[0] if rel else None


def first_start_from(b, o):
    """The first record start at or after relative offset o, less o."""
    return min(x for x in b.rel() + [b.n - b.p] if x >= o) - o


def fixed_fields(b, i):
    o = int(b.rec_off[i])
    f = struct.unpack_from("<iiiBBHHHiiii", b.data, o)
    return dict(zip(("block_size", "tid", "pos", "l_read_name", "mapq", "bin", "n_cigar", "flag", "l_seq", "mate_tid",
                     "mate_pos", "tlen"), f), offset=o)


def test_walk_defaults_are_the_kernel_sources_constants():
    """The defaults the builders sit on are the constants csrc/ganon_bam.hip spells out (the GPU tests
    ask the built library through ganon_bam_walk_params)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genomeanonymizer_amd", "csrc",
                            "ganon_bam.hip")).read()
    assert int(re.search(r"constexpr int64_t kChunk = (\d+);", src).group(1)) == S.CHUNK
    assert int(re.search(r"constexpr int kProbe = (\d+);", src).group(1)) == S.PROBE
    assert re.search(r"constexpr int64_t kGuessSpan = 2 \* kChunk;", src) and S.GUESS_SPAN == 2 * S.CHUNK
    assert int(re.search(r"#define GANON_SCAT_STAGE (\d+)", src).group(1)) == S.SCAT_STAGE
    assert int(re.search(r"#define GANON_SCAT_RECS (\d+)", src).group(1)) == S.SCAT_RECS


def test_grid_stream_sits_on_the_chunk_grid(streams):
    b = streams["grid"]
    rel, ends = b.rel(), b.rel()[1:] + [b.n - b.p]
    assert C in rel and C in ends                       # a start at a chunk's start, an end at a chunk's end
    assert b.props["start_at_chunk_start"] == C
    assert b.props["straddle"] == [2 * C - 1, 3 * C - 2, 4 * C - 3]
    for o in b.props["straddle"]:
        assert o in rel                                 # the size field [o, o + 4) crosses the boundary
    assert b.props["first_start_at_candidate"] == {5: 63, 6: 64}
    assert first_start_in_chunk(b, 5) == 63 and first_start_in_chunk(b, 6) == 64
    assert b.props["first_start_at_span"] == {8: SPAN - 1, 11: SPAN}
    assert first_start_from(b, 8 * C) == SPAN - 1       # the last candidate of chunk 8's window
    assert first_start_from(b, 11 * C) == SPAN          # one past chunk 11's window
    assert b.props["tail_chunks_without_start"] == [15, 16]
    assert (b.n - b.p) == 17 * C and max(rel) < 15 * C and max(rel) >= 14 * C
    for c in (15, 16):
        assert c * C + SPAN >= b.n - b.p                # the window reaches n: the guess is n


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("tail_")])
def test_tail_streams_end_where_they_claim(streams, name):
    b = streams[name]
    assert b.p % 4 == b.props["p_mod4"] and b.n % 4 == b.props["n_mod4"]
    o = b.p + b.props["last_start"]
    assert o == b.rec_off[-1]
    last_chunk = (b.n - b.p - 1) // C
    assert last_chunk >= 2 and (o - b.p) // C == last_chunk
    if b.props.get("odd_aux"):
        assert b.cols["aux_len"][-1] % 2 == 1 and b.cols["l_seq"][-1] > 0
        return
    assert fixed_fields(b, -1)["block_size"] == 33 and fixed_fields(b, -1)["l_read_name"] == 1
    assert o + 36 <= b.n < o + 40
    in_last = [x for x in b.rel() if x >= last_chunk * C]
    assert len(in_last) == b.props["starts_in_last_chunk"]


def test_tail_streams_cover_every_residue_pair(streams):
    seen = {(b.p % 4, b.n % 4, b.props["starts_in_last_chunk"]) for b in streams.values()
            if b.name.startswith("tail_p")}
    assert seen == {(p, n, k) for p in range(4) for n in range(4) for k in (1, 2)}
    assert {b.n % 4 for b in streams.values() if b.name.startswith("tail_oddaux")} == {0, 1, 2, 3}


def test_decoy_stream_holds_its_copies_at_chunk_starts(streams):
    b = streams["decoy"]
    d1, d2 = S.decoy_records()
    rel, d, p = set(b.rel()), b.data, b.p
    at = b.props
    for o in at.values():
        assert o % C == 0 and o not in rel              # a chunk's first candidate, and no record start
    negative = lambda o: int.from_bytes(d[p + o:p + o + 4], "little", signed=True) < 0
    o = at["chain_tiles_host_at"]
    assert d[p + o:p + o + len(d1 + d2)] == d1 + d2 and o + len(d1 + d2) in rel
    o = at["single_then_filler_at"]
    assert d[p + o:p + o + len(d1)] == d1 and negative(o + len(d1))
    o = at["chain_then_filler_at"]
    assert d[p + o:p + o + len(d1 + d2)] == d1 + d2 and negative(o + len(d1 + d2))
    o = at["single_to_n_at"]
    assert d[p + o:] == d1 and o // C == (b.n - p - 1) // C


FIELD_EDGES = {
    "l_read_name_1": lambda f, c: f["l_read_name"] == 1 and c["name_len"] == 0,
    "l_read_name_2": lambda f, c: f["l_read_name"] == 2 and c["name_len"] == 1,
    "l_read_name_255": lambda f, c: f["l_read_name"] == 255 and c["name_len"] == 254 and c["last_name_byte"] == 0,
    "name_without_nul": lambda f, c: f["l_read_name"] == 5 and c["last_name_byte"] != 0 and c["name_len"] == 4,
    "name_without_nul_255": lambda f, c: f["l_read_name"] == 255 and c["last_name_byte"] != 0 and c["name_len"] == 254,
    "n_cigar_0": lambda f, c: f["n_cigar"] == 0 and c["end"] == f["pos"] + 1,
    "n_cigar_1": lambda f, c: f["n_cigar"] == 1,
    "n_cigar_63": lambda f, c: f["n_cigar"] == 63 and c["ops"] == set(range(9)),
    "n_cigar_64": lambda f, c: f["n_cigar"] == 64 and c["ops"] == set(range(9)),
    "n_cigar_65": lambda f, c: f["n_cigar"] == 65 and c["ops"] == set(range(9)),
    "n_cigar_200": lambda f, c: f["n_cigar"] == 200 and c["ops"] == set(range(9)),
    "only_I_S_ops": lambda f, c: c["ops"] == {1, 4} and c["end"] == f["pos"] + 1 and not f["flag"] & 4,
    "unmapped_with_M": lambda f, c: f["flag"] & 4 and 0 in c["ops"] and c["end"] == f["pos"] + 1,
    "largest_end": lambda f, c: c["end"] == 2**31 - 1,
    "l_seq_0": lambda f, c: f["l_seq"] == 0,
    "l_seq_1": lambda f, c: f["l_seq"] == 1,
    "l_seq_2": lambda f, c: f["l_seq"] == 2,
    "l_seq_255": lambda f, c: f["l_seq"] == 255,
    "aux_len_0": lambda f, c: c["aux_len"] == 0,
    "all_minus_one": lambda f, c: (f["tid"], f["pos"], f["mate_tid"], f["mate_pos"]) == (-1, -1, -1, -1) and c["end"] == 0,
    "pos_minus_one_mapped": lambda f, c: f["pos"] == -1 and c["end"] == 9,
    "negative_tlen": lambda f, c: f["tlen"] == -(2**31),
    "flag_ffff_mapq_255": lambda f, c: f["flag"] == 0xFFFF and f["mapq"] == 255,
}
FIELD_EDGES.update({f"body_{n}": (lambda f, c, n=n: f["block_size"] - 32 == n) for n in (255, 256, 257, 1023, 1024, 1025)})


def test_fields_stream_has_one_record_per_edge(streams):
    b = streams["fields"]
    assert set(b.props) == set(FIELD_EDGES)
    for label, i in b.props.items():
        f = fixed_fields(b, i)
        co, nc = int(b.cols["cig_off"][i]), f["n_cigar"]
        c = dict(name_len=int(b.cols["name_len"][i]), end=int(b.cols["end"][i]), aux_len=int(b.cols["aux_len"][i]),
                 ops={int(w) & 15 for w in b.cols["cigar"][co:co + nc]},
                 last_name_byte=b.data[f["offset"] + 36 + f["l_read_name"] - 1])
        assert FIELD_EDGES[label](f, c), label
    # the reference lengths counted are those of M / D / N / = / X alone, in the spec's own words
    i = b.props["n_cigar_200"]
    co = int(b.cols["cig_off"][i])
    rl = sum(int(w) >> 4 for w in b.cols["cigar"][co:co + 200] if int(w) & 15 in (0, 2, 3, 7, 8))
    assert rl > 0 and b.cols["end"][i] == b.cols["pos"][i] + rl
    # a name without its NUL: the blob holds the l_read_name bytes and one NUL after them
    i = b.props["name_without_nul"]
    no = int(b.cols["name_off"][i])
    assert b.cols["names_blob"][no:no + 6].tobytes() == b"nonul\x00" and b.cols["name_off"][i + 1] == no + 6


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("staging_")])
def test_staging_streams_sit_on_the_stage(streams, name):
    b = streams[name]
    off = b.rec_off.tolist() + [b.n]
    s0 = off[0]
    assert s0 == b.p and s0 % 4 == b.props["s0_mod4"]
    span0 = off[RECS] - (s0 & ~3)
    assert span0 == b.props["first_run_span"] and span0 in (STAGE, STAGE + 1)
    assert ("fits" in name) == (span0 <= STAGE)
    big = b.props["big_record"]
    assert RECS <= big < 2 * RECS and off[big + 1] - off[big] > STAGE
    assert len(b.rec_off) == b.props["n_records"] and len(b.rec_off) in (3 * RECS, 3 * RECS + 1)
    assert off[3 * RECS] - (off[2 * RECS] & ~3) <= STAGE            # the third workgroup is staged
    # (the last workgroup, of RECS records or of one, ends at n by construction: off[-1] == n)


def test_staging_streams_cover_every_case(streams):
    st = [b for b in streams.values() if b.name.startswith("staging_")]
    assert {(b.props["s0_mod4"], b.props["first_run_span"]) for b in st} == {(r, STAGE + o) for r in range(4) for o in (0, 1)}
    assert {len(b.rec_off) % RECS for b in st} == {0, 1}


@pytest.mark.parametrize("name", NAMES)
def test_host_decoder_equals_the_restatement(streams, tmp_path, name):
    from genomeanonymizer_amd.io.bam import ReadTable
    b = streams[name]
    path = str(tmp_path / "s.bam")
    write_raw_bam(path, b.data)
    t = ReadTable(path, threads=2)
    assert t.n == len(b.rec_off)
    for f in S.COLS + S.BLOBS:
        assert np.array_equal(np.asarray(getattr(t, f)), b.cols[f]), f


@pytest.mark.parametrize("name", NAMES)
def test_boundary_proof_restatement_gives_the_literal_fixes(streams, name):
    b = streams[name]
    assert len(b.data) <= 512 << 10
    recs, fixes = _walk_chunks(b.data, b.p, S.CHUNK, probe=S.PROBE, span=S.GUESS_SPAN)
    assert recs == b.rec_off.tolist()
    assert fixes == b.fixes


def test_fixes_literals_depend_on_the_constants(streams):
    """The literals are properties of the streams at the device's constants, not of the streams alone:
    another probe depth or window gives other counts (so a retuned kernel cannot pass by accident)."""
    b = streams["decoy"]
    assert _walk_chunks(b.data, b.p, S.CHUNK, probe=1, span=S.GUESS_SPAN)[1] != b.fixes
    b = streams["grid"]
    assert _walk_chunks(b.data, b.p, S.CHUNK, probe=S.PROBE, span=S.GUESS_SPAN + 1)[1] != b.fixes
    assert _walk_chunks(b.data, b.p, S.CHUNK, probe=S.PROBE, span=S.GUESS_SPAN - 1)[1] != b.fixes


@pytest.mark.parametrize("bad", S.error_streams(), ids=lambda e: e.name)
def test_host_decoder_refuses_the_error_streams(tmp_path, bad):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    path = str(tmp_path / "bad.bam")
    write_raw_bam(path, bad.data)
    with pytest.raises(native.GanonError, match=bad.host_error):
        ReadTable(path, threads=1)


def test_error_streams_are_bad_where_they_claim():
    """Each malformed stream read back: the sequential walk meets the claimed fault, in the chunk the
    device is expected to name, or the first record whose fields pass its block is the one named."""
    import re
    for e in S.error_streams():
        d, o, n, i = e.data, e.p, len(e.data), 0
        while True:
            assert o < n, e.name
            bs = int.from_bytes(d[o:o + 4], "little", signed=True) if o + 4 <= n else None
            if bs is None or bs < 32 or o + 4 + bs > n:
                m = re.search(r"chunk (\d+)", e.device_error)
                assert m and int(m.group(1)) == (o - e.p) // C, e.name
                if e.name.startswith("past_n_tail"):
                    assert ((o & ~3) + 8 > n) and o + 4 <= n, e.name   # (the size is read byte by byte)
                break
            l_rn, ncig, lseq = d[o + 12], int.from_bytes(d[o + 16:o + 18], "little"), int.from_bytes(d[o + 20:o + 24], "little", signed=True)
            if lseq < 0 or 32 + l_rn + 4 * ncig + (lseq + 1) // 2 + lseq > bs:
                assert re.search(r"record (\d+):", e.device_error).group(1) == str(i), e.name
                break
            o += 4 + bs
            i += 1
