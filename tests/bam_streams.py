"""Hand-built inflated BAM streams for the device record walk (csrc/ganon_bam.hip: k_bam_guess,
k_bam_check, k_bam_fix, k_bam_offsets, k_bam_sizes, k_bam_scatter), each placed on an edge the kernel
code spells out: the chunk grid, the stream's last bytes, the scatter's LDS stage, the per-record
arithmetic, the decoys that make a guess wrong, and the malformed streams.

Every builder is deterministic (no random generator: the literal ``fixes`` of a stream must not move
with a library version) and returns a ``Built``: the stream, the offset ``p`` of its first record, the
expected columns — from the specification's restatement ``bam_reference.parse_stream`` / ``table``, not
from either of the project's decoders —, the sequential record offsets, the properties it claims (read
back from the bytes by tests/test_bam_streams.py) and the failing chunks the boundary proof meets
(``fixes``, a literal: the restatement ``test_bam_device._walk_chunks`` at the device's constants must
give it, and the device must report it).

The walk's constants are parameters with today's values as defaults (WALK_DEFAULTS); the GPU tests
assert that ``native.bam_walk_params()`` reports exactly these, so a retune fails there instead of
silently moving the edges.

Filler bytes (aux padding, sequence, qualities) are all >= 0x80: any 32-bit word read inside filler is
negative, so no record start is ever plausible there and the guesses of a stream are decided by its
records and its decoys alone.
"""
import struct
from dataclasses import dataclass, field

import numpy as np

import bam_reference as R

CHUNK = 2048          # kChunk: stream bytes per chunk
PROBE = 2             # kProbe: chained plausible records that make a guess
GUESS_SPAN = 4096     # kGuessSpan: the guess window from a chunk's start
SCAT_STAGE = 16384    # GANON_SCAT_STAGE: LDS bytes the scatter stages per workgroup
SCAT_RECS = 32        # GANON_SCAT_RECS: records per scatter workgroup
WALK_DEFAULTS = dict(chunk=CHUNK, probe=PROBE, guess_span=GUESS_SPAN, scat_stage=SCAT_STAGE, scat_recs=SCAT_RECS)

CONTIGS = (("c1", 10**6), ("c2", 2 * 10**6))
MIN_RECORD = 37       # block_size 33: the fixed fields and a one-byte name

COLS = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len", "aux_len",
        "name_off", "cig_off", "seq_off", "qual_off", "aux_off")
BLOBS = ("names_blob", "cigar", "seq", "qual", "aux")


def _header(contigs, extra_text: str = "") -> bytes:
    text = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in contigs) + extra_text
    h = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs))
    for n, l in contigs:
        nb = n.encode() + b"\x00"
        h += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
    return h


def _record(rng, i: int, aux: bytes = b"", l_seq: int = None, nul: bool = True, flag: int = None) -> bytes:
    name = f"q{i}".encode() + (b"\x00" if nul else b"")
    l_seq = int(rng.integers(0, 300)) if l_seq is None else l_seq
    ops = []
    for _ in range(int(rng.integers(0, 6))):
        ops.append((int(rng.integers(1, 80)) << 4) | int(rng.choice([0, 1, 2, 3, 4, 7, 8])))
    flag = int(rng.choice([0, 1 | 2 | 64, 1 | 16 | 128, 4, 1 | 4 | 8])) if flag is None else flag
    body = struct.pack("<iiBBHHHiiii", int(rng.integers(-1, 3)), int(rng.integers(-1, 10**6)), len(name),
                       int(rng.integers(0, 61)), 4680, len(ops), flag, l_seq, int(rng.integers(-1, 3)),
                       int(rng.integers(-1, 10**6)), int(rng.integers(-500, 500)))
    body += name + struct.pack(f"<{len(ops)}I", *ops)
    body += rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
    body += rng.integers(0, 60, l_seq, dtype=np.uint8).tobytes() + aux
    return struct.pack("<i", len(body)) + body


# ---- the expectation ---------------------------------------------------------------------------------

def sequential_offsets(d: bytes, p: int) -> np.ndarray:
    """The record starts of d[p:], one dependent read per record (what the chunked walk must equal)."""
    out = []
    while p < len(d):
        out.append(p)
        p += 4 + int.from_bytes(d[p:p + 4], "little", signed=True)
    assert p == len(d)
    return np.array(out, np.int64)


def apply_nulless_name_rule(records) -> list:
    """The one rule the project adds to the specification, for a read name stored without its NUL
    (l_read_name bytes, the last one not 0; htslib would read such a record's name past its end): both
    decoders keep the l_read_name bytes, append a NUL to the name blob, and report
    ``name_len = l_read_name - 1`` as for every other record. Applied to ``parse_stream``'s records in
    place; returns the indices it touched: ``bam_reference.table`` reports len(name) - 1, which now
    counts the record's last name byte, and ``expected_columns`` takes that one off again."""
    touched = []
    for i, r in enumerate(records):
        if len(r["name"]) > 0 and r["name"][-1] != 0:
            r["name"] = r["name"] + b"\x00"
            touched.append(i)
    return touched


def expected_columns(d: bytes, p: int) -> dict:
    """The 17 columns and 5 blobs of d[p:], from the specification's restatement alone."""
    recs = R.parse_stream(d, p)
    touched = apply_nulless_name_rule(recs)
    t = R.table(recs)
    for i in touched:
        t["name_len"][i] -= 1
    return t


@dataclass
class Built:
    name: str
    data: bytes
    p: int
    fixes: int
    props: dict = field(default_factory=dict)
    cols: dict = None
    rec_off: np.ndarray = None

    def __post_init__(self):
        self.rec_off = sequential_offsets(self.data, self.p)
        self.cols = expected_columns(self.data, self.p)

    @property
    def n(self) -> int:
        return len(self.data)

    def array(self) -> np.ndarray:
        return np.frombuffer(self.data, np.uint8)

    def rel(self) -> list:
        """Record starts relative to p (the chunk grid's origin)."""
        return (self.rec_off - self.p).tolist()


# ---- records -----------------------------------------------------------------------------------------

def fill(n: int, salt: int) -> bytes:
    """n filler bytes, every one >= 0x80, varied by position and ``salt``."""
    k = np.arange(n, dtype=np.int64)
    return (0x80 | ((salt * 11 + k * 37 + (k >> 7) * 5) % 128)).astype(np.uint8).tobytes()


def rec(name: bytes = b"r\x00", cigar=(), l_seq: int = 0, aux: bytes = b"", tid: int = 0, pos: int = 100, mapq: int = 30,
        flag: int = 0, mate_tid: int = -1, mate_pos: int = -1, tlen: int = 0, salt: int = 0) -> bytes:
    """One record, every field as given; ``name`` is written as it stands (the caller adds the NUL, or
    leaves it out); sequence and qualities are filler."""
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, 4680, len(cigar), flag, l_seq, mate_tid, mate_pos, tlen)
    body += name + struct.pack(f"<{len(cigar)}I", *cigar) + fill((l_seq + 1) // 2, salt + 1) + fill(l_seq, salt + 2) + aux
    return struct.pack("<i", len(body)) + body


def sized(total: int, salt: int = 0, **kw) -> bytes:
    """A record of exactly ``total`` bytes (its size field included): aux filler pads it."""
    base = len(rec(salt=salt, **kw))
    assert total >= base, (total, base)
    r = rec(salt=salt, aux=fill(total - base, salt + 3), **kw)
    assert len(r) == total
    return r


def cigar_ops(n: int, salt: int = 0) -> tuple:
    """n CIGAR words cycling through all nine op codes (M I D N S H P = X), lengths 1..90."""
    return tuple(((1 + (j * 7 + salt) % 90) << 4) | (j % 9) for j in range(n))


class _Layout:
    """Records laid back to back after a header; ``rel`` is the next record's start relative to p."""

    def __init__(self, p_mod4: int = None):
        extra = ""
        if p_mod4 is not None:   # a comment line whose length puts the first record at p = p_mod4 (mod 4)
            for k in range(4):
                extra = "@CO\t" + "x" * k + "\n"
                if len(_header(CONTIGS, extra)) % 4 == p_mod4:
                    break
        self.head = _header(CONTIGS, extra)
        self.p = len(self.head)
        assert p_mod4 is None or self.p % 4 == p_mod4
        self.recs = []
        self.rel = 0

    def add(self, r: bytes) -> int:
        off = self.rel
        self.recs.append(r)
        self.rel += len(r)
        return off

    def ordinary(self, total: int = None) -> int:
        """An everyday mapped record (varied by its index), of ``total`` bytes when given."""
        i = len(self.recs)
        kw = dict(name=b"q%d\x00" % i, cigar=((40 + i % 50) << 4,), l_seq=20 + (i * 7) % 60, pos=1000 + 3 * i, tid=i % 2,
                  flag=(0, 99, 147, 16)[i % 4], mapq=i % 61, mate_tid=i % 2, mate_pos=1200 + 3 * i,
                  tlen=(200 + i) * (-1 if i % 2 else 1), salt=i)
        base = len(rec(**kw))
        if total is None:
            total = base + (i * 13) % 90
        if total < base:
            kw = dict(name=b"s\x00", pos=1000 + 3 * i, salt=i)   # (38 bytes at the least)
        return self.add(sized(total, **kw))

    def fill_to(self, rel: int) -> None:
        """Ordinary records until the next one starts exactly at ``rel``."""
        assert rel == self.rel or rel - self.rel >= 450, (rel, self.rel)
        while rel - self.rel > 700:
            self.ordinary()
        gap = rel - self.rel
        if gap >= 400:
            self.ordinary(gap // 2)
        if rel - self.rel:
            self.ordinary(rel - self.rel)
        assert self.rel == rel

    def one_to(self, rel: int) -> int:
        """One record from here to ``rel``: no record starts in between."""
        return self.ordinary(rel - self.rel)

    def container(self, at: int, payload: bytes, tail: int) -> int:
        """One record whose aux holds ``payload`` at stream offset p + ``at`` (filler before it and
        ``tail`` filler bytes after it)."""
        i = len(self.recs)
        kw = dict(name=b"host%d\x00" % i, pos=7000 + i, salt=i)
        lead = at - self.rel - len(rec(**kw))
        assert lead >= 0
        return self.add(rec(aux=fill(lead, i + 5) + payload + fill(tail, i + 6), **kw))

    def data(self) -> bytes:
        return self.head + b"".join(self.recs)


# ---- the chunk grid ----------------------------------------------------------------------------------

def grid_stream(chunk: int = CHUNK, span: int = GUESS_SPAN) -> Built:
    """Record starts against the chunk grid (chunk c = [p + c chunk, p + (c + 1) chunk)):

    * a record ends exactly at chunk 0's end and the next starts exactly at chunk 1's start;
    * records start 1, 2 and 3 bytes before the starts of chunks 2, 3 and 4: their size fields straddle;
    * after a record that crosses into it, chunk 5's first start lies at candidate 63 (the last lane of
      the guess's first ballot) and chunk 6's at candidate 64 (the first lane of its second);
    * a record from just before chunk 8 ends at span offset ``span - 1`` of it: the last candidate the
      guess tests, still found, no fix;
    * a record from just before chunk 11 ends at span offset ``span`` of it: chunk 11 finds no start
      (entry -1) and chunk 12, whose guess is right, no longer follows its predecessor's exit: one
      failing run of two chunks, fixes = 2;
    * the last record starts in chunk 14 and ends with chunk 16: chunks 15 and 16 hold no start and
      their windows reach the stream's end, so both guess entry = n.
    """
    assert span == 2 * chunk   # (the chunk numbers below and the literal fixes)
    C = chunk
    L = _Layout()
    props = {}
    L.fill_to(C)
    props["start_at_chunk_start"] = C
    props["straddle"] = []
    for c, back in ((2, 1), (3, 2), (4, 3)):
        L.fill_to(c * C - back)
        props["straddle"].append(L.ordinary())
    L.fill_to(5 * C - 200)
    L.one_to(5 * C + 63)
    L.fill_to(6 * C - 200)
    L.one_to(6 * C + 64)
    props["first_start_at_candidate"] = {5: 63, 6: 64}
    L.fill_to(8 * C - 100)
    L.one_to(8 * C + span - 1)
    props["first_start_at_span"] = {8: span - 1, 11: span}
    L.fill_to(11 * C - 100)
    L.one_to(11 * C + span)
    L.fill_to(14 * C + 500)
    L.one_to(17 * C)
    props["tail_chunks_without_start"] = [15, 16]
    return Built("grid", L.data(), L.p, fixes=2, props=props)


# ---- the stream's end --------------------------------------------------------------------------------

def tail_streams(chunk: int = CHUNK) -> list:
    """The 16 combinations of p mod 4 and n mod 4, each twice: the last record is the smallest there is
    (block_size 33, a one-byte name, no CIGAR, no bases: its start o has o + 36 <= n < o + 40, the branch
    of the guess's ``plausible`` that reads the last bytes one by one), once as the second record of the
    last chunk (probed as the second of the guess's chain) and once as its only one (probed as the
    guess itself, its chain ending at n). Then four streams whose last record is an everyday one with
    an odd number of aux bytes, one per n mod 4. The last scatter workgroup of every stream is staged
    and ends at n: its last dword is cut by the stream's end unless n mod 4 = 0. No guess is wrong."""
    C = chunk
    out = []
    for pm in range(4):
        for nm in range(4):
            for variant in ("second", "only"):
                L = _Layout(p_mod4=pm)
                L.fill_to(2 * C - 150)
                body = (MIN_RECORD if variant == "only" else MIN_RECORD + 120)
                adj = (nm - (L.p + 2 * C + 100 + body)) % 4
                L.one_to(2 * C + 100 + adj)
                if variant == "second":
                    L.ordinary(120)
                last = L.add(rec(name=b"\x00", tid=1, pos=77, mapq=1, flag=4, tlen=-1))
                b = Built(f"tail_p{pm}_n{nm}_{variant}", L.data(), L.p, fixes=0,
                          props=dict(p_mod4=pm, n_mod4=nm, last_start=last, starts_in_last_chunk=2 if variant == "second" else 1))
                out.append(b)
    for nm in range(4):
        L = _Layout(p_mod4=(nm + 1) % 4)
        L.fill_to(2 * C + 300)
        done = False
        for name in (b"t\x00", b"tt\x00"):
            for adj in range(4):
                kw = dict(name=name, cigar=(33 << 4,), l_seq=33, pos=4242, salt=70 + nm)
                total = 150 + adj
                if (L.p + L.rel + total) % 4 == nm and (total - len(rec(**kw))) % 2 == 1 and not done:
                    last = L.add(sized(total, **kw))
                    done = True
        assert done
        out.append(Built(f"tail_oddaux_n{nm}", L.data(), L.p, fixes=0,
                         props=dict(p_mod4=(nm + 1) % 4, n_mod4=nm, last_start=last, odd_aux=True)))
    return out


# ---- decoys ------------------------------------------------------------------------------------------

def decoy_records() -> tuple:
    """Two records plausible on their own, whose byte copies are laid into other records' aux."""
    d1 = rec(name=b"decoy1\x00", cigar=(30 << 4,), l_seq=30, pos=5000, salt=90, aux=b"NMC\x01")
    d2 = rec(name=b"decoy2\x00", l_seq=11, pos=6000, flag=16, salt=91)
    return d1, d2


def decoy_stream(chunk: int = CHUNK, probe: int = PROBE) -> Built:
    """Byte copies of records inside aux, each exactly at a chunk's start (the guess's first candidate):

    * chunk 2: a chain of two that tiles the rest of its host record, so the walk from the wrong guess
      runs on into the true records and leaves at the true exit: chunk 2 alone fails (1);
    * chunk 4: one copy followed by filler: the chain's second record is not plausible, the guess moves
      on to the true start: no fix (0);
    * chunk 6: a chain of two followed by filler: the guess is wrong and its walk stops on a bad size —
      no error, since the chunk is not proven —, so chunk 7, guessed right, no longer follows: (2);
    * chunk 9, the last: one copy that ends exactly at n, a chain that reaches the stream's end after
      one record: the guess is wrong and counts one record too many until the fix (1).

    fixes = 4."""
    assert probe == 2
    C = chunk
    d1, d2 = decoy_records()
    L = _Layout()
    L.fill_to(2 * C - 100)
    L.container(2 * C, d1 + d2, 0)
    L.fill_to(4 * C - 100)
    L.container(4 * C, d1, 60)
    L.fill_to(6 * C - 100)
    L.container(6 * C, d1 + d2, 60)
    L.fill_to(9 * C - 100)
    L.container(9 * C, d1, 0)
    props = dict(chain_tiles_host_at=2 * C, single_then_filler_at=4 * C, chain_then_filler_at=6 * C, single_to_n_at=9 * C)
    return Built("decoy", L.data(), L.p, fixes=4, props=props)


# ---- per-record arithmetic ---------------------------------------------------------------------------

INT32_MAX = 2**31 - 1


def fields_stream() -> Built:
    """One record per edge of the per-record pass; ``props`` maps each label to its record's index."""
    L = _Layout()
    props = {}

    def put(label, r):
        props[label] = len(L.recs)
        L.add(r)
    nonzero = bytes(1 + k % 255 for k in range(255))
    L.ordinary()
    put("l_read_name_1", rec(name=b"\x00", cigar=(10 << 4,), l_seq=10, salt=1))
    put("l_read_name_2", rec(name=b"a\x00", cigar=(10 << 4,), l_seq=10, salt=2))
    put("l_read_name_255", rec(name=nonzero[:254] + b"\x00", cigar=(10 << 4,), l_seq=10, salt=3))
    put("name_without_nul", rec(name=b"nonul", cigar=(10 << 4,), l_seq=10, salt=4))
    put("name_without_nul_255", rec(name=nonzero, l_seq=3, salt=5))
    for nc in (0, 1, 63, 64, 65, 200):
        put(f"n_cigar_{nc}", rec(name=b"cig%d\x00" % nc, cigar=cigar_ops(nc, nc), l_seq=40, pos=10000 + nc, salt=10 + nc))
    put("only_I_S_ops", rec(name=b"is\x00", cigar=((10 << 4) | 4, (5 << 4) | 1, (20 << 4) | 4), l_seq=35, pos=300, salt=20))
    put("unmapped_with_M", rec(name=b"um\x00", cigar=(50 << 4, (7 << 4) | 2), l_seq=50, pos=400, flag=4 | 1, salt=21))
    put("largest_end", rec(name=b"big\x00", cigar=(100 << 4, (50 << 4) | 2), l_seq=100, pos=INT32_MAX - 150, salt=22))
    for ls in (0, 1, 2, 255):
        put(f"l_seq_{ls}", rec(name=b"ls%d\x00" % ls, cigar=((ls << 4),) if ls else (), l_seq=ls, pos=500 + ls, salt=30 + ls))
    for body in (255, 256, 257, 1023, 1024, 1025):
        put(f"body_{body}", sized(body + 36, name=b"b%d\x00" % body, cigar=(20 << 4, (3 << 4) | 1), l_seq=23, pos=600, salt=body))
    put("aux_len_0", rec(name=b"noaux\x00", cigar=(8 << 4,), l_seq=8, salt=40))
    put("all_minus_one", rec(name=b"m1\x00", tid=-1, pos=-1, mate_tid=-1, mate_pos=-1, flag=4 | 8 | 1, l_seq=12, salt=41))
    put("pos_minus_one_mapped", rec(name=b"m2\x00", tid=0, pos=-1, cigar=(10 << 4,), l_seq=10, salt=42))
    put("negative_tlen", rec(name=b"tl\x00", cigar=(9 << 4,), l_seq=9, tlen=-(2**31), mate_tid=1, mate_pos=5, salt=43))
    put("flag_ffff_mapq_255", rec(name=b"ff\x00", cigar=(9 << 4,), l_seq=9, flag=0xFFFF, mapq=255, salt=44))
    L.ordinary()
    return Built("fields", L.data(), L.p, fixes=0, props=props)


# ---- the scatter's LDS stage -------------------------------------------------------------------------

def staging_streams(stage: int = SCAT_STAGE, recs: int = SCAT_RECS, chunk: int = CHUNK, span: int = GUESS_SPAN) -> list:
    """Per s0 mod 4 = r (the first record's start; a0 = s0 rounded down to a dword) two streams: the
    first workgroup's ``recs`` records span exactly ``stage`` bytes from a0 (staged), or ``stage`` + 1
    (read from global memory). The second workgroup holds one record larger than ``stage`` (never
    staged; it lies on the chunk grid at [10 chunks - 100, 18 chunks + 200): chunks 10..16 find no start
    in their windows and chunk 17, guessed right, no longer follows: one failing run, fixes = 8). A third
    workgroup of everyday records, then none or one more record: 3 ``recs`` or 3 ``recs`` + 1 records,
    the last workgroup one record, every last run ending at n."""
    assert (stage, recs, chunk, span) == (16384, 32, 2048, 4096)   # (the layout below and the literal fixes)
    out = []
    for r in range(4):
        for over in (0, 1):
            L = _Layout(p_mod4=r)
            for i in range(recs - 1):
                L.ordinary(400 + (i * 29) % 200)
            L.ordinary(stage + over - r - L.rel)
            assert len(L.recs) == recs
            for _ in range(14):
                L.ordinary(250)
            L.ordinary(10 * chunk - 100 - L.rel)
            big = len(L.recs)
            L.one_to(18 * chunk + 200)
            for _ in range(recs - 16):
                L.ordinary()
            assert len(L.recs) == 2 * recs
            for _ in range(recs):
                L.ordinary()
            extra = (r + over) % 2
            if extra:
                L.ordinary()
            out.append(Built(f"staging_r{r}_{'over' if over else 'fits'}", L.data(), L.p, fixes=8,
                             props=dict(s0_mod4=r, first_run_span=stage + over, big_record=big,
                                        n_records=3 * recs + extra)))
    return out


# ---- malformed streams -------------------------------------------------------------------------------

@dataclass
class BadStream:
    name: str
    data: bytes
    p: int
    host_error: str       # the host decoder's message (a regular expression)
    device_error: str     # the device's, naming the chunk of the bad size or the first bad record

    def array(self) -> np.ndarray:
        return np.frombuffer(self.data, np.uint8)


def error_streams(chunk: int = CHUNK, span: int = GUESS_SPAN) -> list:
    """Streams both decoders must refuse, with the host's messages: a size field cut by the stream's end
    (1 to 3 bytes of it); block_size 31; a negative block_size; a record that runs past n — its start
    4 to 7 bytes before n, where the walk reads its size byte by byte, and a long one a byte short —;
    two records whose fields exceed their block (the smaller index is reported); a bad size in a
    chunk that lies after a failing run, reported once that run is fixed and the chunks before the bad
    one are exact. The device names the chunk that holds the bad size field's first byte."""
    C = chunk
    out = []

    def good(n_recs=40):
        L = _Layout()
        for _ in range(n_recs):
            L.ordinary()
        return L

    def size_error(name, L, at, data):
        out.append(BadStream(name, data, L.p, "record size", rf"bad record size \(chunk {at // C}\)"))
    for k in (1, 2, 3):
        L = good()
        size_error(f"size_cut_{k}", L, L.rel, L.data() + struct.pack("<i", 100)[:k])
    for name, bs in (("block_size_31", 31), ("block_size_negative", -5), ("block_size_most_negative", -(2**31))):
        L = good(20)
        at = L.rel
        L.add(struct.pack("<i", bs) + fill(40, 3))
        for _ in range(20):
            L.ordinary()
        size_error(name, L, at, L.data())
    for k in (4, 5, 6, 7):   # the bad record starts on a dword, k bytes before n: its dword pair would pass n
        L = good(39)
        L.ordinary(200 + (-(L.p + L.rel + 200)) % 4)
        assert (L.p + L.rel) % 4 == 0
        size_error(f"past_n_tail_{k}", L, L.rel, L.data() + struct.pack("<i", 100) + fill(k - 4, k))
    L = good()
    at = L.rel
    size_error("past_n_by_one", L, at, L.data() + sized(5000, name=b"long\x00")[:-1])
    L = good()
    recs = list(L.recs)
    for i in (25, 10):
        bad = bytearray(recs[i])
        bad[4 + 16:4 + 20] = struct.pack("<i", 10**5)   # l_seq
        recs[i] = bytes(bad)
    out.append(BadStream("fields_two_records", L.head + b"".join(recs), L.p, "exceed block size",
                         r"record 10: fields exceed block size"))
    L = good()
    recs = list(L.recs)
    bad = bytearray(recs[39])
    bad[4 + 12:4 + 14] = struct.pack("<H", 60000)       # n_cigar_op, in the last record
    recs[39] = bytes(bad)
    out.append(BadStream("fields_last_record", L.head + b"".join(recs), L.p, "exceed block size",
                         r"record 39: fields exceed block size"))
    assert span == 2 * C
    L = _Layout()
    L.fill_to(3 * C - 100)
    L.one_to(3 * C + span)          # (chunks 3 and 4 fail first)
    L.fill_to(7 * C + 300)
    at = L.rel
    L.add(struct.pack("<i", 31) + fill(31, 9))
    for _ in range(30):
        L.ordinary()
    size_error("bad_size_after_failing_run", L, at, L.data())
    return out


def all_streams() -> list:
    """Every well-formed stream, in a fixed order."""
    return [grid_stream()] + tail_streams() + [decoy_stream(), fields_stream()] + staging_streams()
