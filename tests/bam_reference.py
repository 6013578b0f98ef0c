"""A plain restatement of what ``AlignmentFile.fetch(contig, beg, end)`` returns, for the region
tests: gzip (BGZF is multi-member gzip), struct and numpy only — no ctypes, none of the project's
decoders. Written from the SAM/BAM v1 specification (§4.2 the record layout) and htslib's
``bam_endpos`` / ``reg2bins``:

* a record's end is ``pos + rl``, rl the summed lengths of its M/D/N/=/X ops, rl = 0 when the
  unmapped flag is set or it has no CIGAR, and ``pos + 1`` when rl == 0;
* a region keeps, in file order, the records with ``tid == tid and pos < end and bam_endpos > beg``,
  and nothing when ``beg >= end`` (reg2bins yields no bin for an empty interval).
"""
import gzip
import struct

import numpy as np

I32_COLS = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len",
            "aux_len")
_REF_OPS = (0, 2, 3, 7, 8)   # M D N = X


def parse(path):
    """Every record of the file, in file order, as a dict of its fixed fields, ``end`` (bam_endpos)
    and its variable parts: ``name`` (bytes, NUL included), ``cigar`` (list of uint32 words), ``seq``
    (packed bytes), ``qual`` and ``aux`` (bytes)."""
    with open(path, "rb") as fh:
        d = gzip.decompress(fh.read())
    return parse_stream(d, header_end(d))


def header_end(d) -> int:
    """The offset of the first record of the inflated stream ``d``: after the header text and the
    reference sequence list (SAM/BAM v1 §4.2)."""
    assert d[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", d, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, p)
        p += 4 + l_name + 4
    return p


def parse_stream(d, p):
    """``parse`` on an inflated stream: the records that lie back to back in ``d`` from offset ``p`` to
    its end."""
    out = []
    while p < len(d):
        block_size, = struct.unpack_from("<i", d, p)
        tid, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, mate_tid, mate_pos, tlen = \
            struct.unpack_from("<iiBBHHHiiii", d, p + 4)
        q = p + 36
        name = d[q:q + l_read_name]
        q += l_read_name
        cigar = list(struct.unpack_from(f"<{n_cigar}I", d, q))
        q += 4 * n_cigar
        seq = d[q:q + (l_seq + 1) // 2]
        q += (l_seq + 1) // 2
        qual = d[q:q + l_seq]
        q += l_seq
        aux = d[q:p + 4 + block_size]
        assert q <= p + 4 + block_size
        rl = 0
        if not (flag & 4) and n_cigar:
            rl = sum(w >> 4 for w in cigar if (w & 0xF) in _REF_OPS)
        out.append(dict(tid=tid, pos=pos, end=pos + (rl if rl else 1), flag=flag, mapq=mapq, l_seq=l_seq,
                        n_cigar=n_cigar, mate_tid=mate_tid, mate_pos=mate_pos, tlen=tlen, name=name, cigar=cigar,
                        seq=seq, qual=qual, aux=aux))
        p += 4 + block_size
    assert p == len(d)
    return out


def fetch(records, tid, beg, end):
    if beg >= end:
        return []
    return [r for r in records if r["tid"] == tid and r["pos"] < end and r["end"] > beg]


def table(records):
    """The ReadTable columns of ``records``: a dict of numpy arrays."""
    t = {}
    for f in I32_COLS:
        if f == "name_len":
            v = [len(r["name"]) - 1 for r in records]
        elif f == "aux_len":
            v = [len(r["aux"]) for r in records]
        else:
            v = [r[f] for r in records]
        t[f] = np.array(v, np.int32).reshape(-1)
    # exclusive prefix sums; cig_off counts ops (the cigar blob is uint32 words)
    for off, part in (("name_off", "name"), ("cig_off", "cigar"), ("seq_off", "seq"), ("qual_off", "qual"),
                      ("aux_off", "aux")):
        sizes = np.array([len(r[part]) for r in records], np.int64).reshape(-1)
        t[off] = np.cumsum(sizes) - sizes
    t["names_blob"] = np.frombuffer(b"".join(r["name"] for r in records), np.uint8)
    t["cigar"] = np.array([w for r in records for w in r["cigar"]], np.uint32).reshape(-1)
    t["seq"] = np.frombuffer(b"".join(r["seq"] for r in records), np.uint8)
    t["qual"] = np.frombuffer(b"".join(r["qual"] for r in records), np.uint8)
    t["aux"] = np.frombuffer(b"".join(r["aux"] for r in records), np.uint8)
    return t
