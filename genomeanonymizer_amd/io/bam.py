"""Coordinate-sorted BAM -> structure-of-arrays read table (native decoder).

Stands in for what the reference reads through pysam ``AlignedSegment`` objects
(query_name, flags, reference_start/end, cigar, query_sequence, qualities, SA tag): one
numpy column per field, one packed-nt16 sequence blob in BAM layout (which is exactly the
device batch layout of include/ganon.h). ``fetch`` reproduces htslib region semantics:
records of a contig overlapping [start, stop) in file order, overlap computed with
``bam_endpos`` (pos + reference length, or pos + 1 for unmapped / zero-length records).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np

from .. import native

FLAG_PAIRED = 0x1
FLAG_UNMAP = 0x4
FLAG_REVERSE = 0x10
FLAG_READ1 = 0x40
FLAG_READ2 = 0x80
FLAG_SECONDARY = 0x100
FLAG_SUPPLEMENTARY = 0x800


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class _Decoded:
    """Owns one native ``ganon_bam`` (decoded records); released when the last array viewing its
    memory is gone."""
    __slots__ = ("h", "__weakref__")

    def __init__(self, h):
        self.h = h

    def __del__(self):
        if self.h:
            native.host_lib().ganon_bam_close(self.h)
            self.h = None


def _view(ptr, n, dtype, owner: _Decoded):
    """A writable numpy view of n elements of native memory (no copy); the view keeps `owner`, and
    with it the native buffers, alive."""
    if n == 0:
        return np.zeros(0, dtype)
    addr = ptr if isinstance(ptr, int) else C.cast(ptr, C.c_void_p).value
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr)
    buf._owner = owner
    return np.frombuffer(buf, dtype=dtype)


class ReadTable:
    """All records of one BAM file, in file order."""

    def __init__(self, path: str, threads: int = 8, handle=None, name_key: Optional[bytes] = None,
                 known_sites=None, site_tally=None):
        """Decode the whole file, or take the records of an open ``ganon_bam`` handle (one
        reference sequence from ``BamReader.contig``); the table owns the handle from here on.
        ``name_key`` (--hash_read_names): every name is replaced, as it is decoded, by
        hex(BLAKE2s(name, key, digest_size=16)) (``ganon_bam_open_keyed``); a handle's names are
        whatever its reader decoded. ``known_sites`` (--known_sites; a known_sites.SitesTable, or a
        PairPanel that makes the table of this file's header): the panel mask rewrites the bases as they
        are decoded (``ganon_bam_open_ex``); ``known_masked`` counts them. ``site_tally``
        (--discover_sites): a pair (discover_sites.HostTally, dataset 0 tumor / 1 normal): the evidence of
        every record is OR-ed into the tally as it is decoded (``ganon_bam_open_ex2``), before any mask."""
        lib = native.host_lib()
        if handle is None:
            h = C.c_void_p()
            if site_tally is not None:
                tally, dataset = site_tally
                hdr = BamReader(path, threads=1)
                try:
                    seq_of = tally.seq_of_tid(hdr.ref_names)
                    if known_sites is not None:
                        from ..known_sites import resolve
                        known_sites = resolve(known_sites, hdr.ref_names)
                finally:
                    hdr.close()
                self.known_sites = known_sites
                key = bytes(name_key or b"")
                rc = lib.ganon_bam_open_ex2(os.fsencode(path), int(threads), key, len(key),
                                            known_sites.handle if known_sites is not None else None, tally.handle,
                                            int(dataset), native._ptr(seq_of, native._i32p), len(seq_of), C.byref(h))
            elif known_sites is not None:
                from ..known_sites import resolve
                if hasattr(known_sites, "table"):   # (the table goes by sequence id: the header first)
                    hdr = BamReader(path, threads=1)
                    try:
                        known_sites = resolve(known_sites, hdr.ref_names)
                    finally:
                        hdr.close()
                self.known_sites = known_sites   # (kept: the decode below reads its arrays)
                key = bytes(name_key or b"")
                rc = lib.ganon_bam_open_ex(os.fsencode(path), int(threads), key, len(key), known_sites.handle, C.byref(h))
            elif name_key:
                rc = lib.ganon_bam_open_keyed(os.fsencode(path), int(threads), bytes(name_key), len(name_key), C.byref(h))
            else:
                rc = lib.ganon_bam_open(os.fsencode(path), int(threads), C.byref(h))
            if rc != 0:
                raise native.GanonError(f"cannot decode {path}: {lib.ganon_host_last_error().decode()}")
        else:
            h = handle
        owner = _Decoded(h)
        v = native.BamView()
        lib.ganon_bam_view_get(h, C.byref(v))
        self._load(path, v, owner)
        self.known_masked = int(lib.ganon_bam_known_sites_masked(h))
        # --mask_sa_clips (a table with sa_clips): clip bases rewritten through SA tags, entries ignored
        self.sa_masked = int(lib.ganon_bam_sa_clips_masked(h))
        self.sa_ignored = int(lib.ganon_bam_sa_entries_ignored(h))
        self._finish()

    def _load(self, path: str, v, owner: _Decoded) -> None:
        """Per-record columns are copied (small); the byte blobs (names, CIGAR words, sequences,
        qualities, aux) are views of the decoder's buffers, which `owner` frees with the last view."""
        n = int(v.n_records)
        self.path = path
        self.n = n
        self.ref_names: List[str] = []
        ref_name_off = _arr(v.ref_name_off, v.n_ref, np.int64)
        raw = int(v.ref_names) if v.n_ref else 0
        for o in ref_name_off:
            self.ref_names.append(C.string_at(raw + int(o)).decode())
        self.ref_lens = _arr(v.ref_len, v.n_ref, np.int64)
        for f in ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len",
                  "aux_len"):
            setattr(self, f, _arr(getattr(v, f), n, np.int32))
        for f in ("name_off", "cig_off", "seq_off", "qual_off", "aux_off"):
            setattr(self, f, _arr(getattr(v, f), n, np.int64))
        self.names_blob = _view(v.names, int(v.names_bytes), np.uint8, owner)
        self.cigar = _view(v.cigar, int(v.cigar_ops), np.uint32, owner)
        self.seq = _view(v.seq, int(v.seq_bytes), np.uint8, owner)
        self.qual = _view(v.qual, int(v.qual_bytes), np.uint8, owner)
        self.aux = _view(v.aux, int(v.aux_bytes), np.uint8, owner)

    def _finish(self) -> None:
        self._names: Optional[List[str]] = None
        self.is_unmapped = (self.flag & FLAG_UNMAP) != 0
        self.is_reverse = (self.flag & FLAG_REVERSE) != 0
        # pair slot as AnonymizedRead.get_pair_idx (anonymizer_methods.py:119-123): -1 = neither flag
        self.mate_idx = np.where(self.flag & FLAG_READ1, 0, np.where(self.flag & FLAG_READ2, 1, -1)).astype(np.int8)
        self.has_cigar = self.n_cigar > 0
        self._index: Dict[int, tuple] = {}

    @property
    def names(self) -> List[str]:
        """Read names as str (built on first use: the native planner and the formatters work on
        ``names_blob`` / ``name_off`` / ``name_len`` directly)."""
        if self._names is None:
            nb = self.names_blob.tobytes()
            self._names = [nb[o:o + l].decode() for o, l in zip(self.name_off.tolist(), self.name_len.tolist())]
        return self._names

    def name(self, i: int) -> str:
        o = int(self.name_off[i])
        return self.names_blob[o:o + int(self.name_len[i])].tobytes().decode()

    # -- htslib-style region query -----------------------------------------------------
    def _tid_index(self, tid: int):
        ix = self._index.get(tid)
        if ix is None:
            rows = np.nonzero(self.tid == tid)[0].astype(np.int64)
            # int64: searchsorted with a Python int would cast an int32 array on every call
            pos = self.pos[rows].astype(np.int64)
            if len(pos) > 1 and np.any(np.diff(pos) < 0):
                raise ValueError(f"{self.path}: records of contig {tid} are not coordinate sorted")
            span = int((self.end[rows] - pos).max()) if len(rows) else 1
            ix = (rows, pos, span)
            self._index[tid] = ix
        return ix

    def tid_of(self, contig: str) -> int:
        try:
            return self.ref_names.index(contig)
        except ValueError:
            raise ValueError(f"invalid contig `{contig}`") from None

    def fetch(self, contig: str, start: Optional[int] = None, stop: Optional[int] = None) -> np.ndarray:
        """Record indices overlapping [start, stop) of ``contig`` in file order.

        Region errors follow pysam's region parser (raised as ValueError), which the
        reference hits for windows closer than 2003 bp or starting before 1001.
        """
        tid = self.tid_of(contig)
        length = int(self.ref_lens[tid])
        rstart = 0 if start is None else int(start)
        rstop = length if stop is None else int(stop)
        if rstart > rstop:
            raise ValueError(f"invalid coordinates: start ({rstart}) > stop ({rstop})")
        if rstart < 0:
            raise ValueError(f"start out of range ({rstart})")
        rows, pos, span = self._tid_index(tid)
        lo = int(np.searchsorted(pos, rstart - span, side="left"))
        hi = int(np.searchsorted(pos, rstop, side="left"))
        cand = rows[lo:hi]
        return cand[self.end[cand] > rstart]

    def has_tag(self, i: int, tag: bytes) -> bool:
        a = self.aux[self.aux_off[i]:self.aux_off[i] + self.aux_len[i]].tobytes()
        j = 0
        sizes = {ord(c): s for c, s in zip("AcCsSiIf", (1, 1, 1, 2, 2, 4, 4, 4))}
        while j + 3 <= len(a):
            t, ty = a[j:j + 2], a[j + 2]
            if t == tag:
                return True
            j += 3
            if ty in sizes:
                j += sizes[ty]
            elif ty in (ord("Z"), ord("H")):
                j = a.index(b"\x00", j) + 1
            elif ty == ord("B"):
                sub = a[j]
                cnt = int.from_bytes(a[j + 1:j + 5], "little")
                j += 5 + sizes[sub] * cnt
            else:
                raise ValueError(f"bad aux type in record {i}")
        return False

    def may_be_complex(self) -> bool:
        """Any secondary / supplementary record or SA tag candidate (cheap pre-check)."""
        return bool(np.any(self.flag & (FLAG_SECONDARY | FLAG_SUPPLEMENTARY))) or self._sa_candidates().size > 0

    def _sa_candidates(self) -> np.ndarray:
        a = self.aux
        if len(a) < 3:
            return np.zeros(0, np.int64)
        hit = np.nonzero((a[:-2] == ord("S")) & (a[1:-1] == ord("A")) & (a[2:] == ord("Z")))[0]
        if not len(hit):
            return np.zeros(0, np.int64)
        rows = np.searchsorted(self.aux_off, hit, side="right") - 1
        return np.unique(rows[(rows >= 0)])

    def tag_value(self, i: int, tag: bytes):
        """The value of a Z/H/A or integer tag of record ``i`` (None without it)."""
        a = self.aux[self.aux_off[i]:self.aux_off[i] + self.aux_len[i]].tobytes()
        j = 0
        sizes = {ord(c): s for c, s in zip("AcCsSiIf", (1, 1, 1, 2, 2, 4, 4, 4))}
        while j + 3 <= len(a):
            t, ty = a[j:j + 2], a[j + 2]
            j += 3
            if ty in (ord("Z"), ord("H")):
                k = a.index(b"\x00", j)
                if t == tag:
                    return a[j:k].decode()
                j = k + 1
            elif ty in sizes:
                if t == tag:
                    return a[j:j + sizes[ty]]
                j += sizes[ty]
            elif ty == ord("B"):
                sub = a[j]
                cnt = int.from_bytes(a[j + 1:j + 5], "little")
                j += 5 + sizes[sub] * cnt
            else:
                raise ValueError(f"bad aux type in record {i}")
        return None

    def sa_count(self) -> np.ndarray:
        """Per record: entries of its SA tag (``len(tag.rstrip(';').split(';'))``, AM:103-106), -1
        without one (cached)."""
        c = getattr(self, "_sa", None)
        if c is None:
            c = np.full(self.n, -1, np.int32)
            if self.n and self._sa_candidates().size:
                aux = np.ascontiguousarray(self.aux)
                off = np.ascontiguousarray(self.aux_off, np.int64)
                ln = np.ascontiguousarray(self.aux_len, np.int32)
                native.host_lib().ganon_aux_sa_count(aux.ctypes.data_as(native._u8p), off.ctypes.data_as(native._i64p),
                                                     ln.ctypes.data_as(native._i32p), self.n,
                                                     c.ctypes.data_as(native._i32p))
            self._sa = c
        return c

    def cigar_of(self, i: int) -> np.ndarray:
        o = int(self.cig_off[i])
        return self.cigar[o:o + int(self.n_cigar[i])]


class BamReader:
    """One BAM file read a reference sequence at a time (``ganon_bam_reader``, include/
    ganon_host.h): the bounded-memory counterpart of ``ReadTable(path)``. ``contig(tid)`` returns a
    ReadTable of that sequence's records only (file order, full reference list); the reader seeks
    through ``<bam>.bai`` when present, else streams forward. ``inflater``: a native.GpuInflater
    that inflates the reader's BGZF block windows instead of its zlib threads. ``name_key``
    (--hash_read_names): every table carries hashed names (``ganon_bam_reader_set_name_key``), and an
    inflater set on the reader hashes with the same key on the device (``GpuInflater.set_name_key``).
    ``known_sites`` (--known_sites; a known_sites.SitesTable, or a PairPanel that makes the table of
    this file's header): every table is masked by the panel (``ganon_bam_reader_set_known_sites``), and
    an inflater set on the reader holds the same table on the device (``GpuInflater.set_known_sites``)."""

    def __init__(self, path: str, threads: int = 8, window: int = 0, inflater=None,
                 name_key: Optional[bytes] = None, known_sites=None):
        lib = native.host_lib()
        h = C.c_void_p()
        rc = lib.ganon_bam_reader_open(os.fsencode(path), int(threads), C.byref(h))
        if rc != 0:
            raise native.GanonError(f"cannot open {path}: {lib.ganon_host_last_error().decode()}")
        self._h = h
        self.path = path
        self.name_key = bytes(name_key) if name_key else None
        if self.name_key and lib.ganon_bam_reader_set_name_key(h, self.name_key, len(self.name_key)) != 0:
            msg = lib.ganon_host_last_error().decode()
            self.close()
            raise native.GanonError(msg)
        if window:
            lib.ganon_bam_reader_set_window(h, int(window))
        self.inflater = None
        self.known_sites = None
        self.site_tally = None
        self._dev_masked0 = 0
        self._dev_sa0 = (0, 0)
        v = native.BamView()
        lib.ganon_bam_reader_header(h, C.byref(v))
        off = _arr(v.ref_name_off, v.n_ref, np.int64)
        raw = int(v.ref_names) if v.n_ref else 0
        self.ref_names: List[str] = [C.string_at(raw + int(o)).decode() for o in off]
        self.ref_lens = _arr(v.ref_len, v.n_ref, np.int64)
        self.has_index = bool(lib.ganon_bam_reader_has_index(h))
        if known_sites is not None:
            from ..known_sites import resolve
            self.known_sites = resolve(known_sites, self.ref_names)
            if lib.ganon_bam_reader_set_known_sites(h, self.known_sites.handle) != 0:
                msg = lib.ganon_host_last_error().decode()
                self.close()
                raise native.GanonError(msg)
        if inflater is not None:
            self.set_inflater(inflater)

    def set_inflater(self, inflater) -> None:
        """Block windows inflate on the GPU from now on (a native.GpuInflater, kept alive here: the
        reader calls into its context)."""
        if hasattr(inflater, "set_name_key"):
            # (set or cleared on every attach: the inflaters are kept across runs, stream._INFLATERS)
            inflater.set_name_key(self.name_key)
        elif self.name_key:
            raise native.GanonError("this inflater cannot hash read names (no set_name_key)")
        if hasattr(inflater, "set_known_sites"):
            inflater.set_known_sites(self.known_sites)   # (set or cleared on every attach, as the key)
            self._dev_masked0 = inflater.known_sites_masked() if self.known_sites is not None else 0
            if getattr(self.known_sites, "sa_clips", False):
                if not hasattr(inflater, "sa_clips_counts"):
                    raise native.GanonError("this inflater cannot mask SA clips (no sa_clips_counts)")
                self._dev_sa0 = inflater.sa_clips_counts()
        elif self.known_sites is not None:
            raise native.GanonError("this inflater cannot mask known sites (no set_known_sites)")
        native.host_lib().ganon_bam_reader_set_inflater(self._h, inflater.fn, inflater.handle, inflater.min_blocks)
        self.inflater = inflater
        if isinstance(inflater, native.GpuInflater) and os.environ.get("GANON_PINNED_SCAN", "1") != "0":
            # the scans' inflated bytes in one page-locked buffer kept by the reader: the inflater's
            # device-to-host copies go by DMA instead of through the runtime's staging copies
            hl = native.hip_lib()
            native.host_lib().ganon_bam_reader_set_buffer_alloc(
                self._h, C.cast(hl.ganon_pinned_alloc, C.c_void_p), C.cast(hl.ganon_pinned_free, C.c_void_p))
            if os.environ.get("GANON_DEVICE_REGION", "1") != "0":
                # region reads: the first window inflated, walked and filtered on the device, the
                # kept records' columns back by DMA (no host record walk or column copies)
                native.host_lib().ganon_bam_reader_set_region_decoder(
                    self._h, inflater.region_fn, inflater.handle, inflater.min_blocks,
                    C.cast(hl.ganon_pinned_free, C.c_void_p))

    def set_site_tally(self, tally, dataset: int = 0) -> None:
        """--discover_sites: the records of ``contig`` and ``region`` are tallied into ``tally`` (a
        discover_sites.HostTally) as dataset 0 (tumor) or 1 (normal) from now on, on the reader's threads
        (``ganon_bam_reader_set_site_tally``); None turns it off. Region reads a GPU inflater decodes are
        tallied on its context instead (``GpuInflater.set_site_tally``)."""
        lib = native.host_lib()
        if tally is None:
            lib.ganon_bam_reader_set_site_tally(self._h, None, 0, None, 0)
            self.site_tally = None
            return
        seq_of = tally.seq_of_tid(self.ref_names)
        if lib.ganon_bam_reader_set_site_tally(self._h, tally.handle, int(dataset), native._ptr(seq_of, native._i32p),
                                               len(seq_of)) != 0:
            raise native.GanonError(lib.ganon_host_last_error().decode())
        self.site_tally = (tally, int(dataset))   # (kept alive: the reader's threads read its genome)

    def sa_clips_counts(self) -> dict:
        """--mask_sa_clips: clip bases rewritten through SA tags by this reader's host decodes and, since
        it was attached, by its inflater's context, and the SA entries both ignored."""
        lib = native.host_lib()
        out = {"host": int(lib.ganon_bam_reader_sa_clips_masked(self._h)) if self._h else 0, "device": 0,
               "ignored": int(lib.ganon_bam_reader_sa_entries_ignored(self._h)) if self._h else 0}
        if (getattr(self.known_sites, "sa_clips", False) and self.inflater is not None
                and hasattr(self.inflater, "sa_clips_counts")):
            m, g = self.inflater.sa_clips_counts()
            out["device"] = m - self._dev_sa0[0]
            out["ignored"] += g - self._dev_sa0[1]
        return out

    def known_masked(self) -> int:
        """--known_sites: bases rewritten in this reader's tables so far, by its host decodes
        (``ganon_bam_reader_known_sites_masked``) and, since it was attached, by its inflater's context."""
        n = int(native.host_lib().ganon_bam_reader_known_sites_masked(self._h)) if self._h else 0
        if self.known_sites is not None and self.inflater is not None and hasattr(self.inflater, "known_sites_masked"):
            n += self.inflater.known_sites_masked() - self._dev_masked0
        return n

    def tid_of(self, contig: str) -> int:
        try:
            return self.ref_names.index(contig)
        except ValueError:
            return -1

    def contig(self, tid: int) -> ReadTable:
        """The records of BAM sequence ``tid`` (an empty table for tid < 0)."""
        if tid < 0:
            return self.empty()
        lib = native.host_lib()
        h = C.c_void_p()
        rc = lib.ganon_bam_reader_contig(self._h, int(tid), C.byref(h))
        if rc != 0:
            raise native.GanonError(f"cannot decode {self.path} sequence {tid}: "
                                    f"{lib.ganon_host_last_error().decode()}")
        return ReadTable(self.path, handle=h)

    def region(self, tid: int, beg: int, end: int) -> ReadTable:
        """The records of BAM sequence ``tid`` overlapping [beg, end) (0-based, htslib's fetch
        semantics), through the index (``ganon_bam_reader_region``; an index is required)."""
        if tid < 0:
            return self.empty()
        lib = native.host_lib()
        h = C.c_void_p()
        rc = lib.ganon_bam_reader_region(self._h, int(tid), int(beg), int(end), C.byref(h))
        if rc != 0:
            raise native.GanonError(f"cannot decode {self.path} sequence {tid} [{beg}, {end}): "
                                    f"{lib.ganon_host_last_error().decode()}")
        return ReadTable(self.path, handle=h)

    def empty(self) -> ReadTable:
        """A table with no records and this file's reference list."""
        t = ReadTable.__new__(ReadTable)
        t.path, t.n = self.path, 0
        t.ref_names, t.ref_lens = list(self.ref_names), self.ref_lens.copy()
        for f in ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len",
                  "aux_len"):
            setattr(t, f, np.zeros(0, np.int32))
        for f in ("name_off", "cig_off", "seq_off", "qual_off", "aux_off"):
            setattr(t, f, np.zeros(0, np.int64))
        t.names_blob = np.zeros(0, np.uint8)
        t.cigar = np.zeros(0, np.uint32)
        t.seq = np.zeros(0, np.uint8)
        t.qual = np.zeros(0, np.uint8)
        t.aux = np.zeros(0, np.uint8)
        t.known_masked = 0
        t.sa_masked = t.sa_ignored = 0
        t._finish()
        return t

    def close(self) -> None:
        if self._h:
            native.host_lib().ganon_bam_reader_close(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
