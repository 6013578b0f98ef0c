"""--known_sites PANEL.vcf[.gz]: a population panel of single-nucleotide variants, masked in every
read where its record is decoded.

The masking rule overwrites a germline SNV only when a tumor and a normal read of one pileup scope
show it; reads outside every scope, window-straddling pairs and sites the normal sample happens not to
show reach the FASTQ as sequenced. With a panel, every base that is aligned to a listed position and
shows a listed ALT allele becomes the reference base as its record enters a table — on the host in
``records_to_columns``, on the device in ``k_bam_known_mask`` — so that nothing downstream knows the
difference: the run writes the files a run without the option writes on inputs already rewritten.

* ``load_panel(path, fasta)`` parses the VCF once per process and checks it against the FASTA.
* ``PairPanel`` is the panel less the positions of one tumor/normal pair's own SNV calls (the calls
  the product exists to keep); ``PairPanel.table(ref_names)`` is the table by BAM sequence id that the
  decoders take (``SitesTable``: ``site_off`` / ``site_pos`` / ``site_code`` of include/ganon_host.h).
* ``pair_default(fasta, windows)`` is what the pipelines call: None unless ``GANON_KNOWN_SITES`` names
  a panel.

Used lines: REF one of A, C, G, T (upper-cased first) with at least one one-base ALT of A, C, G, T other
than REF; their other ALTs (longer, symbolic, ``*``, ``.``) are ignored. Lines with a longer REF
(deletions, MNVs) are skipped and counted. Lines and ALTs at one position are OR-ed; two REFs at one
position, a REF that is not the FASTA's base there, a position past the contig's end and an unreadable
file are errors (``KnownSitesError``). Contigs absent from the FASTA or from a BAM header are ignored
and counted: panels are genome-wide.
"""
from __future__ import annotations

import ctypes as C
import gzip
import logging
import os
import time
import zlib
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .variants import VariantType

log = logging.getLogger("genomeanonymizer_amd")

ENV = "GANON_KNOWN_SITES"
SA_ENV = "GANON_MASK_SA_CLIPS"    # --mask_sa_clips: soft clips masked along their SA alignments
NT16_OF = {"A": 1, "C": 2, "G": 4, "T": 8}


class KnownSitesError(native.GanonError):
    """A panel that cannot be used: the command line ends before any output file is opened."""


class Panel:
    """Per contig name: sorted 0-based positions (int32) and codes (uint8, ref_nt16 << 4 | alt_mask)."""

    def __init__(self, path: str, contigs: Dict[str, Tuple[np.ndarray, np.ndarray]], stats: dict):
        self.path = path
        self.contigs = contigs
        self.stats = stats

    @property
    def n_sites(self) -> int:
        return sum(len(p) for p, _ in self.contigs.values())


def load_panel(path: str, fasta) -> Panel:
    """Parse and check the panel (plain or .gz, as io/vcf.py reads a VCF)."""
    t0 = time.time()
    sites: Dict[str, Dict[int, int]] = {}
    skipped = no_alt = 0
    off_fasta: Dict[str, int] = {}
    raw: Dict[str, bytes] = {}
    try:
        opener = gzip.open if path.endswith(".gz") else open
        with opener(path, "rt") as fh:
            for ln, line in enumerate(fh, 1):
                if not line.strip() or line.startswith("#"):
                    continue
                f = line.rstrip("\r\n").split("\t")
                if len(f) < 5:
                    raise KnownSitesError(f"{path}:{ln}: a VCF line has at least five tab-separated fields")
                contig, ref = f[0], f[3].upper()
                try:
                    pos = int(f[1]) - 1
                except ValueError:
                    raise KnownSitesError(f"{path}:{ln}: POS is not a number") from None
                if len(ref) != 1:
                    skipped += 1      # a deletion or an MNV: not used
                    continue
                if ref not in NT16_OF:
                    skipped += 1
                    continue
                alt = 0
                for a in f[4].upper().split(","):
                    if a in NT16_OF and a != ref:
                        alt |= NT16_OF[a]
                if not alt:
                    no_alt += 1       # an insertion, a symbolic allele, '*' or '.' alone
                    continue
                if contig not in fasta.index:
                    off_fasta[contig] = off_fasta.get(contig, 0) + 1
                    continue
                seq = raw.get(contig)
                if seq is None:
                    seq = raw[contig] = fasta.raw(contig)
                if pos < 0 or pos >= len(seq):
                    raise KnownSitesError(f"{path}:{ln}: {contig}:{pos + 1} is past the contig's end ({len(seq)})")
                base = chr(seq[pos]).upper()
                per = sites.setdefault(contig, {})
                if base != ref:   # (two lines with different REF at one position end here: one of them is wrong)
                    raise KnownSitesError(f"{path}:{ln}: REF {ref} at {contig}:{pos + 1}, the reference has {base}"
                                          + (" (an earlier line gave that REF: two REF alleles at one position)"
                                             if pos in per else ""))
                per[pos] = (NT16_OF[ref] << 4) | alt | per.get(pos, 0)
    except (OSError, EOFError, UnicodeDecodeError, zlib.error) as e:
        raise KnownSitesError(f"cannot read the known-sites panel {path}: {e}") from None
    contigs = {}
    for name, per in sites.items():
        pos = np.fromiter(per.keys(), np.int64, len(per))
        code = np.fromiter(per.values(), np.uint8, len(per))
        order = np.argsort(pos, kind="stable")
        contigs[name] = (pos[order].astype(np.int32), code[order])
    stats = {"sites": sum(len(p) for p, _ in contigs.values()), "skipped_long_ref": skipped, "no_snv_alt": no_alt,
             "contigs_not_in_reference": len(off_fasta), "lines_on_them": sum(off_fasta.values()),
             "load_s": round(time.time() - t0, 3)}
    log.info("known sites %s: %d sites used, %d lines skipped (REF longer than one base or not A/C/G/T), %d without a "
             "one-base ALT, %d lines on %d contigs that are not in the reference, loaded in %.3f s", path, stats["sites"],
             skipped, no_alt, stats["lines_on_them"], len(off_fasta), stats["load_s"])
    return Panel(path, contigs, stats)


def mask_sa_clips_default() -> bool:
    """``GANON_MASK_SA_CLIPS=1`` (``--mask_sa_clips``), for library callers and for spawned pair workers
    and ranks."""
    return os.environ.get(SA_ENV, "0") == "1"


def sorted_names(ref_names: Sequence[str]) -> Tuple[bytes, np.ndarray, np.ndarray]:
    """The header's names for the SA rule's binary search: sorted bytewise and distinct (a name listed
    twice: its first sequence), as (blob, name_off int64 [n + 1], name_tid int32 [n])."""
    first: Dict[bytes, int] = {}
    for t, name in enumerate(ref_names):
        first.setdefault(name.encode(), t)
    names = sorted(first)
    off = np.zeros(len(names) + 1, np.int64)
    if names:
        off[1:] = np.cumsum([len(b) for b in names])
    return b"".join(names), off, np.asarray([first[b] for b in names], np.int32)


class SitesTable:
    """The table one decoder takes: per BAM sequence id the slice [site_off[t], site_off[t + 1]) of
    ``site_pos`` / ``site_code``, and the quality a rewritten base gets (-1: qualities stay). ``handle``
    is the host library's ``ganon_sites`` (made on first use, destroyed with this object). With
    ``sa_clips`` (--mask_sa_clips) and the header's ``ref_names`` the decoders also mask each record's
    soft clips along its SA alignments (csrc/ganon_sa_clips.h)."""

    def __init__(self, site_off: np.ndarray, site_pos: np.ndarray, site_code: np.ndarray, quality: int = -1,
                 ref_names: Optional[Sequence[str]] = None, sa_clips: bool = False):
        self.site_off = np.ascontiguousarray(site_off, np.int64)
        self.site_pos = np.ascontiguousarray(site_pos, np.int32)
        self.site_code = np.ascontiguousarray(site_code, np.uint8)
        self.quality = int(quality)
        self.n_ref = len(self.site_off) - 1
        self.sa_clips = bool(sa_clips)
        if self.sa_clips:
            if ref_names is None or len(ref_names) != self.n_ref:
                raise native.GanonError("mask_sa_clips: the table needs the BAM header's sequence names")
            self.sa_blob, self.sa_off, self.sa_tid = sorted_names(ref_names)
        self._h = None

    @property
    def n(self) -> int:
        return int(len(self.site_pos))

    @property
    def handle(self):
        if self._h is None:
            lib = native.host_lib()
            h = C.c_void_p()
            rc = lib.ganon_sites_create(self.n_ref, self.site_off.ctypes.data_as(native._i64p),
                                        self.site_pos.ctypes.data_as(native._i32p),
                                        self.site_code.ctypes.data_as(native._u8p), self.quality, C.byref(h))
            if rc != 0:
                raise native.GanonError(lib.ganon_host_last_error().decode())
            if self.sa_clips and lib.ganon_sites_set_sa_clips(h, len(self.sa_tid), self.sa_blob,
                                                              native._ptr(self.sa_off, native._i64p),
                                                              native._ptr(self.sa_tid, native._i32p), 1) != 0:
                msg = lib.ganon_host_last_error().decode()
                lib.ganon_sites_destroy(h)
                raise native.GanonError(msg)
            self._h = h
        return self._h

    def __del__(self):  # pragma: no cover
        try:
            if self._h:
                native.host_lib().ganon_sites_destroy(self._h)
                self._h = None
        except Exception:
            pass


def own_snv_positions(windows: Iterable) -> Dict[str, np.ndarray]:
    """The 0-based positions [pos, end] of every SNV-type record of a pair's own VCF, by contig: each
    record stands in its windows as their kept variant (planner.get_windows)."""
    out: Dict[str, set] = {}
    for w in windows:
        v = getattr(w, "variant", None)
        if v is not None and v.variant_type is VariantType.SNV:
            out.setdefault(v.seq_name, set()).update(range(int(v.pos), int(v.end) + 1))
    return {k: np.fromiter(s, np.int64, len(s)) for k, s in out.items()}


class PairPanel:
    """A panel less one pair's own SNV positions; ``table(ref_names)`` is cached by BAM header."""

    def __init__(self, panel: Panel, windows: Iterable = (), quality: Optional[int] = None, sa_clips: bool = False):
        self.panel = panel
        self.quality = -1 if quality is None else int(quality)
        self.sa_clips = bool(sa_clips)   # --mask_sa_clips: every table carries its header's names and the switch
        own = own_snv_positions(windows)
        self.contigs: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        self.excluded = 0
        for name, (pos, code) in panel.contigs.items():
            if name in own:
                keep = ~np.isin(pos, own[name])
                self.excluded += int(len(pos) - keep.sum())
                pos, code = pos[keep], code[keep]
            self.contigs[name] = (pos, code)
        self._tables: Dict[Tuple[str, ...], SitesTable] = {}

    def table(self, ref_names: Sequence[str]) -> SitesTable:
        key = tuple(ref_names)
        t = self._tables.get(key)
        if t is None:
            off = np.zeros(len(key) + 1, np.int64)
            ps: List[np.ndarray] = []
            cs: List[np.ndarray] = []
            for i, name in enumerate(key):
                p, c = self.contigs.get(name, (None, None))
                if p is not None and key.index(name) == i:   # (a name listed twice: its first sequence)
                    ps.append(p)
                    cs.append(c)
                    off[i + 1] = off[i] + len(p)
                else:
                    off[i + 1] = off[i]
            ignored = [n for n in self.contigs if n not in key]
            log.info("known sites: %d sites on the BAM's %d sequences (%d of the pair's own SNV positions left out), "
                     "%d panel contigs not in the BAM header ignored", int(off[-1]), len(key), self.excluded, len(ignored))
            t = self._tables[key] = SitesTable(off, np.concatenate(ps) if ps else np.zeros(0, np.int32),
                                               np.concatenate(cs) if cs else np.zeros(0, np.uint8), self.quality,
                                               key, self.sa_clips)
        return t


_PANELS: Dict[Tuple[str, str], Panel] = {}


def panel_default(fasta) -> Optional[Panel]:
    """The panel of ``GANON_KNOWN_SITES`` (``--known_sites``), loaded once per process and FASTA; None
    when the variable is unset or empty. Spawned pair workers and ranks inherit the variable and load
    the panel themselves: nothing travels between them."""
    path = os.environ.get(ENV, "")
    if not path:
        return None
    key = (os.path.abspath(path), os.path.abspath(fasta.filename))
    p = _PANELS.get(key)
    if p is None:
        p = _PANELS[key] = load_panel(path, fasta)
    return p


def pair_default(fasta, windows: Iterable) -> Optional[PairPanel]:
    """What the pipelines decode one pair with (None: the option is off): the default panel less the
    pair's own SNVs, rewritten bases at ``GANON_MASKED_BASE_QUALITY`` when that option is on too, soft
    clips masked along their SA alignments with ``GANON_MASK_SA_CLIPS=1``."""
    panel = panel_default(fasta)
    if panel is None:
        return None
    return PairPanel(panel, windows, native.masked_base_quality_default(), mask_sa_clips_default())


def resolve(known_sites, ref_names: Sequence[str]) -> Optional[SitesTable]:
    """A decoder's ``known_sites`` argument — None, a SitesTable or a PairPanel — as a table."""
    if known_sites is None or isinstance(known_sites, SitesTable):
        return known_sites
    return known_sites.table(ref_names)
