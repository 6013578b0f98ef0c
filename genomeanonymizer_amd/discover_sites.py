"""--discover_sites: mask the SNV alleles both samples of a pair show, wherever they lie.

The masking rule overwrites a germline SNV only when a tumor and a normal read of one pileup scope
show it, and the scopes are the windows around the pair's somatic calls; ``--known_sites`` needs a panel,
which does not list the donor's private variants. The evidence that needs no panel is in the inputs: an
allele other than the reference's that a tumor read and a normal read both show at one position is
germline by the rule itself. Before a pair's jobs start, a pre-pass decodes both BAMs once more with no
table and no name key and tallies, per reference position, the alleles each dataset shows
(csrc/ganon_site_tally.h: on the host in ``records_to_columns``, on the device in ``k_bam_site_tally``);
the positions where the two sets intersect become a ``known_sites.Panel``, and everything after that is
``--known_sites``: the pair's own SNV calls are left out, the readers mask where they decode.

Evidence filters and the rule (``SiteRule``; the four options below need ``--discover_sites``):

* ``--discover_min_base_quality Q`` (0..93): a base is evidence only when its own quality byte is >= Q;
  a record that stores no qualities has 0xFF everywhere and passes.
* ``--discover_min_mapq M`` (0..255) and ``--discover_exclude_flags F`` (0..65535, decimal or 0x...): a
  record with mapq < M, or with a flag bit of F, gives no evidence.
* ``--discover_rule both|normal``: ``both`` is the intersection above. Under ``normal`` an allele a
  normal read shows is a site whatever the tumor shows: where the tumor lost a haplotype (loss of
  heterozygosity, tens of megabases in many tumors) or has a coverage gap, the intersection is empty and
  the donor's heterozygous alleles would reach the normal's FASTQ. The evidence that an allele is germline
  is the normal's; the pair's own SNV calls, which the product keeps, are left out of the table anyway.
  Every sequencing error of the normal is a site under ``normal``: use it with the filters.

The filters apply to both datasets alike and decide which bases are evidence, nothing else: the mask
itself is not filtered and rewrites every base that shows a site's ALT, whatever its quality or its
record's mapq (§4i). All four have environment defaults (``GANON_DISCOVER_MIN_BASE_QUALITY``,
``GANON_DISCOVER_MIN_MAPQ``, ``GANON_DISCOVER_EXCLUDE_FLAGS``, ``GANON_DISCOVER_RULE``), read once per pair.

* ``discover(tumor_bam, normal_bam, fasta, ...)`` is the pre-pass; with several ranks each takes the
  sequences ``i % world`` and the lists are exchanged over a side gloo group.
* ``merge(a, b)`` ORs two panels position by position.
* ``pair_default(...)`` is what the pipelines call: the ``PairPanel`` of ``--known_sites`` and / or
  ``--discover_sites``, None when both are off.

The discovered list is the donor's germline SNV list: it is never logged and never written; the log
lines give counts only.

Limits: indels are not discovered; base-quality, mapq and flag filters exist, depth, read-count, VAF and
strand thresholds do not (one passing base per dataset is enough): the tally is a byte of OR-ed bits per
position, which is what makes records tallied twice — shared by two region reads, by a window decoded
again, by the host and the device half — harmless, and a count would not be; a supplementary record's
bases in the primary's soft clip are not masked (§4i); ``reference_adapter`` does not use it; the
pre-pass decodes every record a second time.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .known_sites import PairPanel, Panel, mask_sa_clips_default, panel_default

log = logging.getLogger("genomeanonymizer_amd")

ENV = "GANON_DISCOVER_SITES"
MIN_BASE_QUALITY_ENV = "GANON_DISCOVER_MIN_BASE_QUALITY"
MIN_MAPQ_ENV = "GANON_DISCOVER_MIN_MAPQ"
EXCLUDE_FLAGS_ENV = "GANON_DISCOVER_EXCLUDE_FLAGS"
RULE_ENV = "GANON_DISCOVER_RULE"
RULE_ENVS = (MIN_BASE_QUALITY_ENV, MIN_MAPQ_ENV, EXCLUDE_FLAGS_ENV, RULE_ENV)
SiteRule = native.SiteRule
REGION_ENV = "GANON_DISCOVER_BP"    # bases per region read of the pre-pass on indexed BAMs (default 8 Mb)


def default_on() -> bool:
    """``GANON_DISCOVER_SITES=1`` (``--discover_sites``), for library callers and for spawned pair workers
    and ranks."""
    return os.environ.get(ENV, "0") == "1"


def parse_flags(text: str) -> int:
    """``--discover_exclude_flags``: decimal or ``0x...``."""
    t = str(text).strip()
    return int(t, 16) if t.lower().startswith("0x") else int(t, 10)


def rule_default() -> SiteRule:
    """The rule of the four environment defaults (``--discover_min_base_quality``, ``--discover_min_mapq``,
    ``--discover_exclude_flags``, ``--discover_rule``), checked; ValueError names the option at fault."""
    def num(env, option, parse=int):
        v = os.environ.get(env, "") or "0"
        try:
            return parse(v)
        except ValueError:
            raise ValueError(f"{option} ({env}): not a number: {v!r}") from None
    return SiteRule(num(MIN_BASE_QUALITY_ENV, "--discover_min_base_quality"), num(MIN_MAPQ_ENV, "--discover_min_mapq"),
                    num(EXCLUDE_FLAGS_ENV, "--discover_exclude_flags", parse_flags),
                    os.environ.get(RULE_ENV, "") or "both").checked()


class HostTally:
    """The host library's evidence tally (``ganon_site_tally``, include/ganon_host.h) over named
    sequences of a packed nt16 genome: ``names[i]`` has ``lengths[i]`` bases from nibble ``nib_off[i]`` of
    ``packed`` on (-1: no reference). Readers take it with a dataset (0 tumor, 1 normal):
    ``BamReader.set_site_tally``, ``ReadTable(site_tally=)``. ``rule``: a SiteRule the readers and
    ``finish`` read from the tally (None: no filter, mode "both")."""

    def __init__(self, names: Sequence[str], packed: np.ndarray, nib_off: Sequence[int], lengths: Sequence[int],
                 rule: Optional[SiteRule] = None):
        self.names = list(names)
        self.index = {}
        for i, n in enumerate(self.names):
            self.index.setdefault(n, i)
        self.packed = np.ascontiguousarray(packed, np.uint8)    # (kept: the library reads it)
        self.nib_off = np.ascontiguousarray(nib_off, np.int64)
        self.lengths = np.ascontiguousarray(lengths, np.int64)
        lib = native.host_lib()
        h = C.c_void_p()
        self.rule = (rule or SiteRule()).checked()
        if lib.ganon_site_tally_create_ex(len(self.names), native._ptr(self.packed, native._u8p),
                                          native._ptr(self.nib_off, native._i64p), native._ptr(self.lengths, native._i64p),
                                          *self.rule.c_args(), C.byref(h)) != 0:
            raise native.GanonError(lib.ganon_host_last_error().decode())
        self._h = h

    @classmethod
    def of_fasta(cls, fasta, rule: Optional[SiteRule] = None) -> "HostTally":
        packed, off = fasta.packed()
        names = list(fasta.references)
        return cls(names, packed, [off[n] for n in names], list(fasta.lengths), rule)

    @property
    def handle(self):
        return self._h

    def seq_of_tid(self, ref_names: Sequence[str]) -> np.ndarray:
        """The tally's sequence of each BAM sequence id (-1: none; a name listed twice: its first id)."""
        out = np.full(len(ref_names), -1, np.int32)
        seen = set()
        for t, n in enumerate(ref_names):
            if n not in seen:
                seen.add(n)
                out[t] = self.index.get(n, -1)
        return out

    def reference_of(self, seq: int) -> np.ndarray:
        """The packed bases of one sequence (a sequence starts on a byte)."""
        o, L = int(self.nib_off[seq]), int(self.lengths[seq])
        if o < 0 or o & 1:
            raise native.GanonError("HostTally.reference_of: a sequence without a reference or off a byte boundary")
        return self.packed[o // 2:o // 2 + (L + 1) // 2]

    def bytes_address(self, seq: int) -> Optional[int]:
        """The address of a sequence's tally bytes (None: no evidence arrived)."""
        return native.host_lib().ganon_site_tally_bytes(self._h, int(seq)) or None

    def touched(self, seq: int) -> bool:
        return self.bytes_address(seq) is not None

    def release(self, seq: int) -> None:
        native.host_lib().ganon_site_tally_release(self._h, int(seq))

    def finish(self, seq: int) -> Tuple[np.ndarray, np.ndarray]:
        """(positions int32, codes uint8) of a sequence's sites, in position order; its bytes are freed."""
        lib = native.host_lib()
        n = int(lib.ganon_site_tally_count(self._h, int(seq)))
        if n < 0:
            raise native.GanonError("no such sequence in the site tally")
        pos, code = np.empty(n, np.int32), np.empty(n, np.uint8)
        got = int(lib.ganon_site_tally_finish(self._h, int(seq), native._ptr(pos, native._i32p),
                                              native._ptr(code, native._u8p), n))
        if got != n:
            raise native.GanonError(lib.ganon_host_last_error().decode())
        return pos, code

    def close(self) -> None:
        if self._h:
            native.host_lib().ganon_site_tally_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def merge(a: Optional[Panel], b: Optional[Panel]) -> Optional[Panel]:
    """The OR of two panels position by position (REF is the FASTA's base in both, so the codes of one
    position agree in their high nibble)."""
    if a is None or b is None:
        return a if b is None else b
    contigs: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
    for name in list(a.contigs) + [n for n in b.contigs if n not in a.contigs]:
        pa, ca = a.contigs.get(name, (np.zeros(0, np.int32), np.zeros(0, np.uint8)))
        pb, cb = b.contigs.get(name, (np.zeros(0, np.int32), np.zeros(0, np.uint8)))
        pos = np.union1d(pa, pb).astype(np.int32)
        code = np.zeros(len(pos), np.uint8)
        code[np.searchsorted(pos, pa)] |= ca
        code[np.searchsorted(pos, pb)] |= cb
        contigs[name] = (pos, code)
    return Panel(a.path, contigs, dict(a.stats, merged_sites=sum(len(p) for p, _ in contigs.values())))


def _pass_one(reader, tid: int, region_bp: int) -> None:
    """Decode every record of one BAM sequence (the tables are dropped: the tally is the result).
    Indexed files go region by region — the reads a GPU inflater's region decoder takes; a record two
    regions share is tallied twice, which the OR does not see."""
    if reader.has_index and region_bp > 0:
        L = max(1, int(reader.ref_lens[tid]))
        for a in range(0, L, region_bp):
            reader.region(tid, a, min(L, a + region_bp))
    else:
        reader.contig(tid)


def discover(tumor_bam: str, normal_bam: str, fasta, threads: int = 8, inflater=None, dist=None,
             window_bytes: int = 0, stats: Optional[dict] = None, rule: Optional[SiteRule] = None) -> Panel:
    """The pre-pass: the positions where a tumor read and a normal read show one allele other than the
    reference's — under ``rule`` (None: the environment defaults, ``rule_default``) with its evidence
    filters, and with mode "normal" the positions where a normal read shows one —, as a Panel (contig
    name -> sorted positions, codes ref_nt16 << 4 | alt). ``inflater``: a
    native.GpuInflater whose context inflates and, in region reads, decodes and tallies on the device
    (None: the host decoder). ``dist``: the initialised torch.distributed world; every rank returns the
    same Panel."""
    from .io.bam import BamReader
    t0 = time.time()
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    region_bp = int(os.environ.get(REGION_ENV, "8000000") or 0)
    rule = (rule_default() if rule is None else rule).checked()
    tally = HostTally.of_fasta(fasta, rule)
    readers = [BamReader(p, threads, window_bytes, inflater=inflater) for p in (tumor_bam, normal_bam)]
    on_device = inflater is not None and hasattr(inflater, "set_site_tally")
    contigs: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
    try:
        for d, r in enumerate(readers):
            r.set_site_tally(tally, d)
        maps = [tally.seq_of_tid(r.ref_names) for r in readers]
        for i, name in enumerate(tally.names):
            if i % world != rank or int(tally.lengths[i]) == 0 or tally.index[name] != i:
                continue
            tids = [int(np.nonzero(m == i)[0][0]) if (m == i).any() else -1 for m in maps]
            if max(tids) < 0:
                continue
            dt = native.DeviceTally(inflater, tally.reference_of(i), int(tally.lengths[i]), rule) if on_device else None
            try:
                for d, r in enumerate(readers):
                    if tids[d] < 0:
                        continue
                    if dt is not None:
                        inflater.set_site_tally(dt, d, tids[d])
                    _pass_one(r, tids[d], region_bp)
                if dt is not None:
                    # (host decodes happen with an inflater too — windows under its block minimum —: the
                    # two sides are OR-ed on the device before the intersection)
                    pos, code = dt.finish(tally.bytes_address(i))
                    dt = None
                    tally.release(i)
                else:
                    pos, code = tally.finish(i)
            finally:
                if dt is not None:
                    dt.close()
            if len(pos):
                contigs[name] = (pos, code)
    finally:
        if on_device:
            inflater.set_site_tally(None)
        for r in readers:
            r.close()
        tally.close()
    if world > 1:
        from .distributed import return_side_group, take_side_group
        group = take_side_group(dist, "discover")
        parts: List[Optional[dict]] = [None] * world
        dist.all_gather_object(parts, contigs, group=group)   # (between the ranks of this run only)
        return_side_group(dist, "discover", group, True)
        contigs = {}
        for part in parts:
            contigs.update(part)
        contigs = {n: contigs[n] for n in tally.names if n in contigs}
    out = {"sites": sum(len(p) for p, _ in contigs.values()), "prepass_s": round(time.time() - t0, 3)}
    if stats is not None:
        stats.update(out)
    log.info("discovered sites: %d positions where %s one allele (min base quality %d, min mapq %d, excluded flags 0x%x, "
             "rule %s), pre-pass %.3f s", out["sites"],
             "normal reads show" if rule.mode == "normal" else "tumor and normal reads show", rule.min_base_quality,
             rule.min_mapq, rule.exclude_flags, rule.mode, out["prepass_s"])
    return Panel("<discovered>", contigs, out)


def prepass_inflater(anonymizer, paths: Sequence[str]):
    """The GPU inflater the pre-pass decodes with, chosen as the streamed path chooses its readers'
    (GANON_GPU_INFLATE, GANON_GPU_INFLATE_MIN; the first sample's, kept for the run that follows), or
    None: the host decoder."""
    if anonymizer is None:
        return None
    gi = os.environ.get("GANON_GPU_INFLATE", "auto")
    min_blocks = int(os.environ.get("GANON_GPU_INFLATE_MIN", "512"))
    gpu_engine = anonymizer._engine is None or isinstance(anonymizer._engine, native.HipMasker)
    big = max(os.path.getsize(p) for p in paths) >= 2 * min_blocks * 36_000
    if not (gi == "1" or (gi == "auto" and gpu_engine and big)):
        return None
    from .stream import _INFLATERS
    key = (anonymizer.device, min_blocks, 0)
    if key not in _INFLATERS:
        _INFLATERS[key] = native.GpuInflater(anonymizer.device, min_blocks)
    return _INFLATERS[key]


def pair_default(fasta, windows, tumor_bam: str, normal_bam: str, threads: int = 8, anonymizer=None, dist=None,
                 window_bytes: int = 0, timing: Optional[dict] = None) -> Optional[PairPanel]:
    """What the pipelines decode one pair with (None: both options off): the panel of ``--known_sites``
    OR-ed with the sites ``--discover_sites`` finds in the pair's own BAMs, less the pair's own SNVs,
    rewritten bases at ``GANON_MASKED_BASE_QUALITY`` when that option is on too, soft clips masked along
    their SA alignments with ``GANON_MASK_SA_CLIPS=1``."""
    panel = panel_default(fasta)
    if default_on():
        stats: dict = {}
        found = discover(tumor_bam, normal_bam, fasta, threads, prepass_inflater(anonymizer, (tumor_bam, normal_bam)),
                         dist, window_bytes, stats)
        if timing is not None:
            timing["discover_sites"] = stats["sites"]
            timing["discover_prepass_s"] = stats["prepass_s"]
        panel = merge(panel, found)
    if panel is None:
        return None
    return PairPanel(panel, windows, native.masked_base_quality_default(), mask_sa_clips_default())
