"""Command line, same flags as the reference (genome_anonymizer.py:16-112):

  python -m genomeanonymizer_amd.genome_anonymizer -d DIR -s samples.tsv -r ref.fa \\
      [-m complete_germline] [-c CPUS] [--record_statistics] [--enhanced_multiprocessing] [-v N]
      [--compress_output] [--masked_base_quality Q] [--hash_read_names] [--known_sites PANEL.vcf[.gz]]
      [--discover_sites] [--mask_sa_clips]
      [--discover_min_base_quality Q] [--discover_min_mapq M] [--discover_exclude_flags F] [--discover_rule both|normal]

samples.tsv: tumor<TAB>normal<TAB>vcf per line, paths relative to DIR, '#' lines skipped.
Outputs next to the inputs: re.sub('.bam|.sam|.cram', '.anonymized', path) + .1/.2.fastq
(+ .single_end.fastq), and {normal_bam}.statistics.txt with --record_statistics.
--compress_output (an extension: the reference writes plain FASTQ) writes .1/.2/.single_end.fastq.gz
instead, BGZF members deflated on the GPU; GANON_COMPRESS_OUTPUT=1 is the same default.
--masked_base_quality Q (an extension, 0..93; GANON_MASKED_BASE_QUALITY=Q is the same default): every
base a germline SNV mask wrote is printed with quality chr(33 + Q), so that a caller run on the
anonymized FASTQ does not read the synthetic base with the confidence of the one sequenced there.
--hash_read_names (an extension; GANON_HASH_READ_NAMES=1 is the same default): every read name is
replaced, where its record is decoded, by hex(BLAKE2s(name, key=K, digest_size=16)), 32 hex characters
— an Illumina name holds instrument, run, flowcell, lane, tile and x/y. Mates still pair (equal names
hash equally); record order, which records are mates and the /1 and /2 suffixes stay as they are. K
comes from GANON_READ_NAME_KEY (2 to 64 hex digits; there is no key flag: it would show in ps). Without
it 32 random bytes are drawn once per invocation: the names are then unlinkable and the run cannot be
repeated. A supplied key makes runs reproducible and must be kept as secret as the original names.
The key is never logged or written; one key serves every pair of the invocation, tumor and normal.
--known_sites PANEL.vcf[.gz] (an extension; GANON_KNOWN_SITES=path is the same default): a population
panel (dbSNP, gnomAD, a cohort's own). The masking rule rewrites a germline SNV only where a tumor and
a normal read of one pileup scope show it; with a panel, every read base that is aligned (CIGAR M, =, X)
to a listed position and shows a listed one-base ALT allele becomes the reference base where its
record is decoded, in every read that reaches any output, in a scope or not. The run writes exactly
what a run without the option writes on BAMs rewritten that way. Lines with REF one of A, C, G, T and a
one-base ALT are used (the other ALTs of such a line are ignored), lines with a longer REF (indels,
MNVs) are skipped and counted, contigs absent from the BAM header are ignored. REF must be the FASTA's
base: a mismatch, two REFs at one position, a position past the contig's end or an unreadable file end
the run before any output file is opened. The positions of each pair's own VCF SNVs are left out of
the panel for that pair: those calls are what the product keeps. With --masked_base_quality Q the
rewritten bases are printed with quality Q too. Limits: a supplementary record is masked along its own
alignment, the primary's soft-clipped copy of those bases is not (--mask_sa_clips closes this); indels
and MNVs of the panel are not used. Each process logs how many bases it rewrote.
--discover_sites (an extension; --no-discover_sites; GANON_DISCOVER_SITES=1 is the same default): the
panel the pair's own BAMs give. Before a pair's jobs start a pre-pass decodes both BAMs once more and
notes, per reference position, which alleles other than the reference's the tumor reads and the normal
reads show (aligned bases only — CIGAR M, =, X —, A, C, G, T against a reference A, C, G, T; no quality,
depth or strand filter: one tumor read and one normal read are enough, as in the masking rule). Every
position where both show one allele becomes a site with that allele as ALT, and from there on the run is
a --known_sites run with that table: the pair's own VCF SNV positions are left out, every read base at
a site that shows its ALT becomes the reference base where its record is decoded, and with
--masked_base_quality Q its quality becomes Q. With --known_sites as well the two tables are OR-ed. The
run writes exactly what a run without the option writes on BAMs rewritten that way. The discovered list
is the donor's germline SNV list: it is never logged or written, the log gives counts only. Limits:
indels are not discovered; a supplementary record's bases in the primary's soft clip are not masked
(--mask_sa_clips closes this); the pre-pass decodes every record a second time.
--discover_min_base_quality Q (0..93, default 0), --discover_min_mapq M (0..255, default 0),
--discover_exclude_flags F (0..65535, decimal or 0x..., default 0) and --discover_rule both|normal
(default both) refine --discover_sites and are command-line errors without it (environment defaults:
GANON_DISCOVER_MIN_BASE_QUALITY, GANON_DISCOVER_MIN_MAPQ, GANON_DISCOVER_EXCLUDE_FLAGS, GANON_DISCOVER_RULE).
The first three filter the evidence, for tumor and normal alike: a base counts only when its own quality
is at least Q (a record without qualities stores 0xFF and passes), on a record with mapq at least M and
no flag bit of F (1024 duplicates, 512 QC failures, 256 secondary, 2048 supplementary). Rule both is the
intersection above. Under rule normal every allele a normal read shows is a site, whatever the tumor
shows: where the tumor lost a haplotype (loss of heterozygosity) or has no coverage the intersection is
empty and the donor's heterozygous alleles would stay in the normal's FASTQ; the evidence that an allele
is germline is the normal's, and the pair's own SNV positions are left out of the table anyway. Without a
filter every sequencing error of the normal becomes a site under rule normal: give it with Q and M. The
mask itself is not filtered: every base that shows a site's ALT is rewritten, whatever its quality or
its record's mapq. There are no depth, read-count or strand thresholds: the tally keeps OR-ed bits, not
counts, which is what lets records be tallied twice. The log gains the four settings and counts only.
--mask_sa_clips (an extension; --no-mask_sa_clips; GANON_MASK_SA_CLIPS=1 is the same default): with a
table (--known_sites, --discover_sites or both; without one the option is a command-line error) the mask
also follows each record's SA:Z tag. A chimeric read's primary record holds the whole sequence, and the
bases it soft-clips are aligned only in the supplementary record; the written sequence comes from the
primary. For every record with a soft clip, each SA entry rname,pos,strand,CIGAR,mapQ,NM is projected
onto the read as the SAM specification says (reverse-complemented when the entry's strand is not the
record's), and a clipped base that the entry aligns (M, =, X) to a listed position and that shows a
listed ALT becomes the reference base, with --masked_base_quality Q its quality Q. Aligned, inserted and
hard-clipped bases are never touched through SA. An entry is used whole or not at all: six fields, a
header sequence name, pos 1..2^31-1, strand + or -, a well-formed CIGAR whose query length is the full
read's; other entries are ignored and counted. The run writes what a run without the option writes on
BAMs rewritten that way. Limits: secondary alignments carry no clips and are untouched; --discover_sites
still takes its evidence from aligned bases only; a supplementary record whose bases the aligner did not
reverse-complement for its strand is projected as the specification says, not as that file holds them.

Multi-GPU: launch under ``torchrun --nproc-per-node N`` (or set WORLD_SIZE/RANK/LOCAL_RANK):
contigs are sharded round-robin over the ranks; each rank decodes, masks and writes its own
contigs at their offsets of the shared output files (distributed.py, stream.py). More ranks than
GPUs (e.g. 4 per GPU) spread the host work (decode, planning, output) over more processes: rank r
uses GPU LOCAL_RANK % GPUs and the ranks talk over gloo instead of RCCL.
"""
from __future__ import annotations

import logging
import os
import sys
import time
from argparse import ArgumentParser, BooleanOptionalAction
from typing import List, Tuple

from .anonymizer_methods import ANONYMIZER_ALGORITHMS, CompleteGermlineAnonymizer
from .short_read_tumor_normal_anonymizer import name_output, run_short_read_tumor_normal_anonymizer

COMPLETE_GERMLINE_ANONYMIZER_ALGORITHM = "complete_germline"


def exec_parser(argv=None):
    parser = ArgumentParser(prog="GenomeAnonymizer",
                            description="Anonymization of sequencing data by removing germline variation "
                                        "(MI355X build)")
    parser.add_argument("-d", "--directory", type=str, required=True,
                        help="Directory in which the tumor-normal sample pairs and the samples text file are stored")
    parser.add_argument("-s", "--samples", type=str, required=True,
                        help="Text file with the tumor, normal and vcf file names of each sample, tab separated")
    parser.add_argument("-r", "--reference", type=str, required=True,
                        help="reference genome to which the reads are mapped")
    parser.add_argument("-m", "--method", type=str, required=False, default="complete_germline",
                        choices=["complete_germline"],
                        help="anonymization method: complete_germline masks all germline SNVs in the reads")
    parser.add_argument("-c", "--cpu", type=int, required=False, default=1,
                        help="Number of CPUs available (host BAM decode threads)")
    parser.add_argument("--record_statistics", action=BooleanOptionalAction,
                        help="Record statistics about the number of anonymized variants by region and type")
    parser.add_argument("--enhanced_multiprocessing", action=BooleanOptionalAction,
                        help="Accepted for compatibility; no effect (see SURVEY Q12)")
    parser.add_argument("--compress_output", action=BooleanOptionalAction,
                        help="Write BGZF-compressed .fastq.gz files, deflated on the GPU (default: GANON_COMPRESS_OUTPUT)")
    parser.add_argument("--masked_base_quality", type=int, choices=range(0, 94), metavar="Q", default=None,
                        help="Phred quality 0..93 printed under every base a germline SNV mask wrote "
                             "(default: GANON_MASKED_BASE_QUALITY, else the qualities stay as they are)")
    parser.add_argument("--hash_read_names", action=BooleanOptionalAction,
                        help="Replace every read name by its keyed BLAKE2s-128 hash, 32 hex characters (default: "
                             "GANON_HASH_READ_NAMES; key: GANON_READ_NAME_KEY as hex, else random per invocation)")
    parser.add_argument("--known_sites", type=str, metavar="PANEL.vcf[.gz]", default=None,
                        help="Population panel: read bases showing a listed one-base ALT at a listed position "
                             "become the reference base where the record is decoded (default: GANON_KNOWN_SITES)")
    parser.add_argument("--discover_sites", action=BooleanOptionalAction,
                        help="Mask every SNV allele that a tumor read and a normal read of the pair both show, "
                             "genome-wide: a pre-pass over both BAMs builds the pair's own site table (default: "
                             "GANON_DISCOVER_SITES)")
    parser.add_argument("--discover_min_base_quality", type=_int_in("--discover_min_base_quality", 0, 93), metavar="Q",
                        default=None,
                        help="With --discover_sites: a base is evidence only when its own quality is >= Q, 0..93 "
                             "(default: GANON_DISCOVER_MIN_BASE_QUALITY, else 0)")
    parser.add_argument("--discover_min_mapq", type=_int_in("--discover_min_mapq", 0, 255), metavar="M", default=None,
                        help="With --discover_sites: records with mapq < M give no evidence, 0..255 (default: "
                             "GANON_DISCOVER_MIN_MAPQ, else 0)")
    parser.add_argument("--discover_exclude_flags", type=_int_in("--discover_exclude_flags", 0, 65535), metavar="F",
                        default=None,
                        help="With --discover_sites: records with a flag bit of F give no evidence, 0..65535, decimal or "
                             "0x... (default: GANON_DISCOVER_EXCLUDE_FLAGS, else 0)")
    parser.add_argument("--discover_rule", type=str, choices=["both", "normal"], default=None,
                        help="With --discover_sites: both, an allele is a site when a tumor and a normal read show it; "
                             "normal, when a normal read shows it, whatever the tumor shows (default: GANON_DISCOVER_RULE, "
                             "else both). The mask itself is never filtered")
    parser.add_argument("--mask_sa_clips", action=BooleanOptionalAction,
                        help="With --known_sites and / or --discover_sites: mask soft-clipped bases too, along the "
                             "alignments the record's SA tag names (default: GANON_MASK_SA_CLIPS)")
    parser.add_argument("-v", "--verbose", type=int, required=False, default=2, help="Verbosity of logging")
    parser.add_argument("--device", type=int, default=None, help="GPU index (default: LOCAL_RANK or 0)")
    return parser.parse_args(argv)


def _int_in(option: str, lo: int, hi: int):
    """An argparse type: an integer lo..hi, decimal or 0x...."""
    from argparse import ArgumentTypeError

    def parse(text: str) -> int:
        try:
            v = int(text, 16) if text.strip().lower().startswith("0x") else int(text, 10)
        except ValueError:
            raise ArgumentTypeError(f"{option}: not a number: {text!r}") from None
        if not lo <= v <= hi:
            raise ArgumentTypeError(f"{option} is {lo}..{hi}, not {v}")
        return v
    parse.__name__ = "int"
    return parse


def join_dir_file(directory: str, param: str) -> str:
    return "".join((directory, "/", param)) if not directory.endswith("/") else "".join((directory, param))


def read_samples(path_to_samples: str, directory: str):
    samples: List[Tuple[str, str]] = []
    outputs: List[Tuple[str, str]] = []
    vcfs: List[str] = []
    with open(path_to_samples) as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            f = line.strip().split("\t")
            t, n, v = (join_dir_file(directory, x) for x in f[:3])
            samples.append((t, n))
            vcfs.append(v)
            outputs.append((name_output(t), name_output(n)))
    return vcfs, samples, outputs


def run_anonymizer(argv=None) -> None:
    config = exec_parser(argv)
    logging.basicConfig(level=config.verbose * 10)
    t0 = time.time()
    logging.info("Beginning execution of GenomeAnonymizer (MI355X build)")
    if config.method not in ANONYMIZER_ALGORITHMS:
        logging.error("Anonymizer algorithm %s is not a valid option", config.method)
        sys.exit(1)
    if config.compress_output is not None:   # (the environment reaches spawned pair workers and every rank's paths)
        os.environ["GANON_COMPRESS_OUTPUT"] = "1" if config.compress_output else "0"
    if config.masked_base_quality is not None:
        os.environ["GANON_MASKED_BASE_QUALITY"] = str(config.masked_base_quality)
    if config.hash_read_names is not None:
        os.environ["GANON_HASH_READ_NAMES"] = "1" if config.hash_read_names else "0"
    if config.known_sites is not None:
        os.environ["GANON_KNOWN_SITES"] = config.known_sites
    if config.discover_sites is not None:
        os.environ["GANON_DISCOVER_SITES"] = "1" if config.discover_sites else "0"
    if config.mask_sa_clips is not None:
        os.environ["GANON_MASK_SA_CLIPS"] = "1" if config.mask_sa_clips else "0"
    if (os.environ.get("GANON_MASK_SA_CLIPS", "0") == "1" and not os.environ.get("GANON_KNOWN_SITES")
            and os.environ.get("GANON_DISCOVER_SITES", "0") != "1"):   # (before any file is opened)
        logging.error("--mask_sa_clips needs a site table: give --known_sites PANEL.vcf[.gz], --discover_sites or both")
        sys.exit(1)
    for value, env in ((config.discover_min_base_quality, "GANON_DISCOVER_MIN_BASE_QUALITY"),
                       (config.discover_min_mapq, "GANON_DISCOVER_MIN_MAPQ"),
                       (config.discover_exclude_flags, "GANON_DISCOVER_EXCLUDE_FLAGS"),
                       (config.discover_rule, "GANON_DISCOVER_RULE")):
        if value is not None:
            os.environ[env] = str(value)
    from . import discover_sites
    try:   # (before any file is opened: a value out of range, or a filter or rule with nothing to refine)
        rule = discover_sites.rule_default()
    except ValueError as e:
        logging.error("%s", e)
        sys.exit(1)
    given = [o for o, v in (("--discover_min_base_quality", config.discover_min_base_quality),
                            ("--discover_min_mapq", config.discover_min_mapq),
                            ("--discover_exclude_flags", config.discover_exclude_flags),
                            ("--discover_rule", config.discover_rule)) if v is not None]
    if not discover_sites.default_on() and (given or rule != discover_sites.SiteRule()):
        logging.error("%s needs --discover_sites: the evidence filters and the rule refine the pair's own site table",
                      ", ".join(given) if given else "a GANON_DISCOVER_* filter or rule default")
        sys.exit(1)
    from . import native
    try:   # (a malformed key ends the run here, before any file is opened)
        if os.environ.get("GANON_HASH_READ_NAMES", "0") == "1" and native.NAME_KEY_ENV in os.environ:
            native.parse_name_key(os.environ[native.NAME_KEY_ENV])
    except native.GanonError as e:
        logging.error("%s", e)
        sys.exit(1)
    vcfs, samples, outputs = read_samples(join_dir_file(config.directory, config.samples), config.directory)
    if os.environ.get("GANON_KNOWN_SITES"):   # (a panel that cannot be used ends the run here, too)
        from .io.fasta import FastaRef
        from .known_sites import panel_default
        try:
            panel_default(FastaRef(config.reference))
        except native.GanonError as e:
            logging.error("%s", e)
            sys.exit(1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    # launched by torchrun (any world size, one included): the process-group path
    launched = world > 1 or ("RANK" in os.environ and "MASTER_ADDR" in os.environ)
    n_dev = 1
    if launched:
        import torch
        n_dev = max(1, torch.cuda.device_count())   # (counting devices does not initialise the GPU)
    device = config.device if config.device is not None else local % n_dev
    anonymizer = CompleteGermlineAnonymizer(device=device)
    if launched:
        import torch.distributed as dist
        from .distributed import run_pairs_sharded
        if local_world > n_dev:   # ranks share a GPU: RCCL takes one rank per device
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(device)
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        logging.info("rank %d of %d: process group backend %s", dist.get_rank(), dist.get_world_size(),
                     dist.get_backend())
        native.share_read_name_key(dist)   # rank 0's key on every rank, before any rank opens a reader
        # one pair per GPU when there are enough pairs, else each pair's contigs over all GPUs
        tots = run_pairs_sharded(vcfs, samples, config.reference, anonymizer, outputs, bool(config.record_statistics),
                                 dist, threads=max(1, config.cpu))
        logging.info("rank %d totals %s", dist.get_rank(), tots)
        from .distributed import release_side_groups
        release_side_groups(dist)
        dist.destroy_process_group()
    else:
        native.share_read_name_key(draw=True)   # (in the environment: spawned pair workers inherit it)
        run_short_read_tumor_normal_anonymizer(vcfs, samples, config.reference, anonymizer, outputs,
                                               bool(config.record_statistics), config.cpu,
                                               bool(config.enhanced_multiprocessing))
    logging.info("Finished execution of GenomeAnonymizer successfully")
    logging.debug("Total execution time: %s s", time.time() - t0)


if __name__ == "__main__":
    run_anonymizer()
