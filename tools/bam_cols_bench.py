"""Device BAM record walk (ganon_bam_columns) against the host decoder on one large stream.

The stream: the records of a generated configs[0] BAM tiled to about --mb MB of inflated records
(150 bp paired reads, ~265 bytes a record). The device side is timed per kernel with HIP events
(ganon_last_kernel_times: k_bam_guess, k_bam_check, k_bam_fix, k_bam_offsets, k_bam_sizes, the
five scans, k_bam_scatter) with the stream already in device memory; the host side is
libganon_host.so's ganon_bam_open on the same records written as stored (level-0) BGZF blocks, so
that its inflate is a copy and the time is mostly the record walk's (one thread and --threads
threads; the file read included). Every device column must equal the host decoder's. Prints one
JSON line (bench.py's `bam_decode` side line runs this as a child).

--hash_names: the same with a read-name key on both sides (--hash_read_names: GANON_READ_NAME_KEY as
hex, else a fixed benchmark key): k_bam_name_hash joins the kernel list, the names block is 33 bytes a
record, and the host decoder hashes inside its column pass.

--known_sites SITES_PER_KB: the same with a synthetic panel on both sides (--known_sites: that many random
positions per 1,000 bases of each sequence, REF the FASTA's base, one random ALT): k_bam_known_mask joins
the kernel list, the host decoder masks inside its column pass, and the line reports the sites and the
bases rewritten.

--sa_clips FRAC (with --known_sites): a share FRAC of the one-op mapped records gets a trailing soft clip
(the last third of the read) and an SA:Z entry that aligns the clip at a random position of the record's
own sequence, and the table carries the header's names and the switch of --mask_sa_clips on both sides:
k_bam_sa_clips joins the kernel list after k_bam_known_mask, and the line reports the clipped records, the
clip bases rewritten and the entries ignored on both sides.

--site_tally: the same with an evidence tally on both sides (--discover_sites): a device tally of the
sequence most records lie on, as the tumor dataset — k_bam_site_tally joins the kernel list —, the host
decoder tallying inside its column pass; the line reports the positions with evidence on both sides (they
must agree), k_site_compact over that sequence and over a synthetic 20 Mb sequence whose bytes come up
from the host (one position in a thousand a site), under both modes of --discover_rule.

--min_base_quality Q, --min_mapq M, --exclude_flags F, --rule both|normal (with --site_tally): the tally on
both sides carries that rule (--discover_min_base_quality, --discover_min_mapq, --discover_exclude_flags,
--discover_rule). With an evidence filter set k_bam_site_tally runs as its filtered instantiation, and the
records are given mapqs 0, 20, 40 and 60 in equal shares and the duplicate flag on one in twenty (the
generator's base qualities are uniform in 2..40 already), so that every filter passes and drops records;
without one the stream is the plain one, and the kernel is the one a tally without a rule runs.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLS = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len", "aux_len",
        "name_off", "cig_off", "seq_off", "qual_off", "aux_off")
BLOBS = ("names_blob", "cigar", "seq", "qual", "aux")
HBM_PEAK_GBPS = 8000.0


BENCH_KEY = bytes(range(32))


def synthetic_panel(ref_path: str, ref_names, per_kb: float, seed: int = 1):
    """A known_sites.SitesTable of about ``per_kb`` sites per 1,000 bases of each BAM sequence."""
    from genomeanonymizer_amd.io.fasta import FastaRef
    from genomeanonymizer_amd.known_sites import SitesTable
    fa = FastaRef(ref_path)
    rng = np.random.default_rng(seed)
    lut = np.zeros(256, np.uint8)
    for c, v in zip(b"ACGTacgt", (1, 2, 4, 8) * 2):
        lut[c] = v
    off, pos, code = [0], [], []
    for name in ref_names:
        seq = np.frombuffer(fa.raw(name), np.uint8)
        p = np.unique(rng.integers(0, len(seq), int(len(seq) * per_kb / 1000)))
        ref = lut[seq[p]]
        p, ref = p[ref != 0], ref[ref != 0]
        alt = np.uint8(1) << rng.integers(0, 4, len(p)).astype(np.uint8)
        alt = np.where(alt == ref, np.where(ref == 8, 1, ref << 1), alt).astype(np.uint8)
        pos.append(p.astype(np.int32))
        code.append(((ref << 4) | alt).astype(np.uint8))
        off.append(off[-1] + len(p))
    return SitesTable(np.array(off, np.int64), np.concatenate(pos), np.concatenate(code))


def with_sa_clips(recs: bytes, frac: float, ref_names, ref_lens, seed: int = 3):
    """``recs`` (BAM records back to back) with a share ``frac`` of the mapped records whose CIGAR is one M op
    rewritten to kM(L-k)S, k = 2L/3, and given an SA:Z entry (L-k bases at a random position of the record's
    own sequence, same strand). Returns (the new records, how many were rewritten)."""
    import struct
    rng = np.random.default_rng(seed)
    out, p, n, changed = [], 0, len(recs), 0
    while p < n:
        bs = struct.unpack_from("<i", recs, p)[0]
        r = recs[p + 4:p + 4 + bs]
        p += 4 + bs
        tid, _, l_rn, _, _, ncig, flag, lseq = struct.unpack_from("<iiBBHHHi", r, 0)
        if ncig == 1 and not (flag & 4) and 0 <= tid < len(ref_names) and lseq >= 3 and rng.random() < frac:
            w = struct.unpack_from("<I", r, 32 + l_rn)[0]
            if (w & 15) == 0 and (w >> 4) == lseq:
                k = 2 * lseq // 3
                at = int(rng.integers(1, max(2, int(ref_lens[tid]) - lseq)))
                sa = f"SAZ{ref_names[tid]},{at},{'-' if flag & 16 else '+'},{k}S{lseq - k}M,60,0;".encode() + b"\x00"
                cig = struct.pack("<II", k << 4, ((lseq - k) << 4) | 4)
                r = r[:12] + struct.pack("<H", 2) + r[14:32 + l_rn] + cig + r[36 + l_rn:] + sa
                changed += 1
        out.append(struct.pack("<i", len(r)) + r)
    return b"".join(out), changed


def with_mapqs_and_duplicates(recs: bytes, seed: int = 5) -> bytes:
    """``recs`` (BAM records back to back) with mapq 0, 20, 40 or 60 at random and flag 0x400 on one record in
    twenty."""
    import struct
    rng = np.random.default_rng(seed)
    out, p, n = bytearray(recs), 0, len(recs)
    while p < n:
        bs = struct.unpack_from("<i", out, p)[0]
        out[p + 4 + 9] = int(rng.integers(0, 4)) * 20
        if rng.random() < 0.05:
            struct.pack_into("<H", out, p + 4 + 14, struct.unpack_from("<H", out, p + 4 + 14)[0] | 0x400)
        p += 4 + bs
    return bytes(out)


def compact_20mb(g, n: int = 20_000_000, seed: int = 2, mode: str = "both") -> dict:
    """k_site_compact on a synthetic ``n``-base sequence: the evidence bytes uploaded as a host tally's."""
    from genomeanonymizer_amd import native
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, n).astype(np.uint8)
    packed = ((np.uint8(1) << ref[0::2]) << 4 | (np.uint8(1) << ref[1::2])).astype(np.uint8)
    host = np.zeros(n, np.uint8)
    at = rng.choice(n, n // 1000, replace=False)
    alt = (np.uint8(1) << ((ref[at] + 1) % 4)).astype(np.uint8)
    host[at] = alt | (alt << 4)
    host[rng.choice(n, n // 100, replace=False)] |= 0x10      # evidence on one side alone
    dt = native.DeviceTally(g, packed, n, native.SiteRule(mode=mode))
    pos, code = dt.finish(host.ctypes.data)
    per: dict = {}
    for k, v in g.kernel_times():
        per[k] = per.get(k, 0.0) + v
    alt = ((host if mode == "both" else 15) & (host >> 4) & 15).astype(np.uint8)
    exp = np.nonzero(alt)[0]
    return {"bases": n, "rule": mode, "sites": int(len(pos)), "kernels_ms": {k: round(v, 3) for k, v in per.items()},
            "equals_numpy": bool(np.array_equal(pos, exp) and np.array_equal(code & 15, alt[exp])
                                 and np.array_equal(code >> 4, np.uint8(1) << ref[exp]))}


def measure(mb: int = 256, threads: int = 16, reps: int = 3, name_key: bytes = None, sites_per_kb: float = 0.0,
            site_tally: bool = False, sa_clips: float = 0.0, rule=None) -> dict:
    import gzip
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import first_record_offset, write_bgzf
    from genomeanonymizer_amd.synth.generate import generate, scenario
    tmp = tempfile.mkdtemp(prefix="bamcols_")
    try:
        paths = generate(scenario("config1"), os.path.join(tmp, "in"))
        d = gzip.decompress(open(paths["T"], "rb").read())
        p = first_record_offset(d)
        head, recs = d[:p], d[p:]
        n_clipped = 0
        if sa_clips > 0:
            if sites_per_kb <= 0:
                raise SystemExit("--sa_clips needs a panel: give --known_sites SITES_PER_KB too")
            from genomeanonymizer_amd.io.bam import BamReader
            hdr = BamReader(paths["T"], 1)
            recs, n_clipped = with_sa_clips(recs, sa_clips, hdr.ref_names, hdr.ref_lens)
            hdr.close()
        if site_tally and rule is not None and rule.filtered:
            recs = with_mapqs_and_duplicates(recs)
        tiles = max(1, (mb << 20) // max(1, len(recs)))
        stream = np.frombuffer(head + recs * tiles, np.uint8)
        g = native.GpuInflater(0, min_blocks=1)
        lib = native.hip_lib()
        g.set_profiling(True)
        g.set_name_key(name_key)
        table = None
        if sites_per_kb > 0:
            from genomeanonymizer_amd.io.bam import BamReader
            hdr = BamReader(paths["T"], 1)
            table = synthetic_panel(paths["ref"], hdr.ref_names, sites_per_kb)
            if sa_clips > 0:
                from genomeanonymizer_amd.known_sites import SitesTable
                table = SitesTable(table.site_off, table.site_pos, table.site_code, table.quality, hdr.ref_names, True)
            hdr.close()
        g.set_known_sites(table)
        tally = dtally = None
        tally_tid = -1
        if site_tally:
            from genomeanonymizer_amd.discover_sites import HostTally
            from genomeanonymizer_amd.io.bam import BamReader
            from genomeanonymizer_amd.io.fasta import FastaRef
            hdr = BamReader(paths["T"], 1)
            tally = HostTally.of_fasta(FastaRef(paths["ref"]), rule)
            seq_of = tally.seq_of_tid(hdr.ref_names)
            hdr.close()
            tally_tid = int(np.frombuffer(recs[4:8], np.int32)[0])   # (the first record's sequence)
            seq = int(seq_of[tally_tid])
            dtally = native.DeviceTally(g, tally.reference_of(seq), int(tally.lengths[seq]), rule)
            g.set_site_tally(dtally, 0, tally_tid)
        runs = []
        cols, _ = native.bam_columns_device(g.handle, stream, p, len(stream), on_host=True)   # (warm: blocks cached)
        for _ in range(reps):
            t0 = time.perf_counter()
            cols, fixes = native.bam_columns_device(g.handle, stream, p, len(stream), on_host=True)
            wall = time.perf_counter() - t0
            arr = (native.KernelTime * 32)()
            k = lib.ganon_last_kernel_times(g.handle, arr, 32)
            per = {}
            for i in range(min(k, 32)):
                name = arr[i].name.decode()
                per[name] = per.get(name, 0.0) + float(arr[i].ms)
            runs.append((sum(per.values()), per, wall, fixes))
        dev_masked = g.known_sites_masked() // (reps + 1) if table is not None else 0
        dev_sa = [c // (reps + 1) for c in g.sa_clips_counts()] if sa_clips > 0 else [0, 0]
        tally_out = None
        if site_tally:
            # the tumor evidence again as the normal dataset: every position with evidence is a site
            g.set_site_tally(dtally, 1, tally_tid)
            native.bam_columns_device(g.handle, stream, p, len(stream), on_host=True)
            dpos, dcode = dtally.finish()
            per_c: dict = {}
            for k, v in g.kernel_times():
                per_c[k] = per_c.get(k, 0.0) + v
            tally_out = {"tid": tally_tid, "sequence_bases": int(tally.lengths[seq]), "positions_with_evidence_device": int(len(dpos)),
                         "rule": None if rule is None else dict(rule._asdict()),
                         "compact_kernels_ms": {k: round(v, 3) for k, v in per_c.items()}, "compact_20Mb": compact_20mb(g),
                         "compact_20Mb_normal": compact_20mb(g, mode="normal")}
        g.close()
        best = min(runs, key=lambda x: x[0])
        nr = len(cols["pos"])
        path = os.path.join(tmp, "big0.bam")
        write_bgzf(path, stream.tobytes(), level=0)
        host = {}
        t = None
        for th in (1, threads):
            t0 = time.perf_counter()
            t = ReadTable(path, threads=th, name_key=name_key, known_sites=table,
                          site_tally=(tally, 0) if site_tally else None)
            host[th] = time.perf_counter() - t0
        if site_tally:
            ReadTable(path, threads=threads, site_tally=(tally, 1))
            hpos, hcode = tally.finish(seq)
            tally_out["positions_with_evidence_host"] = int(len(hpos))
            tally_out["device_equals_host"] = bool(np.array_equal(hpos, dpos) and np.array_equal(hcode, dcode))
        equal = len(cols["pos"]) == t.n and all(np.array_equal(cols[f], getattr(t, f)) for f in COLS + BLOBS)
        out_bytes = sum(cols[f].nbytes for f in COLS + BLOBS) + cols["rec_off"].nbytes
        alg = (len(stream) - p) + out_bytes   # the records read once, the columns written once
        ms = best[0]
        return {
            "metric": "BAM records decoded to columns per second (device record walk)", "unit": "records/s",
            "value": round(nr / (ms / 1e3), 1), "records": nr, "stream_MB": round(len(stream) / 2**20, 1),
            "device_ms": round(ms, 3), "device_kernels_ms": {k: round(v, 3) for k, v in best[1].items()},
            "roofline": {"bound": "hbm", "achieved": round(alg / (ms / 1e3) / 1e9, 1), "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": round(alg / (ms / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                         "algorithmic_bytes": int(alg), "traffic": None},
            "device_call_wall_s": round(best[2], 3), "guess_fixes": best[3],
            "host_decoder_s": {str(k): round(v, 3) for k, v in host.items()},
            "host_records_per_s": {str(k): round(nr / v, 1) for k, v in host.items()},
            "columns_equal_host_decoder": bool(equal), "hashed_names": name_key is not None,
            "known_sites": None if table is None else {
                "sites_per_kb": sites_per_kb, "sites": table.n, "table_bytes": int(5 * table.n + 8 * (table.n_ref + 1)),
                "bases_rewritten_device": int(dev_masked), "bases_rewritten_host": int(t.known_masked)},
            "sa_clips": None if sa_clips <= 0 else {
                "frac": sa_clips, "records_clipped": int(n_clipped) * tiles, "clip_bases_rewritten_device": int(dev_sa[0]),
                "clip_bases_rewritten_host": int(t.sa_masked), "entries_ignored_device": int(dev_sa[1]),
                "entries_ignored_host": int(t.sa_ignored)},
            "site_tally": tally_out,
            "workload": f"configs[0] tumor BAM records tiled x{tiles} ({nr} records, 150 bp); device: the stream "
                        f"resident in HBM, kernels only (HIP events on the context's stream); call wall adds the H2D "
                        f"copy, the scans' host reads and the D2H of the columns; host: ganon_bam_open of the same "
                        f"records as stored BGZF blocks (inflate = copy), file read included",
        }
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hash_names", action="store_true",
                    help="decode with a read-name key (GANON_READ_NAME_KEY as hex, else a fixed benchmark key)")
    ap.add_argument("--known_sites", type=float, default=0.0, metavar="SITES_PER_KB",
                    help="decode with a synthetic panel of this many sites per 1,000 bases (both sides)")
    ap.add_argument("--sa_clips", type=float, default=0.0, metavar="FRAC",
                    help="with --known_sites: this share of the records gets a trailing soft clip and an SA entry, and "
                         "the decoders mask the clips along it (--mask_sa_clips)")
    ap.add_argument("--site_tally", action="store_true",
                    help="decode with an evidence tally (--discover_sites) on both sides, and time k_site_compact")
    ap.add_argument("--min_base_quality", type=int, default=0, metavar="Q", help="with --site_tally: the rule's base quality")
    ap.add_argument("--min_mapq", type=int, default=0, metavar="M", help="with --site_tally: the rule's mapq")
    ap.add_argument("--exclude_flags", type=lambda t: int(t, 0), default=0, metavar="F", help="with --site_tally: excluded flags")
    ap.add_argument("--rule", choices=["both", "normal"], default="both", help="with --site_tally: --discover_rule")
    args = ap.parse_args()
    key = None
    if args.hash_names:
        from genomeanonymizer_amd import native
        v = os.environ.get(native.NAME_KEY_ENV)
        key = native.parse_name_key(v) if v is not None else BENCH_KEY
    rule = None
    if args.site_tally:
        from genomeanonymizer_amd import native
        rule = native.SiteRule(args.min_base_quality, args.min_mapq, args.exclude_flags, args.rule).checked()
    elif args.min_base_quality or args.min_mapq or args.exclude_flags or args.rule != "both":
        raise SystemExit("--min_base_quality, --min_mapq, --exclude_flags and --rule need --site_tally")
    print(json.dumps(measure(args.mb, args.threads, args.reps, key, args.known_sites, args.site_tally, args.sa_clips, rule)))


if __name__ == "__main__":
    main()
