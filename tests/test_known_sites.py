"""--known_sites / GANON_KNOWN_SITES on the CPU: a read base that is aligned to a panel position and
shows a listed ALT becomes the reference base where its record is decoded. Every expectation comes from
the plain-Python restatement of the rule in known_sites_helpers. The decoders (whole file, per contig,
per region; 1 and 3 threads) against the rule over the tables decoded without the option, on golden
scenarios and on a hand-built stream of the rule's corners; the defining property — a run with the
option on inputs X writes the files a run without it writes on X' (X with the rule applied to every
record) — in streamed, whole-sample and job mode, with each of the other three options and on two
gloo ranks; the panel loader and the command line. tests/test_gpu_known_sites.py repeats it on the
device."""
import logging
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
from test_distributed import _free_port, _worker


# ---- tables ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def indexed_inputs(tmp_path_factory):
    import dataclasses
    from genomeanonymizer_amd.synth.generate import generate, scenario
    out = {}
    for name in ("tiny", "edge", "fuzz2000"):
        d = tmp_path_factory.mktemp(name)
        out[name] = generate(dataclasses.replace(scenario(name), bam_index=True), str(d / "in"))
    return out


@pytest.mark.parametrize("quality", [None, 2])
@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz2000"])
def test_masked_readers_match_the_rule(indexed_inputs, name, quality):
    from genomeanonymizer_amd.io.bam import BamReader, ReadTable
    sites = K.scenario_panel(name)["sites"]
    rng = np.random.default_rng(len(name))
    total = 0
    for s in ("T", "N"):
        path = indexed_inputs[name][s]
        whole = ReadTable(path, threads=3)
        table = K.table_of(sites, whole.ref_names, quality)
        for threads in (1, 3):
            got = ReadTable(path, threads=threads, known_sites=table)
            n = K.assert_masked_table(got, whole, sites, quality, "file")
            assert got.known_masked == n
        total += n
        plain, masked = BamReader(path, 3), BamReader(path, 3, known_sites=table)
        one = BamReader(path, 1, known_sites=table)
        assert plain.has_index and masked.has_index
        counted = 0
        for tid, L in enumerate(plain.ref_lens.tolist()):
            p = plain.contig(tid)
            for r in (masked, one):
                g = r.contig(tid)
                c = K.assert_masked_table(g, p, sites, quality, ("contig", tid))
                assert g.known_masked == c
            counted += 2 * c
            regions = [(0, L), (0, 1), (L // 2, L // 2), (L - 1, L + 5)]
            for _ in range(6):
                a = int(rng.integers(0, L))
                regions.append((a, int(min(L + 10, a + rng.integers(1, max(2, L // 3))))))
            for a, b in regions:
                p = plain.region(tid, a, b)
                g = masked.region(tid, a, b)
                c = K.assert_masked_table(g, p, sites, quality, ("region", tid, a, b))
                assert g.known_masked == c
                counted += c
        assert masked.known_masked() + one.known_masked() == counted and plain.known_masked() == 0
        for r in (plain, masked, one):
            r.close()
    assert total >= K.MIN_CHANGED


def _hand_file(tmp_path, recs):
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    stream, _ = K.stream_of(recs)
    path = str(tmp_path / "hand.bam")
    write_bgzf(path, stream.tobytes())
    return path


@pytest.mark.parametrize("quality", [None, 0, 41])
def test_hand_built_stream(tmp_path, quality):
    from genomeanonymizer_amd.io.bam import ReadTable
    recs, sites = K.hand_built()
    path = _hand_file(tmp_path, recs)
    plain = ReadTable(path)
    assert plain.n == len(recs)
    exp, total = K.expected_of(recs, sites, quality=quality)
    assert total >= 30
    for threads in (1, 3):
        got = ReadTable(path, threads=threads, known_sites=K.table_of(sites, plain.ref_names, quality))
        assert K.assert_masked_table(got, plain, sites, quality) == total == got.known_masked
        # ... and the table rule is the record rule
        for i, (nib, qual) in enumerate(exp):
            assert K.table_nibbles(got, i) == nib, i
            o = int(got.qual_off[i])
            assert np.asarray(got.qual[o:o + len(qual)]).tolist() == qual, i
    # what the cases are there for: spot checks against the literal expectation
    first = exp[0][0]
    r0 = recs[0]["nib"]
    assert first[:2] == r0[:2] and first[2] == 1 and first[5] == 1 and first[6:8] == r0[6:8]     # clip; 100, 103; the I
    assert first[8] == 1 and first[10] == 1 and first[11] == 1 and first[14] == 1                # 106, 108, 209, 212
    assert first[15] == 1 and first[17] == 1 and first[18] == 1 and first[19] == 1               # = and X
    assert first[20:] == r0[20:]                                                                 # the trailing clip
    assert exp[1][0] == [1, 1] + recs[1]["nib"][2:6] + [1] and exp[3][0] == [1]
    assert exp[4][0] == [1, 2, 1, 1, 2, 2]
    assert exp[5][0] == recs[5]["nib"][:5] + [1]                                                 # codes stay, T goes
    for k in (6, 7, 8, 9, 10):
        assert exp[k][0] == recs[k]["nib"], k                                                    # the skipped records
    assert exp[11][0] == [1] + recs[11]["nib"][1:4] + [1]
    if quality is not None:
        assert exp[12][1] == [0xFF] * 5 and exp[13][1] == [0xFF, 20, 20, 20, 20]
        assert exp[14][1] == [quality, quality, quality, quality, quality]
        assert exp[1][1][0] == quality and exp[1][1][1] == quality and exp[1][1][2] == recs[1]["qual"][2]


def test_tables_without_sites(tmp_path):
    """A sequence with no sites, a panel with none at all, and sites on other sequences only."""
    from genomeanonymizer_amd.io.bam import BamReader, ReadTable
    from genomeanonymizer_amd.known_sites import SitesTable
    recs, sites = K.hand_built()
    path = _hand_file(tmp_path, recs)
    plain = ReadTable(path)
    empty = K.Sites({})
    for s in (empty, K.Sites({"c3": {}}), K.Sites({"c9": {5: (1, 2)}})):
        got = ReadTable(path, known_sites=K.table_of(s, plain.ref_names, 3))
        assert K.assert_masked_table(got, plain, s, 3) == 0 == got.known_masked
    only_c3 = K.Sites({"c3": {p: (1, 14) for p in range(10, 30)}})
    got = ReadTable(path, known_sites=K.table_of(only_c3, plain.ref_names))
    assert K.assert_masked_table(got, plain, only_c3) == 20
    r = BamReader(path, known_sites=SitesTable(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8)))
    assert K.assert_masked_table(r.contig(0), BamReader(path).contig(0), empty) == 0
    r.close()


def test_sites_create_checks_its_arrays():
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.known_sites import SitesTable

    def make(off, pos, code, q=-1):
        return SitesTable(np.array(off, np.int64), np.array(pos, np.int32), np.array(code, np.uint8), q).handle
    assert make([0, 2, 2], [5, 9], [0x12, 0x87])
    for bad in (([0, 2], [9, 5], [0x12, 0x12]), ([0, 2], [5, 5], [0x12, 0x12]), ([0, 1], [-1], [0x12]),
                ([0, 1], [5], [0x10]), ([0, 1], [5], [0x02]), ([0, 1], [5], [0x33]), ([0, 1], [5], [0x13]),
                ([1, 1], [5], [0x12]), ([0, 2, 1], [5, 6], [0x12, 0x12])):
        with pytest.raises(native.GanonError):
            make(*bad)
    with pytest.raises(native.GanonError):
        make([0, 1], [5], [0x12], 94)


# ---- the panel loader ----------------------------------------------------------------------------------

def test_loader_reads_what_the_helpers_wrote():
    """The loader's table for a scenario equals the helpers' own reading of the panel they wrote: used
    lines, OR-ed ALTs, lower case, skipped indel / MNV / symbolic lines, the contig the BAM lacks, and
    the pair's own SNV position left out."""
    from genomeanonymizer_amd.io.fasta import FastaRef
    from genomeanonymizer_amd.io.vcf import read_vcf
    from genomeanonymizer_amd.known_sites import PairPanel, load_panel
    from genomeanonymizer_amd.planner import get_windows
    for name in ("tiny", "fuzz2000"):
        sp = K.scenario_panel(name)
        paths = sp["plain_inputs"]
        fa = FastaRef(paths["ref"])
        panel = load_panel(sp["vcf"], fa)
        assert panel.stats["skipped_long_ref"] == 2 and panel.stats["no_snv_alt"] == 1
        assert panel.stats["contigs_not_in_reference"] == 1 and panel.stats["load_s"] < 5
        pair = PairPanel(panel, get_windows(read_vcf(paths["vcf"]), fa.index), 7)
        assert sp["own"] is not None and pair.excluded >= 1
        names = list(fa.references)
        got, exp = pair.table(names), K.table_of(sp["sites"], names, 7)
        for f in ("site_off", "site_pos", "site_code"):
            assert np.array_equal(getattr(got, f), getattr(exp, f)), (name, f)
        assert got.quality == 7 and got.n == sp["sites"].n() > 40
        c, p = sp["own"]
        assert p not in got.site_pos[got.site_off[names.index(c)]:got.site_off[names.index(c) + 1]].tolist()
        assert p in panel.contigs[c][0].tolist()
        # a BAM header with another order and a sequence the panel does not know
        other = pair.table(["zz"] + names[::-1])
        assert other.n == got.n and other.site_off[1] == 0


# ---- the pipeline: X with the option against X' without --------------------------------------------------

@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz2000", "fuzz3000", "long1"])
def test_option_equals_plain_run_on_rewritten_inputs(name, mode, tmp_path, monkeypatch):
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    K.assert_option_equals_plain_on_rewritten(name, tmp_path, monkeypatch, H.oracle_anonymizer, index,
                                              base=M.golden_files(name))


def test_hash_read_names_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, H.KEY)
    got = K.assert_option_equals_plain_on_rewritten("edge", tmp_path, monkeypatch, H.oracle_anonymizer)
    assert all(len(n) == 32 for n, _, _, _ in H.fastq_records(got["tumor.1.fastq"]))


def test_masked_base_quality_composes(tmp_path, monkeypatch):
    """X' carries the quality patch: the rewritten bases have quality 2 there, as the option's bases have
    in the run on X."""
    M.set_mode(monkeypatch, "jobs", 2)
    H.set_option(monkeypatch, False)
    got = K.assert_option_equals_plain_on_rewritten("fuzz2000", tmp_path, monkeypatch, H.oracle_anonymizer, True,
                                                    quality=2)
    # (the patch is needed: X' without it gives other quality lines)
    M.set_mode(monkeypatch, "jobs", 2)
    K.set_option(monkeypatch, None)
    exp = K.run_files("fuzz2000", str(tmp_path / "noq"), H.oracle_anonymizer(), True, K.scenario_panel("fuzz2000")["sites"],
                      monkeypatch)
    assert any(got[f] != exp[f] for f in got)


def test_compress_output_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    K.assert_option_equals_plain_on_rewritten("tiny", tmp_path, monkeypatch, H.oracle_anonymizer, gz=True,
                                              base=M.golden_files("tiny"))


# ---- two gloo ranks --------------------------------------------------------------------------------------

def _two_ranks(name, workdir):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    paths = generate(scenario(name), os.path.join(workdir, "in"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, name, workdir, q, "oracle")) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    alive = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert alive == [False, False] and [p.exitcode for p in procs] == [0, 0]
    return H.collect(paths)


def test_two_ranks_equal_one_process(tmp_path, monkeypatch):
    """Each rank loads the panel itself (the variable is inherited): two ranks write one process's files."""
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, K.scenario_panel("fuzz3000")["vcf"])
    got = _two_ranks("fuzz3000", str(tmp_path / "two"))
    exp = K.run_files("fuzz3000", str(tmp_path / "one"), H.oracle_anonymizer())
    assert got == exp and len(exp) == 7
    K.set_option(monkeypatch, None)
    assert got != K.run_files("fuzz3000", str(tmp_path / "off"), H.oracle_anonymizer())


# ---- the command line ------------------------------------------------------------------------------------

def _cli(ga, d, paths, extra=()):
    ga.run_anonymizer(["-d", d, "-s", "samples.tsv", "-r", paths["ref"], "--record_statistics", "-v", "1", *extra])


@pytest.fixture
def cli(monkeypatch):
    from genomeanonymizer_amd import genome_anonymizer as ga
    from genomeanonymizer_amd import writer
    monkeypatch.setattr(ga, "CompleteGermlineAnonymizer", lambda device=0: H.oracle_anonymizer())
    monkeypatch.setattr(writer, "io_block_size", lambda d: 4096)
    M.set_mode(monkeypatch, "streamed", None)
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "0")
    monkeypatch.setenv("GANON_HASH_READ_NAMES", "0")
    monkeypatch.setenv("GANON_KNOWN_SITES", "")     # (the flag writes it: restored afterwards)
    return ga


def test_cli_flag_and_environment_default(cli, tmp_path, monkeypatch, caplog):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    base = ["-d", "x", "-s", "s", "-r", "r"]
    assert cli.exec_parser(base).known_sites is None
    assert cli.exec_parser(base + ["--known_sites", "p.vcf.gz"]).known_sites == "p.vcf.gz"
    sp = K.scenario_panel("tiny")
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    with caplog.at_level(logging.INFO):
        _cli(cli, d, paths, ["--known_sites", sp["vcf"]])
    got = H.collect(paths)
    assert os.environ["GANON_KNOWN_SITES"] == sp["vcf"]
    assert "sites used" in caplog.text and "bases rewritten" in caplog.text
    K.set_option(monkeypatch, None)
    exp = K.run_files("tiny", str(tmp_path / "xp"), H.oracle_anonymizer(), False, sp["sites"], monkeypatch)
    assert got == exp and len(got) == 7 and got != M.golden_files("tiny")
    # the environment default, without the flag
    d2 = str(tmp_path / "env")
    paths2 = generate(scenario("tiny"), d2)
    K.set_option(monkeypatch, sp["vcf"])
    _cli(cli, d2, paths2)
    assert H.collect(paths2) == exp
    # the option off: the plain files
    monkeypatch.setenv("GANON_KNOWN_SITES", "")
    _cli(cli, d2, paths2)
    assert H.collect(paths2) == M.golden_files("tiny")


@pytest.mark.parametrize("bad", ["ref_mismatch", "past_end", "missing", "conflict", "truncated_gz"])
def test_cli_bad_panel_ends_before_any_output(cli, tmp_path, bad):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    fa = K._fasta(paths["ref"])
    c = sorted(fa)[0]
    ref = fa[c][99].upper()
    wrong = next(b for b in "ACGT" if b != ref)
    alt = next(b for b in "ACGT" if b not in (ref, wrong))
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    panel = str(tmp_path / "panel.vcf")
    body = {"ref_mismatch": f"{c}\t100\t.\t{wrong}\t{alt}\t.\t.\t.\n",
            "past_end": f"{c}\t{len(fa[c]) + 1}\t.\tA\tC\t.\t.\t.\n",
            "conflict": f"{c}\t100\t.\t{ref}\t{alt}\t.\t.\t.\n{c}\t100\t.\t{wrong}\t{alt}\t.\t.\t.\n"}.get(bad)
    if body is not None:
        open(panel, "w").write(head + body)
    elif bad == "truncated_gz":
        import gzip
        panel += ".gz"
        blob = gzip.compress((head + f"{c}\t100\t.\t{ref}\t{alt}\t.\t.\t.\n" * 2000).encode())
        open(panel, "wb").write(blob[:len(blob) // 2])
    before = sorted(os.listdir(d))
    with pytest.raises(SystemExit) as e:
        _cli(cli, d, paths, ["--known_sites", panel])
    assert e.value.code not in (0, None)
    assert sorted(os.listdir(d)) == before
