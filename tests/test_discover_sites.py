"""--discover_sites / GANON_DISCOVER_SITES on the CPU: a pre-pass over a pair's own BAMs finds the
positions where a tumor read and a normal read show one allele other than the reference's, and the run
masks them as --known_sites masks a panel's. Every expectation comes from the plain-Python restatement of
the tally in discover_helpers (and of the mask in known_sites_helpers). The host tally against the
restatement on a hand-built record set (whole file, per contig, per region; 1 and 3 threads; either
dataset first; every record twice) and on golden scenarios through overlapping region reads; the
defining property — a run with the option on inputs X writes the files a run without it writes on X'
(X with the mask of D(X) less the pair's own SNVs applied to every record) — in streamed, whole-sample
and job mode, with each of the other four options and on two gloo ranks; what the log may say; the
command line. tests/test_gpu_discover_sites.py repeats it on the device."""
import logging
import os
import re

import numpy as np
import pytest

import discover_helpers as D
import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
from test_known_sites import _two_ranks


def set_option(monkeypatch, on) -> None:
    if on:
        monkeypatch.setenv("GANON_DISCOVER_SITES", "1")
    else:
        monkeypatch.delenv("GANON_DISCOVER_SITES", raising=False)


def _finish_all(t) -> dict:
    return D.lists_as_dict(t.names, [t.finish(i) for i in range(len(t.names))])


# ---- the host tally -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    from genomeanonymizer_amd.io.fasta import FastaRef
    d = str(tmp_path_factory.mktemp("hand"))
    plain, indexed = D.write_hand_files(d, False), D.write_hand_files(d, True)
    return {"plain": plain, "indexed": indexed, "fasta": FastaRef(plain["ref"]), "exp": D.expected_hand()}


def test_hand_built_expectations_are_the_literal_ones():
    """The restatement gives the outcomes stated by hand: tumor-only and normal-only evidence and tumor C
    with normal G are no sites, tumor {a, b} with normal {b, c} is a site with ALT b alone, two shared
    alleles are both ALT; reference N, ambiguity codes, read codes 15 / 3 / 5, clips, insertions,
    positions inside D and N and past the contig's end give nothing; lower case is folded."""
    exp = D.expected_hand()
    assert len(exp["h2"]) == 7 and len(exp["h3"]) >= 300 + 25
    for p in (D.TILE - 1, D.TILE, D.TILE + 1, 2 * D.TILE, 0, 3 * D.TILE):
        assert p in exp["h3"]


@pytest.mark.parametrize("threads", [1, 3])
def test_host_tally_whole_file(hand, threads):
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    files = hand["plain"]
    t = HostTally.of_fasta(hand["fasta"])
    assert not any(t.touched(i) for i in range(3))
    tables = [ReadTable(files[s], threads=threads, site_tally=(t, ds)) for ds, s in enumerate("TN")]
    plain = [ReadTable(files[s], threads=threads) for s in "TN"]
    for a, b in zip(tables, plain):     # the tally changes no column
        for f in K.I32 + K.I64 + K.BLOBS + ("seq", "qual"):
            assert np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f))), f
    assert t.touched(0) and t.touched(1) and t.touched(2)       # (h1: tumor evidence alone)
    assert _finish_all(t) == hand["exp"]
    assert not any(t.touched(i) for i in range(3))              # finish released the bytes
    # normal before tumor, and every record twice
    t2 = HostTally.of_fasta(hand["fasta"])
    for ds, s in ((1, "N"), (0, "T"), (0, "T"), (1, "N")):
        ReadTable(files[s], threads=threads, site_tally=(t2, ds))
    assert _finish_all(t2) == hand["exp"]
    # the datasets swapped give the same sites (the intersection is symmetric)
    t3 = HostTally.of_fasta(hand["fasta"])
    for ds, s in ((1, "T"), (0, "N")):
        ReadTable(files[s], threads=threads, site_tally=(t3, ds))
    assert _finish_all(t3) == hand["exp"]
    # one dataset alone: evidence, no site
    t4 = HostTally.of_fasta(hand["fasta"])
    ReadTable(files["T"], threads=threads, site_tally=(t4, 0))
    assert t4.touched(2) and _finish_all(t4) == {}


@pytest.mark.parametrize("threads", [1, 3])
def test_host_tally_per_contig_and_per_region(hand, threads):
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import BamReader
    files = hand["indexed"]
    rng = np.random.default_rng(threads)
    for how in ("contig", "region"):
        t = HostTally.of_fasta(hand["fasta"])
        for ds, s in enumerate("TN"):
            r = BamReader(files[s], threads)
            assert r.has_index
            r.set_site_tally(t, ds)
            for tid, L in enumerate(r.ref_lens.tolist()):
                if how == "contig":
                    r.contig(tid)
                    continue
                cuts = sorted(set([0, L] + rng.integers(0, L + 1, 4).tolist()))
                for a, b in zip(cuts[:-1], cuts[1:]):
                    r.region(tid, max(0, a - 7), min(L, b + 7))        # overlapping: records tallied twice
            r.set_site_tally(None)
            r.contig(2)                                                 # ... and no more once it is off
            r.close()
        assert _finish_all(t) == hand["exp"], how


def test_discover_returns_the_panel(hand):
    from genomeanonymizer_amd.discover_sites import discover, merge
    from genomeanonymizer_amd.known_sites import Panel
    for files in (hand["plain"], hand["indexed"]):
        stats = {}
        p = discover(files["T"], files["N"], hand["fasta"], 2, stats=stats)
        assert D.panel_as_dict(p) == hand["exp"] and list(p.contigs) == ["h2", "h3"]
        assert stats["sites"] == p.n_sites == sum(len(v) for v in hand["exp"].values())
        for pos, code in p.contigs.values():
            assert pos.dtype == np.int32 and code.dtype == np.uint8
    # the OR of two panels
    a = Panel("a", {"c": (np.array([1, 5, 9], np.int32), np.array([0x12, 0x24, 0x81], np.uint8))}, {})
    b = Panel("b", {"c": (np.array([5, 7], np.int32), np.array([0x28, 0x41], np.uint8)),
                    "d": (np.array([3], np.int32), np.array([0x12], np.uint8))}, {})
    m = merge(a, b)
    assert m.contigs["c"][0].tolist() == [1, 5, 7, 9] and m.contigs["c"][1].tolist() == [0x12, 0x2C, 0x41, 0x81]
    assert m.contigs["d"][0].tolist() == [3] and merge(a, None) is a and merge(None, b) is b


def test_tally_checks_its_arguments(hand):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import BamReader
    t = HostTally.of_fasta(hand["fasta"])
    lib = native.host_lib()
    r = BamReader(hand["indexed"]["T"], 1)
    ok = t.seq_of_tid(r.ref_names)
    assert ok.tolist() == [0, 1, 2, -1]
    for ds, m in ((2, ok), (-1, ok), (0, ok[:3]), (0, np.array([0, 1, 3, -1], np.int32)), (0, np.array([0, 1, -2, -1], np.int32))):
        assert lib.ganon_bam_reader_set_site_tally(r._h, t.handle, ds, native._ptr(m, native._i32p), len(m)) != 0
    r.close()
    with pytest.raises(native.GanonError):
        HostTally(["x"], np.zeros(1, np.uint8), [0], [-1])
    assert lib.ganon_site_tally_count(t.handle, 9) == -1 and t.bytes_address(9) is None


@pytest.fixture(scope="module")
def indexed_inputs(tmp_path_factory):
    import dataclasses
    from genomeanonymizer_amd.synth.generate import generate, scenario
    out = {}
    for name in ("tiny", "edge", "fuzz2000"):
        d = tmp_path_factory.mktemp(name)
        out[name] = generate(dataclasses.replace(scenario(name), bam_index=True), str(d / "in"))
    return out


@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz2000"])
def test_golden_regions_equal_whole_file(indexed_inputs, name):
    """Overlapping random regions that together cover each contig give the whole file's sites, and both
    give the restatement's D(X)."""
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import BamReader, ReadTable
    from genomeanonymizer_amd.io.fasta import FastaRef
    paths = indexed_inputs[name]
    fasta = FastaRef(paths["ref"])
    exp = D.scenario_sites(name)["sites"]
    whole = HostTally.of_fasta(fasta)
    for ds, s in enumerate("TN"):
        ReadTable(paths[s], threads=3, site_tally=(whole, ds))
    assert _finish_all(whole) == exp
    rng = np.random.default_rng(len(name))
    t = HostTally.of_fasta(fasta)
    for ds, s in enumerate("TN"):
        r = BamReader(paths[s], 2)
        r.set_site_tally(t, ds)
        for tid, L in enumerate(r.ref_lens.tolist()):
            cuts = sorted(set([0, L] + rng.integers(0, L + 1, 5).tolist()))
            for a, b in zip(cuts[:-1], cuts[1:]):
                r.region(tid, max(0, a - int(rng.integers(0, 300))), min(L, b + int(rng.integers(0, 300))))
        r.close()
    assert _finish_all(t) == exp


# ---- the pipeline: X with the option against X' without --------------------------------------------------

_REWRITTEN: dict = {}


def _rewritten(name, sites, monkeypatch, tmp_path) -> int:
    """How many bases of X the mask of ``sites`` rewrites (known_sites_helpers' record rule)."""
    if name not in _REWRITTEN:
        _REWRITTEN[name] = K.make_inputs(name, str(tmp_path / "count"), False, sites, monkeypatch)["_changed"]
    return _REWRITTEN[name]


def _or_sites(a: K.Sites, b: K.Sites) -> K.Sites:
    by: dict = {}
    for s in (a, b):
        for c in s.pos:
            d = by.setdefault(c, {})
            for p, (ref, alt) in zip(s.pos[c], s.val[c]):
                assert d.get(p, (ref, 0))[0] == ref
                d[p] = (ref, alt | d.get(p, (ref, 0))[1])
    return K.Sites(by)


def assert_property(name, tmp_path, monkeypatch, index=False, quality=None, gz=False, base=None, panel=None) -> dict:
    """The defining property on scenario ``name`` under the mode and options the caller set: the option on
    X writes the files the plain run writes on X' under D(X) less own (OR-ed with ``panel``'s sites when
    --known_sites is on too), byte for byte, and not the files the plain run writes on X."""
    ss = D.scenario_sites(name)
    sites = ss["less_own"] if panel is None else _or_sites(ss["less_own"], panel["sites"])
    set_option(monkeypatch, True)
    K.set_option(monkeypatch, panel["vcf"] if panel else None)
    got = K.run_files(name, str(tmp_path / "x"), H.oracle_anonymizer(), index, gz=gz)
    set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    exp = K.run_files(name, str(tmp_path / "xp"), H.oracle_anonymizer(), index, sites, monkeypatch, gz=gz, quality=quality)
    if base is None:
        base = K.run_files(name, str(tmp_path / "x0"), H.oracle_anonymizer(), index, gz=gz)
    assert sorted(got) == sorted(exp)
    for f in exp:
        assert got[f] == exp[f], f
    assert any(base.get(f) != exp[f] for f in exp), "the plain runs on X and X' wrote the same files"
    return got


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz2000", "fuzz3000", "long1"])
def test_option_equals_plain_run_on_rewritten_inputs(name, mode, tmp_path, monkeypatch):
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    ss = D.scenario_sites(name)
    n_sites, n_less = sum(len(v) for v in ss["sites"].values()), ss["less_own"].n()
    changed = _rewritten(name, ss["less_own"], monkeypatch, tmp_path)
    print(f"{name}: {n_sites} sites ({n_less} less own), {changed} bases rewritten")
    assert n_less >= 50 and changed >= 500 and n_less < n_sites
    assert_property(name, tmp_path, monkeypatch, index, base=M.golden_files(name))


def test_known_sites_composes(tmp_path, monkeypatch):
    """Both options: the two tables are OR-ed position by position before the pair's own SNVs leave."""
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    sp = K.scenario_panel("tiny")
    both = _or_sites(D.scenario_sites("tiny")["less_own"], sp["sites"])
    assert both.n() > max(D.scenario_sites("tiny")["less_own"].n(), sp["sites"].n())     # neither holds the other
    assert_property("tiny", tmp_path, monkeypatch, panel=sp, base=M.golden_files("tiny"))


def test_hash_read_names_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, H.KEY)
    got = assert_property("edge", tmp_path, monkeypatch)
    assert all(len(n) == 32 for n, _, _, _ in H.fastq_records(got["tumor.1.fastq"]))


def test_masked_base_quality_composes(tmp_path, monkeypatch):
    """X' carries the quality patch: the rewritten bases have quality 2 there, as the option's bases have
    in the run on X."""
    M.set_mode(monkeypatch, "jobs", 2)
    H.set_option(monkeypatch, False)
    got = assert_property("fuzz2000", tmp_path, monkeypatch, True, quality=2)
    M.set_mode(monkeypatch, "jobs", 2)       # (the patch is needed: X' without it gives other quality lines)
    exp = K.run_files("fuzz2000", str(tmp_path / "noq"), H.oracle_anonymizer(), True,
                      D.scenario_sites("fuzz2000")["less_own"], monkeypatch)
    assert any(got[f] != exp[f] for f in got)


def test_compress_output_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    assert_property("tiny", tmp_path, monkeypatch, gz=True, base=M.golden_files("tiny"))


def test_two_ranks_equal_one_process(tmp_path, monkeypatch):
    """Each rank discovers the sequences dealt to it and the lists are exchanged: two ranks write one
    process's files, which are those of the plain run on X'."""
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    set_option(monkeypatch, True)
    got = _two_ranks("fuzz3000", str(tmp_path / "two"))
    exp = K.run_files("fuzz3000", str(tmp_path / "one"), H.oracle_anonymizer())
    assert got == exp and len(exp) == 7
    set_option(monkeypatch, False)
    assert got == K.run_files("fuzz3000", str(tmp_path / "xp"), H.oracle_anonymizer(), False,
                              D.scenario_sites("fuzz3000")["less_own"], monkeypatch)


# ---- what the log and the output directory may hold ---------------------------------------------------------

def test_the_site_list_is_neither_logged_nor_written(tmp_path, monkeypatch, caplog):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    set_option(monkeypatch, True)
    plain_dir = str(tmp_path / "off")
    with caplog.at_level(logging.DEBUG):
        K.run_files("fuzz2000", str(tmp_path / "on"), H.oracle_anonymizer())
    text = caplog.text
    assert "discovered sites" in text and "pre-pass" in text and "bases rewritten" in text and "left out" in text
    ss = D.scenario_sites("fuzz2000")
    sites = ss["sites"]
    assert sum(len(v) for v in sites.values()) > 1000
    for c, d in sites.items():
        ps = sorted(d)
        for p in ps:
            for q in (p, p + 1):        # 0- and 1-based
                assert not re.search(rf"{re.escape(c)}[:\t ]{q}\b", text), (c, q)
        # no list of positions: no three neighbouring sites one after another, whatever separates them
        for a, b, e in zip(ps, ps[1:], ps[2:]):
            for k in (0, 1):
                assert not re.search(rf"\b{a + k}\D{{1,3}}{b + k}\D{{1,3}}{e + k}\b", text)
    set_option(monkeypatch, False)
    K.run_files("fuzz2000", plain_dir, H.oracle_anonymizer())

    def listing(d):
        return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    assert listing(str(tmp_path / "on")) == listing(plain_dir)


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
    monkeypatch.setenv("GANON_KNOWN_SITES", "")
    monkeypatch.setenv("GANON_DISCOVER_SITES", "0")     # (the flag writes it: restored afterwards)
    return ga


def test_cli_flag_and_environment_default(cli, tmp_path, monkeypatch, caplog):
    from genomeanonymizer_amd import discover_sites
    from genomeanonymizer_amd.synth.generate import generate, scenario
    base = ["-d", "x", "-s", "s", "-r", "r"]
    assert cli.exec_parser(base).discover_sites is None
    assert cli.exec_parser(base + ["--discover_sites"]).discover_sites is True
    assert cli.exec_parser(base + ["--no-discover_sites"]).discover_sites is False
    assert not discover_sites.default_on()
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    with caplog.at_level(logging.INFO):
        _cli(cli, d, paths, ["--discover_sites"])
    got = H.collect(paths)
    assert os.environ["GANON_DISCOVER_SITES"] == "1" and discover_sites.default_on()
    assert "discovered sites" in caplog.text and "bases rewritten" in caplog.text
    monkeypatch.setenv("GANON_DISCOVER_SITES", "0")
    exp = K.run_files("tiny", str(tmp_path / "xp"), H.oracle_anonymizer(), False, D.scenario_sites("tiny")["less_own"],
                      monkeypatch)
    assert got == exp and len(got) == 7 and got != M.golden_files("tiny")
    # the environment default, without the flag
    d2 = str(tmp_path / "env")
    paths2 = generate(scenario("tiny"), d2)
    monkeypatch.setenv("GANON_DISCOVER_SITES", "1")
    _cli(cli, d2, paths2)
    assert H.collect(paths2) == exp
    # --no-discover_sites over the environment: the plain files, no pre-pass, no tally, nothing masked
    calls = []
    monkeypatch.setattr(discover_sites, "discover", lambda *a, **k: calls.append(a) or pytest.fail("pre-pass ran"))
    monkeypatch.setattr(discover_sites, "HostTally", lambda *a, **k: pytest.fail("a tally was made"))
    _cli(cli, d2, paths2, ["--no-discover_sites"])
    assert H.collect(paths2) == M.golden_files("tiny") and not calls


def test_option_off_leaves_the_readers_alone(tmp_path, monkeypatch):
    from genomeanonymizer_amd import discover_sites
    from genomeanonymizer_amd.io.bam import BamReader, ReadTable
    from genomeanonymizer_amd.io.fasta import FastaRef
    from genomeanonymizer_amd.synth.generate import generate, scenario
    set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    paths = generate(scenario("tiny"), str(tmp_path / "in"))
    assert discover_sites.pair_default(FastaRef(paths["ref"]), [], paths["T"], paths["N"]) is None
    t = ReadTable(paths["T"])
    r = BamReader(paths["T"])
    assert t.known_masked == 0 and r.site_tally is None and r.contig(0).known_masked == 0 and r.known_masked() == 0
    r.close()
