"""--discover_sites' evidence filters and rule on the CPU: --discover_min_base_quality, --discover_min_mapq
and --discover_exclude_flags decide which bases may set a tally bit, --discover_rule both|normal how the
byte is read (normal: an allele the normal shows is a site, whatever the tumor shows — the tumor's loss of
heterozygosity must not keep the donor's alleles in the normal's FASTQ). Every expectation comes from the
plain-Python restatement in discover_rules_helpers. The host tally against it on a hand-built record set
(plain streams and an indexed reader, 1 and 3 threads, a handful of rules); the defining property — a run
with the options on X writes what a plain run writes on X' under D(X; Q, M, F, rule) less the pair's own
SNVs — on golden scenarios, with the other options and on two gloo ranks; the command line.
tests/test_gpu_discover_rules.py repeats it on the device."""
import ctypes as C
import logging
import os

import numpy as np
import pytest

import discover_helpers as D
import discover_rules_helpers as R
import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
import sa_clips_helpers as S
from test_discover_sites import _or_sites, set_option
from test_known_sites import _two_ranks

Q20 = R.Rule(20, 0, 0, "both")
Q20N = R.Rule(20, 0, 0, "normal")


def _finish_all(t) -> dict:
    return D.lists_as_dict(t.names, [t.finish(i) for i in range(len(t.names))])


# ---- the host tally -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    from genomeanonymizer_amd.io.fasta import FastaRef
    d = str(tmp_path_factory.mktemp("rules"))
    plain, indexed = R.write_hand_files(d, False), R.write_hand_files(d, True)
    return {"plain": plain, "indexed": indexed, "fasta": FastaRef(plain["ref"])}


def test_hand_built_expectations_are_the_literal_ones():
    """The restatement gives the outcomes stated by hand under Q 20, mapq 30, flags 0x700 in both modes, and
    the rules differ from each other on the set: no rule is covered by another's expectation."""
    t, n, _, lit = R.hand_built()
    assert 300 < len(t) < 1000 and 300 < len(n) < 1000
    assert {48, 49, 64, 65, 129} <= {len(r["cigar"]) for r in t}
    exp = {rule: R.expected_hand(rule) for rule in R.RULES}
    assert len(lit["both"]["site"]) > 200 and len(lit["both"]["none"]) > 100
    assert len(lit["normal"]["site"]) > len(lit["both"]["site"])
    for a in range(len(R.RULES)):
        for b in range(a):
            assert exp[R.RULES[a]] != exp[R.RULES[b]], (R.RULES[a], R.RULES[b])
    # the zero rule is discover_helpers' rule
    ev: dict = {}
    D.tally_records(ev, t, R.HAND_CONTIGS, R.hand_built()[2], 0)
    D.tally_records(ev, n, R.HAND_CONTIGS, R.hand_built()[2], 1)
    assert D.sites_of(ev, R.hand_built()[2]) == exp[R.ZERO]
    for p in (R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE):
        assert p in exp[R.FULL_NORMAL]["h3"] and p not in exp[R.FULL]["h3"]


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: f"q{r.q}m{r.m}f{r.f:x}{r.mode}")
def test_host_tally_streams_and_indexed_reader(hand, rule, threads):
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import BamReader, ReadTable
    exp = R.expected_hand(rule)
    files = hand["plain"]
    t = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
    tables = [ReadTable(files[s], threads=threads, site_tally=(t, ds)) for ds, s in enumerate("TN")]
    plain = [ReadTable(files[s], threads=threads) for s in "TN"]
    for a, b in zip(tables, plain):     # the tally changes no column, whatever the rule
        for f in K.I32 + K.I64 + K.BLOBS + ("seq", "qual"):
            assert np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f))), f
    assert _finish_all(t) == exp
    # normal before tumor and every record twice: the filters leave the OR what it is
    t2 = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
    for ds, s in ((1, "N"), (0, "T"), (0, "T"), (1, "N")):
        ReadTable(files[s], threads=threads, site_tally=(t2, ds))
    assert _finish_all(t2) == exp
    # the indexed reader, per contig and through overlapping regions
    rng = np.random.default_rng(threads)
    for how in ("contig", "region"):
        t3 = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
        for ds, s in enumerate("TN"):
            r = BamReader(hand["indexed"][s], threads)
            assert r.has_index
            r.set_site_tally(t3, ds)
            for tid, L in enumerate(r.ref_lens.tolist()):
                if how == "contig":
                    r.contig(tid)
                    continue
                cuts = sorted(set([0, L] + rng.integers(0, L + 1, 4).tolist()))
                for a, b in zip(cuts[:-1], cuts[1:]):
                    r.region(tid, max(0, a - 7), min(L, b + 7))
            r.close()
        assert _finish_all(t3) == R.expected_indexed(rule), how


def test_one_dataset_alone(hand):
    """Mode normal needs the normal's evidence and nothing else; the tumor's alone is no site in either mode."""
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    t, n, fa, _ = R.hand_built()
    for rule in (R.FULL, R.FULL_NORMAL):
        a = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
        ReadTable(hand["plain"]["T"], threads=2, site_tally=(a, 0))
        assert a.touched(2) and _finish_all(a) == {}
        b = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
        ReadTable(hand["plain"]["N"], threads=2, site_tally=(b, 1))
        ev: dict = {}
        R.tally_records(ev, n, fa, 1, rule)
        want = R.sites_of(ev, fa, rule.mode)
        assert _finish_all(b) == want and (want != {}) == (rule.mode == "normal")


def test_create_is_create_ex_with_the_zero_rule(hand):
    """The tally bytes of ganon_site_tally_create and of ganon_site_tally_create_ex with a zero rule are
    equal, byte for byte, and so are the sites; a filtered tally's bytes differ."""
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    lib = native.host_lib()

    def bytes_of(t):
        out = []
        for i in range(3):
            a = t.bytes_address(i)
            out.append(C.string_at(a, int(t.lengths[i])) if a else None)
        return out
    ex = HostTally.of_fasta(hand["fasta"], R.site_rule(R.ZERO))
    old = HostTally.of_fasta(hand["fasta"])
    lib.ganon_site_tally_destroy(old._h)
    h = C.c_void_p()
    assert lib.ganon_site_tally_create(len(old.names), native._ptr(old.packed, native._u8p),
                                       native._ptr(old.nib_off, native._i64p), native._ptr(old.lengths, native._i64p),
                                       C.byref(h)) == 0
    old._h = h
    filt = HostTally.of_fasta(hand["fasta"], R.site_rule(R.FULL))
    for t in (ex, old, filt):
        for ds, s in enumerate("TN"):
            ReadTable(hand["plain"][s], threads=2, site_tally=(t, ds))
    b_ex, b_old, b_f = bytes_of(ex), bytes_of(old), bytes_of(filt)
    assert b_ex == b_old and b_ex[1] is not None and b_ex[2] is not None and b_f[2] != b_ex[2]   # (h1 has no record)
    assert _finish_all(old) == _finish_all(ex) == R.expected_hand(R.ZERO)


def test_rules_are_checked():
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    lib = native.host_lib()
    z = np.zeros(1, np.uint8)
    one = np.array([0], np.int64), np.array([1], np.int64)
    for bad in ((94, 0, 0, 0), (-1, 0, 0, 0), (0, 256, 0, 0), (0, -1, 0, 0), (0, 0, 65536, 0), (0, 0, 0, 2), (0, 0, 0, -1)):
        h = C.c_void_p()
        assert lib.ganon_site_tally_create_ex(1, native._ptr(z, native._u8p), native._ptr(one[0], native._i64p),
                                              native._ptr(one[1], native._i64p), *bad, C.byref(h)) != 0 and not h.value
    for q, m, f, mode in ((94, 0, 0, "both"), (0, 256, 0, "both"), (0, 0, 1 << 16, "both"), (0, 0, 0, "tumor"), (-1, 0, 0, "normal")):
        with pytest.raises(ValueError):
            HostTally(["x"], z, [0], [1], native.SiteRule(q, m, f, mode))
    t = HostTally(["x"], z, [0], [1], native.SiteRule(93, 255, 65535, "normal"))
    assert t.rule.filtered and not native.SiteRule().filtered
    t.close()


# ---- the pipeline: X with the options against X' without -------------------------------------------------

def _check_not_vacuous(name, rule) -> dict:
    """On the restatement alone: D(X; rule) is non-empty and differs from D(X) (K.make_inputs asserts that the
    rewritten inputs differ from X)."""
    ss = R.scenario_sites(name, rule)
    n, n_plain = sum(len(v) for v in ss["sites"].values()), sum(len(v) for v in ss["plain"].values())
    print(f"{name} {rule}: {n} sites ({ss['less_own'].n()} less own) against {n_plain} without filters")
    assert n > 0 and ss["less_own"].n() >= 20 and ss["sites"] != ss["plain"]
    return ss


def assert_property(name, rule, tmp_path, monkeypatch, index=False, quality=None, panel=None, base=None) -> dict:
    """The defining property under the mode and the other options the caller set: the options on X write the
    files the plain run writes on X' under D(X; rule) less own (OR-ed with ``panel``'s sites), byte for byte,
    not the files of the plain run on X, and not the files --discover_sites without the options writes."""
    ss = _check_not_vacuous(name, rule)
    sites = ss["less_own"] if panel is None else _or_sites(ss["less_own"], panel["sites"])
    set_option(monkeypatch, True)
    R.set_rule(monkeypatch, rule)
    K.set_option(monkeypatch, panel["vcf"] if panel else None)
    got = K.run_files(name, str(tmp_path / "x"), H.oracle_anonymizer(), index)
    R.set_rule(monkeypatch, None)
    unfiltered = K.run_files(name, str(tmp_path / "xu"), H.oracle_anonymizer(), index)
    set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    exp = K.run_files(name, str(tmp_path / "xp"), H.oracle_anonymizer(), index, sites, monkeypatch, quality=quality)
    if base is None:
        base = K.run_files(name, str(tmp_path / "x0"), H.oracle_anonymizer(), index)
    assert sorted(got) == sorted(exp)
    for f in exp:
        assert got[f] == exp[f], f
    assert any(base.get(f) != exp[f] for f in exp), "the plain runs on X and X' wrote the same files"
    assert any(unfiltered[f] != got[f] for f in got), "the filters and the rule changed nothing"
    return got


@pytest.mark.parametrize("rule", [Q20, Q20N], ids=["q20both", "q20normal"])
@pytest.mark.parametrize("name", ["tiny", "fuzz2000"])
def test_option_equals_plain_run_on_rewritten_inputs(name, rule, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "whole", None)
    H.set_option(monkeypatch, False)
    assert_property(name, rule, tmp_path, monkeypatch, base=M.golden_files(name))


@pytest.mark.parametrize("mode", ["streamed", "jobs"])
def test_streamed_and_job_mode(mode, tmp_path, monkeypatch):
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    assert_property("tiny", Q20N, tmp_path, monkeypatch, index, base=M.golden_files("tiny"))


def test_normal_rule_holds_the_filtered_intersection():
    """On the restatement: with equal filters every site of rule both is a site of rule normal with at least
    its ALTs, and normal has more; the quality filter removes sites under either rule."""
    for name in ("tiny", "fuzz2000"):
        b, n = R.scenario_sites(name, Q20)["sites"], R.scenario_sites(name, Q20N)["sites"]
        n0 = R.scenario_sites(name, R.Rule(0, 0, 0, "normal"))["sites"]
        for c, d in b.items():
            for p, (ref, alt) in d.items():
                assert n[c][p][0] == ref and n[c][p][1] & alt == alt
        count = lambda s: sum(len(v) for v in s.values())   # noqa: E731
        assert count(b) < count(n) < count(n0)


def test_known_sites_composes(tmp_path, monkeypatch):
    """The discovered table under the rule is OR-ed with the panel's position by position."""
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    sp = K.scenario_panel("tiny")
    mine = R.scenario_sites("tiny", Q20N)["less_own"]
    assert _or_sites(mine, sp["sites"]).n() > max(mine.n(), sp["sites"].n())
    assert_property("tiny", Q20N, tmp_path, monkeypatch, panel=sp, base=M.golden_files("tiny"))


def test_masked_base_quality_composes(tmp_path, monkeypatch):
    """The mask is not filtered: a rewritten base gets quality 2 whatever quality it had, in X' and in the run."""
    M.set_mode(monkeypatch, "streamed", 2)
    H.set_option(monkeypatch, False)
    assert_property("tiny", Q20, tmp_path, monkeypatch, quality=2)


def test_mask_sa_clips_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    ss = _check_not_vacuous("fuzz2000", Q20N)
    set_option(monkeypatch, True)
    R.set_rule(monkeypatch, Q20N)
    S.set_option(monkeypatch, True)
    got = S.run_files("fuzz2000", str(tmp_path / "x"), H.oracle_anonymizer())
    S.set_option(monkeypatch, False)
    table_only = S.run_files("fuzz2000", str(tmp_path / "xt"), H.oracle_anonymizer())
    set_option(monkeypatch, False)
    R.set_rule(monkeypatch, None)
    exp = S.run_files("fuzz2000", str(tmp_path / "xpp"), H.oracle_anonymizer(), False, ss["less_own"], monkeypatch)
    assert got == exp and got != table_only


def test_two_ranks_get_one_panel(tmp_path, monkeypatch):
    """Mode normal on two gloo ranks: the variables are inherited, each rank discovers the sequences dealt to
    it under the rule and every rank masks with the same panel — the files are one process's, which are the
    plain run's on X'."""
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    ss = _check_not_vacuous("fuzz3000", Q20N)
    set_option(monkeypatch, True)
    R.set_rule(monkeypatch, Q20N)
    got = _two_ranks("fuzz3000", str(tmp_path / "two"))
    set_option(monkeypatch, False)
    R.set_rule(monkeypatch, None)
    assert len(got) == 7
    assert got == K.run_files("fuzz3000", str(tmp_path / "xp"), H.oracle_anonymizer(), False, ss["less_own"], monkeypatch)


def test_discover_takes_a_rule_and_logs_settings_and_counts_only(hand, caplog, monkeypatch):
    from genomeanonymizer_amd.discover_sites import discover, rule_default
    R.set_rule(monkeypatch, None)
    assert rule_default() == R.site_rule(R.ZERO)
    for rule in (R.FULL, R.FULL_NORMAL):
        with caplog.at_level(logging.INFO):
            p = discover(hand["plain"]["T"], hand["plain"]["N"], hand["fasta"], 2, rule=R.site_rule(rule))
        assert D.panel_as_dict(p) == R.expected_hand(rule)
    assert "min base quality 20" in caplog.text and "min mapq 30" in caplog.text and "0x700" in caplog.text
    assert "rule normal" in caplog.text and "rule both" in caplog.text
    # the environment defaults, read by discover itself
    R.set_rule(monkeypatch, R.FULL_NORMAL)
    assert rule_default() == R.site_rule(R.FULL_NORMAL)
    p = discover(hand["indexed"]["T"], hand["indexed"]["N"], hand["fasta"], 2)
    assert D.panel_as_dict(p) == R.expected_indexed(R.FULL_NORMAL)
    monkeypatch.setenv("GANON_DISCOVER_EXCLUDE_FLAGS", "0x700")
    assert rule_default().exclude_flags == 0x700
    for env, v in (("GANON_DISCOVER_MIN_BASE_QUALITY", "94"), ("GANON_DISCOVER_MIN_MAPQ", "256"),
                   ("GANON_DISCOVER_EXCLUDE_FLAGS", "65536"), ("GANON_DISCOVER_RULE", "tumor"),
                   ("GANON_DISCOVER_MIN_MAPQ", "x")):
        R.set_rule(monkeypatch, None)
        monkeypatch.setenv(env, v)
        with pytest.raises(ValueError):
            rule_default()


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
    monkeypatch.setenv("GANON_MASK_SA_CLIPS", "0")
    monkeypatch.setenv("GANON_DISCOVER_SITES", "0")     # (the flags write these: restored afterwards)
    for env in R.ENVS:
        monkeypatch.setenv(env, "")
    return ga


def _listing(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


FLAGS = (["--discover_min_base_quality", "20"], ["--discover_min_mapq", "30"], ["--discover_exclude_flags", "0x400"],
         ["--discover_rule", "normal"], ["--discover_rule", "both"], ["--discover_min_base_quality", "0"])


def test_cli_parses_the_flags(cli):
    base = ["-d", "x", "-s", "s", "-r", "r"]
    c = cli.exec_parser(base)
    assert (c.discover_min_base_quality, c.discover_min_mapq, c.discover_exclude_flags, c.discover_rule) == (None,) * 4
    c = cli.exec_parser(base + ["--discover_min_base_quality", "93", "--discover_min_mapq", "255",
                                "--discover_exclude_flags", "0xFFFF", "--discover_rule", "normal"])
    assert (c.discover_min_base_quality, c.discover_min_mapq, c.discover_exclude_flags, c.discover_rule) == (93, 255, 65535, "normal")
    assert cli.exec_parser(base + ["--discover_exclude_flags", "1796"]).discover_exclude_flags == 1796
    for bad in (["--discover_min_base_quality", "94"], ["--discover_min_base_quality", "-1"], ["--discover_min_mapq", "256"],
                ["--discover_exclude_flags", "65536"], ["--discover_exclude_flags", "0x10000"], ["--discover_rule", "tumor"],
                ["--discover_min_mapq", "q"]):
        with pytest.raises(SystemExit):
            cli.exec_parser(base + bad)


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "_".join(f).strip("-"))
def test_cli_flag_without_discover_sites_is_an_error_before_any_output(cli, flags, tmp_path, caplog):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    before = _listing(d)
    for extra in (flags, flags + ["--no-discover_sites"]):
        with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as e:
            _cli(cli, d, paths, extra)
        assert e.value.code == 1 and "needs --discover_sites" in caplog.text
        assert _listing(d) == before
    # out of range: an error as well, with --discover_sites on
    with pytest.raises(SystemExit):
        _cli(cli, d, paths, ["--discover_sites", "--discover_min_base_quality", "94"])
    assert _listing(d) == before


def test_environment_default_without_discover_sites_is_an_error_too(cli, tmp_path, monkeypatch, caplog):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    before = _listing(d)
    for env, v in (("GANON_DISCOVER_MIN_BASE_QUALITY", "20"), ("GANON_DISCOVER_RULE", "normal"),
                   ("GANON_DISCOVER_MIN_MAPQ", "999")):
        R.set_rule(monkeypatch, None)
        monkeypatch.setenv(env, v)
        with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as e:
            _cli(cli, d, paths)
        assert e.value.code == 1 and _listing(d) == before
    # ... an out-of-range default is one with the option on
    monkeypatch.setenv("GANON_DISCOVER_SITES", "1")
    with pytest.raises(SystemExit):
        _cli(cli, d, paths)
    assert _listing(d) == before


def test_cli_flags_and_environment_defaults_run_the_rule(cli, tmp_path, monkeypatch, caplog):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    ss = _check_not_vacuous("tiny", Q20N)
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    with caplog.at_level(logging.INFO):
        _cli(cli, d, paths, ["--discover_sites", "--discover_min_base_quality", "20", "--discover_rule", "normal"])
    got = H.collect(paths)
    assert os.environ["GANON_DISCOVER_MIN_BASE_QUALITY"] == "20" and os.environ["GANON_DISCOVER_RULE"] == "normal"
    assert "min base quality 20" in caplog.text and "rule normal" in caplog.text
    # the environment defaults behave like the flags
    d2 = str(tmp_path / "env")
    paths2 = generate(scenario("tiny"), d2)
    R.set_rule(monkeypatch, Q20N)
    monkeypatch.setenv("GANON_DISCOVER_SITES", "1")
    _cli(cli, d2, paths2)
    assert H.collect(paths2) == got
    # ... and a flag goes over its default
    d3 = str(tmp_path / "over")
    paths3 = generate(scenario("tiny"), d3)
    monkeypatch.setenv("GANON_DISCOVER_RULE", "both")
    monkeypatch.setenv("GANON_DISCOVER_MIN_BASE_QUALITY", "0")
    _cli(cli, d3, paths3, ["--discover_min_base_quality", "20", "--discover_rule", "normal"])
    assert H.collect(paths3) == got
    monkeypatch.setenv("GANON_DISCOVER_SITES", "0")
    R.set_rule(monkeypatch, None)
    exp = K.run_files("tiny", str(tmp_path / "xp"), H.oracle_anonymizer(), False, ss["less_own"], monkeypatch)
    assert got == exp and len(got) == 7 and got != M.golden_files("tiny")
