"""--mask_sa_clips / GANON_MASK_SA_CLIPS on the CPU: with a site table, the soft-clipped bases of a record
are masked along the alignments its SA:Z tag names (csrc/ganon_sa_clips.h). Every expectation
comes from the plain-Python restatement of the rule in sa_clips_helpers. The host decoder against the
rule on the hand-built stream of its corners (1 and 3 threads, with and without a quality); the command
line; the defining property — a run with the option and a table on inputs X writes the files a run
without either writes on X″ (X with §4i's rule and then this rule applied to every record) — in
streamed, whole-sample and job mode, with each of the other options and on two gloo ranks.
tests/test_gpu_sa_clips.py repeats it on the device."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
import sa_clips_helpers as S
from test_distributed import _free_port, _worker


# ---- the host decoder on the hand-built stream ------------------------------------------------------------

@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    recs, sites, notes = S.hand_built()
    stream, _ = S.stream_of(recs)
    path = str(tmp_path_factory.mktemp("hand") / "hand.bam")
    write_bgzf(path, stream.tobytes())
    return {"recs": recs, "sites": sites, "notes": notes, "path": path, "plain": ReadTable(path)}


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("quality", [None, 7])
def test_host_columns_match_the_rule(hand, quality, threads):
    from genomeanonymizer_amd.io.bam import ReadTable
    plain, sites = hand["plain"], hand["sites"]
    assert plain.n == S.HAND_RECORDS
    got = ReadTable(hand["path"], threads=threads, known_sites=S.table_of(sites, plain.ref_names, quality))
    n_ks, n_sa, n_ign = S.assert_masked_table(got, plain, sites, quality)
    assert n_sa >= S.MIN_HAND_REWRITTEN and n_ign == S.N_IGNORED
    assert (got.known_masked, got.sa_masked, got.sa_ignored) == (n_ks, n_sa, n_ign)
    # ... and the table rule is the record rule
    exp, tot = S.expected_of(hand["recs"], sites, quality=quality)
    assert tot == (n_ks, n_sa, n_ign)
    for i, (nib, qual) in enumerate(exp):
        assert K.table_nibbles(got, i) == nib, i
        o = int(got.qual_off[i])
        assert np.asarray(got.qual[o:o + len(qual)]).tolist() == qual, i


def test_hand_built_literals(hand):
    """What the cases are there for, spelled out: the literals pin the Python rule independently of the
    code under test, and the host decoder's bases of the same records are held to them too."""
    from genomeanonymizer_amd.io.bam import ReadTable
    recs, notes = hand["recs"], hand["notes"]
    exp, _ = S.expected_of(recs, hand["sites"], quality=7)
    got = ReadTable(hand["path"], threads=2, known_sites=S.table_of(hand["sites"], hand["plain"].ref_names, 7))
    for note, i in notes.items():
        assert K.table_nibbles(got, i) == exp[i][0], note
        o = int(got.qual_off[i])
        assert np.asarray(got.qual[o:o + len(exp[i][1])]).tolist() == exp[i][1], note

    def changed(note):
        i = notes[note]
        a, (b, _) = recs[i]["nib"], exp[i]
        return {x: (a[x], b[x]) for x in range(len(a)) if a[x] != b[x]}

    def q_changed(note):
        i = notes[note]
        return [x for x in range(len(recs[i]["qual"])) if recs[i]["qual"][x] != exp[i][1][x]]
    assert changed("trailing") == {20: (2, 1), 34: (2, 1)}            # r0 and r0 + len - 1; r0 - 1, r0 + len: no base
    assert changed("leading") == {0: (2, 1), 5: (2, 1)}               # another ALT, REF, N and M stay
    assert changed("opposite_even") == {29: (4, 8), 26: (4, 8), 20: (4, 8)}
    assert changed("opposite_odd") == {30: (4, 8), 27: (4, 8), 20: (4, 8)}
    assert changed("rev_same") == {25: (2, 1)} and changed("rev_opposite") == {24: (4, 8)}
    assert changed("one_base") == {30: (2, 1)}
    shared = changed("shared_byte")
    assert set(shared) == {20, 21} and shared[21] == (2, 1) and shared[20][1] == 1     # §4i's base and the clip's
    assert changed("structured") == {x: (2, 1) for x in (29, 30, 34, 38, 49)}          # 410, 411: in the D; 35..37: the I
    assert changed("overlap") == {20: (2, 1)}                         # index 15 is aligned in the record: it stays
    assert changed("own_hard") == {0: (2, 1), 9: (2, 1)}              # the leading H offsets the index
    assert changed("order_ab") == {25: (2, 4)} and changed("order_ba") == {25: (2, 1)}
    assert changed("other_tid") == {20: (2, 1), 29: (2, 1)}
    for k in range(S.N_IGNORED):                                      # skipped whole; the used entry goes on
        assert len(changed(f"malformed{k}")) == 1, k
    assert changed("empty_pieces") == {20: (2, 1)}
    for note in ("tags_before", "tags_after", "type_a_then_z", "second_sa"):
        assert len(changed(note)) == 1, note
    for note in ("type_a_only", "no_nul", "bad_tag_first", "empty_aux", "unmapped", "no_bases", "no_cigar", "no_clip",
                 "hard_only"):
        assert changed(note) == {} and q_changed(note) == [], note
    assert len(changed("qual_ff")) == 10 and q_changed("qual_ff") == []
    assert len(changed("qual_ff_first")) == 10 and q_changed("qual_ff_first") == []
    assert q_changed("trailing") == [20, 34] and exp[notes["trailing"]][1][20] == 7


def test_table_without_sites_walks_nothing(hand):
    """Host and device agree on an empty table: no base changes and no entry is counted."""
    from genomeanonymizer_amd.io.bam import ReadTable
    plain = hand["plain"]
    got = ReadTable(hand["path"], threads=2, known_sites=S.table_of(K.Sites({}), plain.ref_names, 7))
    assert K.assert_masked_table(got, plain, K.Sites({}), 7) == 0
    assert (got.known_masked, got.sa_masked, got.sa_ignored) == (0, 0, 0)


def test_option_off_decodes_as_the_table_alone(hand):
    from genomeanonymizer_amd.io.bam import ReadTable
    plain, sites = hand["plain"], hand["sites"]
    for table in (K.table_of(sites, plain.ref_names, 7), S.table_of(sites, plain.ref_names, 7, sa_clips=False)):
        got = ReadTable(hand["path"], threads=2, known_sites=table)
        total = K.assert_masked_table(got, plain, sites, 7)
        assert (got.known_masked, got.sa_masked, got.sa_ignored) == (total, 0, 0)


def test_names_are_checked():
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.known_sites import SitesTable, sorted_names
    blob, off, tid = sorted_names(["c1", "c", "c12", "c1", "b"])
    assert blob == b"bcc1c12" and off.tolist() == [0, 1, 2, 4, 7] and tid.tolist() == [4, 1, 0, 2]
    z = np.zeros(0, np.int32)
    with pytest.raises(native.GanonError):      # the names of another header
        SitesTable(np.zeros(3, np.int64), z, z.astype(np.uint8), -1, ["c1"], True)
    lib = native.host_lib()
    t = K.table_of(K.Sites({"c1": {5: (1, 2)}}), ["c1", "c2"])
    h = t.handle
    i64, i32 = native._i64p, native._i32p
    bad = [(b"c2c1", [0, 2, 4], [1, 0]),       # not sorted
           (b"c1c1", [0, 2, 4], [0, 1]),       # not distinct
           (b"c1c2", [0, 2, 4], [0, 2])]       # a sequence id outside the table
    for names, o, ti in bad:
        o, ti = np.array(o, np.int64), np.array(ti, np.int32)
        assert lib.ganon_sites_set_sa_clips(h, 2, names, native._ptr(o, i64), native._ptr(ti, i32), 1) != 0


# ---- the command line ------------------------------------------------------------------------------------

def test_cli_option_without_a_table_ends_before_any_output(tmp_path, monkeypatch):
    from genomeanonymizer_amd import genome_anonymizer as ga
    from genomeanonymizer_amd.synth.generate import generate, scenario
    base = ["-d", "x", "-s", "s", "-r", "r"]
    assert ga.exec_parser(base).mask_sa_clips is None
    assert ga.exec_parser(base + ["--mask_sa_clips"]).mask_sa_clips is True
    assert ga.exec_parser(base + ["--no-mask_sa_clips"]).mask_sa_clips is False
    monkeypatch.setattr(ga, "CompleteGermlineAnonymizer", lambda device=0: H.oracle_anonymizer())
    for var in ("GANON_KNOWN_SITES", "GANON_DISCOVER_SITES", "GANON_MASK_SA_CLIPS"):
        monkeypatch.setenv(var, "")     # (the flags write them: restored afterwards)
    d = str(tmp_path / "cli")
    paths = generate(scenario("tiny"), d)
    before = sorted(os.listdir(d))
    args = ["-d", d, "-s", "samples.tsv", "-r", paths["ref"], "--record_statistics", "-v", "1"]
    for extra, env in ((["--mask_sa_clips"], ""), ([], "1")):
        monkeypatch.setenv("GANON_MASK_SA_CLIPS", env)
        with pytest.raises(SystemExit) as e:
            ga.run_anonymizer(args + extra)
        assert e.value.code == 1 and sorted(os.listdir(d)) == before


# ---- the pipeline: X with the option and a table against X″ without either ------------------------------------

SCENARIOS = ["fuzz1001", "fuzz2000", "fuzz3000"]


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenarios_have_clip_bases_to_mask(name, tmp_path, monkeypatch):
    """X″ differs from X′ in at least MIN_CHANGED clip bases (a condition on the inputs), and the host
    decoder of X with the table and the option counts exactly the bases the generator-side rule rewrote."""
    from genomeanonymizer_amd.io.bam import ReadTable
    sp = S.scenario_sa_panel(name)
    paths = S.make_inputs(name, str(tmp_path / "in"), False, sp["sites"], monkeypatch)
    print(name, "sites added", sp["added"], "bases rewritten (4i, SA)", paths["_changed"])
    assert paths["_changed"][1] >= S.MIN_CHANGED
    n_ks = n_sa = 0
    for s in ("T", "N"):
        x = sp["plain_inputs"][s]
        names = ReadTable(x, threads=1).ref_names
        t = ReadTable(x, threads=2, known_sites=S.table_of(sp["sites"], names))
        n_ks, n_sa = n_ks + t.known_masked, n_sa + t.sa_masked
    assert (n_ks, n_sa) == paths["_changed"]


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", SCENARIOS)
def test_option_equals_plain_run_on_rewritten_inputs(name, mode, tmp_path, monkeypatch):
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    S.assert_option_equals_plain_on_rewritten(name, tmp_path, monkeypatch, H.oracle_anonymizer, index)


def test_discover_sites_alone_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    S.assert_option_equals_plain_on_rewritten("fuzz2000", tmp_path, monkeypatch, H.oracle_anonymizer, discover=True)


def test_masked_base_quality_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "jobs", 2)
    H.set_option(monkeypatch, False)
    S.assert_option_equals_plain_on_rewritten("fuzz2000", tmp_path, monkeypatch, H.oracle_anonymizer, True, quality=2)


def test_hash_read_names_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, H.KEY)
    got = S.assert_option_equals_plain_on_rewritten("fuzz3000", tmp_path, monkeypatch, H.oracle_anonymizer)
    assert all(len(n) == 32 for n, _, _, _ in H.fastq_records(got["tumor.1.fastq"]))


def test_compress_output_composes(tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    S.assert_option_equals_plain_on_rewritten("fuzz1001", tmp_path, monkeypatch, H.oracle_anonymizer, gz=True)


# ---- two gloo ranks --------------------------------------------------------------------------------------

def test_two_ranks_equal_one_process(tmp_path, monkeypatch):
    """Each rank inherits the variables and builds its tables itself: two ranks write one process's files."""
    from genomeanonymizer_amd.synth.generate import generate, scenario
    name = "fuzz3000"
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, S.scenario_sa_panel(name)["vcf"])
    S.set_option(monkeypatch, True)
    workdir = str(tmp_path / "two")
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
    got = H.collect(paths)
    exp = S.run_files(name, str(tmp_path / "one"), H.oracle_anonymizer())
    assert got == exp and len(exp) == 7
    S.set_option(monkeypatch, False)
    assert got != S.run_files(name, str(tmp_path / "off"), H.oracle_anonymizer())
