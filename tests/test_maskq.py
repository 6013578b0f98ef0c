"""--masked_base_quality / GANON_MASKED_BASE_QUALITY=Q on the CPU: the host formatter
``ganon_fastq_format_mq`` against a numpy restatement of the definition, and the product pipeline
with the oracle engine against the files the reference writes with its own quality hook switched on
(tests/golden/maskq2, tools/make_maskq_golden.py: ``mask_or_modify_base_pair(..., modify_qualities=
True, new_quality=2)``). The hooked reference cannot finish fuzz2000 and fuzz2003 (it writes into a
record it formatted once already: ``'reversed' object does not support item assignment``); there the
definition holds and invariants are checked. tests/test_gpu_maskq.py repeats it on the device."""
import gzip
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import maskq_helpers as M
from test_distributed import _free_port, _worker

SCENARIOS = ["tiny", "edge", "fuzz9", "fuzz1001", "fuzz3000", "long1"]


def _anon():
    from pyoracle import OracleEngine
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(engine=OracleEngine())


# ---- the formatter -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def crafted():
    """quality -> (records, plain bytes, restated bytes); the plain bytes are formatted once."""
    from genomeanonymizer_amd import native
    out = {}
    plain = None
    for q in (0, 2, 93):
        recs = M.crafted_records(q)
        if plain is None:
            plain = native.host_format_fastq(M.plain_of(recs))
        out[q] = (recs, plain, M.restate(recs, plain))
    return out


@pytest.mark.parametrize("q", [0, 2, 93])
def test_host_formatter_matches_restatement(crafted, q):
    from genomeanonymizer_amd import native
    recs, plain, exp = crafted[q]
    got = native.host_format_fastq(recs)
    assert len(got) == len(plain)
    assert got == exp
    assert got != plain
    assert set(recs["seq_len"].tolist()) >= set(M.LENGTHS)


def test_shared_quality_range_shows_each_mask_alone(crafted):
    """The last two crafted records print the same quality bytes; one is masked at its first base
    (forward: text index 0), the other at its last (reverse: text index 0 as well, but of its own
    line) — each line differs from the shared qualities only where its own record is masked."""
    from genomeanonymizer_amd import native
    recs, plain, _ = crafted[2]
    got = native.host_format_fastq(recs).split(b"\n")
    base = plain.split(b"\n")
    assert recs["qual_off"][-1] == recs["qual_off"][-2]
    qa, qb = got[-6], got[-2]
    assert base[-6] == base[-2]
    diff = lambda x, y: [i for i, (a, b) in enumerate(zip(x, y)) if a != b]
    assert diff(qa, base[-6]) == [0] and qa[0:1] == b"#"
    assert diff(qb, base[-2]) == [0] and qb[0:1] == b"#"     # reverse, masked at p = L-1: printed first
    assert recs["reverse"][-1] == 1 and recs["_truth"][-1] == [149] and recs["_truth"][-2] == [0]


def test_no_original_is_the_plain_formatter(crafted):
    """The new binding with selector 255 everywhere: ganon_fastq_format's bytes."""
    from genomeanonymizer_amd import native
    recs, plain, _ = crafted[2]
    n = len(recs["seq_len"])
    off = dict(recs, orig_sel=np.full(n, 255, np.uint8))
    a = native._fastq_args(off)
    out = native._new_bytes(None, len(plain))
    w = native.host_lib().ganon_fastq_format_mq(*a, off["orig_sel"].ctypes.data_as(native._u8p),
                                                off["orig_nib_off"].ctypes.data_as(native._i64p), 2, out, len(plain))
    assert w == len(plain) and out == plain
    assert native.host_format_fastq(off) == plain
    assert native.host_lib().ganon_fastq_format_mq(*a, off["orig_sel"].ctypes.data_as(native._u8p),
                                                   off["orig_nib_off"].ctypes.data_as(native._i64p), 94, out,
                                                   len(plain)) == native.FASTQ_FAILED


# ---- the goldens ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENARIOS)
def test_goldens_differ_only_in_quality_lines(name):
    changed = M.quality_diff(M.golden_files(name), M.golden_files(name, M.MASKQ_GOLDEN), qc=None)
    assert changed > 0


# ---- the pipeline --------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", SCENARIOS)
def test_pipeline_matches_hooked_reference(name, mode, tmp_path, monkeypatch):
    index = M.set_mode(monkeypatch, mode)
    assert M.run_vs_maskq_golden(name, str(tmp_path / name), _anon(), bam_index=index) == {}


@pytest.mark.parametrize("name", ["fuzz2000", "fuzz2003"])
def test_scenarios_without_a_reference_answer(name, tmp_path, monkeypatch):
    """Equal to the plain goldens outside the quality lines, every changed character '#', at least
    one changed, the three modes and the two object replays agree."""
    plain = M.golden_files(name)
    runs = {}
    for mode in M.MODES:
        index = M.set_mode(monkeypatch, mode)
        runs[mode] = M.run_pipeline_files(name, str(tmp_path / mode), _anon(), bam_index=index)
        assert M.quality_diff(plain, runs[mode]) > 0, mode
    assert runs["streamed"] == runs["whole"] == runs["jobs"]
    M.set_mode(monkeypatch, "streamed")
    monkeypatch.setenv("GANON_OBJECTS", "python")
    assert M.run_pipeline_files(name, str(tmp_path / "py"), _anon()) == runs["streamed"]


@pytest.mark.parametrize("name", ["fuzz1001", "fuzz3000"])
def test_python_object_replay_matches_hooked_reference(name, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed")
    monkeypatch.setenv("GANON_OBJECTS", "python")
    assert M.run_vs_maskq_golden(name, str(tmp_path / name), _anon()) == {}


@pytest.mark.parametrize("name", ["edge", "fuzz3000"])
def test_two_ranks(name, tmp_path, monkeypatch):
    """Two gloo ranks (the variable reaches the spawned children; the objects' packed ingredients
    travel between them): the files are the hooked reference's."""
    from genomeanonymizer_amd.short_read_tumor_normal_anonymizer import name_output
    from genomeanonymizer_amd.synth.generate import generate, scenario
    monkeypatch.setenv("GANON_MASKED_BASE_QUALITY", str(M.MASKQ_Q))
    workdir = str(tmp_path / name)
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
    exp = M.golden_files(name, M.MASKQ_GOLDEN)
    for tag, pre in (("tumor", name_output(paths["T"])), ("normal", name_output(paths["N"]))):
        for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
            if tag + suf in exp:
                assert open(pre + suf, "rb").read() == exp[tag + suf], tag + suf
    assert open(paths["N"] + ".statistics.txt", "rb").read() == exp["statistics"]


def test_compress_output_composes(tmp_path, monkeypatch):
    import deflate_fixtures as F
    M.set_mode(monkeypatch, "streamed")
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    paths, t_out, n_out = F.run_compressed("tiny", str(tmp_path / "tiny"), _anon())
    exp = M.golden_files("tiny", M.MASKQ_GOLDEN)
    for tag, pre in (("tumor", t_out), ("normal", n_out)):
        for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
            assert not os.path.exists(pre + suf)
            assert gzip.open(pre + suf + ".gz").read() == exp[tag + suf], tag + suf


# ---- the command line ----------------------------------------------------------------------------

def test_cli_flag(tmp_path, monkeypatch):
    from genomeanonymizer_amd import genome_anonymizer as ga
    from genomeanonymizer_amd import native, writer
    from genomeanonymizer_amd.synth.generate import generate, scenario
    base = ["-d", "x", "-s", "s", "-r", "r"]
    assert ga.exec_parser(base).masked_base_quality is None
    assert ga.exec_parser(base + ["--masked_base_quality", "2"]).masked_base_quality == 2
    assert ga.exec_parser(base + ["--masked_base_quality", "93"]).masked_base_quality == 93
    for bad in ("94", "-1", "x"):
        with pytest.raises(SystemExit):
            ga.exec_parser(base + ["--masked_base_quality", bad])
    monkeypatch.setattr(ga, "CompleteGermlineAnonymizer", lambda device=0: _anon())
    monkeypatch.setattr(writer, "io_block_size", lambda d: 4096)
    monkeypatch.setenv("GANON_WHOLE_SAMPLE", "0")
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "0")
    for flag, root in ((["--masked_base_quality", "2"], M.MASKQ_GOLDEN), ([], M.helpers.GOLDEN)):
        monkeypatch.setenv("GANON_MASKED_BASE_QUALITY", "")      # unset or empty: off (and restored afterwards)
        assert native.masked_base_quality_default() is None
        d = str(tmp_path / ("on" if flag else "off"))
        paths = generate(scenario("tiny"), d)
        ga.run_anonymizer(["-d", d, "-s", "samples.tsv", "-r", paths["ref"], "--record_statistics"] + flag)
        assert os.environ["GANON_MASKED_BASE_QUALITY"] == ("2" if flag else "")
        exp = M.golden_files("tiny", root)
        for tag in ("tumor", "normal"):
            for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
                assert open(os.path.join(d, f"{tag}.anonymized{suf}"), "rb").read() == exp[tag + suf], (flag, tag + suf)


def test_environment_value_is_validated(monkeypatch):
    from genomeanonymizer_amd import native
    monkeypatch.delenv("GANON_MASKED_BASE_QUALITY", raising=False)
    assert native.masked_base_quality_default() is None
    monkeypatch.setenv("GANON_MASKED_BASE_QUALITY", "93")
    assert native.masked_base_quality_default() == 93
    monkeypatch.setenv("GANON_MASKED_BASE_QUALITY", "94")
    with pytest.raises(native.GanonError):
        native.masked_base_quality_default()
