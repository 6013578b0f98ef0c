"""--compress_output / GANON_COMPRESS_OUTPUT=1 on the CPU: the product pipeline with the oracle
engine and native.ZlibDeflater (the deflater of a run whose engine is not the GPU's). The
decompressed files must equal, byte for byte, the plain files of the same run — the reference's
(tests/golden) — for the whole-sample path, the streamed path, several jobs per contig, and two
ranks; no plain file and no spool may be left. tests/test_gpu_deflate.py repeats it on the device."""
import gzip
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import deflate_fixtures as F
from test_distributed import _free_port, _worker


def _anon():
    from pyoracle import OracleEngine
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(engine=OracleEngine())


def test_zlib_deflater_members():
    from genomeanonymizer_amd import native
    z = native.ZlibDeflater()
    blocks = [b for _, b in F.fixture_blocks()]
    for b in blocks[:6] + blocks[-2:]:
        stream, sizes = z.bgzf(b)
        F.check_members(stream.tobytes(), [b])
        assert sizes.tolist() == [len(stream)]
    text = F.golden_text("edge")
    parts = [text[:1000], np.frombuffer(text[1000:70000], np.uint8), text[70000:]]
    stream, sizes = z.bgzf(parts)
    assert len(sizes) == -(-len(text) // F.MAX_IN) and int(sizes.sum()) == len(stream)
    F.check_members(stream.tobytes(), [text[i:i + F.MAX_IN] for i in range(0, len(text), F.MAX_IN)])
    stream, sizes = z.bgzf(b"")
    assert len(stream) == 0 and len(sizes) == 0
    z.close()
    assert native.BGZF_EOF == F.EOF_MEMBER
    assert isinstance(native.deflater_for(object(), 0), native.ZlibDeflater)


@pytest.mark.parametrize("mode", ["streamed", "whole_sample", "jobs"])
@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz2003"])
def test_compressed_outputs_match_reference(name, mode, tmp_path, monkeypatch):
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    monkeypatch.setenv("GANON_WHOLE_SAMPLE", "1" if mode == "whole_sample" else "0")
    if mode == "jobs":     # several jobs per contig, and the tail: each starts new members
        monkeypatch.setenv("GANON_JOB_BP", "2500")
    paths, t_out, n_out = F.run_compressed(name, str(tmp_path / name), _anon(), bam_index=mode == "jobs")
    n = F.check_compressed_outputs(name, paths, t_out, n_out)
    if mode == "jobs":
        text = sum(len(gzip.open(p).read()) for p in (f"{t_out}.1.fastq.gz", f"{n_out}.1.fastq.gz",
                                                      f"{t_out}.2.fastq.gz", f"{n_out}.2.fastq.gz"))
        assert n > -(-text // F.MAX_IN) + 4          # more members than one stream per file would have


def test_option_off_writes_plain_files(tmp_path, monkeypatch):
    from helpers import run_pipeline_vs_golden
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "0")
    monkeypatch.setenv("GANON_WHOLE_SAMPLE", "0")
    assert run_pipeline_vs_golden("tiny", str(tmp_path / "tiny"), _anon()) == {}
    assert [f for f in os.listdir(tmp_path / "tiny" / "in") if f.endswith(".gz") or "spool" in f] == []


def _spawn(name, workdir, world, **kw):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, workdir, q, "oracle"), kwargs=kw)
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    alive = [p.is_alive() for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert alive == [False] * world
    return [p.exitcode for p in procs]


@pytest.mark.parametrize("name", ["edge", "fuzz3000"])
def test_two_ranks_compressed(name, tmp_path, monkeypatch):
    """Two gloo ranks (the environment variable reaches the spawned children): every rank's spool
    segments land at the prefix sums of the gathered compressed lengths."""
    from genomeanonymizer_amd.short_read_tumor_normal_anonymizer import name_output
    from genomeanonymizer_amd.synth.generate import generate, scenario
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    workdir = str(tmp_path / name)
    paths = generate(scenario(name), os.path.join(workdir, "in"))
    assert _spawn(name, workdir, 2) == [0, 0]
    F.check_compressed_outputs(name, paths, name_output(paths["T"]), name_output(paths["N"]))


def test_failing_rank_leaves_no_spool(tmp_path, monkeypatch):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    workdir = str(tmp_path / "tiny")
    generate(scenario("tiny"), os.path.join(workdir, "in"))
    codes = _spawn("tiny", workdir, 2, fail_rank=1, fail_stage="job")
    assert all(c != 0 for c in codes)
    assert [f for f in os.listdir(os.path.join(workdir, "in")) if "spool" in f] == []


def test_cli_flag(tmp_path, monkeypatch):
    """The flag parses (a BooleanOptionalAction); --no-compress_output overrides the environment's
    default and gives plain files, --compress_output gives .fastq.gz (the CLI's anonymizer replaced
    by the oracle engine's: no GPU here)."""
    from genomeanonymizer_amd import genome_anonymizer as ga
    from genomeanonymizer_amd import writer
    from genomeanonymizer_amd.synth.generate import generate, scenario
    base = ["-d", "x", "-s", "s", "-r", "r"]
    assert ga.exec_parser(base).compress_output is None
    assert ga.exec_parser(base + ["--compress_output"]).compress_output is True
    assert ga.exec_parser(base + ["--no-compress_output"]).compress_output is False
    monkeypatch.setattr(ga, "CompleteGermlineAnonymizer", lambda device=0: _anon())
    monkeypatch.setattr(writer, "io_block_size", lambda d: 4096)
    monkeypatch.setenv("GANON_WHOLE_SAMPLE", "0")
    for flag, env in (("--no-compress_output", "1"), ("--compress_output", "0")):
        monkeypatch.setenv("GANON_COMPRESS_OUTPUT", env)
        d = str(tmp_path / flag.strip("-"))
        paths = generate(scenario("tiny"), d)
        ga.run_anonymizer(["-d", d, "-s", "samples.tsv", "-r", paths["ref"], "--record_statistics", flag])
        pre = {"tumor": os.path.join(d, "tumor.anonymized"), "normal": os.path.join(d, "normal.anonymized")}
        if flag == "--compress_output":
            F.check_compressed_outputs("tiny", paths, pre["tumor"], pre["normal"])
        else:
            for tag in pre:
                for suf in (".1.fastq", ".2.fastq"):
                    gp = os.path.join(F.REPO, "tests", "golden", "tiny", f"{tag}{suf}.gz")
                    assert open(pre[tag] + suf, "rb").read() == gzip.open(gp).read()
                    assert not os.path.exists(pre[tag] + suf + ".gz")
