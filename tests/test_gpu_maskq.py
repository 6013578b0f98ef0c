"""--masked_base_quality on the device: k_fq_maskq (csrc/ganon_fastq.hip), the post-pass over the
formatter's output, against the numpy restatement and the host formatter on crafted records (host
buffers and a resident batch, formatter instances 0 and 12), and the product pipeline on the GPU
against the hooked reference's files (tests/golden/maskq2). tests/test_maskq.py is the CPU side."""
import gzip
import os

import numpy as np
import pytest

import maskq_helpers as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, 12], ids=["span3", "rows"])
def masker(hip_built, request):
    from genomeanonymizer_amd import native
    m = native.HipMasker(0)
    m.set_param(native.PARAM_FASTQ_KD, request.param)
    yield m
    m.close()


@pytest.fixture(scope="module")
def crafted():
    from genomeanonymizer_amd import native
    recs = M.crafted_records(M.MASKQ_Q)
    plain = native.host_format_fastq(M.plain_of(recs))
    return recs, plain, M.restate(recs, plain)


def test_crafted_records_from_host_buffers(masker, crafted):
    """The one-shot entry point and the handle path (upload, set, run twice, download): the 70,001-base
    and 255-character-name records make quality fields straddle 8 KiB tiles."""
    from genomeanonymizer_amd import native
    recs, plain, exp = crafted
    assert exp != plain
    assert native.host_format_fastq(recs) == exp
    assert masker.format_fastq(recs) == exp
    assert masker.format_fastq(M.plain_of(recs)) == plain
    f = masker.fastq_upload(recs)
    try:
        for _ in range(2):
            f.run()
            assert f.download() == exp
    finally:
        f.free()
    for q in (0, 93):
        r = dict(recs, maskq=q)
        assert masker.format_fastq(r) == M.restate(r, plain)


def test_crafted_records_from_a_resident_batch(masker, crafted):
    """The crafted set read in place from a small uploaded batch: its three buffers ride behind the
    batch's reads in the sequence blob (no read covers them, so the run copies them to the masked
    output unchanged); the copies are read from the batch's output, the originals from its input."""
    from genomeanonymizer_amd.synth.batch import config2_batch
    recs, plain, exp = crafted
    arr, _ = config2_batch(n_reads=2_000, genome=1_000_000, seed=3)
    bufs = recs["seq_bufs"]
    base = np.cumsum([len(arr["seq_nt16"])] + [len(b) for b in bufs[:-1]]).astype(np.int64)
    arr = dict(arr, seq_nt16=np.concatenate([arr["seq_nt16"]] + bufs))
    osel = recs["orig_sel"]
    r = dict(recs, seq_sel=np.zeros(len(osel), np.uint8), seq_nib_off=recs["seq_nib_off"] + 2 * base[0],
             orig_sel=np.where(osel == 255, 255, 1).astype(np.uint8),
             orig_nib_off=recs["orig_nib_off"] + np.where(osel == 255, 0, 2 * base[np.minimum(osel, 2)]))
    db = masker.upload(arr)
    try:
        db.run()
        f = masker.fastq_upload(r, seq_batch=db)
        try:
            f.run()
            assert f.download() == exp
        finally:
            f.free()
    finally:
        db.free()


def test_records_from_a_resident_batch(masker):
    """A small masked batch on the device: every read's masked copy (buffer 0) against its input
    (buffer 1) at the read's own offset, as the product formats a job; some records without an
    original, some unmasked ones, and some whose original is another read's bases (a difference at
    most positions, another offset than the copy's)."""
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.batch import config2_batch
    from genomeanonymizer_amd.synth.fastq import fastq_records
    arr, _ = config2_batch(n_reads=20_000, genome=6_000_000, seed=5)
    db = masker.upload(arr)
    try:
        db.run()
        out, _, _, _ = db.download()
        recs = fastq_records(arr, seed=5)
        n = len(recs["seq_len"])
        i = np.arange(n)
        recs["seq_sel"] = (i % 7 == 3).astype(np.uint8)                 # 1: the unmasked input
        recs["orig_sel"] = np.where(i % 11 == 5, 255, 1).astype(np.uint8)
        off = recs["seq_nib_off"].copy()
        nxt = np.roll(np.arange(n), -1)
        other = (i % 101 == 7) & (recs["seq_len"][nxt] == recs["seq_len"])
        off[other] = recs["seq_nib_off"][nxt][other]
        recs["orig_nib_off"] = off
        recs["maskq"] = M.MASKQ_Q
        host = dict(recs, seq_bufs=[out, arr["seq_nt16"]])
        exp = native.host_format_fastq(host)
        plain = native.host_format_fastq(M.plain_of(host))
        assert exp != plain
        nib = [np.stack([b >> 4, b & 15], axis=1).reshape(-1) for b in host["seq_bufs"]]
        host["_truth"] = [np.nonzero(nib[int(s)][int(a):int(a) + int(L)] != nib[1][int(b):int(b) + int(L)])[0].tolist()
                          if o != 255 else [] for s, a, b, L, o in
                          zip(recs["seq_sel"], recs["seq_nib_off"], off, recs["seq_len"], recs["orig_sel"])]
        assert M.restate(host, plain) == exp
        assert sum(1 for t in host["_truth"] if 0 < len(t) < 10) > 100     # real SNV masks among them
        f = masker.fastq_upload(recs, seq_batch=db)
        try:
            for _ in range(2):
                f.run()
                assert f.download() == exp
        finally:
            f.free()
    finally:
        db.free()


def test_kernel_list(hip_built, crafted):
    """With profiling on: no k_fq_maskq in a formatter run's kernel times with the option off (or
    with no record that has an original), one with it on."""
    from genomeanonymizer_amd import native
    recs, plain, exp = crafted
    m = native.HipMasker(0)
    try:
        m.set_profiling(True)
        none = dict(recs, orig_sel=np.full(len(recs["seq_len"]), 255, np.uint8))
        for r, want, data in ((M.plain_of(recs), False, plain), (none, False, plain), (recs, True, exp)):
            f = m.fastq_upload(r)
            try:
                f.run()
                f.sync()
                names = [k for k, _, _ in f.kernel_times()]
                assert ("k_fq_maskq" in names) == want, names
                assert "k_fq_format" in names
                assert f.download() == data
            finally:
                f.free()
    finally:
        m.set_profiling(False)
        m.close()


@pytest.fixture(scope="module")
def gpu_anon(hip_built):
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(device=0)


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz3000", "long1"])
def test_hip_pipeline_matches_hooked_reference(name, mode, gpu_anon, tmp_path, monkeypatch):
    index = M.set_mode(monkeypatch, mode)
    assert M.run_vs_maskq_golden(name, str(tmp_path / name), gpu_anon, bam_index=index) == {}


def test_hip_pipeline_without_a_reference_answer(gpu_anon, tmp_path, monkeypatch):
    """fuzz2003 (the hooked reference raises): the invariants, and the CPU oracle-engine run's files."""
    from pyoracle import OracleEngine
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    M.set_mode(monkeypatch, "streamed")
    got = M.run_pipeline_files("fuzz2003", str(tmp_path / "gpu"), gpu_anon)
    assert M.quality_diff(M.golden_files("fuzz2003"), got) > 0
    cpu = M.run_pipeline_files("fuzz2003", str(tmp_path / "cpu"), CompleteGermlineAnonymizer(engine=OracleEngine()))
    assert got == cpu


def test_hip_pipeline_compressed(gpu_anon, tmp_path, monkeypatch):
    import deflate_fixtures as F
    M.set_mode(monkeypatch, "streamed")
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    paths, t_out, n_out = F.run_compressed("edge", str(tmp_path / "edge"), gpu_anon)
    exp = M.golden_files("edge", M.MASKQ_GOLDEN)
    for tag, pre in (("tumor", t_out), ("normal", n_out)):
        for suf in (".1.fastq", ".2.fastq", ".single_end.fastq"):
            if tag + suf in exp:
                assert not os.path.exists(pre + suf)
                assert gzip.open(pre + suf + ".gz").read() == exp[tag + suf], tag + suf
