"""--hash_read_names on the device: k_bam_name_hash (csrc/ganon_bam.hip) hashes the names of the records
``ganon_bam_columns`` and ``ganon_region_decode`` decode, with the core the host decoder uses
(csrc/ganon_name_hash.h). Expected names come from ``hashlib.blake2s`` over the unkeyed call's names;
the pipelines run with the HIP engine and the device decoder serving the small inputs
(GANON_GPU_INFLATE=1, GANON_GPU_INFLATE_MIN=1) against the CPU oracle-engine run with the same key.
tests/test_namehash.py is the CPU side."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import maskq_helpers as M
import namehash_helpers as H
from test_distributed import _free_port, _worker

pytestmark = pytest.mark.gpu

PLAIN_KERNELS = {"k_bam_guess", "k_bam_check", "k_bam_fix", "k_bam_offsets", "k_bam_sizes", "bam_scans", "k_bam_scatter"}
COLS = ("tid", "pos", "end", "flag", "mapq", "l_seq", "n_cigar", "mate_tid", "mate_pos", "tlen", "name_len",
        "aux_len", "name_off", "cig_off", "seq_off", "qual_off", "aux_off", "names_blob", "cigar", "seq", "qual",
        "aux")


@pytest.fixture(scope="module")
def inflater(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.set_name_key(None)
    g.close()


class _Cols:
    """A column dict of ``bam_columns_device`` with a table's attribute names."""
    def __init__(self, cols):
        self.__dict__.update(cols)
        self.n = len(cols["pos"])


def test_columns_with_a_key_on_the_crafted_stream(inflater):
    from genomeanonymizer_amd import native
    d, p = H.crafted_stream()
    assert len(d) < 1 << 20
    run = lambda: native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)[0]
    inflater.set_name_key(None)
    plain = run()
    rel = (plain["rec_off"] - p) % H.CHUNK
    assert {H.CHUNK - t for t in H.TAIL_STARTS} <= set(rel.tolist())     # records starting in a chunk's last bytes
    cnt = np.bincount(plain["name_len"], minlength=255)
    assert len(cnt) == 255 and cnt.min() >= 2                             # every name length 0..254, twice
    long_run = np.nonzero(plain["l_seq"] == 2000)[0]
    assert len(long_run) == 40 and (np.diff(long_run) == 1).all()         # scatter groups past the LDS stage
    for key in (H.KEY, H.KEYS[0]):
        inflater.set_name_key(key)
        keyed = run()
        H.assert_keyed_table(_Cols(keyed), _Cols(plain), key)
        assert np.array_equal(keyed["rec_off"], plain["rec_off"])
        again = run()
        for f in keyed:
            assert np.array_equal(again[f], keyed[f]), f
    inflater.set_name_key(None)
    back = run()
    for f in plain:
        assert np.array_equal(back[f], plain[f]), f


def test_kernel_list(inflater):
    """A keyed call lists the new kernel after the unkeyed call's kernels, which are the parent's."""
    from genomeanonymizer_amd import native
    d, p = H.crafted_stream()
    inflater.set_profiling(True)
    try:
        inflater.set_name_key(None)
        native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)
        plain = [k for k, _ in inflater.kernel_times()]
        inflater.set_name_key(H.KEY)
        native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)
        keyed = [k for k, _ in inflater.kernel_times()]
    finally:
        inflater.set_profiling(False)
        inflater.set_name_key(None)
    assert set(plain) <= PLAIN_KERNELS and PLAIN_KERNELS - {"k_bam_fix"} <= set(plain), plain
    assert keyed == plain + ["k_bam_name_hash"], (plain, keyed)


def _compare_regions(paths, inflater, window, rng, k):
    """Device-decoded keyed regions against the host reader's keyed regions, column for column, and
    their names against hashlib over the unkeyed host regions."""
    from genomeanonymizer_amd.io.bam import BamReader
    n_tables = 0
    for path in paths:
        plain = BamReader(path, 4)
        host = BamReader(path, 4, name_key=H.KEY)
        dev = BamReader(path, 4, window, inflater=inflater, name_key=H.KEY)
        for tid, L in enumerate(int(x) for x in plain.ref_lens):
            regions = [(0, L), (0, L + 1000), (L - 1, L + 5), (0, 1), (L // 2, L // 2)]
            for _ in range(k):
                a = int(rng.integers(0, L))
                regions.append((a, int(min(L + 10, a + rng.integers(1, max(2, L // 3))))))
            for a, b in regions:
                exp, got = host.region(tid, a, b), dev.region(tid, a, b)
                assert got.n == exp.n, (path, tid, a, b)
                for f in COLS:
                    assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(exp, f))), (path, tid, a, b, f)
                H.assert_keyed_table(got, plain.region(tid, a, b), H.KEY, (path, tid, a, b))
                n_tables += 1
        for r in (dev, host, plain):
            r.close()
    return n_tables


def test_keyed_device_regions_equal_keyed_host_regions(inflater, tmp_path):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.fastpair import make_pair
    d = str(tmp_path / "in")
    make_pair(d, n_contigs=2, contig_len=300_000, pairs_per_contig=12_000, window_every=20_000)
    paths = [os.path.join(d, f"{k}.bam") for k in ("tumor", "normal")]
    native.decode_phase_times(reset=True)
    n = _compare_regions(paths, inflater, 0, np.random.default_rng(5), 6)
    ph = native.decode_phase_times(reset=True)
    assert n > 0 and ph["device_regions"] > 0.5 * n, ph
    # a 128 KiB window: the larger regions run past the decoder's first window and the host walk takes
    # over from the bytes it inflated (the device-then-host hand-over), hashing with the same core
    _compare_regions(paths, inflater, 1 << 17, np.random.default_rng(6), 6)
    ph = native.decode_phase_times(reset=True)
    assert ph["device_fallbacks"] > 0 and ph["device_regions"] > 0, ph


@pytest.mark.parametrize("name", ["edge", "fuzz3500"])
def test_keyed_device_regions_on_scenarios(inflater, name, tmp_path):
    import dataclasses
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario(name), bam_index=True), str(tmp_path / "in"))
    native.decode_phase_times(reset=True)
    n = _compare_regions([p["T"], p["N"]], inflater, 0, np.random.default_rng(len(name)), 8)
    assert n > 0 and native.decode_phase_times(reset=True)["device_regions"] > 0


# ---- the pipeline ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_anon(hip_built):
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(device=0)


def _device_decode(monkeypatch):
    monkeypatch.setenv("GANON_GPU_INFLATE", "1")
    monkeypatch.setenv("GANON_GPU_INFLATE_MIN", "1")


@pytest.mark.parametrize("mode", ["streamed", "jobs"])
@pytest.mark.parametrize("name", ["tiny", "edge", "fuzz3000"])
def test_hip_pipeline_equals_the_oracle_engine_run(name, mode, gpu_anon, tmp_path, monkeypatch):
    from genomeanonymizer_amd import native
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, H.KEY)
    cpu = H.run_files(name, str(tmp_path / "cpu"), H.oracle_anonymizer(), index)
    _device_decode(monkeypatch)
    native.decode_phase_times(reset=True)
    got = H.run_files(name, str(tmp_path / "gpu"), gpu_anon, index)
    ph = native.decode_phase_times(reset=True)
    assert got == cpu and len(cpu) == 7
    if mode == "jobs":
        assert ph["device_regions"] > 0, ph          # (region reads decoded, and hashed, on the device)
    if (name, mode) == ("edge", "streamed"):          # ... and the defining property on the device path
        H.set_option(monkeypatch, False)
        assert got == H.run_files(name, str(tmp_path / "xp"), gpu_anon, index, H.KEY, monkeypatch)


def test_hip_pipeline_composes_with_compress_output(gpu_anon, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, H.KEY)
    plain = H.run_files("edge", str(tmp_path / "cpu"), H.oracle_anonymizer())
    _device_decode(monkeypatch)
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    assert H.run_files("edge", str(tmp_path / "gz"), gpu_anon, gz=True) == plain


def test_hip_pipeline_composes_with_masked_base_quality(gpu_anon, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", 2)
    H.set_option(monkeypatch, H.KEY)
    cpu = H.run_files("edge", str(tmp_path / "cpu"), H.oracle_anonymizer())
    _device_decode(monkeypatch)
    got = H.run_files("edge", str(tmp_path / "gpu"), gpu_anon)
    assert got == cpu
    mq = M.golden_files("edge", M.MASKQ_GOLDEN)
    assert H.record_multiset(got["tumor.1.fastq"]) == H.record_multiset(mq["tumor.1.fastq"], H.KEY)


def test_two_hip_ranks_with_a_key_equal_one_process(hip_built, tmp_path, monkeypatch):
    from genomeanonymizer_amd.synth.generate import generate, scenario
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, H.KEY)
    exp = H.run_files("fuzz3000", str(tmp_path / "one"), H.oracle_anonymizer())
    workdir = str(tmp_path / "two")
    paths = generate(scenario("fuzz3000"), os.path.join(workdir, "in"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, "fuzz3000", workdir, q, "hip")) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert codes == [0, 0], codes
    assert H.collect(paths) == exp and len(exp) == 7


@pytest.mark.parametrize("with_key", [True, False], ids=["key", "random"])
def test_cli_under_an_rccl_process_group(hip_built, tmp_path, monkeypatch, with_key):
    """The command line as torchrun starts it, one rank: rank 0's key is broadcast over the nccl (RCCL)
    process group before a reader opens. With a key the files are the oracle-engine run's; without one
    the names are 32 hex characters, the other lines the plain goldens', and .1 and .2 hold one set of
    names. The key appears nowhere in the log."""
    import subprocess
    import sys
    from genomeanonymizer_amd.synth.generate import generate, scenario
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, H.KEY if with_key else None)
    d = str(tmp_path / "rccl")
    paths = generate(scenario("fuzz3000"), d)
    env = dict(os.environ, PYTHONPATH=H.helpers_repo(), GANON_IO_BLOCK="4096", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               LOCAL_WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    env.pop("GANON_HASH_READ_NAMES")     # (the flag turns it on)
    r = subprocess.run([sys.executable, "-m", "genomeanonymizer_amd.genome_anonymizer", "-d", d, "-s", "samples.tsv",
                        "-r", paths["ref"], "--record_statistics", "-c", "4", "-v", "1", "--hash_read_names"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "process group backend nccl" in r.stderr, r.stderr[-2000:]
    assert H.KEY.hex() not in r.stderr + r.stdout
    got = H.collect(paths)
    if with_key:
        assert got == H.run_files("fuzz3000", str(tmp_path / "cpu"), H.oracle_anonymizer())
        return
    gold = M.golden_files("fuzz3000")
    assert sorted(got) == sorted(gold) and got["statistics"] == gold["statistics"]
    for f in gold:
        if f != "statistics":
            g, e = H.fastq_records(got[f]), H.fastq_records(gold[f])
            assert sorted(x[1:] for x in g) == sorted(x[1:] for x in e), f
            assert all(len(x[0]) == 32 and set(x[0]) <= set(b"0123456789abcdef") for x in g), f
    for tag in ("tumor", "normal"):
        n1 = {x[0] for x in H.fastq_records(got[tag + ".1.fastq"])}
        assert n1 and n1 == {x[0] for x in H.fastq_records(got[tag + ".2.fastq"])}
