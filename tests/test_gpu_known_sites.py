"""--known_sites on the device: k_bam_known_mask (csrc/ganon_bam.hip) applies the panel mask to the
columns ``ganon_bam_columns`` and ``ganon_region_decode`` decode: a thread per record, a wave per record
with more than 48 CIGAR ops. Expectations come from the plain-Python rule of known_sites_helpers over
the call without a table, and the host decoder must agree; the pipelines run with the HIP engine and
the device decoder serving the small inputs (GANON_GPU_INFLATE=1, GANON_GPU_INFLATE_MIN=1) against the
CPU oracle-engine run with the same panel. tests/test_known_sites.py is the CPU side."""
import os

import numpy as np
import pytest

import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H

pytestmark = pytest.mark.gpu

PLAIN_KERNELS = {"k_bam_guess", "k_bam_check", "k_bam_fix", "k_bam_offsets", "k_bam_sizes", "bam_scans", "k_bam_scatter"}
COLS = K.I32 + K.I64 + K.BLOBS + ("seq", "qual")


@pytest.fixture(scope="module")
def inflater(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.set_known_sites(None)
    g.close()


class _Cols:
    """A column dict of ``bam_columns_device`` with a table's attribute names."""
    def __init__(self, cols, ref_names):
        self.__dict__.update(cols)
        self.n = len(cols["pos"])
        self.ref_names = ref_names

    def cigar_of(self, i):
        o = int(self.cig_off[i])
        return self.cigar[o:o + int(self.n_cigar[i])]


def _stream():
    """The hand-built records, then records of 48 and 49 ops (thread path against wave path) and of 63,
    64, 65, 128 and 129 ops (the wave's chunks of 64), M 1 alternating with I 1 / D 1; 300 more records
    so that the call has more than one workgroup."""
    recs, sites = K.hand_built()
    recs = recs + K.long_cigar_records()
    rng = np.random.default_rng(3)
    for k in range(300):
        L = int(rng.integers(1, 60))
        recs.append(dict(tid=1, pos=200 + 3 * k, flag=0, cigar=[("S", 1), ("M", L)],
                         nib=[int(x) for x in rng.choice([1, 2, 4, 8, 15], L + 1)], qual=[int(x) for x in rng.integers(2, 40, L + 1)]))
    recs += K.long_cigar_records((129, 64, 49), seed=4)
    return recs, sites


def _panels(sites):
    c1 = dict(zip(sites.pos["c1"], sites.val["c1"]))
    return {"hand": sites,
            "one": K.Sites({"c2": {103: (8, 7)}}),
            "every": K.Sites({"c1": c1, "c2": {p: (8, 7) for p in range(3000)}}),
            "none": K.Sites({})}


@pytest.mark.parametrize("quality", [None, 7])
def test_columns_with_a_table_match_the_rule_and_the_host(inflater, tmp_path, quality):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    recs, sites = _stream()
    d, p = K.stream_of(recs)
    names = [c for c, _ in K.HAND_CONTIGS]
    path = str(tmp_path / "hand.bam")
    write_bgzf(path, d.tobytes())
    run = lambda: _Cols(native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)[0], names)
    inflater.set_known_sites(None)
    plain = run()
    assert plain.n == len(recs) > 256 and sorted(set(plain.n_cigar.tolist()) & {48, 49, 63, 64, 65, 128, 129}) == \
        [48, 49, 63, 64, 65, 128, 129]
    for tag, s in _panels(sites).items():
        table = K.table_of(s, names, quality)
        before = inflater.known_sites_masked()
        inflater.set_known_sites(table)
        assert (inflater.known_sites is None) == (s.n() == 0)
        got = run()
        total = K.assert_masked_table(got, plain, s, quality, tag)
        assert inflater.known_sites_masked() - before == total, tag
        host = ReadTable(path, threads=2, known_sites=table)
        assert host.known_masked == total
        for f in COLS:
            assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(host, f))), (tag, f)
        if tag == "every":
            assert total > 1000
            again = run()
            for f in COLS:
                assert np.array_equal(getattr(again, f), getattr(got, f)), f
    inflater.set_known_sites(None)
    back = run()
    for f in COLS:
        assert np.array_equal(getattr(back, f), getattr(plain, f)), f


def test_kernel_list(inflater):
    """Without a table the kernels are those of a context that never had one; with one, the new kernel
    follows them."""
    from genomeanonymizer_amd import native
    recs, sites = _stream()
    d, p = K.stream_of(recs)
    names = [c for c, _ in K.HAND_CONTIGS]
    fresh = native.GpuInflater(0, min_blocks=1)
    lists = {}
    try:
        for tag, g in (("fresh", fresh), ("cleared", inflater), ("table", inflater)):
            g.set_profiling(True)
            g.set_known_sites(K.table_of(sites, names) if tag == "table" else None)
            native.bam_columns_device(g.handle, d, p, len(d), on_host=True)
            lists[tag] = [k for k, _ in g.kernel_times()]
            g.set_profiling(False)
    finally:
        inflater.set_known_sites(None)
        fresh.close()
    assert set(lists["fresh"]) <= PLAIN_KERNELS and PLAIN_KERNELS - {"k_bam_fix"} <= set(lists["fresh"]), lists
    assert lists["cleared"] == lists["fresh"]
    assert lists["table"] == lists["fresh"] + ["k_bam_known_mask"], lists


def _compare_regions(paths, sites, inflater, window, rng, k, quality=None, rule_span=1.0):
    """Device-decoded regions with a table against the host reader's with the same table, column for
    column, and — over the first ``rule_span`` of each sequence (0: not at all) — against the rule over
    the host region without one."""
    from genomeanonymizer_amd.io.bam import BamReader
    n_tables = total = 0
    for path in paths:
        plain = BamReader(path, 4)
        table = K.table_of(sites, plain.ref_names, quality)
        host = BamReader(path, 4, known_sites=table)
        dev = BamReader(path, 4, window, inflater=inflater, known_sites=table)
        extra = 0
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
                n_tables += 1
            if rule_span:
                e = int(L * rule_span)
                extra += K.assert_masked_table(dev.region(tid, 0, e), plain.region(tid, 0, e), sites, quality, (path, tid))
        # (the device reader decoded the host reader's regions and, for the rule, one more per sequence)
        assert not rule_span or dev.known_masked() == host.known_masked() + extra
        total += extra
        for r in (dev, host, plain):
            r.close()
    return n_tables, total


def _dense_sites(ref_path, every: int, seed: int) -> K.Sites:
    """A site about every ``every`` bases of each contig of a FASTA, ALT = the three other bases."""
    rng = np.random.default_rng(seed)
    by = {}
    for name, seq in K._fasta(ref_path).items():
        pos = np.unique(rng.integers(0, len(seq), max(1, len(seq) // every)))
        by[name] = {int(p): (K.CODE[seq[p].upper()], 15 ^ K.CODE[seq[p].upper()]) for p in pos.tolist()
                    if seq[p].upper() in K.CODE}
    return K.Sites(by)


def test_device_regions_equal_host_regions_on_an_indexed_pair(inflater, tmp_path):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.fastpair import make_pair
    d = str(tmp_path / "in")
    make_pair(d, n_contigs=2, contig_len=600_000, pairs_per_contig=12_000, window_every=40_000)
    paths = [os.path.join(d, f"{k}.bam") for k in ("tumor", "normal")]
    sites = _dense_sites(os.path.join(d, "ref.fa"), 37, 2)
    native.decode_phase_times(reset=True)
    n, total = _compare_regions(paths, sites, inflater, 0, np.random.default_rng(5), 3, rule_span=0.25)
    ph = native.decode_phase_times(reset=True)
    assert n > 0 and total >= K.MIN_CHANGED and ph["device_regions"] > 0.5 * n, (ph, total)
    # a 128 KiB window: the larger regions run past the decoder's first window and the host walk takes
    # over from the bytes it inflated (the device-then-host hand-over), masking with the same rule
    _compare_regions(paths, sites, inflater, 1 << 17, np.random.default_rng(6), 2, quality=4, rule_span=0)
    ph = native.decode_phase_times(reset=True)
    assert ph["device_fallbacks"] > 0 and ph["device_regions"] > 0, ph


@pytest.mark.parametrize("name", ["fuzz3500", "long1"])
def test_device_regions_on_scenarios(inflater, name, tmp_path):
    import dataclasses
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario(name), bam_index=True), str(tmp_path / "in"))
    sites = _dense_sites(p["ref"], 37, 7)
    native.decode_phase_times(reset=True)
    n, total = _compare_regions([p["T"], p["N"]], sites, inflater, 0, np.random.default_rng(len(name)), 4, quality=11)
    assert n > 0 and total >= K.MIN_CHANGED and native.decode_phase_times(reset=True)["device_regions"] > 0


# ---- the pipeline ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_anon(hip_built):
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(device=0)


def _device_decode(monkeypatch):
    monkeypatch.setenv("GANON_GPU_INFLATE", "1")
    monkeypatch.setenv("GANON_GPU_INFLATE_MIN", "1")


@pytest.mark.parametrize("mode", ["streamed", "jobs"])
@pytest.mark.parametrize("name", ["tiny", "fuzz2000", "long1"])
def test_hip_pipeline_equals_the_oracle_engine_run(name, mode, gpu_anon, tmp_path, monkeypatch):
    from genomeanonymizer_amd import native
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    sp = K.scenario_panel(name)
    K.set_option(monkeypatch, sp["vcf"])
    cpu = K.run_files(name, str(tmp_path / "cpu"), H.oracle_anonymizer(), index)
    _device_decode(monkeypatch)
    native.decode_phase_times(reset=True)
    got = K.run_files(name, str(tmp_path / "gpu"), gpu_anon, index)
    ph = native.decode_phase_times(reset=True)
    assert got == cpu
    if mode == "jobs":
        assert ph["device_regions"] > 0, ph          # (region reads decoded, and masked, on the device)
        # ... and the defining property on the device path: the plain run on X'
        K.set_option(monkeypatch, None)
        assert got == K.run_files(name, str(tmp_path / "xp"), gpu_anon, index, sp["sites"], monkeypatch)


def test_hip_pipeline_composes_with_hash_read_names(gpu_anon, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "jobs", None)
    H.set_option(monkeypatch, H.KEY)
    K.set_option(monkeypatch, K.scenario_panel("edge")["vcf"])
    cpu = K.run_files("edge", str(tmp_path / "cpu"), H.oracle_anonymizer(), True)
    _device_decode(monkeypatch)
    assert K.run_files("edge", str(tmp_path / "gpu"), gpu_anon, True) == cpu


def test_hip_pipeline_composes_with_masked_base_quality(gpu_anon, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "jobs", 2)
    H.set_option(monkeypatch, False)
    sp = K.scenario_panel("fuzz2000")
    K.set_option(monkeypatch, sp["vcf"])
    _device_decode(monkeypatch)
    got = K.run_files("fuzz2000", str(tmp_path / "gpu"), gpu_anon, True)
    K.set_option(monkeypatch, None)
    assert got == K.run_files("fuzz2000", str(tmp_path / "xp"), gpu_anon, True, sp["sites"], monkeypatch, quality=2)


def test_hip_pipeline_composes_with_compress_output(gpu_anon, tmp_path, monkeypatch):
    M.set_mode(monkeypatch, "streamed", None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, K.scenario_panel("tiny")["vcf"])
    plain = K.run_files("tiny", str(tmp_path / "cpu"), H.oracle_anonymizer())
    _device_decode(monkeypatch)
    monkeypatch.setenv("GANON_COMPRESS_OUTPUT", "1")
    assert K.run_files("tiny", str(tmp_path / "gz"), gpu_anon, gz=True) == plain
