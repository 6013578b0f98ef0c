"""--mask_sa_clips on the device: k_bam_sa_clips (csrc/ganon_bam.hip) masks, after k_bam_known_mask, the
soft-clipped bases of the columns ``ganon_bam_columns`` and ``ganon_region_decode`` decode along the
records' SA alignments. Expectations come from the plain-Python rule of sa_clips_helpers over the call
without a table, and the host decoder must agree; the pipelines run with the HIP engine and the device
decoder serving the small inputs (GANON_GPU_INFLATE=1, GANON_GPU_INFLATE_MIN=1) against the CPU
oracle-engine run with the same panel and option. tests/test_sa_clips.py is the CPU side."""
import dataclasses

import numpy as np
import pytest

import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
import sa_clips_helpers as S

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def hand():
    recs, sites, _ = S.hand_built()
    d, p = S.stream_of(recs)
    return {"recs": recs, "sites": sites, "d": d, "p": p, "names": [c for c, _ in K.HAND_CONTIGS]}


@pytest.mark.parametrize("quality", [None, 7])
def test_columns_match_the_rule_and_the_host(inflater, hand, tmp_path, quality):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    d, p, names, sites = hand["d"], hand["p"], hand["names"], hand["sites"]
    path = str(tmp_path / "hand.bam")
    write_bgzf(path, d.tobytes())
    run = lambda: _Cols(native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)[0], names)
    inflater.set_known_sites(None)
    plain = run()
    assert plain.n == S.HAND_RECORDS
    table = S.table_of(sites, names, quality)
    ks0, (m0, g0) = inflater.known_sites_masked(), inflater.sa_clips_counts()
    inflater.set_known_sites(table)
    got = run()
    n_ks, n_sa, n_ign = S.assert_masked_table(got, plain, sites, quality)
    assert n_sa >= S.MIN_HAND_REWRITTEN and n_ign == S.N_IGNORED
    m1, g1 = inflater.sa_clips_counts()
    assert (inflater.known_sites_masked() - ks0, m1 - m0, g1 - g0) == (n_ks, n_sa, n_ign)
    host = ReadTable(path, threads=2, known_sites=table)
    assert (host.known_masked, host.sa_masked, host.sa_ignored) == (n_ks, n_sa, n_ign)
    for f in COLS:
        assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(host, f))), f
    again = run()      # (the counts keep running; the bytes are the same)
    for f in COLS:
        assert np.array_equal(getattr(again, f), getattr(got, f)), f
    assert inflater.sa_clips_counts() == (m1 + n_sa, g1 + n_ign)
    # the table without the switch: §4i's rule alone, and no count moves
    inflater.set_known_sites(K.table_of(sites, names, quality))
    assert K.assert_masked_table(run(), plain, sites, quality) == n_ks
    assert inflater.sa_clips_counts() == (m1 + n_sa, g1 + n_ign)
    inflater.set_known_sites(None)
    back = run()
    for f in COLS:
        assert np.array_equal(getattr(back, f), getattr(plain, f)), f


def test_kernel_list(inflater, hand):
    """With the option the kernels are the table-only list and k_bam_sa_clips after it; without it the
    table-only list exactly."""
    from genomeanonymizer_amd import native
    d, p, names, sites = hand["d"], hand["p"], hand["names"], hand["sites"]
    lists = {}
    try:
        for tag, table in (("table", K.table_of(sites, names)), ("option", S.table_of(sites, names)),
                           ("table_again", S.table_of(sites, names, sa_clips=False))):
            inflater.set_profiling(True)
            inflater.set_known_sites(table)
            native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)
            lists[tag] = [k for k, _ in inflater.kernel_times()]
            inflater.set_profiling(False)
    finally:
        inflater.set_known_sites(None)
    assert lists["table"][-1] == "k_bam_known_mask" and "k_bam_sa_clips" not in lists["table"], lists
    assert lists["option"] == lists["table"] + ["k_bam_sa_clips"], lists
    assert lists["table_again"] == lists["table"], lists


def test_device_regions_equal_host_regions(inflater, tmp_path):
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.io.bam import BamReader
    from genomeanonymizer_amd.synth.generate import generate, scenario
    name = "fuzz2000"
    paths = generate(dataclasses.replace(scenario(name), bam_index=True), str(tmp_path / "in"))
    sites = S.scenario_sa_panel(name)["sites"]
    rng = np.random.default_rng(8)
    native.decode_phase_times(reset=True)
    n_tables = 0
    for path in (paths["T"], paths["N"]):
        plain = BamReader(path, 4)
        table = S.table_of(sites, plain.ref_names, 11)
        host = BamReader(path, 4, known_sites=table)
        dev = BamReader(path, 4, 0, inflater=inflater, known_sites=table)
        extra = [0, 0, 0]
        for tid, L in enumerate(int(x) for x in plain.ref_lens):
            regions = [(0, L), (0, L + 1000), (L - 1, L + 5), (0, 1), (L // 2, L // 2)]
            for _ in range(4):
                a = int(rng.integers(0, L))
                regions.append((a, int(min(L + 10, a + rng.integers(1, max(2, L // 3))))))
            for a, b in regions:
                exp, got = host.region(tid, a, b), dev.region(tid, a, b)
                assert got.n == exp.n, (path, tid, a, b)
                for f in COLS:
                    assert np.array_equal(np.asarray(getattr(got, f)), np.asarray(getattr(exp, f))), (path, tid, a, b, f)
                n_tables += 1
            c = S.assert_masked_table(dev.region(tid, 0, L), plain.region(tid, 0, L), sites, 11, (path, tid))
            extra = [x + y for x, y in zip(extra, c)]
        # (the device reader decoded the host reader's regions and, for the rule, one more per sequence)
        hc, dc = host.sa_clips_counts(), dev.sa_clips_counts()
        assert hc["device"] == 0 and dc["host"] + dc["device"] == hc["host"] + extra[1]
        assert dc["ignored"] == hc["ignored"] + extra[2]
        assert dev.known_masked() == host.known_masked() + extra[0]
        assert extra[1] >= S.MIN_CHANGED
        for r in (dev, host, plain):
            r.close()
    assert n_tables > 0 and native.decode_phase_times(reset=True)["device_regions"] > 0


# ---- the pipeline ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_anon(hip_built):
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(device=0)


@pytest.mark.parametrize("mode", ["streamed", "jobs"])
def test_hip_pipeline_equals_the_oracle_engine_run(mode, gpu_anon, tmp_path, monkeypatch):
    from genomeanonymizer_amd import native
    name = "fuzz2000"
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, S.scenario_sa_panel(name)["vcf"])
    S.set_option(monkeypatch, True)
    cpu = S.run_files(name, str(tmp_path / "cpu"), H.oracle_anonymizer(), index)
    monkeypatch.setenv("GANON_GPU_INFLATE", "1")
    monkeypatch.setenv("GANON_GPU_INFLATE_MIN", "1")
    native.decode_phase_times(reset=True)
    got = S.run_files(name, str(tmp_path / "gpu"), gpu_anon, index)
    ph = native.decode_phase_times(reset=True)
    assert got == cpu
    if mode == "jobs":
        assert ph["device_regions"] > 0, ph          # (region reads decoded, and masked, on the device)
    S.set_option(monkeypatch, False)
    assert got != S.run_files(name, str(tmp_path / "off"), gpu_anon, index)
