"""--discover_sites on the device: k_bam_site_tally (csrc/ganon_bam.hip) ORs the evidence of the columns
``ganon_bam_columns`` and ``ganon_region_decode`` decode into a byte per position — a thread per record,
a wave per record with more than 48 CIGAR ops — and k_site_compact turns the bytes, OR-ed with the host
tally's, into the site list. Expectations come from the plain-Python restatement of discover_helpers, and
the host tally must agree; the pipelines run with the HIP engine and the device decoder serving the small
inputs (GANON_GPU_INFLATE=1, GANON_GPU_INFLATE_MIN=1) against the CPU oracle-engine run with the option.
tests/test_discover_sites.py is the CPU side."""
import os

import numpy as np
import pytest

import discover_helpers as D
import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
from test_discover_sites import set_option

pytestmark = pytest.mark.gpu

PLAIN_KERNELS = {"k_bam_guess", "k_bam_check", "k_bam_fix", "k_bam_offsets", "k_bam_sizes", "bam_scans", "k_bam_scatter"}


@pytest.fixture(scope="module")
def inflater(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.set_site_tally(None)
    g.close()


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    from genomeanonymizer_amd.io.fasta import FastaRef
    d = str(tmp_path_factory.mktemp("hand"))
    plain = D.write_hand_files(d, False)
    t, n, fa, _ = D.hand_built()
    return {"files": plain, "fasta": FastaRef(plain["ref"]), "exp": D.expected_hand(), "recs": (t, n)}


def _device_lists(inflater, hand, plan, host=None):
    """The compacted lists of the three FASTA sequences after the calls of ``plan`` — (dataset, records)
    pairs, each decoded by ``bam_columns`` once per sequence with that sequence's tally set; ``host``: a
    HostTally whose bytes are OR-ed in by the compaction."""
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    ref = HostTally.of_fasta(hand["fasta"])
    streams = [(ds, *D.stream_of(recs)) for ds, recs in plan]
    lists = []
    for seq in range(3):
        dt = native.DeviceTally(inflater, ref.reference_of(seq), int(ref.lengths[seq]))
        for ds, d, p in streams:
            inflater.set_site_tally(dt, ds, seq)          # (the hand-built header lists the FASTA's order)
            native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)
        lists.append(dt.finish(host.bytes_address(seq) if host is not None else None))
        assert inflater.site_tally is None
    return D.lists_as_dict(ref.names, lists)


def test_tile_is_the_helpers_tile(hip_built):
    from genomeanonymizer_amd import native
    assert native.site_compact_tile() == D.TILE


def test_columns_with_a_tally_match_the_restatement_and_the_host(inflater, hand):
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    t, n = hand["recs"]
    assert len(t) > 256 and len(n) > 256
    assert {48, 49, 63, 64, 65, 128, 129} <= {len(r["cigar"]) for r in t}
    exp = hand["exp"]
    host = HostTally.of_fasta(hand["fasta"])
    for ds, s in enumerate("TN"):
        ReadTable(hand["files"][s], threads=2, site_tally=(host, ds))
    assert D.lists_as_dict(host.names, [host.finish(i) for i in range(3)]) == exp
    assert _device_lists(inflater, hand, [(0, t), (1, n)]) == exp
    # either dataset first, and the stream tallied twice
    assert _device_lists(inflater, hand, [(1, n), (0, t), (0, t), (1, n)]) == exp
    # one dataset alone: evidence, no site
    assert _device_lists(inflater, hand, [(0, t)]) == {}


def test_host_and_device_halves_are_ored_before_the_intersection(inflater, hand):
    """Half of each dataset's records tallied by the host object and half on the device — the tumor's
    even records with the normal's odd ones on the device —: evidence for one position sits on both
    sides, and the compaction ORs them before it intersects."""
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    t, n = hand["recs"]
    exp = hand["exp"]
    d = os.path.dirname(hand["files"]["T"])
    host = HostTally.of_fasta(hand["fasta"])
    for ds, recs, tag in ((0, t[1::2], "t_odd"), (1, n[0::2], "n_even")):
        path = os.path.join(d, tag + ".bam")
        write_bgzf(path, D.stream_of(recs)[0].tobytes())
        ReadTable(path, threads=2, site_tally=(host, ds))
    dev_only = _device_lists(inflater, hand, [(0, t[0::2]), (1, n[1::2])])
    assert dev_only != exp                                   # (neither side alone has the sites)
    assert _device_lists(inflater, hand, [(0, t[0::2]), (1, n[1::2])], host) == exp
    host_only = D.lists_as_dict(host.names, [host.finish(i) for i in range(3)])
    assert host_only != exp


def test_kernel_list(inflater, hand):
    """Without a tally the kernels are those of a context that never had one; with one, the new kernel
    follows them."""
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    d, p = D.stream_of(hand["recs"][0])
    ref = HostTally.of_fasta(hand["fasta"])
    fresh = native.GpuInflater(0, min_blocks=1)
    dt = native.DeviceTally(inflater, ref.reference_of(2), int(ref.lengths[2]))
    lists = {}
    try:
        for tag, g in (("fresh", fresh), ("cleared", inflater), ("tally", inflater), ("again", inflater)):
            g.set_profiling(True)
            g.set_site_tally(dt if tag == "tally" else None, 0, 2)
            native.bam_columns_device(g.handle, d, p, len(d), on_host=True)
            lists[tag] = [k for k, _ in g.kernel_times()]
            g.set_profiling(False)
        inflater.set_profiling(True)
        pos, _ = dt.finish()
        lists["compact"] = [k for k, _ in inflater.kernel_times()]
        inflater.set_profiling(False)
    finally:
        inflater.set_site_tally(None)
        fresh.close()
    assert set(lists["fresh"]) <= PLAIN_KERNELS and PLAIN_KERNELS - {"k_bam_fix"} <= set(lists["fresh"]), lists
    assert lists["cleared"] == lists["fresh"] == lists["again"]
    assert lists["tally"] == lists["fresh"] + ["k_bam_site_tally"], lists
    assert lists["compact"] == ["k_site_compact", "site_scan"] and len(pos) == 0, lists    # (tumor alone: no site)


@pytest.mark.parametrize("name", ["fuzz3500", "long1"])
def test_device_region_reads_discover_what_host_region_reads_do(inflater, name, tmp_path):
    import dataclasses
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import discover
    from genomeanonymizer_amd.io.fasta import FastaRef
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario(name), bam_index=True), str(tmp_path / "in"))
    fasta = FastaRef(p["ref"])
    host = discover(p["T"], p["N"], fasta, 4)
    native.decode_phase_times(reset=True)
    dev = discover(p["T"], p["N"], fasta, 4, inflater=inflater)
    ph = native.decode_phase_times(reset=True)
    assert ph["device_regions"] > 0, ph
    assert D.panel_as_dict(dev) == D.panel_as_dict(host) and host.n_sites >= 50
    if name == "long1":
        assert D.panel_as_dict(host) == D.scenario_sites(name)["sites"]


# ---- the pipeline ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_anon(hip_built):
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(device=0)


@pytest.mark.parametrize("mode", ["streamed", "jobs"])
@pytest.mark.parametrize("name", ["tiny", "fuzz2000", "long1"])
def test_hip_pipeline_equals_the_oracle_engine_run(name, mode, gpu_anon, tmp_path, monkeypatch):
    from genomeanonymizer_amd import native
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    set_option(monkeypatch, True)
    cpu = K.run_files(name, str(tmp_path / "cpu"), H.oracle_anonymizer(), index)
    monkeypatch.setenv("GANON_GPU_INFLATE", "1")
    monkeypatch.setenv("GANON_GPU_INFLATE_MIN", "1")
    native.decode_phase_times(reset=True)
    got = K.run_files(name, str(tmp_path / "gpu"), gpu_anon, index)
    ph = native.decode_phase_times(reset=True)
    assert got == cpu and got != M.golden_files(name)
    if mode == "jobs":
        assert ph["device_regions"] > 0, ph          # (region reads decoded, tallied and masked on the device)
