"""--discover_sites' evidence filters and rule on the device: with a DeviceTally that carries a rule,
k_bam_site_tally runs as its filtered instantiation (csrc/ganon_bam.hip: the mapq column, the excluded
flags, a quality byte per mismatch — thread path and wave path) and k_site_compact reads the bytes under
the rule's mode. Expectations come from the plain-Python restatement of discover_rules_helpers, and the
host tally must agree; the pipelines run with the HIP engine and the device decoder serving the small
inputs against the CPU oracle-engine run with the same options. tests/test_discover_rules.py is the CPU
side."""
import os

import pytest

import discover_helpers as D
import discover_rules_helpers as R
import known_sites_helpers as K
import maskq_helpers as M
import namehash_helpers as H
from test_discover_sites import set_option

pytestmark = pytest.mark.gpu

Q20 = R.Rule(20, 0, 0, "both")
Q20N = R.Rule(20, 0, 0, "normal")


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
    d = str(tmp_path_factory.mktemp("rules"))
    plain = R.write_hand_files(d, False)
    t, n, _, _ = R.hand_built()
    return {"files": plain, "fasta": FastaRef(plain["ref"]), "recs": (t, n), "dir": d}


def _device_lists(inflater, hand, plan, rule=None, host=None, create=None):
    """The compacted lists of the three FASTA sequences after the calls of ``plan`` — (dataset, records)
    pairs, each decoded by ``bam_columns`` once per sequence with that sequence's tally set. ``rule``: the
    DeviceTally's (None: made without one, the existing call); ``host``: a HostTally whose bytes the
    compaction ORs in."""
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    ref = HostTally.of_fasta(hand["fasta"])
    streams = [(ds, *R.stream_of(recs)) for ds, recs in plan]
    lists = []
    for seq in range(3):
        if rule is None:
            dt = native.DeviceTally(inflater, ref.reference_of(seq), int(ref.lengths[seq]))
        else:
            dt = native.DeviceTally(inflater, ref.reference_of(seq), int(ref.lengths[seq]), R.site_rule(rule))
        for ds, d, p in streams:
            inflater.set_site_tally(dt, ds, seq)
            native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)
        lists.append(dt.finish(host.bytes_address(seq) if host is not None else None))
        assert inflater.site_tally is None
    return D.lists_as_dict(ref.names, lists)


def _host_lists(hand, rule) -> dict:
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    host = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
    for ds, s in enumerate("TN"):
        ReadTable(hand["files"][s], threads=2, site_tally=(host, ds))
    return D.lists_as_dict(host.names, [host.finish(i) for i in range(3)])


@pytest.mark.parametrize("rule", R.RULES, ids=lambda r: f"q{r.q}m{r.m}f{r.f:x}{r.mode}")
def test_columns_with_a_ruled_tally_match_the_restatement_and_the_host(inflater, hand, rule):
    t, n = hand["recs"]
    assert len(t) > 256 and len(n) > 256 and {48, 49, 64, 65, 129} <= {len(r["cigar"]) for r in t}
    exp = R.expected_hand(rule)
    assert _host_lists(hand, rule) == exp
    assert _device_lists(inflater, hand, [(0, t), (1, n)], rule) == exp
    # either dataset first and the stream tallied twice: the filters leave the OR what it is
    assert _device_lists(inflater, hand, [(1, n), (0, t), (0, t), (1, n)], rule) == exp


def test_zero_rule_is_the_existing_call(inflater, hand):
    t, n = hand["recs"]
    exp = R.expected_hand(R.ZERO)
    assert _device_lists(inflater, hand, [(0, t), (1, n)], None) == exp
    assert _device_lists(inflater, hand, [(0, t), (1, n)], R.ZERO) == exp
    # one dataset alone: no site under both; under normal the normal's alone is enough, the tumor's is not
    assert _device_lists(inflater, hand, [(0, t)], R.FULL) == {} == _device_lists(inflater, hand, [(0, t)], R.FULL_NORMAL)
    ev: dict = {}
    fa = R.hand_built()[2]
    R.tally_records(ev, n, fa, 1, R.FULL_NORMAL)
    assert _device_lists(inflater, hand, [(1, n)], R.FULL_NORMAL) == R.sites_of(ev, fa, "normal") != {}
    assert _device_lists(inflater, hand, [(1, n)], R.FULL) == {}


@pytest.mark.parametrize("host_side", ["normal_on_host", "tumor_on_host", "halves"])
def test_host_and_device_halves_are_ored_in_the_compaction_under_normal(inflater, hand, host_side):
    """Mode normal reads the high nibble of the OR of both sides: with the normal's evidence on the host side
    alone (the device saw tumor records only) the sites are all there; with it on the device side alone the
    host's tumor bytes change nothing; with each dataset split over both sides the halves add up."""
    from genomeanonymizer_amd.discover_sites import HostTally
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    t, n = hand["recs"]
    rule = R.FULL_NORMAL
    exp = R.expected_hand(rule)
    on_host, on_dev = {"normal_on_host": ([(1, n)], [(0, t)]), "tumor_on_host": ([(0, t)], [(1, n)]),
                       "halves": ([(0, t[1::2]), (1, n[0::2])], [(0, t[0::2]), (1, n[1::2])])}[host_side]
    host = HostTally.of_fasta(hand["fasta"], R.site_rule(rule))
    for k, (ds, recs) in enumerate(on_host):
        path = os.path.join(hand["dir"], f"{host_side}_{k}.bam")
        write_bgzf(path, R.stream_of(recs)[0].tobytes())
        ReadTable(path, threads=2, site_tally=(host, ds))
    dev_only = _device_lists(inflater, hand, on_dev, rule)
    assert (dev_only == exp) == (host_side == "tumor_on_host")
    assert _device_lists(inflater, hand, on_dev, rule, host) == exp
    # ... and the same split under rule both
    hb = HostTally.of_fasta(hand["fasta"], R.site_rule(R.FULL))
    for k, (ds, recs) in enumerate(on_host):
        ReadTable(os.path.join(hand["dir"], f"{host_side}_{k}.bam"), threads=2, site_tally=(hb, ds))
    assert _device_lists(inflater, hand, on_dev, R.FULL) != R.expected_hand(R.FULL)
    assert _device_lists(inflater, hand, on_dev, R.FULL, hb) == R.expected_hand(R.FULL)


def test_kernel_list(inflater, hand):
    """A filtered tally runs under the kernel names an unfiltered one runs under; without a tally no kernel
    is added."""
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import HostTally
    d, p = R.stream_of(hand["recs"][1])
    ref = HostTally.of_fasta(hand["fasta"])
    lists = {}
    tallies = {"plain": native.DeviceTally(inflater, ref.reference_of(2), int(ref.lengths[2])),
               "filtered": native.DeviceTally(inflater, ref.reference_of(2), int(ref.lengths[2]), R.site_rule(R.FULL_NORMAL))}
    try:
        for tag in ("none", "plain", "filtered", "cleared"):
            inflater.set_profiling(True)
            inflater.set_site_tally(tallies.get(tag), 1, 2)
            native.bam_columns_device(inflater.handle, d, p, len(d), on_host=True)
            lists[tag] = [k for k, _ in inflater.kernel_times()]
            inflater.set_profiling(False)
        for tag, dt in tallies.items():
            inflater.set_profiling(True)
            pos, _ = dt.finish()
            lists["compact_" + tag] = [k for k, _ in inflater.kernel_times()]
            lists["n_" + tag] = len(pos)
            inflater.set_profiling(False)
    finally:
        inflater.set_site_tally(None)
    assert "k_bam_site_tally" not in lists["none"] and lists["none"] == lists["cleared"]
    assert lists["plain"] == lists["filtered"] == lists["none"] + ["k_bam_site_tally"], lists
    assert lists["n_plain"] == 0 and lists["n_filtered"] > 0                 # (the normal alone: sites under normal only)
    # (the context reports a name once, with its launches: the write pass of a tally with sites adds no name)
    assert lists["compact_plain"] == lists["compact_filtered"] == ["k_site_compact", "site_scan"], lists


def test_device_region_reads_discover_what_host_region_reads_do(inflater, tmp_path):
    import dataclasses
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.discover_sites import discover
    from genomeanonymizer_amd.io.fasta import FastaRef
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario("fuzz3500"), bam_index=True), str(tmp_path / "in"))
    fasta = FastaRef(p["ref"])
    plain = discover(p["T"], p["N"], fasta, 4)
    for rule in (Q20, Q20N):
        host = discover(p["T"], p["N"], fasta, 4, rule=R.site_rule(rule))
        native.decode_phase_times(reset=True)
        dev = discover(p["T"], p["N"], fasta, 4, inflater=inflater, rule=R.site_rule(rule))
        ph = native.decode_phase_times(reset=True)
        assert ph["device_regions"] > 0, ph
        assert D.panel_as_dict(dev) == D.panel_as_dict(host) and host.n_sites >= 50
        assert D.panel_as_dict(host) != D.panel_as_dict(plain)


# ---- the pipeline ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_anon(hip_built):
    from genomeanonymizer_amd.anonymizer_methods import CompleteGermlineAnonymizer
    return CompleteGermlineAnonymizer(device=0)


@pytest.mark.parametrize("mode", ["streamed", "jobs"])
def test_hip_pipeline_equals_the_oracle_engine_run(mode, gpu_anon, tmp_path, monkeypatch):
    from genomeanonymizer_amd import native
    index = M.set_mode(monkeypatch, mode, None)
    H.set_option(monkeypatch, False)
    K.set_option(monkeypatch, None)
    set_option(monkeypatch, True)
    unfiltered = K.run_files("tiny", str(tmp_path / "cpu0"), H.oracle_anonymizer(), index)
    R.set_rule(monkeypatch, Q20N)
    cpu = K.run_files("tiny", str(tmp_path / "cpu"), H.oracle_anonymizer(), index)
    monkeypatch.setenv("GANON_GPU_INFLATE", "1")
    monkeypatch.setenv("GANON_GPU_INFLATE_MIN", "1")
    native.decode_phase_times(reset=True)
    got = K.run_files("tiny", str(tmp_path / "gpu"), gpu_anon, index)
    ph = native.decode_phase_times(reset=True)
    assert got == cpu and got != M.golden_files("tiny") and got != unfiltered
    if mode == "jobs":
        assert ph["device_regions"] > 0, ph          # (region reads decoded, tallied and masked on the device)
