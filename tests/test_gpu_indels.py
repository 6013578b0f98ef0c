"""The germline indel tally (ganon_indel.hip) on the hand-built batches of tests/indel_batches.py —
needs an MI355X.

Every batch sits on a path or a threshold that the upload chooses from the batch's shape (the thread
or the wave walk at 32 | 33 CIGAR ops, the in-place or the global sort at 4096 | 4097 observations of
a scope, the dense or the hashed map) or on a boundary inside a kernel; tests/test_indel_batches.py
pins the shapes and the expected records without a device. Here each batch runs under the default
settings and under every A/B switch; the records are compared one for one with the builder's, and
``ganon_indel_info``'s route bits must say that the intended route ran.
"""
import numpy as np
import pytest

import indel_batches as ib
from indel_batches import GSORT, HASHED, THREAD_WALK, TSORT

pytestmark = pytest.mark.gpu

CASES = ib.all_cases()
# name -> (environment read at the tally's upload, GANON_PARAM_INDEL_SORT)
ROUTES = {
    "default": ({}, 0),
    "wave_walk": ({"GANON_INDEL_WAVE_WALK": "1"}, 0),
    "dense_map": ({"GANON_INDEL_DENSE_MAP": "1"}, 0),
    "sort_seg": ({"GANON_INDEL_SORTMODE": "seg"}, 0),
    "sort_global": ({"GANON_INDEL_SORTMODE": "global"}, 0),
    "unfiltered": ({}, 1),
    "wave_walk+sort_global": ({"GANON_INDEL_WAVE_WALK": "1", "GANON_INDEL_SORTMODE": "global"}, 0),
    "dense_map+sort_seg": ({"GANON_INDEL_DENSE_MAP": "1", "GANON_INDEL_SORTMODE": "seg"}, 0),
}
_SWITCHES = ("GANON_INDEL_WAVE_WALK", "GANON_INDEL_DENSE_MAP", "GANON_INDEL_SORTMODE")


@pytest.fixture(scope="module")
def masker(hip_built):
    from genomeanonymizer_amd import native
    m = native.HipMasker(0)
    yield m
    m.close()


def expected_info(arr: dict, e: ib.Expect, env: dict, unfiltered: int) -> dict:
    """What ``info()`` must say after a run and a download: the route the switches leave of the
    batch's default route (a batch that wave-walks by its shape cannot thread-walk, and only a thread
    walk has the in-place and the global sort), and the counts that follow from it."""
    thread = bool(e.route & THREAD_WALK) and env.get("GANON_INDEL_WAVE_WALK") != "1"
    mode = env.get("GANON_INDEL_SORTMODE", "")
    tsort = thread and bool(e.route & TSORT) and mode == ""
    gsort = thread and not tsort and mode != "seg"
    dense = env.get("GANON_INDEL_DENSE_MAP") == "1" or not e.route & HASHED
    route = (THREAD_WALK if thread else 0) | (TSORT if tsort else 0) | (GSORT if gsort else 0) | (0 if dense else HASHED)
    pos_bits = max(1, int(arr["scope_span_len"].max()).bit_length())
    scope_bits = max(1, (len(arr["scope_span_len"]) - 1).bit_length())
    return {
        "route": route, "thread_walk": thread, "tsort": tsort, "gsort": gsort, "hashed_map": not dense,
        "map_log2_cells": 0 if dense else e.route >> 8,
        "observations": e.observations, "records": len(e.records), "global_sort": unfiltered,
        "emitted": e.observations if unfiltered else e.emitted_dense if dense else e.emitted,
        "key_bits": pos_bits + scope_bits if unfiltered or gsort else pos_bits,
    }


def tally(masker, arr, env, unfiltered, monkeypatch):
    """(records, info) of one upload, run and download under the given switches."""
    from genomeanonymizer_amd import native
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    db = masker.upload(arr)
    try:
        t = db.indel_tally(arr)
        try:
            masker.set_param(native.PARAM_INDEL_SORT, unfiltered)
            t.run()
            got = t.download()
            return got, t.info()
        finally:
            masker.set_param(native.PARAM_INDEL_SORT, 0)
            t.free()
    finally:
        db.free()


def assert_records(got: np.ndarray, e: ib.Expect, what):
    from genomeanonymizer_amd import native
    want = native.indel_records_array(e.records)
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got, want), (what, [tuple(r) for r in got[got != want][:4]],
                                       [tuple(r) for r in want[got != want][:4]])


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_batch_on_every_route(name, route, masker, monkeypatch):
    """Records, observations, filtered observations and route bits of every batch: under the default
    settings what the builder expects, under a switch what the switch leaves of it. The records are
    the same on every route."""
    arr, e = CASES[name]
    env, unfiltered = ROUTES[route]
    got, info = tally(masker, arr, env, unfiltered, monkeypatch)
    want = expected_info(arr, e, env, unfiltered)
    if route == "default":
        assert want["route"] | want["map_log2_cells"] << 8 == e.route and want["emitted"] == e.emitted
    assert {k: info[k] for k in want} == want, (name, route)
    assert_records(got, e, (name, route))


def test_walk_threshold_pair_takes_both_walks(masker, monkeypatch):
    """32 CIGAR ops of a read with an I/D op: a thread per read; 33: a wave per block. The 40-op read
    without an I/D op does not count."""
    infos = []
    for name in ("walk_32", "walk_33"):
        arr, e = CASES[name]
        got, info = tally(masker, arr, {}, 0, monkeypatch)
        assert_records(got, e, name)
        infos.append(info)
    assert (infos[0]["thread_walk"], infos[1]["thread_walk"]) == (True, False)
    assert (infos[0]["tsort"], infos[1]["tsort"]) == (True, False) and not infos[1]["gsort"]


def test_tsort_threshold_pair_takes_both_sorts(masker, monkeypatch):
    """4096 unfiltered observations in a scope: sorted in place with 32-bit keys; 4097: one 64-bit
    radix sort of the capacity (16 of the 4097 slots filled, the rest filler keys)."""
    infos = []
    for name in ("tsort_4096", "tsort_4097"):
        arr, e = CASES[name]
        got, info = tally(masker, arr, {}, 0, monkeypatch)
        assert_records(got, e, name)
        assert info["thread_walk"] and info["emitted"] == 16
        infos.append(info)
    assert (infos[0]["tsort"], infos[0]["gsort"]) == (True, False)
    assert (infos[1]["tsort"], infos[1]["gsort"]) == (False, True)
    assert (infos[0]["key_bits"], infos[1]["key_bits"]) == (7, 8)


def test_hash_collision_only_adds_positions(masker, monkeypatch):
    """Two positions of one cell, one with a tumor and one with a normal op, pass the hashed filter
    (and a third joins the real call's cell): more observations than under the dense map, classified
    to nothing — the same records."""
    arr, e = CASES["hash_collision"]
    got, info = tally(masker, arr, {}, 0, monkeypatch)
    assert (info["hashed_map"], info["map_log2_cells"], info["emitted"]) == (True, 12, e.emitted)
    assert_records(got, e, "hashed")
    got, info = tally(masker, arr, {"GANON_INDEL_DENSE_MAP": "1"}, 0, monkeypatch)
    assert (info["hashed_map"], info["map_log2_cells"], info["emitted"]) == (False, 0, e.emitted_dense)
    assert_records(got, e, "dense")
    assert e.emitted == e.emitted_dense + 3


@pytest.mark.parametrize("name", ["run_chunk", "tsort_order"])
def test_one_handle_runs_and_downloads_again(name, masker):
    """run, run, download, download; then the unfiltered run, and the filtered one again, on one
    handle: every download is the expectation, and the counts follow the last run."""
    from genomeanonymizer_amd import native
    arr, e = CASES[name]
    db = masker.upload(arr)
    t = db.indel_tally(arr)
    try:
        t.run()
        t.run()
        assert_records(t.download(), e, "run, run, download")
        assert_records(t.download(), e, "download again")
        assert t.info()["emitted"] == e.emitted
        for unfiltered in (1, 0):
            masker.set_param(native.PARAM_INDEL_SORT, unfiltered)
            t.run()
            assert_records(t.download(), e, ("unfiltered", unfiltered))
            info = t.info()
            assert info["global_sort"] == unfiltered
            assert info["emitted"] == (e.observations if unfiltered else e.emitted)
            assert info["records"] == len(e.records)
    finally:
        masker.set_param(native.PARAM_INDEL_SORT, 0)
        t.free()
        db.free()
