"""The hand-built FASTQ record sets (tests/fastq_sets.py) through every compiled HIP formatter
instance, against the plain per-record formatter that tests/test_fastq_sets.py holds equal to the
oracle and to the host formatter on the same sets. The expected bytes are computed once per set, not
once per instance.

Found by these sets (test_lattice_* on every instance and test_many_records_cross_the_scan_carry
failed on the formatter as it was before them): ganon_fastq_upload packed the offset of an empty
base or quality field relative to its buffer's lowest *used* byte; an empty field uses none, so its
offset can lie below that, and the negative difference overwrote the record's buffer, reverse,
qual_rev and mate bits (a '/' where the mate digit belongs, qualities printed backwards)."""
import functools

import pytest

import fastq_sets as S
from genomeanonymizer_amd import native


@pytest.fixture(scope="module", params=[0, 15, 17, 13, 14, 16, 12, 9, 11],
                ids=["span3", "span3_search", "span3_coarse", "span2", "span2_t2", "quad2", "rows", "quad1",
                     "quad2_select"])
def masker(hip_built, request):
    """Every compiled formatter instance (GANON_PARAM_FASTQ_KD), as in test_fastq.py."""
    m = native.HipMasker(0)
    m.set_param(native.PARAM_FASTQ_KD, request.param)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def _lattice(spaced):
    r = S.phase_lattice(spaced=spaced)
    return r, S.ref_format(r)


@functools.lru_cache(maxsize=None)
def _ladder(style):
    r = S.boundary_ladder(style)
    return r, S.ref_format(r)


@functools.lru_cache(maxsize=None)
def _aligned():
    return [(name, r, S.ref_format(r)) for name, r in S.aligned_tiles().items()]


@functools.lru_cache(maxsize=None)
def _long():
    r = S.long_fields()
    return r, S.ref_format(r)


@functools.lru_cache(maxsize=None)
def _wide():
    r = S.wide_qualities()
    return r, S.ref_format(r)


@functools.lru_cache(maxsize=None)
def _q7():
    return [(r, want, S.ref_format(r)) for r, want in S.q7_probes()]


def _first_diff(got, exp):
    n = min(len(got), len(exp))
    k = next((i for i in range(n) if got[i] != exp[i]), n)
    return f"lengths {len(got)} / {len(exp)}, first difference at byte {k}: {got[max(0, k - 24):k + 24]!r} != " \
           f"{exp[max(0, k - 24):k + 24]!r}"


def _same(got, exp):
    assert isinstance(exp, bytes)
    assert got == exp, _first_diff(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("spaced", [False, True], ids=["plain", "spaced"])
def test_lattice_one_shot(masker, spaced):
    recs, exp = _lattice(spaced)
    _same(masker.format_fastq(recs), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("spaced", [False, True], ids=["plain", "spaced"])
def test_lattice_resident_two_runs(masker, spaced):
    """upload / run / run / download: the second run gives the same bytes (k_fq_bscan re-arms the
    error slot and the dense-tile counter)."""
    recs, exp = _lattice(spaced)
    f = masker.fastq_upload(recs)
    try:
        assert f.n_bytes == len(exp)
        f.run()
        _same(f.download(), exp)
        f.run()
        _same(f.download(), exp)
    finally:
        f.free()


@pytest.mark.gpu
@pytest.mark.parametrize("style", ["sparse", "dense"])
def test_boundary_ladder(masker, style):
    recs, exp = _ladder(style)
    _same(masker.format_fastq(recs), exp)


@pytest.mark.gpu
def test_aligned_tiles(masker):
    for name, recs, exp in _aligned():
        assert isinstance(exp, bytes)
        got = masker.format_fastq(recs)
        assert got == exp, f"{name}: {_first_diff(got, exp)}"


@pytest.mark.gpu
def test_long_fields(masker):
    recs, exp = _long()
    _same(masker.format_fastq(recs), exp)


@pytest.mark.gpu
def test_wide_qualities(masker):
    recs, exp = _wide()
    _same(masker.format_fastq(recs), exp)


@pytest.mark.gpu
def test_q7_index_at_every_position_of_a_cut_read(masker):
    n = 0
    for k, (recs, want, ref) in enumerate(_q7()):
        if want is None:
            continue
        assert ref == want
        with pytest.raises(native.FastqBadRecord) as ei:
            masker.format_fastq(recs)
        assert ei.value.index == want, f"probe {k}"
        n += 1
    assert n == 81


@pytest.mark.gpu
def test_q7_clean_neighbours(masker):
    clean = [(recs, ref) for recs, want, ref in _q7() if want is None]
    assert len(clean) == 2
    for recs, ref in clean:
        _same(masker.format_fastq(recs), ref)      # (a FastqBadRecord here: a neighbour's nibble was flagged)


@pytest.mark.gpu
def test_many_records_cross_the_scan_carry(hip_built):
    """More than 2048 x 1024 records: k_fq_bscan carries its running sum into a second and a third
    round. The scan kernels are shared by every instance, so the default one runs."""
    recs = S.many_records()
    exp = S.many_expected()
    m = native.HipMasker(0)
    try:
        got = m.format_fastq(recs)
    finally:
        m.close()
    assert len(got) == native.fastq_bytes(recs)
    assert got == exp, _first_diff(got, exp)
