"""The device record walk (csrc/ganon_bam.hip: k_bam_guess, k_bam_check, k_bam_fix, k_bam_offsets,
k_bam_sizes, k_bam_scatter) on the hand-built streams of tests/bam_streams.py. The expectation is the
specification's restatement (tests/bam_reference.py) with the one documented rule for names without
their NUL — neither of the project's decoders —, ``rec_off`` is the sequential walk, and ``fixes`` is
each stream's literal, which tests/test_bam_streams.py ties to the boundary proof's restatement at the
constants the library reports here. What each stream pins is in its builder's docstring."""
import numpy as np
import pytest

import bam_streams as S
import namehash_helpers as H

pytestmark = pytest.mark.gpu

STREAMS = S.all_streams()
BY_NAME = {b.name: b for b in STREAMS}
ERRORS = S.error_streams()


@pytest.fixture(scope="module")
def ctx(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.close()


def assert_built(cols, fixes, b, names=True):
    assert len(cols["pos"]) == len(b.rec_off), b.name
    for f in S.COLS + S.BLOBS:
        if not names and f in ("name_len", "name_off", "names_blob"):
            continue
        assert np.array_equal(cols[f], b.cols[f]), (b.name, f)
    assert np.array_equal(cols["rec_off"], b.rec_off), b.name
    assert fixes == b.fixes, b.name


def decode(ctx, b):
    from genomeanonymizer_amd import native
    return native.bam_columns_device(ctx.handle, b.array(), b.p, b.n, on_host=True)


def inflate_on_device(ctx, tmp_path, data: bytes) -> None:
    """``data`` BGZF-packed by the project's writer and inflated by the device inflate: the bytes
    stay on the device for ``ctx.bam_columns``."""
    from test_bam_device import write_raw_bam
    path = str(tmp_path / "packed.bam")
    write_raw_bam(path, data)
    raw = open(path, "rb").read()
    pay, isz, off = [], [], 0
    while off < len(raw):
        xlen = raw[off + 10] | (raw[off + 11] << 8)
        blen = (raw[off + 16] | (raw[off + 17] << 8)) + 1   # (the writer's BC subfield is the only one)
        n = int.from_bytes(raw[off + blen - 4:off + blen], "little")
        if n:
            pay.append(raw[off + 12 + xlen:off + blen - 8])
            isz.append(n)
        off += blen
    in_len = np.array([len(x) for x in pay], np.int32)
    in_off = np.concatenate([[0], np.cumsum(in_len[:-1])]).astype(np.int64)
    out = ctx.inflate(np.frombuffer(b"".join(pay), np.uint8), in_off, in_len, np.array(isz, np.int32))
    assert out.tobytes() == data


def test_library_reports_the_constants_the_streams_sit_on(hip_built):
    """A retuned kChunk, kProbe, kGuessSpan, GANON_SCAT_STAGE or GANON_SCAT_RECS fails here: the
    streams would no longer lie on the kernel's edges."""
    from genomeanonymizer_amd import native
    assert native.bam_walk_params() == S.WALK_DEFAULTS


@pytest.mark.parametrize("name", [b.name for b in STREAMS])
def test_columns_offsets_and_fixes(ctx, name):
    b = BY_NAME[name]
    cols, fixes = decode(ctx, b)
    assert_built(cols, fixes, b)


def test_walk_from_a_later_record_and_an_empty_range(ctx):
    """The grid stream entered at its record 40 (another grid origin: the same records, found again)
    and at n (no record)."""
    from genomeanonymizer_amd import native
    b = BY_NAME["grid"]
    k = int(b.rec_off[40])
    cols, fixes = native.bam_columns_device(ctx.handle, b.array(), k, b.n, on_host=True)
    from test_bam_device import _walk_chunks
    recs, want = _walk_chunks(b.data, k, S.CHUNK, probe=S.PROBE, span=S.GUESS_SPAN)
    assert recs == b.rec_off[40:].tolist() and fixes == want
    assert np.array_equal(cols["rec_off"], b.rec_off[40:])
    for f in ("pos", "end", "tlen", "aux_len"):
        assert np.array_equal(cols[f], b.cols[f][40:]), f
    assert np.array_equal(cols["aux"], b.cols["aux"][b.cols["aux_off"][40]:])
    cols, fixes = native.bam_columns_device(ctx.handle, b.array(), b.n, b.n, on_host=True)
    assert len(cols["pos"]) == 0 and len(cols["aux"]) == 0 and fixes == 0


def test_device_resident_streams_do_not_see_stale_bytes(ctx, tmp_path):
    """The tail and grid streams inflated on the device and decoded where the inflate left them,
    after a larger stream went through the same context: the cached buffers then hold that stream's
    bytes past n and its chunk flags, and nothing may depend on them."""
    big = BY_NAME["staging_r3_fits"]
    for b in [BY_NAME["grid"]] + [x for x in STREAMS if x.name.startswith("tail_")]:
        inflate_on_device(ctx, tmp_path, big.data)
        cols, fixes = ctx.bam_columns(big.p, big.n)
        assert_built(cols, fixes, big)
        inflate_on_device(ctx, tmp_path, b.data)
        cols, fixes = ctx.bam_columns(b.p, b.n)
        assert_built(cols, fixes, b)


def test_large_small_large_on_one_context_equals_fresh_contexts(hip_built):
    from genomeanonymizer_amd import native
    seq = [BY_NAME["staging_r1_over"], BY_NAME["tail_p3_n1_only"], BY_NAME["staging_r1_over"]]
    one = native.GpuInflater(0, min_blocks=1)
    try:
        kept = [decode(one, b) for b in seq]
    finally:
        one.close()
    for b, (cols, fixes) in zip(seq, kept):
        g = native.GpuInflater(0, min_blocks=1)
        try:
            fresh, fresh_fixes = decode(g, b)
        finally:
            g.close()
        assert fixes == fresh_fixes == b.fixes
        assert set(cols) == set(fresh)
        for f in cols:
            assert np.array_equal(cols[f], fresh[f]), (b.name, f)
        assert_built(cols, fixes, b)


@pytest.mark.parametrize("name", ["fields", "staging_r2_fits", "staging_r1_over"])
def test_hashed_instantiations(ctx, name):
    """k_bam_sizes<true> / k_bam_scatter<true>: with a name key every column but the names is the
    unkeyed expectation; the names are hashlib's of the names the restatement reports."""
    b = BY_NAME[name]
    ctx.set_name_key(H.KEY)
    try:
        cols, fixes = decode(ctx, b)
    finally:
        ctx.set_name_key(None)
    assert_built(cols, fixes, b, names=False)
    n = len(b.rec_off)
    assert np.array_equal(cols["name_len"], np.full(n, 32, np.int32))
    assert np.array_equal(cols["name_off"], 33 * np.arange(n, dtype=np.int64))
    blob = b.cols["names_blob"].tobytes()
    plain = [blob[o:o + l] for o, l in zip(b.cols["name_off"].tolist(), b.cols["name_len"].tolist())]
    assert cols["names_blob"].tobytes() == b"".join(H.hashed(x, H.KEY) + b"\x00" for x in plain)
    cols, fixes = decode(ctx, b)   # (the key cleared: the unkeyed kernels again)
    assert_built(cols, fixes, b)


@pytest.mark.parametrize("bad", ERRORS, ids=lambda e: e.name)
def test_error_streams_raise_the_hosts_message(ctx, bad):
    from genomeanonymizer_amd import native
    with pytest.raises(native.GanonError, match=bad.host_error) as ei:
        native.bam_columns_device(ctx.handle, bad.array(), bad.p, len(bad.data), on_host=True)
    import re
    assert re.search(bad.device_error, str(ei.value)), str(ei.value)
    good = BY_NAME["tail_p2_n3_second"]   # the context then decodes a good stream
    cols, fixes = decode(ctx, good)
    assert_built(cols, fixes, good)
