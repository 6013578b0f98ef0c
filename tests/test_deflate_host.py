"""The GPU deflate's encoder source run on the host (tools/deflate_host_check.cpp over
csrc/ganon_deflate_core.h, one lane): DEFLATE and gzip are fixed formats (RFC 1951 / 1952), so
Python's zlib is the oracle — every member must inflate to its block and carry zlib's CRC32. The
same program runs under ASan/UBSan as a stand-alone executable. CPU only."""
import gzip
import shutil
from fractions import Fraction

import pytest

import deflate_fixtures as F


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    return F.build_host_check(tmp_path_factory.mktemp("dhc"))


@pytest.fixture(scope="module")
def members(exe, tmp_path_factory):
    blocks = [b for _, b in F.fixture_blocks()]
    stream, sizes = F.run_blocks(exe, tmp_path_factory.mktemp("dhc_io"), blocks)
    return blocks, stream, sizes


def test_members_inflate_to_their_blocks(members):
    blocks, stream, sizes = members
    types = F.check_members(stream, blocks)
    assert [m[3] for m in F.walk_members(stream)] == sizes
    # the whole stream is one valid multi-member gzip file
    assert gzip.decompress(stream + F.EOF_MEMBER) == b"".join(blocks)
    by_name = dict(zip([n for n, _ in F.fixture_blocks()], zip(types, sizes, blocks)))
    assert set(types) == {0, 2}                          # stored and dynamic first blocks both occur
    for name in ("one_byte", "two_bytes", "noise_full", "three"):
        assert by_name[name][0] == 0, name
        assert by_name[name][1] == len(by_name[name][2]) + 31
    assert by_name["noise_full"][1] <= 65536
    for name in ("zeros_full", "run259", "no_repeat", "one_distance", "window_edge", "config1", "longpair"):
        assert by_name[name][0] == 2, name
    assert by_name["zeros_full"][1] < 400                # length-258 matches at distance 1
    assert by_name["run259"][1] < 60
    assert by_name["window_edge"][1] < 32768 + 1500      # the second half is matches at distance 32768
    assert by_name["one_distance"][1] < by_name["no_repeat"][1] + 30


def test_deterministic(exe, members, tmp_path):
    blocks, stream, _ = members
    again, _ = F.run_blocks(exe, tmp_path, blocks)
    assert again == stream
    # a block's member does not depend on the blocks before it
    one, _ = F.run_blocks(exe, tmp_path, blocks[-2:])
    assert stream.endswith(one)


def _kraft(lens):
    return sum(Fraction(1, 2 ** l) for l in lens if l)


def _fib(n):
    a, b, out = 1, 1, []
    for _ in range(n):
        out.append(a)
        a, b = b, a + b
    return out


def test_lengths_mode(exe):
    counts = _fib(22)
    assert sum(counts) == 46367
    lens = F.run_lengths(exe, 15, counts)
    assert all(1 <= l <= 15 for l in lens) and _kraft(lens) == 1
    assert lens == sorted(lens, reverse=True)            # rarer symbols never get shorter codes
    # (an unrestricted Huffman code of this histogram is 21 deep)
    lens = F.run_lengths(exe, 7, _fib(19))
    assert all(1 <= l <= 7 for l in lens) and _kraft(lens) == 1
    # unused symbols get no code; padded into the literal alphabet's size
    lens = F.run_lengths(exe, 15, [0, 5, 0, 9, 0, 0, 2] + [0] * 279)
    assert [l for l in lens if l] and all(l == 0 for i, l in enumerate(lens) if i not in (1, 3, 6))
    assert _kraft(lens) == 1 and lens[3] == 1 and lens[1] == lens[6] == 2
    # fewer than two used symbols: two one-bit codes (a complete code, the header logic's contract)
    assert F.run_lengths(exe, 15, [0] * 30) == [1, 1] + [0] * 28
    assert F.run_lengths(exe, 15, [0] * 7 + [12] + [0] * 22) == [1] + [0] * 6 + [1] + [0] * 22
    assert F.run_lengths(exe, 15, [4] + [0] * 29) == [1, 1] + [0] * 28
    assert F.run_lengths(exe, 7, [3, 0] + [0] * 17) == [1, 1] + [0] * 17


def test_under_sanitizers(members, tmp_path_factory):
    """The same program built with ASan/UBSan (a stand-alone executable, nothing preloaded): the same
    fixtures, the same bytes, no report."""
    blocks, stream, _ = members
    d = tmp_path_factory.mktemp("dhc_san")
    san = F.build_host_check(d, sanitize=True)
    got, _ = F.run_blocks(san, d, blocks)
    assert got == stream
    lens = F.run_lengths(san, 15, _fib(22))
    assert _kraft(lens) == 1
    assert F.run_lengths(san, 7, [0] * 19) == [1, 1] + [0] * 17
