"""The GPU inflate (ganon_inflate.hip) against hand-built DEFLATE streams.

tests/test_inflate.py feeds the decoder what zlib's deflate writes; this module feeds it the rest
of RFC 1951 (tests/inflate_cases.py, written with tests/deflate_craft.py): runs of tiny stored
blocks, overlapping matches across the output ring's wrap, matches at the near/far split and the
flush frontier, rounds at their literal / match / output limits, 15-bit codes, lone and absent
distance codes, every way a stream can end, ~150 seeded random streams; and a malformed set.

Two independent references: the token list expanded in Python (``expand``) and zlib's inflate. The
decoder runs three ways: its source on the host with one lane (tools/inflate_host_check.cpp, also
as a stand-alone ASan + UBSan build: the tool allocates every output at exactly ISIZE bytes), the
kernel with token rounds, and the scalar-only kernel (GANON_INFLATE_ROUNDS=0, a child process).
"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

from inflate_cases import malformed_set, valid_set
from test_inflate import _soa

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _pairs(cases):
    return [(s, t) for s, t, _ in cases]


def _first_diff(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if len(a) != len(b):
        return "length %d, expected %d" % (len(a), len(b))
    d = np.flatnonzero(a != b)
    return "%d wrong bytes, the first at %d" % (len(d), d[0])


def _check_outputs(out, cases, what):
    """out: the cases' outputs back to back."""
    bad, off = [], 0
    for _, t, label in cases:
        got = bytes(out[off:off + len(t)])
        if got != t:
            bad.append("%s: %s" % (label, _first_diff(got, t)))
        off += len(t)
    assert not bad, "%s: %d of %d streams differ from zlib:\n%s" % (what, len(bad), len(cases), "\n".join(bad[:20]))


def test_crafted_streams_are_what_zlib_inflates():
    """The writer itself: zlib inflates every crafted valid stream to the direct expansion of its
    tokens. (A stream zlib refuses is a bug in tests/deflate_craft.py.)"""
    cases = valid_set()
    assert len(cases) > 180
    for s, t, label in cases:
        assert len(t) <= 65536, label
        assert zlib.decompress(s, -15) == t, label
    kinds = {(s[0] >> 1) & 3 for s, _, _ in cases}
    assert kinds == {0, 1, 2}


def test_malformed_streams_are_refused_by_zlib():
    """Every malformed case is one zlib rejects, or one that inflates to another length than its
    isize. (inflate_cases.malformed_set: an incomplete literal/length code that the stream never
    exercises is accepted by this decoder and rejected by zlib; it is left out of the set.)"""
    for s, n, label in malformed_set():
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(s)
            ok = d.eof and len(got) == n
        except zlib.error:
            ok = False
        assert not ok, label


# ---- the decoder source on the host ------------------------------------------------------------

def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not available")
    return hipcc


def _run_tool(exe, d, streams):
    """(statuses, outputs back to back, the tool's stderr) of tools/inflate_host_check over
    (stream, bytes of the expected length) pairs."""
    comp, in_off, in_len, out_len = _soa(streams)
    comp.tofile(d / "comp.bin")
    meta = np.stack([in_off, in_len.astype(np.int64), out_len.astype(np.int64)], 1).ravel()
    np.concatenate([[len(streams)], meta]).astype(np.int64).tofile(d / "meta.bin")
    r = subprocess.run([exe, str(d / "comp.bin"), str(d / "meta.bin"), str(d / "out.bin")], capture_output=True,
                       text=True)
    assert r.returncode == 0, "inflate_host_check exited with %d:\n%s" % (r.returncode, r.stderr[-4000:])
    return [int(x) for x in r.stdout.split()], open(d / "out.bin", "rb").read(), r.stderr


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/inflate_host_check.cpp built as tests/test_inflate.py builds it, but for the host code
    at -O0: a build of seconds (the decoder is one function once inlined; -O2 takes over a minute)."""
    hipcc = _hipcc()
    exe = str(tmp_path_factory.mktemp("ihc2") / "inflate_host_check")
    subprocess.run([hipcc, "-O0", "-Xarch_device", "-O2", "-std=c++17", "--offload-arch=gfx950", "-x", "hip",
                    os.path.join(ROOT, "tools", "inflate_host_check.cpp"), "-o", exe], check=True)
    d = tmp_path_factory.mktemp("ihc2_io")
    return lambda streams: _run_tool(exe, d, streams)


@pytest.fixture(scope="module")
def host_check_sanitized(tmp_path_factory):
    """The same tool with its host code under AddressSanitizer and UBSan (a stand-alone program:
    nothing is preloaded). The sanitizer flags reach the host compile only (-Xarch_host) and the
    link of the finished object; the device code is compiled without them."""
    hipcc = _hipcc()
    d = tmp_path_factory.mktemp("ihc_san")
    obj, exe = str(d / "inflate_host_check_san.o"), str(d / "inflate_host_check_san")
    # (host code at -O0: the optimizer takes minutes over the instrumented decoder, one function
    # once inlined, and seconds without)
    subprocess.run([hipcc, "-O0", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-Xarch_device", "-O2",
                    "-Xarch_host", "-g",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    "-c", os.path.join(ROOT, "tools", "inflate_host_check.cpp"), "-o", obj], check=True)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fno-gpu-sanitize", "-fsanitize=address,undefined", obj, "-o", exe], check=True)
    d = tmp_path_factory.mktemp("ihc_san_io")
    return lambda streams: _run_tool(exe, d, streams)


def test_decoder_source_on_crafted_streams(host_check):
    """On the commit before the stored-block flush fix, "3000 blocks of 3 bytes" returned status 0
    with 804 wrong bytes among the first 808 (the 8 KiB ring wrapped before the only flush), and the
    match at distance 4300 behind 1500 such blocks copied 99 wrong bytes out of 100."""
    cases = valid_set()
    status, out, _ = host_check(_pairs(cases))
    bad = [label for st, (_, _, label) in zip(status, cases) if st != 0]
    assert not bad, "rejected valid streams: %s" % bad[:20]
    _check_outputs(out, cases, "host decoder")


def test_decoder_source_rejects_malformed(host_check):
    bad = malformed_set()
    status, _, _ = host_check([(s, b"\x00" * n) for s, n, _ in bad])
    assert len(status) == len(bad)
    accepted = [label for st, (_, _, label) in zip(status, bad) if st == 0]
    assert not accepted, "accepted malformed streams: %s" % accepted


def test_decoder_source_sanitized(host_check_sanitized):
    """ASan + UBSan over both sets: exit 0, no report, the expected statuses and bytes."""
    cases, bad = valid_set(), malformed_set()
    status, out, err = host_check_sanitized(_pairs(cases))
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert status == [0] * len(cases)
    _check_outputs(out, cases, "sanitized host decoder")
    status, _, err = host_check_sanitized([(s, b"\x00" * n) for s, n, _ in bad])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert len(status) == len(bad) and all(st != 0 for st in status), \
        [label for st, (_, _, label) in zip(status, bad) if st == 0]


# ---- the kernel --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_inflater(hip_built):
    from genomeanonymizer_amd import native
    g = native.GpuInflater(0, min_blocks=1)
    yield g
    g.close()


def _inflate_at(g, streams, out_off, out_total):
    """ganon_inflate with the caller's output offsets (GpuInflater.inflate always packs the slots):
    (return code, first bad block, the host output buffer, the context's last error)."""
    comp, in_off, in_len, out_len = _soa(streams)
    out_off = np.ascontiguousarray(out_off, np.int64)
    out = np.full(out_total, 0xEE, np.uint8)
    bad = np.full(1, -1, np.int64)
    u8, i32, i64 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    lib = g._lib
    rc = lib.ganon_inflate(g.handle, comp.ctypes.data_as(u8), len(comp), in_off.ctypes.data_as(i64),
                           in_len.ctypes.data_as(i32), out_off.ctypes.data_as(i64), out_len.ctypes.data_as(i32),
                           len(streams), out.ctypes.data_as(u8), out_total, bad.ctypes.data_as(i64))
    return rc, int(bad[0]), out, lib.ganon_last_error(g.handle).decode(errors="replace")


@pytest.mark.gpu
def test_gpu_crafted_streams_one_launch(gpu_inflater):
    cases = valid_set()
    comp, in_off, in_len, out_len = _soa(_pairs(cases))
    out = gpu_inflater.inflate(comp, in_off, in_len, out_len)
    _check_outputs(out.tobytes(), cases, "k_inflate")


@pytest.mark.gpu
@pytest.mark.parametrize("rem", [1, 2, 3])
def test_gpu_crafted_streams_unaligned_output(gpu_inflater, rem):
    """Output slots at offsets = rem (mod 4): flush_out's byte path, and its dword path behind a
    byte head."""
    cases = [c for i, c in enumerate(valid_set()) if not c[2].startswith("random") or i % 4 == 0]
    out_off, off = [], 0
    for _, t, _ in cases:
        off += (rem - off) % 4
        out_off.append(off)
        off += len(t)
    rc, bad, out, msg = _inflate_at(gpu_inflater, _pairs(cases), out_off, off + 5)
    assert rc == 0, msg
    wrong = ["%s: %s" % (label, _first_diff(out[o:o + len(t)].tobytes(), t))
             for o, (_, t, label) in zip(out_off, cases) if out[o:o + len(t)].tobytes() != t]
    assert not wrong, "\n".join(wrong[:20])


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
from genomeanonymizer_amd import native
from inflate_cases import valid_set
from test_inflate import _soa
cases = valid_set()
g = native.GpuInflater(0, min_blocks=1)
out = g.inflate(*_soa([(s, t) for s, t, _ in cases])).tobytes()
g.close()
off, bad = 0, []
for _, t, label in cases:
    if out[off:off + len(t)] != t:
        bad.append(label)
    off += len(t)
print("crafted", len(cases), "bad", len(bad))
for b in bad:
    print("differs:", b)
sys.exit(1 if bad else 0)
"""


@pytest.mark.gpu
def test_gpu_crafted_streams_scalar_only_kernel(hip_built):
    """k_inflate<false> (GANON_INFLATE_ROUNDS=0 is read once per process: a fresh child)."""
    env = dict(os.environ, GANON_INFLATE_ROUNDS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.dirname(os.path.abspath(__file__))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "crafted %d bad 0" % len(valid_set()) in r.stdout


@pytest.mark.gpu
def test_gpu_rejected_block_leaves_its_neighbours_alone(gpu_inflater):
    """A malformed block between two good ones: the call fails and names it, both neighbours are
    exact, and no byte of the 256-byte gaps around it is touched. The gaps are read through the
    context's grow-only output buffer, which a first call fills with a known byte; a control call
    of good blocks proves that premise before anything is concluded from it."""
    from deflate_craft import DeflateWriter
    fill = 0x5A
    valid = {label: (s, t) for s, t, label in valid_set()}
    a = valid["overlap: distances 160..257, lengths 258 and d + 1, dynamic"]
    b = valid["boundary: a full round, then 258 at distance 4097"]
    c = valid["slow codes: 286 + 30 symbols in use, lengths to 15 (1)"]
    gap = 256
    total = len(a[1]) + gap + 65536 + gap + len(b[1])
    tiles, o = [], 0
    while o < total:
        n = min(65535, total - o)
        w = DeflateWriter()
        w.stored(bytes([fill]) * n, True)
        tiles.append((w.getvalue(), bytes([fill]) * n, o))
        o += n

    def paint():
        rc, _, out, msg = _inflate_at(gpu_inflater, [(s, t) for s, t, _ in tiles], [o for _, _, o in tiles], total)
        assert rc == 0, msg
        assert (out == fill).all()

    def layout(mid_len):
        o1 = len(a[1]) + gap
        o2 = total - len(b[1])   # (the last block ends the buffer: the call copies back up to its end)
        assert o2 >= o1 + mid_len + gap
        return [0, o1, o2]

    def check_around(out, offs, mid_len):
        assert out[:len(a[1])].tobytes() == a[1], "the block before: " + _first_diff(out[:len(a[1])].tobytes(), a[1])
        got = out[offs[2]:offs[2] + len(b[1])].tobytes()
        assert got == b[1], "the block after: " + _first_diff(got, b[1])
        gaps = np.concatenate([out[len(a[1]):offs[1]], out[offs[1] + mid_len:offs[2]]])
        return int((gaps != fill).sum())

    # control: good blocks and gaps; the gaps still hold the first call's bytes
    paint()
    offs = layout(len(c[1]))
    rc, _, out, msg = _inflate_at(gpu_inflater, [a, c, b], offs, total)
    assert rc == 0, msg
    assert out[offs[1]:offs[1] + len(c[1])].tobytes() == c[1]
    assert check_around(out, offs, len(c[1])) == 0, \
        "premise broken: the context did not keep its output buffer between calls; the gap check proves nothing"
    for s, n, label in malformed_set():
        paint()
        offs = layout(n)
        rc, bad, out, msg = _inflate_at(gpu_inflater, [a, (s, b"\x00" * n), b], offs, total)
        assert rc != 0 and bad == 1 and "block 1" in msg, (label, rc, bad, msg)
        touched = check_around(out, offs, n)
        assert touched == 0, "%s: %d gap bytes were overwritten" % (label, touched)
    # the context still works
    rc, _, out, msg = _inflate_at(gpu_inflater, [c], [0], len(c[1]))
    assert rc == 0 and out.tobytes() == c[1], msg
