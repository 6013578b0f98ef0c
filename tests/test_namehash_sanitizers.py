"""ASan/UBSan build of the read-name hash (--hash_read_names): the shared core
(csrc/ganon_name_hash.h) and the keyed ``records_to_columns`` of csrc/ganon_host.cpp, linked into a
stand-alone driver (tests/sanitize/namehash_driver.cpp) with the sanitizer runtime — in the manner of
tests/test_sanitizers.py: nothing is preloaded and nothing is loaded into Python. Every hash the
driver prints is checked against ``hashlib.blake2s``. CPU only."""
import os
import shutil
import subprocess

import pytest

import namehash_helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "namehash_driver")
    r = subprocess.run(["g++", *SAN, "-std=c++17", "-pthread", "-o", exe,
                        os.path.join(REPO, "tests", "sanitize", "namehash_driver.cpp"),
                        os.path.join(REPO, "genomeanonymizer_amd", "csrc", "ganon_host.cpp"), "-lz", "-ldl"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split("\n")[:-1]


@pytest.mark.parametrize("key", H.KEYS, ids=lambda k: f"key{len(k)}")
def test_core_under_sanitizers(driver, key):
    lines = _run(driver, "core", key.hex())
    assert len(lines) == 256
    for L, line in enumerate(lines):
        name, _, got = line.rpartition(" ")
        name = bytes.fromhex(name)
        assert len(name) == L and got.encode() == H.hashed(name, key), L


def test_keyed_columns_under_sanitizers(driver, tmp_path):
    """The crafted stream of the device tests (every name length, a name without its NUL,
    l_read_name 0) through ganon_bam_open_keyed on one and three threads."""
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    d, _ = H.crafted_stream()
    path = str(tmp_path / "crafted.bam")
    write_bgzf(path, d.tobytes())
    exp = [H.hashed(x, H.KEY16).decode() for x in H.table_names(ReadTable(path))]
    assert len(exp) > 500
    for threads in ("1", "3"):
        assert _run(driver, "file", H.KEY16.hex(), path, threads) == exp


def test_keyed_reader_under_sanitizers(driver, tmp_path):
    import dataclasses
    from genomeanonymizer_amd.io.bam import BamReader
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario("fuzz2000"), bam_index=True), str(tmp_path / "in"))
    r = BamReader(p["T"], 2)
    exp = []
    for tid, L in enumerate(int(x) for x in r.ref_lens):
        exp += H.table_names(r.contig(tid))
        for k in range(3):
            exp += H.table_names(r.region(tid, k * L // 3, (k + 1) * L // 3))
    r.close()
    assert len(exp) > 100
    assert _run(driver, "reader", H.KEY.hex(), p["T"]) == [H.hashed(x).decode() for x in exp]
