"""ASan/UBSan build of the panel mask (--known_sites): csrc/ganon_known_sites.h inside the decoders of
csrc/ganon_host.cpp, linked into a stand-alone driver (tests/sanitize/known_sites_driver.cpp) with the
sanitizer runtime — in the manner of tests/test_namehash_sanitizers.py: nothing is preloaded and
nothing is loaded into Python. The bases and qualities the driver prints are checked against the
plain-Python rule of known_sites_helpers. CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import known_sites_helpers as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "known_sites_driver")
    r = subprocess.run(["g++", *SAN, "-std=c++17", "-pthread", "-o", exe,
                        os.path.join(REPO, "tests", "sanitize", "known_sites_driver.cpp"),
                        os.path.join(REPO, "genomeanonymizer_amd", "csrc", "ganon_host.cpp"), "-lz", "-ldl"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split("\n")[:-1]


def _sites_file(path, table) -> str:
    with open(path, "w") as fh:
        fh.write(f"{table.n_ref} {table.n}\n" + " ".join(str(int(o)) for o in table.site_off) + "\n")
        fh.write("".join(f"{int(p)} {int(c)}\n" for p, c in zip(table.site_pos, table.site_code)))
    return path


def _lines(t, seq, qual) -> list:
    out = []
    for i in range(t.n):
        so, qo, L = int(t.seq_off[i]), int(t.qual_off[i]), int(t.l_seq[i])
        out.append(seq[so:so + (L + 1) // 2].tobytes().hex() + " " + qual[qo:qo + L].tobytes().hex())
    return out


@pytest.mark.parametrize("quality", [None, 5])
def test_hand_built_stream_under_sanitizers(driver, tmp_path, quality):
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    recs, sites = K.hand_built()
    recs += K.long_cigar_records()
    every = K.Sites({"c1": dict(zip(sites.pos["c1"], sites.val["c1"])), "c2": {p: (8, 7) for p in range(3000)}})
    stream, _ = K.stream_of(recs)
    path = str(tmp_path / "hand.bam")
    write_bgzf(path, stream.tobytes())
    plain = ReadTable(path)
    seq, qual, total = K.rule_on_table(every, plain, quality)
    assert total > 100
    sf = _sites_file(str(tmp_path / "sites.txt"), K.table_of(every, plain.ref_names, quality))
    for threads in ("1", "3"):
        got = _run(driver, "file", sf, str(-1 if quality is None else quality), path, threads)
        assert got[:-1] == _lines(plain, seq, qual) and got[-1] == f"count {total}"


def test_reader_under_sanitizers(driver, tmp_path):
    import dataclasses
    from genomeanonymizer_amd.io.bam import BamReader
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario("fuzz2000"), bam_index=True), str(tmp_path / "in"))
    sites = K.scenario_panel("fuzz2000")["sites"]
    r = BamReader(p["T"], 2)
    exp, total = [], 0
    for tid, L in enumerate(int(x) for x in r.ref_lens):
        for t in [r.contig(tid)] + [r.region(tid, k * L // 3, (k + 1) * L // 3) for k in range(3)]:
            seq, qual, n = K.rule_on_table(sites, t, 9)
            exp += _lines(t, seq, qual)
            total += n
    sf = _sites_file(str(tmp_path / "sites.txt"), K.table_of(sites, r.ref_names, 9))
    r.close()
    assert len(exp) > 100 and total >= K.MIN_CHANGED
    got = _run(driver, "reader", sf, "9", p["T"])
    assert got[:-1] == exp and got[-1] == f"count {total}"
