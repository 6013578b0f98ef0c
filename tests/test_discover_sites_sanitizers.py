"""ASan/UBSan build of the evidence tally (--discover_sites): csrc/ganon_site_tally.h inside the decoders
of csrc/ganon_host.cpp and the host compaction, linked into a stand-alone driver
(tests/sanitize/site_tally_driver.cpp) with the sanitizer runtime — in the manner of
tests/test_known_sites_sanitizers.py: nothing is preloaded and nothing is loaded into Python. The sites
the driver prints are checked against the plain-Python restatement of discover_helpers. CPU only."""
import os
import shutil
import subprocess

import pytest

import discover_helpers as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "site_tally_driver")
    r = subprocess.run(["g++", *SAN, "-std=c++17", "-pthread", "-o", exe,
                        os.path.join(REPO, "tests", "sanitize", "site_tally_driver.cpp"),
                        os.path.join(REPO, "genomeanonymizer_amd", "csrc", "ganon_host.cpp"), "-lz", "-ldl"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split("\n")[:-1]


def _ref_file(path, names, fa) -> str:
    with open(path, "w") as fh:
        fh.write(f"{len(names)}\n" + "".join(fa.get(n, "-") + "\n" for n in names))
    return path


def _lines(names, sites) -> list:
    out = [f"{s} {p} {(ref << 4) | alt}" for s, n in enumerate(names) for p, (ref, alt) in sorted(sites.get(n, {}).items())]
    return out + [f"sites {len(out)}"]


@pytest.mark.parametrize("threads", ["1", "3"])
def test_hand_built_records_under_sanitizers(driver, tmp_path, threads):
    names = [c for c, _ in D.HAND_CONTIGS]
    exp = _lines(names, D.expected_hand())
    assert len(exp) > 400
    rf = _ref_file(str(tmp_path / "ref.txt"), names, D.hand_fasta())
    plain = D.write_hand_files(str(tmp_path / "plain"), False)
    assert _run(driver, "file", rf, threads, plain["T"], plain["N"]) == exp
    idx = D.write_hand_files(str(tmp_path / "idx"), True)
    assert _run(driver, "reader", rf, threads, idx["T"], idx["N"]) == exp


def test_scenario_under_sanitizers(driver, tmp_path):
    import dataclasses
    from genomeanonymizer_amd.io.bam import BamReader
    from genomeanonymizer_amd.synth.generate import generate, scenario
    p = generate(dataclasses.replace(scenario("fuzz2000"), bam_index=True), str(tmp_path / "in"))
    ss = D.scenario_sites("fuzz2000")
    r = BamReader(p["T"], 1)
    names = list(r.ref_names)
    r.close()
    exp = _lines(names, ss["sites"])
    assert len(exp) > 1000
    rf = _ref_file(str(tmp_path / "ref.txt"), names, ss["fa"])
    assert _run(driver, "reader", rf, "2", p["T"], p["N"]) == exp
    assert _run(driver, "file", rf, "2", p["T"], p["N"]) == exp
