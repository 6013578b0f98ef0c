"""ASan/UBSan build of --discover_sites' evidence filters and rule: ganon_site_tally_create_ex and the
filtered tally of csrc/ganon_site_tally.h inside the decoders of csrc/ganon_host.cpp, with the host
compaction in both modes, linked into a stand-alone driver (tests/sanitize/site_rule_driver.cpp) with the
sanitizer runtime — in the manner of tests/test_discover_sites_sanitizers.py: nothing is preloaded and
nothing is loaded into Python. The hand-built set of discover_rules_helpers runs under two rules, as plain
streams (with the records placed before a sequence's start, whose clip moves the quality index) and
through the indexed readers; the sites the driver prints are checked against the plain-Python
restatement. CPU only."""
import os
import shutil
import subprocess

import pytest

import discover_rules_helpers as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "site_rule_driver")
    r = subprocess.run(["g++", *SAN, "-std=c++17", "-pthread", "-o", exe,
                        os.path.join(REPO, "tests", "sanitize", "site_rule_driver.cpp"),
                        os.path.join(REPO, "genomeanonymizer_amd", "csrc", "ganon_host.cpp"), "-lz", "-ldl"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split("\n")[:-1]


def _lines(names, sites) -> list:
    out = [f"{s} {p} {(ref << 4) | alt}" for s, n in enumerate(names) for p, (ref, alt) in sorted(sites.get(n, {}).items())]
    return out + [f"sites {len(out)}"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rules")
    names = [c for c, _ in R.HAND_CONTIGS]
    fa = R.hand_built()[2]
    rf = str(d / "ref.txt")
    with open(rf, "w") as fh:
        fh.write(f"{len(names)}\n" + "".join(fa.get(n, "-") + "\n" for n in names))
    return {"names": names, "ref": rf, "plain": R.write_hand_files(str(d / "plain"), False),
            "idx": R.write_hand_files(str(d / "idx"), True)}


@pytest.mark.parametrize("rule", [R.FULL, R.FULL_NORMAL], ids=["both", "normal"])
@pytest.mark.parametrize("threads", ["1", "3"])
def test_hand_built_records_under_sanitizers(driver, files, rule, threads):
    args = (str(rule.q), str(rule.m), hex(rule.f), str(("both", "normal").index(rule.mode)))
    exp = _lines(files["names"], R.expected_hand(rule))
    assert len(exp) > 200 and exp != _lines(files["names"], R.expected_hand(R.ZERO))
    plain, idx = files["plain"], files["idx"]
    assert _run(driver, "file", files["ref"], threads, plain["T"], plain["N"], *args) == exp
    assert _run(driver, "reader", files["ref"], threads, idx["T"], idx["N"], *args) == _lines(files["names"],
                                                                                             R.expected_indexed(rule))
