"""ASan/UBSan build of the SA clip mask (--mask_sa_clips): csrc/ganon_sa_clips.h inside the decoder of
csrc/ganon_host.cpp, linked into a stand-alone driver (tests/sanitize/sa_clips_driver.cpp) with the
sanitizer runtime — in the manner of tests/test_known_sites_sanitizers.py: nothing is preloaded and
nothing is loaded into Python. The bases and qualities the driver prints are checked against the
plain-Python rule of sa_clips_helpers: on the hand-built stream, and on 200 records whose aux bytes are
random around an ``SAZ`` prefix. CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import known_sites_helpers as K
import sa_clips_helpers as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-O1", "-g"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san") / "sa_clips_driver")
    r = subprocess.run(["g++", *SAN, "-std=c++17", "-pthread", "-o", exe,
                        os.path.join(REPO, "tests", "sanitize", "sa_clips_driver.cpp"),
                        os.path.join(REPO, "genomeanonymizer_amd", "csrc", "ganon_host.cpp"), "-lz", "-ldl"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split("\n")[:-1]


def _files(tmp_path, table):
    sf = str(tmp_path / "sites.txt")
    with open(sf, "w") as fh:
        fh.write(f"{table.n_ref} {table.n}\n" + " ".join(str(int(o)) for o in table.site_off) + "\n")
        fh.write("".join(f"{int(p)} {int(c)}\n" for p, c in zip(table.site_pos, table.site_code)))
    nf = str(tmp_path / "names.txt")
    with open(nf, "w") as fh:
        fh.write(f"{len(table.sa_tid)}\n")
        for i, t in enumerate(table.sa_tid.tolist()):
            fh.write(f"{t} {table.sa_blob[int(table.sa_off[i]):int(table.sa_off[i + 1])].decode()}\n")
    return sf, nf


def _lines(t, seq, qual) -> list:
    out = []
    for i in range(t.n):
        so, qo, L = int(t.seq_off[i]), int(t.qual_off[i]), int(t.l_seq[i])
        out.append(seq[so:so + (L + 1) // 2].tobytes().hex() + " " + qual[qo:qo + L].tobytes().hex())
    return out


def _check(driver, tmp_path, recs, sites, quality):
    from genomeanonymizer_amd.io.bam import ReadTable
    from genomeanonymizer_amd.synth.bamwriter import write_bgzf
    stream, _ = S.stream_of(recs)
    path = str(tmp_path / "in.bam")
    write_bgzf(path, stream.tobytes())
    plain = ReadTable(path)
    seq, qual, tot = S.rule_on_table(sites, plain, quality)
    sf, nf = _files(tmp_path, S.table_of(sites, plain.ref_names, quality))
    for threads in ("1", "3"):
        got = _run(driver, sf, nf, str(-1 if quality is None else quality), path, threads)
        assert got[:-1] == _lines(plain, seq, qual) and got[-1] == "count %d %d %d" % tot
    return tot


@pytest.mark.parametrize("quality", [None, 5])
def test_hand_built_stream_under_sanitizers(driver, tmp_path, quality):
    recs, sites, _ = S.hand_built()
    tot = _check(driver, tmp_path, recs, sites, quality)
    assert tot[1] >= S.MIN_HAND_REWRITTEN and tot[2] == S.N_IGNORED


def random_aux_records(n: int = 200, seed: int = 23):
    """Records 20M10S (clip bases C) whose aux is random bytes around an ``SAZ`` prefix: a valid entry
    onto c2:801 (every position there is a site the clip shows) with random bytes substituted, inserted
    and deleted, cut short or not, with and without its NUL, between random bytes."""
    rng = np.random.default_rng(seed)
    alphabet = b"0123456789MIDNSHP=X,;+-*c2 \x00\xff"
    recs = []
    for k in range(n):
        text = bytearray((S.entry("c2", 801, "+-"[k % 2], "10M20S" if k % 2 else "20S10M") + ";").encode() * int(rng.integers(1, 4)))
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(text) + 1))
            kind = int(rng.integers(0, 3))
            b = alphabet[int(rng.integers(0, len(alphabet)))] if rng.random() < 0.8 else int(rng.integers(0, 256))
            if kind == 0 and at < len(text):
                text[at] = b
            elif kind == 1:
                text.insert(at, b)
            elif at < len(text):
                del text[at]
        if k % 7 == 0:
            text = text[:int(rng.integers(0, len(text) + 1))]
        pre = bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8)) if k % 3 == 0 else \
            (b"XBBc" + int(rng.integers(-2, 5)).to_bytes(4, "little", signed=True) + b"\x01\x02\x03" if k % 3 == 1 else b"")
        post = bytes(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8))
        aux = pre + b"SAZ" + bytes(text) + (b"\x00" if k % 5 else b"") + post
        nib = [int(x) for x in rng.choice([2, 4, 8], 20)] + [4 if k % 2 else 2] * 10
        recs.append(dict(tid=0, pos=1000 + k, flag=0, cigar=[("M", 20), ("S", 10)], nib=nib,
                         qual=[int(x) for x in rng.integers(5, 40, 30)], aux=aux))
    return recs


def test_random_aux_under_sanitizers(driver, tmp_path):
    """The runs end clean, and the bases are the Python rule's: unchanged for every entry it ignores."""
    recs = random_aux_records()
    sites = K.Sites({"c2": {p: (1, 2 | 4 | 8) for p in range(800, 810)}})
    _, (n_ks, n_sa, n_ign) = S.expected_of(recs, sites)
    assert n_sa >= 100 and n_ign >= 40, (n_sa, n_ign)     # conditions on the inputs: both outcomes are well represented
    assert _check(driver, tmp_path, recs, sites, 5) == (n_ks, n_sa, n_ign)
