"""Hand-built DEFLATE streams for the GPU inflate (csrc/ganon_inflate.hip), made with
tests/deflate_craft.py: the legal DEFLATE zlib's deflate never emits, placed at the decoder's own
boundaries (the 8 KiB output ring, the 1 KiB flush chunk, the 4 KiB near/far match split, the
256-bit token round and its 2048-byte / 8-match limits), and the malformed streams it must reject.

``valid_set()``: (stream, expected bytes, label); ``malformed_set()``: (stream, isize, label). Both
are deterministic and built once per process. tests/test_inflate_crafted.py runs them through zlib,
the decoder source on the host, and the kernel.
"""
import functools
import random

import numpy as np

from deflate_craft import (DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, DeflateWriter, code_lengths, expand,
                           rle_lengths, tree_lengths)

# the decoder's constants (ganon_inflate.hip): output ring, flush chunk, near/far split
RING, FLUSH, NEAR = 8192, 1024, 4096
BOUNDARY_DISTS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 4098, 8191, 8192, 8193, 16384, 32767, 32768)


def _bytes(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, n, dtype=np.uint8).tobytes()


def _lits(data):
    return [("L", b) for b in data]


class _Stream:
    """A stream under construction and the bytes it must decode to."""

    def __init__(self):
        self.w = DeflateWriter()
        self.exp = bytearray()

    def stored(self, data, final=False):
        self.w.stored(data, final)
        self.exp += data

    def fixed(self, toks, final=False):
        self.w.fixed_block(toks, final)
        self.exp += expand(toks, self.exp)

    def dynamic(self, toks, final=False, **kw):
        self.w.dynamic_block(toks, final, **kw)
        self.exp += expand(toks, self.exp)

    def done(self, label):
        assert len(self.exp) <= 65536, label
        return self.w.getvalue(), bytes(self.exp), label


def _pad(n):
    """Tokens for n cheap output bytes (after at least one byte of output): 258/1 matches, then
    literals."""
    t = []
    while n >= 261:
        t.append(("M", 258, 1))
        n -= 258
    while n > 258:
        t.append(("L", 71))
        n -= 1
    if n >= 3:
        t.append(("M", n, 1))
        n = 0
    return t + [("L", 71)] * n


def _stored_cases(rng):
    out = []
    # runs of tiny stored blocks: each is served from the bit buffer alone
    s = _Stream()
    data = _bytes(rng, 9000)
    for i in range(3000):
        s.stored(data[3 * i:3 * i + 3], final=i == 2999)
    out.append(s.done("stored: 3000 blocks of 3 bytes"))
    # ... and a far match into what those blocks wrote
    s = _Stream()
    s.stored(_bytes(rng, 1024))
    data = _bytes(rng, 4500)
    for i in range(1500):
        s.stored(data[3 * i:3 * i + 3])
    s.fixed([("M", 100, 4300)], final=True)
    out.append(s.done("stored: 1024 + 1500 x 3 bytes, then a match of 100 at distance 4300"))
    # every small and chunk-sized length, each block's header at a bit offset 1..7
    s = _Stream()
    for i, n in enumerate((0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049)):
        if i & 1:
            s.dynamic(_lits(_bytes(rng, 5 + i, 65, 70)) + ([("M", 4, 2)] if i > 2 else []))
        target = i % 7 + 1
        # a fixed block of 8-bit literals ends 2 bits further on, and 1 more per 9-bit literal
        j = (target - 2 - s.w.bit_length()) % 8
        s.fixed(_lits(_bytes(rng, 3, 0, 144) + _bytes(rng, j, 144, 256)))
        assert s.w.bit_length() % 8 == target
        s.stored(_bytes(rng, n))
    s.fixed(_lits(b"end"), final=True)
    out.append(s.done("stored: lengths 0..5, 1023..1025, 2047..2049 from unaligned headers"))
    # exactly 64 KiB
    for kind in ("stored", "fixed"):
        s = _Stream()
        s.stored(_bytes(rng, 65535))
        if kind == "stored":
            s.stored(b"Z", final=True)
        else:
            s.fixed(_lits(b"Z"), final=True)
        assert len(s.exp) == 65536
        out.append(s.done("stored: 65535 bytes, then a 1-byte %s block" % kind))
    return out


def _overlap_cases(rng):
    """Every distance 1..257 with a match of 258 and one of distance + 1, after 8 KiB of output."""
    out = []
    for half, kind in ((range(1, 160), "fixed"), (range(160, 258), "dynamic")):
        s = _Stream()
        s.stored(_bytes(rng, RING + 37))
        pos, toks, straddle = len(s.exp), [], 0
        for d in half:
            for ln in (258, max(3, d + 1)):
                lits = _bytes(rng, 7)
                toks += _lits(lits) + [("M", ln, d)]
                pos += 7
                straddle += pos // RING != (pos + ln - 1) // RING
                pos += ln
        assert straddle >= 3, straddle   # some of them wrap the output ring
        (s.fixed if kind == "fixed" else s.dynamic)(toks, final=True)
        out.append(s.done("overlap: distances %d..%d, lengths 258 and d + 1, %s" % (half[0], half[-1], kind)))
    return out


def _boundary_cases(rng):
    """Matches at the near/far split and the ring size, at the flush frontier's offsets."""
    cases = [(d, ln, cls) for d in (4095, 4096, 4097, 8191, 8192, 8193, 32768) for ln in (3, 257, 258)
             for cls in range(4)]
    runs = (0, 1, 100, 700, 2300)
    targets = ((0, FLUSH), (1, FLUSH), (FLUSH - 1, FLUSH), (RING - 1, RING))
    out, i, k = [], 0, 0
    while i < len(cases):
        s = _Stream()
        s.stored(_bytes(rng, 32768 + 11 * k))
        pos, toks, first = len(s.exp), [], i
        while i < len(cases):
            d, ln, cls = cases[i]
            run = runs[i % len(runs)]
            r, m = targets[cls]
            pad = (r - pos - run) % m
            if pos + pad + run + ln > 65536 - 8:
                break
            # cheap literals: two byte values, nine in ten the same
            lits = rng.choice(np.frombuffer(b"AC", np.uint8), run, p=[.9, .1]).tobytes()
            toks += _pad(pad) + _lits(lits) + [("M", ln, d)]
            pos += pad + run
            assert pos % m == r
            pos += ln
            i += 1
        assert i > first
        toks += _lits(b"tail")
        (s.dynamic if k % 2 == 0 else s.fixed)(toks, final=True)
        out.append(s.done("boundary: cases %d..%d, %s" % (first, i - 1, "dynamic" if k % 2 == 0 else "fixed")))
        k += 1
    # the worst case of one round: from `flushed` 1023 bytes behind, seven 258/1 matches and 234
    # one-bit literals (2040 bytes: all that 256 bits can start), then a 258-byte match
    lit = [0] * 286
    lit[65], lit[285], lit[256], lit[67] = 1, 2, 3, 3
    for d in (4095, 4096, 4097, 8192, 8193, 32768):
        s = _Stream()
        s.stored(_bytes(rng, 32768 + FLUSH - 1))
        dl = [0] * 30
        dl[0] = 1
        dl[[i for i in range(30) if DIST_BASE[i] <= d][-1]] = 1
        toks = [("M", 258, 1)] * 7 + _lits(b"A" * 234) + [("M", 258, d)] + _lits(b"CAC")
        s.dynamic(toks, final=True, lit_lengths=lit, dist_lengths=dl)
        out.append(s.done("boundary: a full round, then 258 at distance %d" % d))
    return out


def _dense_cases(rng):
    out = []
    # 256 literal tokens per round: a 1-bit literal (and no distance code at all)
    lit = [0] * 286
    lit[65], lit[67], lit[256] = 1, 2, 2
    data = bytearray(b"A" * 60000)
    for p in rng.integers(0, 60000, 150):
        data[p] = 67
    s = _Stream()
    s.dynamic(_lits(data), final=True, lit_lengths=lit, dist_lengths=[0] * 30)
    out.append(s.done("dense: 60000 literals, a 1-bit code"))
    # more than 8 matches inside 256 bits (12 bits each)
    toks = _lits(b"xy")
    for i in range(3000):
        toks.append(("M", 3, 1))
        if i % 50 == 49:
            toks.append(("L", int(rng.integers(256))))
    s = _Stream()
    s.fixed(toks, final=True)
    out.append(s.done("dense: 3000 matches of 3 at distance 1"))
    # 8 matches of 258 pass the round's output limit (2064 > 2048) in mid block
    s = _Stream()
    s.fixed(_lits(b"q") + [("M", 258, 1)] * 100 + _lits(b"rs") + [("M", 258, 2)] * 100 + _lits(b"t"), final=True)
    out.append(s.done("dense: runs of 258-byte matches at distances 1 and 2"))
    # ... and the limit met by a literal in mid block: 7 x 258, 100 literals, a match of 100 (2006),
    # then literals through byte 2048 of the round
    lit = [0] * 286
    lit[65], lit[285], lit[279], lit[256], lit[67] = 1, 2, 3, 4, 4
    dl = [0] * 30
    dl[0] = 1
    one = [("M", 258, 1)] * 7 + _lits(b"A" * 100) + [("M", 100, 1)] + _lits(b"A" * 60 + b"C")
    s = _Stream()
    s.stored(_bytes(rng, 700))
    s.dynamic(one * 12, final=False, lit_lengths=lit, dist_lengths=dl)
    s.dynamic(one * 3, final=True, lit_lengths=lit, dist_lengths=dl)
    out.append(s.done("dense: the output limit reached among literals"))
    return out


def _slow_code_cases(rng):
    out = []
    # HLIT = 286, HDIST = 30, every symbol in use, codes up to 15 bits from given length vectors
    for k in range(3):
        ll = tree_lengths(286, rng)
        dl = tree_lengths(30, rng)
        ll = [ll[i] for i in rng.permutation(286)]
        dl = [dl[i] for i in rng.permutation(30)]
        assert max(ll) == 15 and max(dl) >= 11 and any(11 <= x < 15 for x in ll)
        s = _Stream()
        s.stored(_bytes(rng, 32768 + k))
        toks = _lits(bytes(range(256)))
        for i in range(29):
            toks.append(("M", min(257, LEN_BASE[i] + int(rng.integers(1 << LEN_EXTRA[i]))) if i < 28 else 258,
                         1 + int(rng.integers(300))))
        for i in range(30):
            toks.append(("M", 3 + int(rng.integers(256)), min(32768, DIST_BASE[i] + int(rng.integers(1 << DIST_EXTRA[i])))))
        toks.append(("M", 258, 77, "284+31"))   # 258 as code 284 with all extra bits set
        pos = 32768 + k + sum(1 if t[0] == "L" else t[1] for t in toks[:-1])
        for _ in range(2500):
            pos += 1 if toks[-1][0] == "L" else toks[-1][1]
            if pos > 65000:
                break
            if rng.random() < 0.2:
                i, j = int(rng.integers(29)), int(rng.integers(30))
                toks.append(("M", min(258, LEN_BASE[i] + int(rng.integers(1 << LEN_EXTRA[i]))),
                             min(32768, DIST_BASE[j] + int(rng.integers(1 << DIST_EXTRA[j])))))
            else:
                toks.append(("L", int(rng.integers(256))))
        s.dynamic(toks, final=True, lit_lengths=ll, dist_lengths=dl)
        out.append(s.done("slow codes: 286 + 30 symbols in use, lengths to 15 (%d)" % k))
    # exactly one distance code, of length 1: symbol 0, then a symbol with extra bits
    s = _Stream()
    s.dynamic(_lits(b"one distance ") + [("M", 40, 1), ("L", 33), ("M", 3, 1)], final=True)
    out.append(s.done("slow codes: a lone distance code (derived)"))
    dl = [0] * 30
    dl[10] = 1
    toks = _lits(_bytes(rng, 60)) + [("M", 30, 33), ("L", 1), ("M", 258, 48), ("M", 5, 40)]
    s = _Stream()
    s.dynamic(toks, final=True, dist_lengths=dl)
    out.append(s.done("slow codes: a lone distance code (symbol 10)"))
    # no distance code: literals only, HDIST = 1 with a zero length
    s = _Stream()
    s.dynamic(_lits(_bytes(rng, 3000, 60, 90)), final=True)
    assert s.w.getvalue() and len(s.exp) == 3000
    out.append(s.done("slow codes: no distance code"))
    return out


def _end_cases(rng):
    out = []
    s = _Stream()
    s.fixed([], final=True)
    st = s.done("ends: the fixed empty block")
    assert st[0] == b"\x03\x00"
    out.append(st)
    seen = set()
    for k in range(1, 9):   # 10 + 8 k bits: 2 + k payload bytes
        s = _Stream()
        s.fixed(_lits(_bytes(rng, k, 0, 144)), final=True)
        st = s.done("ends: payload of %d bytes" % (k + 2))
        assert len(st[0]) == k + 2
        seen.add(len(st[0]) % 4)
        out.append(st)
    assert seen == {0, 1, 2, 3}
    # end-of-block as the payload's last bits: 3 + 8 a + 9 * 6 + 7 = 64 + 8 a
    for a in (0, 5, 200):
        s = _Stream()
        s.fixed(_lits(_bytes(rng, a, 0, 144) + _bytes(rng, 6, 144, 256)), final=True)
        assert s.w.bit_length() % 8 == 0
        out.append(s.done("ends: end-of-block on a byte boundary (%d literals)" % (a + 6)))
    # the last round starts with fewer than 64 bytes of room, and the output ends exactly at ISIZE
    s = _Stream()
    s.fixed(_lits(_bytes(rng, 1000, 0, 144)), final=True)
    out.append(s.done("ends: 8-bit literals to ISIZE"))
    lit = [0] * 286
    lit[65], lit[67], lit[256] = 1, 2, 2
    s = _Stream()
    s.dynamic(_lits(b"A" * (256 * 10 + 40)), final=True, lit_lengths=lit, dist_lengths=[0] * 30)
    out.append(s.done("ends: 1-bit literals to ISIZE, 40 in the last round"))
    s = _Stream()
    s.fixed(_lits(_bytes(rng, 300)) + [("M", 258, 1)], final=True)
    out.append(s.done("ends: a match of 258 ending at ISIZE"))
    s = _Stream()
    s.fixed(_lits(_bytes(rng, 30)) + [("M", 258, 30)] * 8 + _lits(_bytes(rng, 20)) + [("M", 3, 5)], final=True)
    out.append(s.done("ends: a match of 3 ending at ISIZE after a full round"))
    return out


def _random_case(seed):
    """1-3 mixed blocks: literal skew on or off, match probability in {0.02, 0.3, 0.9}, distances
    from a menu of the decoder's boundaries."""
    r = random.Random(seed)
    skew = bool(seed & 1)
    pm = (0.02, 0.3, 0.9)[seed % 3]
    menu = [r.choice(BOUNDARY_DISTS) for _ in range(4)]
    s = _Stream()
    nb = r.randint(1, 3)
    kinds = []
    if max(menu) > 4096 and r.random() < 0.7:   # history for the long distances
        s.stored(bytes(r.getrandbits(8) for _ in range(r.choice((4200, 8300, 16500, 33000)))))
        kinds.append("S")
    for b in range(nb):
        final = b == nb - 1
        kind = r.choice("SFDD")
        kinds.append(kind)
        pos = len(s.exp)
        if kind == "S":
            n = min(r.choice((0, 1, 2, 3, 4, 5, 7, 300, 1024, 2500)), 65536 - pos)
            s.stored(bytes(r.getrandbits(8) for _ in range(n)), final)
            continue
        toks = []
        for _ in range(r.randint(1, 1500)):
            if pos + 258 > 65536:
                break
            if pos and r.random() < pm:
                ln = r.choice((3, 4, 10, 257, 258, r.randint(3, 258)))
                d = r.choice(menu) if r.random() < 0.7 else r.randint(1, 300)
                if d > pos:
                    d = r.randint(1, pos)
                toks.append(("M", ln, d))
                pos += ln
            else:
                toks.append(("L", r.choice(b"ACGT") if skew and r.random() < 0.95 else r.getrandbits(8)))
                pos += 1
        (s.fixed if kind == "F" else s.dynamic)(toks, final)
    return s.done("random: seed %d (%s, skew %d, p(match) %.2f, distances %s)" % (seed, "".join(kinds), skew, pm, menu))


@functools.lru_cache(maxsize=None)
def valid_set():
    rng = np.random.default_rng(1951)
    out = (_stored_cases(rng) + _overlap_cases(rng) + _boundary_cases(rng) + _dense_cases(rng) +
           _slow_code_cases(rng) + _end_cases(rng))
    out += [_random_case(seed) for seed in range(150)]
    return tuple(out)


# ---- malformed -------------------------------------------------------------------------------

def _dyn_raw(lit_lengths, dist_lengths, body=(), hlit=None, hdist=None, syms=None, final=True):
    """A dynamic block from any code lengths, legal or not: the header, then raw ``body`` bits
    ((value, nbits) pairs)."""
    hlit = hlit or max(257, max(i + 1 for i, l in enumerate(lit_lengths) if l))
    hdist = hdist or max([1] + [i + 1 for i, l in enumerate(dist_lengths) if l])
    if syms is None:
        syms = rle_lengths(list(lit_lengths[:hlit]) + (list(dist_lengths) + [0])[:hdist])
    cf = [0] * 19
    for sym, _ in syms:
        cf[sym] += 1
    w = DeflateWriter()
    w.dynamic_header(final, hlit, hdist, code_lengths(cf, 7, 2), syms)
    for v, k in body:
        w.bits(v, k)
    return w.getvalue()


@functools.lru_cache(maxsize=None)
def malformed_set():
    """(stream, isize, label): zlib rejects the stream, or it inflates to another length than isize.

    Not in the set: an *incomplete* literal/length code whose missing codes the stream never uses.
    zlib rejects it when it reads the header; this decoder builds its tables from it and accepts
    the stream (it rejects a missing code only where one is met). That difference is known and left."""
    out = []
    picks = ("stored: lengths 0..5", "overlap: distances 1..159", "boundary: a full round, then 258 at distance 4097",
             "dense: the output limit", "slow codes: 286 + 30 symbols in use, lengths to 15 (0)",
             "ends: a match of 258")
    subset = [v for p in picks for v in valid_set() if v[2].startswith(p)]
    assert len(subset) == len(picks)
    subset += [v for v in valid_set() if v[2].startswith("random") and 2000 <= len(v[1]) <= 30000][:3]
    for s, t, label in subset:
        n = len(t)
        assert n >= 259
        for isize in (n - 1, n - 258, n // 2, 1, 0):
            out.append((s, isize, "isize %d of %d: %s" % (isize, n, label)))
        out.append((s[:len(s) // 2], n, "cut in half: " + label))
        out.append((s[:-1], n, "cut by one byte: " + label))
    rng = np.random.default_rng(286)
    # a match reaching one byte before the start of the output
    for n in (0, 1, 5000):
        w = DeflateWriter()
        if n == 5000:
            w.stored(_bytes(rng, n), False)
        lits = _lits(b"a") if n == 1 else []
        dsym = [i for i in range(30) if DIST_BASE[i] <= n + 1][-1]
        w.fixed_block(lits + [("S", 257), ("D", dsym, n + 1 - DIST_BASE[dsym])] + _lits(b"zz"), True)
        out.append((w.getvalue(), n + 5, "distance %d after %d bytes" % (n + 1, n)))
    w = DeflateWriter()
    w.fixed_block(_lits(b"a") + [("S", 286), ("D", 0, 0)], True)
    out.append((w.getvalue(), 4, "fixed literal/length symbol 286"))
    w = DeflateWriter()
    w.fixed_block(_lits(b"abc") + [("S", 257), ("D", 30, 0)], True)
    out.append((w.getvalue(), 6, "fixed distance symbol 30"))
    # over-subscribed codes
    lit = [0] * 286
    lit[65], lit[66], lit[256] = 1, 1, 1
    out.append((_dyn_raw(lit, [1], [(0, 32)]), 8, "over-subscribed literal/length code"))
    lit = [0] * 286
    lit[65], lit[256] = 1, 1
    out.append((_dyn_raw(lit, [1, 1, 1], [(0, 32)]), 8, "over-subscribed distance code"))
    w = DeflateWriter()
    cl = [0] * 19
    cl[0] = cl[1] = cl[2] = 1
    w.dynamic_header(True, 257, 1, cl, [(0, 0)] * 40)
    out.append((w.getvalue() + b"\x00" * 40, 8, "over-subscribed code-length code"))
    lit = [0] * 286
    lit[65], lit[66] = 1, 1
    out.append((_dyn_raw(lit, [1], [(0, 64)], hlit=257), 64, "no end-of-block code"))
    lit = [0] * 286
    lit[65], lit[256] = 1, 1
    good = rle_lengths(lit[:257] + [1])
    out.append((_dyn_raw(lit, [1], [(0, 8), (1, 1)], syms=[(16, 0)] + good[1:]), 8, "a 16-repeat as the first length"))
    out.append((_dyn_raw(lit, [1], [(0, 8), (1, 1)], syms=good[:-2] + [(18, 127)]), 8, "a repeat past HLIT + HDIST"))
    out.append((_dyn_raw(lit, [1], [(0, 8), (1, 1)], hlit=287, syms=good + [(0, 0)] * 30), 8, "HLIT = 287"))
    w = DeflateWriter()
    w.stored(_bytes(rng, 100), True)
    out.append((w.getvalue(), 50, "a stored block longer than isize"))
    w = DeflateWriter()
    w.stored(_bytes(rng, 10), True, length=20)
    out.append((w.getvalue(), 20, "a stored block longer than its payload"))
    return tuple(out)
