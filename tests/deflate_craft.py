"""A DEFLATE stream writer for tests, written from RFC 1951 (stdlib and numpy only).

zlib's deflate never emits large parts of legal DEFLATE (runs of tiny stored blocks, 15-bit codes,
a lone distance code, 1-bit literal codes, a match at a chosen output offset); the GPU inflate
(csrc/ganon_inflate.hip) must decode all of it. This module writes such streams token by token:

    w = DeflateWriter()
    w.stored(b"abc", final=False)
    w.fixed_block([("L", 65), ("M", 258, 1)], final=False)
    w.dynamic_block(tokens, final=True)            # codes derived from the token frequencies
    stream = w.getvalue()

A token is ("L", byte) or ("M", length, distance); ``expand(tokens)`` is the output by direct
expansion. For malformed streams the writer also takes raw tokens — ("S", literal/length symbol),
("D", distance symbol, extra value), ("R", value, nbits) — and ``dynamic_header`` writes any
HLIT/HDIST/HCLEN header, legal or not. tests/test_inflate_crafted.py checks every valid stream made
here against zlib, so the writer is itself pinned to an independent decoder.
"""
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

FIXED_LIT_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENGTHS = [5] * 32


def _len_table():
    t = [None] * 259
    for i, (b, e) in enumerate(zip(LEN_BASE, LEN_EXTRA)):
        for v in range(1 << e):
            if b + v <= 258 and t[b + v] is None:
                t[b + v] = (257 + i, e, v)
    t[258] = (285, 0, 0)   # (284 + extra 31 is legal too: a 4th token element asks for it)
    return t


def _dist_table():
    t = [0] * 32769
    for i, (b, e) in enumerate(zip(DIST_BASE, DIST_EXTRA)):
        for d in range(b, min(b + (1 << e), 32769)):
            t[d] = i
    return t


_LEN = _len_table()
_DIST = _dist_table()


def canonical_codes(lengths):
    """Per symbol (code with its bits reversed, i.e. in stream order; length), None for length 0
    (RFC 1951 3.2.2)."""
    bl = [0] * 17
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if not l:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)   # (an over-subscribed set wraps: only malformed headers have one)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def code_lengths(freqs, limit=15, min_used=2):
    """Huffman code lengths of at most ``limit`` bits for the symbols with a non-zero frequency.
    Fewer than ``min_used`` used symbols get unused ones added (weight 1), so that the code is
    complete; min_used=0 leaves a lone symbol a 1-bit code and no symbol no code at all."""
    n = len(freqs)
    f = [int(x) for x in freqs]
    used = [i for i in range(n) if f[i] > 0]
    for i in range(n):
        if len(used) >= min_used:
            break
        if f[i] == 0:
            f[i] = 1
            used.append(i)
    lens = [0] * n
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    while True:
        heap = [(f[i], i, [i]) for i in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        tie = n
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
            tie += 1
        if max(depth.values()) <= limit:
            break
        f = [(x + 1) // 2 if x else 0 for x in f]   # flatter weights until the tree fits
    for s, d in depth.items():
        lens[s] = d
    return lens


def rle_lengths(seq):
    """The code-length alphabet's (symbol, extra value) list for a sequence of code lengths; runs are
    taken over the whole sequence (so they cross from the literal/length into the distance lengths)."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            while run >= 3:
                r = min(run, 10)
                out.append((17, r - 3))
                run -= r
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(v, 0)] * run
        i = j
    return out


def expand(tokens, history=b""):
    """The bytes a token list decodes to, by direct expansion (after ``history``: the stream's
    output before these tokens, which their matches may reach into; not returned)."""
    out = bytearray(history)
    h = len(out)
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        else:
            ln, d = t[1], t[2]
            assert t[0] == "M" and 3 <= ln <= 258 and 1 <= d <= len(out), t
            s = len(out) - d
            if d >= ln:
                out += out[s:s + ln]
            else:
                out += (bytes(out[s:]) * (ln // d + 1))[:ln]
    return bytes(out[h:])


class DeflateWriter:
    """LSB-first bit writer (RFC 1951 3.1.1) with the three block kinds on top. Bits gather in one
    Python int and are spilled to a bytearray every couple of thousand bits."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def _spill(self):
        nb = self.n >> 3
        if nb:
            self.out += (self.acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self.acc >>= 8 * nb
            self.n &= 7

    def bits(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k
        if self.n >= 2048:
            self._spill()

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def align(self):
        self.n = (self.n + 7) & ~7
        self._spill()

    def getvalue(self):
        self.align()
        return bytes(self.out)

    # -- blocks ------------------------------------------------------------------------------
    def stored(self, data, final, length=None):
        """A stored block (``length``: the LEN field, when it is to disagree with the data)."""
        ln = len(data) if length is None else length
        assert ln <= 0xFFFF
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        self.out += ln.to_bytes(2, "little") + (ln ^ 0xFFFF).to_bytes(2, "little") + bytes(data)

    def _tokens(self, tokens, lit, dist, eob=True):
        acc, n = self.acc, self.n
        LEN, DIST, DB, DE = _LEN, _DIST, DIST_BASE, DIST_EXTRA
        for t in tokens:
            k = t[0]
            if k == "L":
                c, l = lit[t[1]]
                acc |= c << n
                n += l
            elif k == "M":
                s, eb, ev = LEN[t[1]] if len(t) == 3 else (284, 5, 31)
                c, l = lit[s]
                acc |= c << n
                n += l
                if eb:
                    acc |= ev << n
                    n += eb
                d = t[2]
                ds = DIST[d]
                c, l = dist[ds]
                acc |= c << n
                n += l
                eb = DE[ds]
                if eb:
                    acc |= (d - DB[ds]) << n
                    n += eb
            elif k == "S":     # a raw literal/length symbol
                c, l = lit[t[1]]
                acc |= c << n
                n += l
            elif k == "D":     # a raw distance symbol and its extra bits' value
                c, l = dist[t[1]]
                acc |= c << n
                n += l
                eb = DE[t[1]] if t[1] < 30 else 13
                acc |= (t[2] & ((1 << eb) - 1)) << n
                n += eb
            else:              # ("R", value, nbits)
                acc |= t[1] << n
                n += t[2]
            if n >= 2048:
                nb = n >> 3
                self.out += (acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
                acc >>= 8 * nb
                n &= 7
        if eob:
            c, l = lit[256]
            acc |= c << n
            n += l
        self.acc, self.n = acc, n
        self._spill()

    def fixed_block(self, tokens, final, eob=True):
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self._tokens(tokens, canonical_codes(FIXED_LIT_LENGTHS), canonical_codes(FIXED_DIST_LENGTHS), eob)

    def dynamic_header(self, final, hlit, hdist, cl_lens, syms, hclen=None):
        """BFINAL, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code's lengths, then ``syms`` —
        (symbol, extra value) of the code-length alphabet — in that code. Nothing is checked."""
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        if hclen is None:
            hclen = 19
            while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
                hclen -= 1
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CL_ORDER[i]], 3)
        codes = canonical_codes(cl_lens)
        for s, e in syms:
            c, l = codes[s]
            self.bits(c, l)
            if s >= 16:
                self.bits(e, (2, 3, 7)[s - 16])

    def dynamic_block(self, tokens, final, lit_lengths=None, dist_lengths=None, eob=True):
        """A dynamic-Huffman block. Code lengths are the given vectors (which must cover every
        symbol the tokens use, and 256) or length-limited Huffman lengths of the token frequencies;
        a block without matches gets HDIST = 1 with a zero length, one with a single distance
        symbol a lone 1-bit code."""
        if lit_lengths is None or dist_lengths is None:
            lf, df = [0] * 286, [0] * 30
            lf[256] = 1
            for t in tokens:
                if t[0] == "L":
                    lf[t[1]] += 1
                else:
                    lf[_LEN[t[1]][0] if len(t) == 3 else 284] += 1
                    df[_DIST[t[2]]] += 1
            if lit_lengths is None:
                lit_lengths = code_lengths(lf, 15, 2)
            if dist_lengths is None:
                dist_lengths = code_lengths(df, 15, 0)
        lit_lengths, dist_lengths = list(lit_lengths), list(dist_lengths)
        hlit = max(257, max(i + 1 for i, l in enumerate(lit_lengths) if l))
        hdist = max([1] + [i + 1 for i, l in enumerate(dist_lengths) if l])
        syms = rle_lengths(lit_lengths[:hlit] + (dist_lengths + [0])[:hdist])
        cf = [0] * 19
        for s, _ in syms:
            cf[s] += 1
        self.dynamic_header(final, hlit, hdist, code_lengths(cf, 7, 2), syms)
        self._tokens(tokens, canonical_codes(lit_lengths), canonical_codes(dist_lengths), eob)


def tree_lengths(n, rng, max_bits=15, deep=True):
    """Lengths of a complete prefix code with n symbols: a binary tree grown by splitting leaves
    (``deep``: the deepest splittable leaf half of the time, so that codes reach max_bits). In the
    order the leaves were made; shuffle or sort as the case needs."""
    leaves = [0]
    while len(leaves) < n:
        cand = [i for i, d in enumerate(leaves) if d < max_bits]
        if deep and rng.random() < 0.5:
            m = max(leaves[i] for i in cand)
            cand = [i for i in cand if leaves[i] == m]
        i = cand[int(rng.integers(len(cand)))]
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    return leaves
