// ganon_deflate_core.h — the BGZF member encoder of ganon_deflate.hip (see there for the phases):
// one block in, one member out, written so that the device (one 256-lane workgroup) and the host
// (one lane; plain C++17, no HIP headers: tools/deflate_host_check.cpp) run the same source and
// give the same bytes. Internal to libganon_hip.so; not part of the C ABI.
#ifndef GANON_DEFLATE_CORE_H
#define GANON_DEFLATE_CORE_H

#include <algorithm>
#include <cstdint>

namespace ganon_deflate_core {

constexpr int kDefThreads = 256;
constexpr int kDefMaxIn = 0xFF00;      // input bytes per member (bgzip's block size)
constexpr int kDefSlot = 65536;        // a member's slot: the BGZF limit
constexpr int kDefRound = 256;         // positions matched per round
constexpr int kDefHashBits = 15;
constexpr int kDefSlices = 256;        // CRC and emission partitions (fixed: not the lane count)
constexpr int kDefInWords = kDefMaxIn / 4 + 4;
constexpr int kDefMaxLen = 258, kDefMaxDist = 32768;
constexpr int kDefMinTable = 4;   // shortest match taken from the hash table (5..10 measured larger on FASTQ)
constexpr uint32_t kCrcPoly = 0xEDB88320u;

struct DefShared {
  uint32_t in[kDefInWords];            // the block's bytes (zero padded); later the bit buffer
  uint32_t head[1 << (kDefHashBits - 1)];   // per hash, 16 bits: position + 1 of the latest earlier-round position
  uint32_t crc_tab[256];
  uint32_t x2n[24];                    // x^(2^k) mod P
  uint32_t freq_ll[288], freq_d[32], freq_cl[19];
  uint8_t len_ll[288], len_d[32], len_cl[19];
  uint16_t code_ll[288], code_d[32], code_cl[19];
  uint16_t order[288];                 // used symbols by (count, symbol)
  uint32_t wt[576];
  uint16_t parent[576];
  uint8_t depth[576];
  int32_t bl[16];
  uint32_t rtok[kDefRound];            // a round's candidate tokens and advances
  uint16_t radv[kDefRound];
  uint16_t cl_tok[320];                // header symbols: symbol | extra << 8
  uint32_t tsum[kDefSlices];
  int32_t n_cl, hlit, hdist, hclen;
  int32_t ntok, next;
  uint32_t total_bits, hdr_bits;
  uint32_t crc_acc;
};

constexpr uint8_t kDefClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

#if defined(__HIP__) || defined(__HIPCC__)
#define DEF_FN __host__ __device__ inline
#else
#define DEF_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define DEF_SYNC() __syncthreads()
// max into the 16-bit half `slot` of a word array (the other half belongs to another hash: a
// compare-and-swap on the word; a failed swap means another lane's succeeded, so the retries are
// bounded by the lanes of a round)
__device__ __forceinline__ void def_amax16(uint32_t *words, uint32_t slot, uint32_t v) {
  uint32_t *w = words + (slot >> 1);
  const int sh = (int)(slot & 1) * 16;
  uint32_t old = *w;
  for (int tries = 0; tries < 4 * kDefRound; ++tries) {
    if (((old >> sh) & 0xFFFFu) >= v) break;
    const uint32_t prev = atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (v << sh));
    if (prev == old) break;
    old = prev;
  }
}
__device__ __forceinline__ void def_aadd(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void def_aor(uint32_t *p, uint32_t v) { atomicOr(p, v); }
__device__ __forceinline__ void def_axor(uint32_t *p, uint32_t v) { atomicXor(p, v); }
#else
#define DEF_SYNC() ((void)0)
inline void def_amax16(uint32_t *words, uint32_t slot, uint32_t v) {
  uint32_t *w = words + (slot >> 1);
  const int sh = (int)(slot & 1) * 16;
  if (((*w >> sh) & 0xFFFFu) < v) *w = (*w & ~(0xFFFFu << sh)) | (v << sh);
}
inline void def_aadd(uint32_t *p, uint32_t v) { *p += v; }
inline void def_aor(uint32_t *p, uint32_t v) { *p |= v; }
inline void def_axor(uint32_t *p, uint32_t v) { *p ^= v; }
#endif

// (tuning build only, -DDEF_PROF: lane 0's s_memtime per phase, summed into g_def_prof of
// ganon_deflate.hip; tools/deflate_prof.py)
#if defined(DEF_PROF) && defined(__HIP_DEVICE_COMPILE__)
#define DEF_PROF_BEGIN() uint64_t prof_last = __builtin_amdgcn_s_memtime()
#define DEF_MARK(i)                                                         \
  do {                                                                      \
    if (t == 0) {                                                           \
      const uint64_t now_ = __builtin_amdgcn_s_memtime();                   \
      atomicAdd(&g_def_prof[i], (unsigned long long)(now_ - prof_last));    \
      prof_last = now_;                                                     \
    }                                                                       \
  } while (0)
#else
#define DEF_PROF_BEGIN() ((void)0)
#define DEF_MARK(i) ((void)0)
#endif

DEF_FN int def_log2(uint32_t v) { return 31 - __builtin_clz(v); }

// a(x) * b(x) mod P in the reflected representation (bit 31 = x^0)
DEF_FN uint32_t def_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

// x^(8k) mod P: the operator that runs a CRC register over k zero bytes
DEF_FN uint32_t def_shift_op(const DefShared &S, uint32_t k) {
  uint32_t p = 0x80000000u;
  for (int i = 3; k; k >>= 1, ++i)
    if (k & 1) p = def_mulmod(S.x2n[i], p);
  return p;
}

DEF_FN uint32_t def_load4(const DefShared &S, int i) {
  const uint64_t w = (uint64_t)S.in[i >> 2] | ((uint64_t)S.in[(i >> 2) + 1] << 32);
  return (uint32_t)(w >> (8 * (i & 3)));
}
DEF_FN uint32_t def_byte(const DefShared &S, int i) { return (S.in[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
DEF_FN uint32_t def_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kDefHashBits); }

// common prefix of the bytes at a < b, at most maxl (b + maxl <= n; the words past n are zero padding
// inside S.in and never counted)
DEF_FN int def_match_len(const DefShared &S, int a, int b, int maxl) {
  int k = 0;
  while (k < maxl) {
    const uint32_t x = def_load4(S, a + k) ^ def_load4(S, b + k);
    if (x) {
      k += __builtin_ctz(x) >> 3;
      break;
    }
    k += 4;
  }
  return k < maxl ? k : maxl;
}

// token: a literal's byte, or bit 31 | (length - 3) << 16 | (distance - 1)
DEF_FN void def_len_code(int l3, int &code, int &eb, int &ev) {
  if (l3 == 255) { code = 285; eb = 0; ev = 0; return; }
  if (l3 < 8) { code = 257 + l3; eb = 0; ev = 0; return; }
  eb = def_log2((uint32_t)l3) - 2;
  code = 257 + 4 * (eb + 1) + ((l3 >> eb) & 3);
  ev = l3 & ((1 << eb) - 1);
}
DEF_FN void def_dist_code(int d1, int &code, int &eb, int &ev) {
  if (d1 < 4) { code = d1; eb = 0; ev = 0; return; }
  eb = def_log2((uint32_t)d1) - 1;
  code = 2 * (eb + 1) + ((d1 >> eb) & 1);
  ev = d1 & ((1 << eb) - 1);
}

DEF_FN void def_count_token(DefShared &S, uint32_t tk) {
  if (tk & 0x80000000u) {
    int c, eb, ev;
    def_len_code((int)((tk >> 16) & 0xFF), c, eb, ev);
    def_aadd(&S.freq_ll[c], 1);
    def_dist_code((int)(tk & 0x7FFF), c, eb, ev);
    def_aadd(&S.freq_d[c], 1);
  } else {
    def_aadd(&S.freq_ll[tk & 0xFF], 1);
  }
}

DEF_FN uint32_t def_token_bits(const DefShared &S, uint32_t tk) {
  if (!(tk & 0x80000000u)) return S.len_ll[tk & 0xFF];
  int c, eb, ev, c2, eb2;
  def_len_code((int)((tk >> 16) & 0xFF), c, eb, ev);
  def_dist_code((int)(tk & 0x7FFF), c2, eb2, ev);
  return (uint32_t)(S.len_ll[c] + eb + S.len_d[c2] + eb2);
}

// Length-limited code lengths of freq[0, nsym) into len (collective; the serial part is lane 0's).
// Fewer than two used symbols: two codes of one bit (the used symbol and symbol 0, or 1 if 0 is the
// used one; symbols 0 and 1 if none is), so that every code an inflater sees is complete.
template <int NL>
DEF_FN void def_build_lengths(DefShared &S, const uint32_t *freq, int nsym, int limit, uint8_t *len, int t) {
  for (int s = t; s < nsym; s += NL) {
    len[s] = 0;
    const uint32_t f = freq[s];
    if (!f) continue;
    int rank = 0;
    for (int j = 0; j < nsym; ++j) {
      const uint32_t g = freq[j];
      rank += (g && (g < f || (g == f && j < s))) ? 1 : 0;
    }
    S.order[rank] = (uint16_t)s;
  }
  DEF_SYNC();
  if (t == 0) {
    int used = 0;
    for (int s = 0; s < nsym; ++s) used += freq[s] ? 1 : 0;
    if (used < 2) {
      const int a = used ? S.order[0] : 0;
      len[a] = 1;
      len[a == 0 ? 1 : 0] = 1;
    } else {
      for (int i = 0; i < used; ++i) S.wt[i] = freq[S.order[i]];
      int li = 0, ii = used, nn = used;
      while (nn < 2 * used - 1) {   // the two lightest of the leaf queue and the node queue
        int pick[2];
        for (int k = 0; k < 2; ++k)
          pick[k] = (li < used && (ii >= nn || S.wt[li] <= S.wt[ii])) ? li++ : ii++;
        S.wt[nn] = S.wt[pick[0]] + S.wt[pick[1]];
        S.parent[pick[0]] = (uint16_t)nn;
        S.parent[pick[1]] = (uint16_t)nn;
        ++nn;
      }
      S.depth[nn - 1] = 0;
      for (int i = nn - 2; i >= 0; --i) S.depth[i] = (uint8_t)(S.depth[S.parent[i]] + 1);
      for (int d = 0; d < 16; ++d) S.bl[d] = 0;
      for (int i = 0; i < used; ++i) S.bl[S.depth[i] < limit ? S.depth[i] : limit] += 1;
      // clamping made the Kraft sum too large: drop one code of the limit's length and split the
      // deepest shorter code in two, one unit of 2^-limit at a time
      int64_t total = 0;
      for (int d = 1; d <= limit; ++d) total += (int64_t)S.bl[d] << (limit - d);
      while (total > ((int64_t)1 << limit)) {
        S.bl[limit] -= 1;
        for (int d = limit - 1; d >= 1; --d)
          if (S.bl[d]) {
            S.bl[d] -= 1;
            S.bl[d + 1] += 2;
            break;
          }
        total -= 1;
      }
      int i = 0;   // rarest symbols take the longest codes
      for (int d = limit; d >= 1; --d)
        for (int c = 0; c < S.bl[d] && i < used; ++c) len[S.order[i++]] = (uint8_t)d;
    }
  }
  DEF_SYNC();
}

// canonical codes, bit-reversed for the LSB-first writer (lane 0)
DEF_FN void def_gen_codes(const uint8_t *len, int nsym, uint16_t *code) {
  int cnt[16], nxt[16];
  for (int d = 0; d < 16; ++d) cnt[d] = 0;
  for (int s = 0; s < nsym; ++s) cnt[len[s]] += 1;
  cnt[0] = 0;
  int c = 0;
  nxt[0] = 0;
  for (int d = 1; d < 16; ++d) {
    c = (c + cnt[d - 1]) << 1;
    nxt[d] = c;
  }
  for (int s = 0; s < nsym; ++s) {
    const int l = len[s];
    uint32_t v = 0;
    if (l) {
      uint32_t x = (uint32_t)nxt[l]++;
      for (int k = 0; k < l; ++k, x >>= 1) v = (v << 1) | (x & 1);
    }
    code[s] = (uint16_t)v;
  }
}

// LSB-first bit writer into the LDS bit buffer: whole words are or-ed in (a word may be shared with
// the neighbouring slice)
struct DefBitW {
  uint32_t *buf;
  uint64_t acc;
  int nb, word, nwords;
  DEF_FN void init(uint32_t *b, uint32_t bitpos, int words) {
    buf = b;
    acc = 0;
    nb = (int)(bitpos & 31);
    word = (int)(bitpos >> 5);
    nwords = words;
  }
  DEF_FN void put(uint32_t v, int n) {
    acc |= (uint64_t)v << nb;
    nb += n;
    if (nb >= 32) {
      if (word < nwords) def_aor(&buf[word], (uint32_t)acc);
      ++word;
      acc >>= 32;
      nb -= 32;
    }
  }
  DEF_FN void finish() {
    if (nb > 0 && (uint32_t)acc && word < nwords) def_aor(&buf[word], (uint32_t)acc);
  }
};

DEF_FN void def_put_token(const DefShared &S, DefBitW &w, uint32_t tk) {
  if (!(tk & 0x80000000u)) {
    w.put(S.code_ll[tk & 0xFF], S.len_ll[tk & 0xFF]);
    return;
  }
  int c, eb, ev;
  def_len_code((int)((tk >> 16) & 0xFF), c, eb, ev);
  w.put(S.code_ll[c], S.len_ll[c]);
  if (eb) w.put((uint32_t)ev, eb);
  def_dist_code((int)(tk & 0x7FFF), c, eb, ev);
  w.put(S.code_d[c], S.len_d[c]);
  if (eb) w.put((uint32_t)ev, eb);
}

struct alignas(16) DefTok4 {
  uint32_t v[4];
};

DEF_FN uint8_t def_seq(const DefShared &S, int i) { return i < S.hlit ? S.len_ll[i] : S.len_d[i - S.hlit]; }

DEF_FN void def_cl_emit(DefShared &S, int sym, int extra) {
  if (S.n_cl < 320) S.cl_tok[S.n_cl++] = (uint16_t)(sym | (extra << 8));
  S.freq_cl[sym] += 1;
}

// One block in[0, n) (1 <= n <= kDefMaxIn) -> one BGZF member in out[0, kDefSlot); tok is the
// block's token scratch (kDefMaxIn words). Returns the member's size (uniform).
template <int NL>
DEF_FN int deflate_block(DefShared &S, const uint8_t *in, int n, uint8_t *out, uint32_t *tok, int t) {
  if (n < 1 || n > kDefMaxIn) return 0;
  DEF_PROF_BEGIN();
  // ---- stage the block, tables
  for (int i = t; i < kDefInWords; i += NL) S.in[i] = 0;
  for (int i = t; i < (1 << (kDefHashBits - 1)); i += NL) S.head[i] = 0;
  for (int i = t; i < 288; i += NL) S.freq_ll[i] = 0;
  for (int i = t; i < 32; i += NL) S.freq_d[i] = 0;
  for (int i = t; i < 19; i += NL) S.freq_cl[i] = 0;
  for (int i = t; i < 256; i += NL) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
    S.crc_tab[i] = c;
  }
  if (t == 0) {
    uint32_t p = 0x40000000u;   // x^1
    for (int k = 0; k < 24; ++k) {
      S.x2n[k] = p;
      p = def_mulmod(p, p);
    }
    S.crc_acc = 0;
    S.ntok = 0;
    S.next = 0;
    S.n_cl = 0;
  }
  DEF_SYNC();
  {
    uint8_t *b = reinterpret_cast<uint8_t *>(S.in);
    for (int i = t; i < n; i += NL) b[i] = in[i];
  }
  DEF_SYNC();

  // ---- CRC32: slices from a zero register, shifted over the bytes behind them
  {
    const int per = (n + kDefSlices - 1) / kDefSlices;
    for (int sl = t; sl < kDefSlices; sl += NL) {
      const int lo = sl * per, hi = lo + per < n ? lo + per : n;
      uint32_t acc = 0;
      if (lo < hi) {
        uint32_t c = 0;
        for (int i = lo; i < hi; ++i) c = S.crc_tab[(c ^ def_byte(S, i)) & 0xFF] ^ (c >> 8);
        acc = def_mulmod(def_shift_op(S, (uint32_t)(n - hi)), c);
      }
      if (sl == 0) acc ^= def_mulmod(def_shift_op(S, (uint32_t)n), 0xFFFFFFFFu);   // the initial register
      if (acc) def_axor(&S.crc_acc, acc);
    }
  }

  DEF_MARK(0);
  // ---- matching and the greedy parse, round by round
  for (int r0 = 0; r0 < n; r0 += kDefRound) {
    for (int k = t; k < kDefRound; k += NL) {
      const int i = r0 + k;
      uint32_t tk = 0;
      int adv = 1;
      if (i < n) {
        tk = def_byte(S, i);
        const int maxl = n - i < kDefMaxLen ? n - i : kDefMaxLen;
        int bl = 0, bd = 0;
        if (maxl >= 3) {
          if (i >= 1) {
            const int l = def_match_len(S, i - 1, i, maxl);
            if (l >= 3) { bl = l; bd = 1; }
          }
          if (maxl >= 4) {
            const uint32_t hs = def_hash(def_load4(S, i));
            const uint32_t c1 = (S.head[hs >> 1] >> ((hs & 1) * 16)) & 0xFFFFu;
            if (c1) {
              const int d = i - (int)(c1 - 1);
              if (d >= 1 && d <= kDefMaxDist) {
                const int l = def_match_len(S, i - d, i, maxl);
                if (l >= kDefMinTable && l > bl) { bl = l; bd = d; }
              }
            }
          }
        }
        if (bl) {
          tk = 0x80000000u | ((uint32_t)(bl - 3) << 16) | (uint32_t)(bd - 1);
          adv = bl;
        }
      }
      S.rtok[k] = tk;
      S.radv[k] = (uint16_t)adv;
    }
    DEF_SYNC();
    for (int k = t; k < kDefRound; k += NL) {
      const int i = r0 + k;
      if (i + 4 <= n) def_amax16(S.head, def_hash(def_load4(S, i)), (uint32_t)i + 1);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if (t < 64) {   // wave 0: the chain through the round's advances, 64 positions at a time
      int p = __builtin_amdgcn_readfirstlane(S.next), nt = __builtin_amdgcn_readfirstlane(S.ntok);
      for (int sub = 0; sub < kDefRound / 64; ++sub) {
        const int base = r0 + sub * 64;
        const int end = base + 64 < n ? base + 64 : n;
        const int adv = S.radv[sub * 64 + t];
        const uint64_t lit = __ballot(adv == 1);   // literal candidates: a run of them is taken at once
        uint64_t mask = 0;
        while (p < end) {
          const int q = p - base;   // (uniform, in [0, 64): p >= base holds from the previous sub-round)
          const uint64_t rest = ~(lit >> q);   // (bits past 63 - q read as set: the run ends at the window)
          const int run = rest ? __builtin_ctzll(rest) : 64 - q;
          if (run) {
            const int take = run < end - p ? run : end - p;
            mask |= (take >= 64 ? ~0ull : ((1ull << take) - 1)) << q;
            p += take;
          } else {
            mask |= 1ull << q;
            p += __builtin_amdgcn_readlane(adv, q);
          }
        }
        if ((mask >> t) & 1) {
          const int idx = nt + __popcll(mask & ((1ull << t) - 1));
          const uint32_t tk = S.rtok[sub * 64 + t];
          if (idx < kDefMaxIn) tok[idx] = tk;
          def_count_token(S, tk);
        }
        nt += __popcll(mask);
      }
      if (t == 0) {
        S.next = p;
        S.ntok = nt;
      }
    }
#else
    if (t == 0) {
      int p = S.next, nt = S.ntok;
      const int end = r0 + kDefRound < n ? r0 + kDefRound : n;
      while (p < end) {
        const uint32_t tk = S.rtok[p - r0];
        if (nt < kDefMaxIn) tok[nt] = tk;
        ++nt;
        def_count_token(S, tk);
        p += S.radv[p - r0];
      }
      S.next = p;
      S.ntok = nt;
    }
#endif
    DEF_SYNC();
  }
  const int ntok = S.ntok;
  DEF_MARK(1);

  // ---- codes
  if (t == 0) S.freq_ll[256] = 1;
  DEF_SYNC();
  def_build_lengths<NL>(S, S.freq_ll, 286, 15, S.len_ll, t);
  def_build_lengths<NL>(S, S.freq_d, 30, 15, S.len_d, t);
  if (t == 0) {
    def_gen_codes(S.len_ll, 286, S.code_ll);
    def_gen_codes(S.len_d, 30, S.code_d);
    int hl = 286, hd = 30;
    while (hl > 257 && !S.len_ll[hl - 1]) --hl;
    while (hd > 1 && !S.len_d[hd - 1]) --hd;
    S.hlit = hl;
    S.hdist = hd;
    const int tot = hl + hd;
    for (int i = 0; i < tot;) {   // run-length code the lengths (a run may cross into the distances)
      const int v = def_seq(S, i);
      int run = 1;
      while (i + run < tot && def_seq(S, i + run) == v) ++run;
      int rem = run;
      if (v == 0) {
        while (rem >= 3) {
          const int r = rem < 138 ? rem : 138;
          if (r <= 10) def_cl_emit(S, 17, r - 3);
          else def_cl_emit(S, 18, r - 11);
          rem -= r;
        }
      } else {
        def_cl_emit(S, v, 0);
        --rem;
        while (rem >= 3) {
          const int r = rem < 6 ? rem : 6;
          def_cl_emit(S, 16, r - 3);
          rem -= r;
        }
      }
      for (; rem > 0; --rem) def_cl_emit(S, v, 0);
      i += run;
    }
  }
  DEF_SYNC();
  def_build_lengths<NL>(S, S.freq_cl, 19, 7, S.len_cl, t);
  if (t == 0) {
    def_gen_codes(S.len_cl, 19, S.code_cl);
    int hc = 19;
    while (hc > 4 && !S.len_cl[kDefClOrder[hc - 1]]) --hc;
    S.hclen = hc;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hc;
    for (int i = 0; i < S.n_cl; ++i) {
      const int sym = S.cl_tok[i] & 0xFF;
      bits += S.len_cl[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
    }
    S.hdr_bits = bits;
  }
  DEF_SYNC();

  DEF_MARK(2);
  // ---- bit lengths of the token slices, their prefix sum
  // (slices of a multiple of four tokens: read four at a time, 16-byte aligned; the scratch is
  // kDefMaxIn words, itself a multiple of four, so a slice's last four stay inside it)
  const int per_tok = ((ntok + kDefSlices - 1) / kDefSlices + 3) & ~3;
  for (int sl = t; sl < kDefSlices; sl += NL) {
    const int lo = sl * per_tok, hi = lo + per_tok < ntok ? lo + per_tok : ntok;
    uint32_t b = 0;
    for (int i = lo; i < hi; i += 4) {
      const DefTok4 q = *reinterpret_cast<const DefTok4 *>(tok + i);
      b += def_token_bits(S, q.v[0]);
      if (i + 1 < hi) b += def_token_bits(S, q.v[1]);
      if (i + 2 < hi) b += def_token_bits(S, q.v[2]);
      if (i + 3 < hi) b += def_token_bits(S, q.v[3]);
    }
    S.tsum[sl] = b;
  }
  DEF_SYNC();
  if (t == 0) {
    uint32_t run = S.hdr_bits;
    for (int sl = 0; sl < kDefSlices; ++sl) {
      const uint32_t b = S.tsum[sl];
      S.tsum[sl] = run;
      run += b;
    }
    S.total_bits = run + S.len_ll[256];
  }
  DEF_SYNC();
  DEF_MARK(3);
  const uint32_t total_bits = S.total_bits;
  const int dyn_bytes = (int)((total_bits + 7) >> 3);
  const uint32_t crc = S.crc_acc ^ 0xFFFFFFFFu;
  const bool dyn = dyn_bytes < n + 5;
  const int payload = dyn ? dyn_bytes : n + 5;
  const int size = 18 + payload + 8;   // <= n + 31 <= 65536
  uint8_t *pl = out + 18;

  if (dyn) {
    // the input is no longer needed: its space becomes the bit buffer (dyn_bytes <= n + 4)
    const int words = (dyn_bytes + 3) >> 2;   // <= kDefInWords
    for (int i = t; i < words; i += NL) S.in[i] = 0;
    DEF_SYNC();
    if (t == 0) {
      DefBitW w;
      w.init(S.in, 0, words);
      w.put(1, 1);   // BFINAL
      w.put(2, 2);   // dynamic
      w.put((uint32_t)(S.hlit - 257), 5);
      w.put((uint32_t)(S.hdist - 1), 5);
      w.put((uint32_t)(S.hclen - 4), 4);
      for (int i = 0; i < S.hclen; ++i) w.put(S.len_cl[kDefClOrder[i]], 3);
      for (int i = 0; i < S.n_cl; ++i) {
        const int sym = S.cl_tok[i] & 0xFF, ex = S.cl_tok[i] >> 8;
        w.put(S.code_cl[sym], S.len_cl[sym]);
        if (sym >= 16) w.put((uint32_t)ex, sym == 16 ? 2 : sym == 17 ? 3 : 7);
      }
      w.finish();
      w.init(S.in, total_bits - S.len_ll[256], words);
      w.put(S.code_ll[256], S.len_ll[256]);
      w.finish();
    }
    for (int sl = t; sl < kDefSlices; sl += NL) {
      const int lo = sl * per_tok, hi = lo + per_tok < ntok ? lo + per_tok : ntok;
      if (lo >= hi) continue;
      DefBitW w;
      w.init(S.in, S.tsum[sl], words);
      for (int i = lo; i < hi; i += 4) {
        const DefTok4 q = *reinterpret_cast<const DefTok4 *>(tok + i);
        def_put_token(S, w, q.v[0]);
        if (i + 1 < hi) def_put_token(S, w, q.v[1]);
        if (i + 2 < hi) def_put_token(S, w, q.v[2]);
        if (i + 3 < hi) def_put_token(S, w, q.v[3]);
      }
      w.finish();
    }
    DEF_SYNC();
    for (int i = t; i < dyn_bytes; i += NL) pl[i] = (uint8_t)def_byte(S, i);
  } else {
    if (t == 0) {
      pl[0] = 1;   // BFINAL, stored
      pl[1] = (uint8_t)(n & 0xFF);
      pl[2] = (uint8_t)(n >> 8);
      pl[3] = (uint8_t)(~n & 0xFF);
      pl[4] = (uint8_t)((~n >> 8) & 0xFF);
    }
    for (int i = t; i < n; i += NL) pl[5 + i] = (uint8_t)def_byte(S, i);
  }
  if (t == 0) {
    const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) out[i] = hdr[i];
    out[16] = (uint8_t)((size - 1) & 0xFF);
    out[17] = (uint8_t)((size - 1) >> 8);
    uint8_t *tr = pl + payload;
    for (int k = 0; k < 4; ++k) {
      tr[k] = (uint8_t)(crc >> (8 * k));
      tr[4 + k] = (uint8_t)((uint32_t)n >> (8 * k));
    }
  }
  DEF_SYNC();   // (S is reused by the caller's next block)
  DEF_MARK(4);
  return size;
}

}  // namespace ganon_deflate_core

#endif  // GANON_DEFLATE_CORE_H
