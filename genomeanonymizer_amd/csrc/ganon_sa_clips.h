// ganon_sa_clips.h — the rule of --mask_sa_clips: the panel mask of ganon_known_sites.h carried to a
// record's soft-clipped bases along the alignments its SA:Z tag names. A chimeric read's
// primary record holds the whole sequence, soft clip included, and the written sequence comes from it;
// the clipped bases are aligned only in the supplementary record. One source for the host decoder
// (records_to_columns, csrc/ganon_host.cpp) and the device decoder (k_bam_sa_clips, csrc/ganon_bam.hip):
// plain C++17, no HIP headers, no local arrays, the same bytes on both sides. Internal to the libraries.
//
// A record's clips are the S op that is its first op after the leading H ops and the S op that is its
// last op before the trailing H ops (the only places SAM allows one): SEQ indices [0, lead) and
// [trail_from, l_seq). Lf, the full read's length, is l_seq plus the leading and the trailing H ops.
// Records without a clip are left at once: their SA entries are neither walked nor counted.
#ifndef GANON_SA_CLIPS_H
#define GANON_SA_CLIPS_H

#include "ganon_known_sites.h"

namespace ganon_sa {

// The BAM header's sequence names, sorted bytewise (a prefix before the longer name): name i is
// blob[off[i], off[i + 1]) and stands for BAM sequence id tid[i].
struct Names {
  int32_t n = 0;
  const int64_t *off = nullptr;   // [n + 1]
  const char *blob = nullptr;
  const int32_t *tid = nullptr;
};

struct Clip {
  int64_t hlead = 0, lf = 0;          // the leading H ops' length; the full read's length
  int64_t lead = 0, trail_from = 0;   // clipped SEQ indices: [0, lead) and [trail_from, l_seq)
};

constexpr int64_t kMaxPos = 2147483647;   // an entry's pos: 1..2^31-1
constexpr int64_t kMaxOpLen = (1 << 28) - 1;

// The record's clips (false: it has none, the rule leaves it).
KS_FN bool own_clip(int32_t ncig, int32_t lseq, const uint32_t *cig, Clip *c) {
  int32_t k0 = 0, k1 = ncig - 1;
  int64_t hl = 0, ht = 0;
  while (k0 < ncig && (cig[k0] & 15u) == 5u) hl += cig[k0++] >> 4;
  if (k0 >= ncig) return false;   // (hard clips only)
  while (k1 > k0 && (cig[k1] & 15u) == 5u) ht += cig[k1--] >> 4;
  const uint32_t w0 = cig[k0], w1 = cig[k1];
  const int64_t l0 = w0 >> 4, l1 = w1 >> 4;
  c->hlead = hl;
  c->lf = (int64_t)lseq + hl + ht;
  c->lead = (w0 & 15u) == 4u ? (l0 < lseq ? l0 : (int64_t)lseq) : 0;
  c->trail_from = (w1 & 15u) == 4u ? (l1 < lseq ? lseq - l1 : 0) : (int64_t)lseq;
  return c->lead > 0 || c->trail_from < lseq;
}

// The BAM sequence id of the header name s[0, len) (-1: not a header name).
KS_FN int32_t find_name(const Names &N, const uint8_t *s, int64_t len) {
  int32_t lo = 0, hi = N.n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    const char *m = N.blob + N.off[mid];
    const int64_t ml = N.off[mid + 1] - N.off[mid];
    int64_t k = 0;
    while (k < ml && k < len && (uint8_t)m[k] == s[k]) ++k;
    if (k == ml && k == len) return N.tid[mid];
    const bool less = k == ml ? true : (k == len ? false : (uint8_t)m[k] < s[k]);   // (name mid < s)
    if (less) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// s[0, n) as a decimal of digits only, at most cap (else -1).
KS_FN int64_t decimal(const uint8_t *s, int64_t n, int64_t cap) {
  if (n <= 0) return -1;
  int64_t v = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int d = (int)s[i] - '0';
    if (d < 0 || d > 9) return -1;
    v = v * 10 + d;
    if (v > cap) return -1;
  }
  return v;
}

// The BAM op code of a CIGAR letter (-1: none).
KS_FN int op_of(uint8_t ch) {
  switch (ch) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    default: return -1;
  }
}

// The next run of the CIGAR text s[i, n): its op and length, i moved past it (false: malformed).
KS_FN bool next_op(const uint8_t *s, int64_t n, int64_t &i, int &op, int64_t &len) {
  int64_t v = 0;
  const int64_t i0 = i;
  while (i < n && s[i] >= '0' && s[i] <= '9') {
    v = v * 10 + (s[i] - '0');
    if (v > kMaxOpLen) return false;
    ++i;
  }
  if (i == i0 || i >= n || v < 1) return false;
  op = op_of(s[i++]);
  len = v;
  return op >= 0;
}

// The complement of a one-base nt16 nibble (A1 <-> T8, C2 <-> G4); 0 for every other nibble.
KS_FN int comp(int b) { return b == 1 ? 8 : b == 8 ? 1 : b == 2 ? 4 : b == 4 ? 2 : 0; }

// One entry e[0, n) of the tag (no ';' inside). *used: it passed every check (else nothing was written).
// Returns the clip bases rewritten.
KS_FN int mask_entry(const ganon_ks::View &S, const Names &N, const Clip &c, bool rec_rev, int32_t lseq, uint8_t *seq,
                     uint8_t *qual, bool q_on, const uint8_t *e, int64_t n, bool *used) {
  *used = false;
  int64_t c0 = -1, c1 = -1, c2 = -1, c3 = -1;
  int nc = 0;
  for (int64_t i = 0; i < n; ++i)
    if (e[i] == ',') {
      if (nc == 0) c0 = i; else if (nc == 1) c1 = i; else if (nc == 2) c2 = i; else if (nc == 3) c3 = i;
      ++nc;
    }
  if (nc != 5) return 0;   // rname,pos,strand,CIGAR,mapQ,NM
  const int32_t tid = find_name(N, e, c0);
  if (tid < 0) return 0;
  const int64_t pos = decimal(e + c0 + 1, c1 - c0 - 1, kMaxPos);
  if (pos < 1) return 0;
  if (c2 - c1 != 2 || (e[c1 + 1] != '+' && e[c1 + 1] != '-')) return 0;
  const bool ent_rev = e[c1 + 1] == '-';
  const uint8_t *cg = e + c2 + 1;
  const int64_t cn = c3 - c2 - 1;
  if (cn <= 0) return 0;
  int64_t qlen = 0;
  for (int64_t i = 0; i < cn;) {
    int op;
    int64_t len;
    if (!next_op(cg, cn, i, op, len)) return 0;
    if (op == 0 || op == 1 || op == 4 || op == 5 || op == 7 || op == 8) qlen += len;
  }
  if (qlen != c.lf) return 0;
  *used = true;
  if (tid >= S.n_ref) return 0;
  const int64_t lo = S.off[tid], hi = S.off[tid + 1];
  if (lo >= hi) return 0;
  const bool flip = rec_rev != ent_rev;
  int64_t r = pos - 1, qs = 0;
  int cnt = 0;
  for (int64_t i = 0; i < cn;) {
    int op;
    int64_t len;
    next_op(cg, cn, i, op, len);
    if (op == 0 || op == 7 || op == 8) {
      for (int64_t j = ganon_ks::lower(S.pos, lo, hi, r); j < hi; ++j) {
        const int64_t p = S.pos[j];
        if (p >= r + len) break;
        const int64_t idx = qs + (p - r);
        const int64_t x = (flip ? c.lf - 1 - idx : idx) - c.hlead;
        if (x < 0 || x >= lseq || (x >= c.lead && x < c.trail_from)) continue;
        const uint8_t code = S.code[j];
        const int sh = (x & 1) ? 0 : 4;
        const uint8_t byte = seq[x >> 1];
        const int own = (byte >> sh) & 15, b = flip ? comp(own) : own;
        if (ganon_ks::hits(b, code)) {
          const int ref = flip ? comp(code >> 4) : (code >> 4);
          seq[x >> 1] = (uint8_t)((byte & ~(15 << sh)) | (ref << sh));
          if (q_on) qual[x] = (uint8_t)S.qual;
          ++cnt;
        }
      }
      r += len;
      qs += len;
    } else if (op == 1 || op == 4 || op == 5) {
      qs += len;
    } else if (op == 2 || op == 3) {
      r += len;
    }
  }
  return cnt;
}

// The value [*v0, *v1) of the record's first SA:Z tag (false: none, or not NUL-terminated inside the aux).
KS_FN bool find_sa(const uint8_t *a, int64_t len, int64_t *v0, int64_t *v1) {
  int64_t j = 0;
  while (j + 3 <= len) {
    const uint8_t t0 = a[j], t1 = a[j + 1], ty = a[j + 2];
    j += 3;
    int sz = 0;
    if (ty == 'Z' || ty == 'H') {
      int64_t k = j;
      while (k < len && a[k]) ++k;
      if (t0 == 'S' && t1 == 'A' && ty == 'Z') {
        *v0 = j;
        *v1 = k;
        return k < len;
      }
      j = k + 1;
      continue;
    }
    const uint8_t st = ty == 'B' ? (j < len ? a[j] : (uint8_t)0) : ty;
    if (st == 'A' || st == 'c' || st == 'C') sz = 1;
    else if (st == 's' || st == 'S') sz = 2;
    else if (st == 'i' || st == 'I' || st == 'f') sz = 4;
    if (ty == 'B') {
      if (j + 5 > len) break;
      const int64_t cnt = (int64_t)((uint32_t)a[j + 1] | (uint32_t)a[j + 2] << 8 | (uint32_t)a[j + 3] << 16 | (uint32_t)a[j + 4] << 24);
      if (cnt > 0x7FFFFFFF) break;   // (a negative count: malformed)
      j += 5 + (int64_t)sz * cnt;
    } else {
      if (!sz) break;   // malformed: leave the rest
      j += sz;
    }
  }
  return false;
}

// The entries of the tag value aux[v0, v1) in tag order (empty pieces dropped) on a record with clips c.
// Returns the clip bases rewritten; *ignored gains the entries that failed a check.
KS_FN int mask_tag(const ganon_ks::View &S, const Names &N, const Clip &c, uint32_t flag, int32_t lseq, uint8_t *seq,
                   uint8_t *qual, const uint8_t *aux, int64_t v0, int64_t v1, int *ignored) {
  const bool q_on = S.qual >= 0 && qual[0] != 0xFF;
  int cnt = 0;
  for (int64_t i = v0; i < v1;) {
    int64_t k = i;
    while (k < v1 && aux[k] != ';') ++k;
    if (k > i) {
      bool used;
      cnt += mask_entry(S, N, c, (flag & 16u) != 0, lseq, seq, qual, q_on, aux + i, k - i, &used);
      if (!used) ++*ignored;
    }
    i = k + 1;
  }
  return cnt;
}

// One record, by one thread, after ganon_ks::mask_record.
KS_FN int mask_record(const ganon_ks::View &S, const Names &N, int32_t tid, uint32_t flag, int32_t ncig, int32_t lseq,
                      const uint32_t *cig, uint8_t *seq, uint8_t *qual, const uint8_t *aux, int64_t aux_len, int *ignored) {
  if (ganon_ks::skips(S, tid, flag, ncig, lseq)) return 0;
  Clip c;
  if (!own_clip(ncig, lseq, cig, &c)) return 0;
  int64_t v0, v1;
  if (!find_sa(aux, aux_len, &v0, &v1)) return 0;
  return mask_tag(S, N, c, flag, lseq, seq, qual, aux, v0, v1, ignored);
}

}  // namespace ganon_sa

#endif  // GANON_SA_CLIPS_H
