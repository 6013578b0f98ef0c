// ganon_site_tally.h — the evidence tally of --discover_sites: which single-base alleles other than the
// reference's the reads of one dataset (tumor 0, normal 1) show at each reference position. One source
// for the host decoder (records_to_columns, csrc/ganon_host.cpp) and the device decoder
// (k_bam_site_tally, csrc/ganon_bam.hip): plain C++17, no HIP headers, the same bytes on both sides (as
// ganon_known_sites.h). Internal to the libraries; not part of the C ABI.
//
// Tally: a byte per position of one reference sequence, low nibble the tumor reads' alleles, high
// nibble the normal reads' (nt16 bit set: A 1, C 2, G 4, T 8). A base at query index q < l_seq aligned
// (CIGAR M, = or X) to position 0 <= r < len is evidence of its nibble b when b is one of 1, 2, 4, 8,
// the reference nibble at r is one of 1, 2, 4, 8 and the two differ; nothing else is. Position r is a
// site when alt = low & high is non-zero, its code ref_nt16 << 4 | alt (ganon_known_sites.h's table).
// Bits are only ever OR-ed in: the tally depends neither on the order of the records nor on a record
// being tallied twice.
//
// Rule (the evidence filters and the mode): a record whose mapq is below min_mapq or whose flag has a
// bit of exclude_flags gives no evidence; a base gives evidence only when its own quality byte, compared
// unsigned, is >= min_base_quality (a record without qualities stores 0xFF and passes: no special
// case). The filters decide which bases may set a bit, nothing else: the bits are still only OR-ed in.
// Mode kBoth reads the byte as above; under kNormal position r is a site when alt = high nibble is
// non-zero and the tumor's nibble is not consulted. Evidence never holds the reference's base, so the
// code stays a valid table code in both modes. The zero Rule is the unfiltered intersection.
#ifndef GANON_SITE_TALLY_H
#define GANON_SITE_TALLY_H

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define ST_FN __host__ __device__ __forceinline__
#else
#define ST_FN inline
#endif

namespace ganon_st {

// One reference sequence: the upper-cased nt16 genome (two bases per byte, base 0 of a byte its high
// nibble — the layout of a BAM record's bases), the nibble index of the sequence's first base in it
// and its length. off < 0: the sequence is not in the FASTA, nothing is evidence.
struct Ref {
  const uint8_t *nt16 = nullptr;
  int64_t off = -1;
  int64_t len = 0;
};

enum Mode : int32_t { kBoth = 0, kNormal = 1 };

struct Rule {
  int32_t min_base_quality = 0;   // 0..93
  int32_t min_mapq = 0;           // 0..255
  uint32_t exclude_flags = 0;     // 0..65535
  int32_t mode = kBoth;
};

ST_FN bool rule_valid(const Rule &u) {
  return u.min_base_quality >= 0 && u.min_base_quality <= 93 && u.min_mapq >= 0 && u.min_mapq <= 255 &&
         u.exclude_flags <= 65535u && (u.mode == kBoth || u.mode == kNormal);
}

// Is any evidence filter set? (the mode is no filter: it is how the bytes are read)
ST_FN bool filtered(const Rule &u) { return u.min_base_quality > 0 || u.min_mapq > 0 || u.exclude_flags != 0; }

// May a record that `skips` leaves in give evidence under the rule's record filters?
ST_FN bool passes(const Rule &u, uint32_t flag, int32_t mapq) { return mapq >= u.min_mapq && !(flag & u.exclude_flags); }

// Does the rule skip the record whole? (ganon_ks::skips: the records the mask later leaves alone)
ST_FN bool skips(int32_t n_ref, int32_t tid, uint32_t flag, int32_t ncig, int32_t lseq) {
  return (flag & 4u) || tid < 0 || tid >= n_ref || ncig <= 0 || lseq <= 0;
}

ST_FN bool one_base(int b) { return b && !(b & (b - 1)); }

// `cnt` (1..8) nibbles of the packed stream p from nibble index x on, nibble x in bits 31..28, x + 1 in
// 27..24, ...; the nibbles past cnt are zero. Only bytes that hold one of the cnt nibbles are read: on
// the device as the aligned dwords around them (p's allocation is dword-aligned and padded to whole
// dwords), funnel-shifted to x's parity and byte; on the host byte by byte.
ST_FN uint32_t nib8(const uint8_t *p, int64_t x, int cnt) {
  const uint32_t keep = cnt >= 8 ? ~0u : ~(~0u >> (4 * cnt));
#if defined(__HIP_DEVICE_COMPILE__)
  const uintptr_t a = reinterpret_cast<uintptr_t>(p + (x >> 1));
  const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
  const int sh = 2 * (int)(a & 3) + (int)(x & 1);   // nibbles of w[0] before x
  const uint64_t hi = __builtin_bswap32(w[0]);
  const uint64_t lo = sh + cnt > 8 ? __builtin_bswap32(w[1]) : 0u;
  return (uint32_t)((((hi << 32) | lo) << (4 * sh)) >> 32) & keep;
#else
  uint64_t v = 0;
  const int64_t b0 = x >> 1, b1 = (x + cnt - 1) >> 1;
  for (int64_t b = b0; b <= b1; ++b) v |= (uint64_t)p[b] << (56 - 8 * (b - b0));   // (at most five bytes)
  return (uint32_t)((v << (4 * (x & 1))) >> 32) & keep;
#endif
}

// The bases of one M / = / X op: query [q, q + len) against reference [r, r + len), clipped to the
// read (q < lseq) and the sequence (0 <= r < R.len). Eight bases a step: read nibbles XOR reference
// nibbles, nibble by nibble only inside a word that differs. store(position, bits) ORs. Qual: a
// differing base is evidence only when qual[its query index] >= min_bq; the quality bytes are read at
// mismatches alone (qual is the record's, indexed like seq: the clip below moves both).
template <bool Qual, class Store>
ST_FN void tally_span(const Ref &R, const uint8_t *seq, const uint8_t *qual, int min_bq, int32_t lseq, int64_t r, int64_t q,
                      int64_t len, int shift, Store &store) {
  if (r < 0) {   // (a record placed before the sequence's start)
    q -= r;
    len += r;
    r = 0;
  }
  int64_t n = len;
  if (n > lseq - q) n = lseq - q;
  if (n > R.len - r) n = R.len - r;
  for (int64_t k = 0; k < n; k += 8) {
    const int cnt = n - k < 8 ? (int)(n - k) : 8;
    const uint32_t rd = nib8(seq, q + k, cnt), rf = nib8(R.nt16, R.off + r + k, cnt);
    uint32_t x = rd ^ rf;
    if (!x) continue;
    for (int j = 0; j < cnt; ++j) {
      const int s = 28 - 4 * j;
      if (!((x >> s) & 15u)) continue;
      const int b = (int)((rd >> s) & 15u), f = (int)((rf >> s) & 15u);
      if (!(one_base(b) && one_base(f))) continue;
      if (Qual && (int)qual[q + k + j] < min_bq) continue;
      store(r + k + j, (uint8_t)(b << shift));
    }
  }
}

// One record, by one thread: its CIGAR walked from pos (M = X advance both, I S the query, D N the
// reference, H P neither). dataset 0 (tumor) ORs into the low nibbles, 1 (normal) into the high ones.
// The caller has checked `skips`, `passes` and that R.off >= 0. Qual: as tally_span (qual: the
// record's lseq quality bytes, not read otherwise).
template <bool Qual, class Store>
ST_FN void tally_record(const Ref &R, int32_t pos, int32_t ncig, int32_t lseq, const uint32_t *cig, const uint8_t *seq,
                        const uint8_t *qual, int min_bq, int dataset, Store &store) {
  int64_t r = pos, q = 0;
  for (int k = 0; k < ncig && q < lseq && r < R.len; ++k) {
    const uint32_t w = cig[k];
    const int op = (int)(w & 15u);
    const int64_t len = w >> 4;
    if (op == 0 || op == 7 || op == 8) {
      tally_span<Qual>(R, seq, qual, min_bq, lseq, r, q, len, 4 * dataset, store);
      r += len;
      q += len;
    } else if (op == 1 || op == 4) {
      q += len;
    } else if (op == 2 || op == 3) {
      r += len;
    }
  }
}

// (pos, code) of the sites of one sequence's tally bytes, in position order; returns their number
// (pos / code null: the count alone). The reference nibble comes from R. mode kBoth: alt = low & high
// nibble; kNormal: alt = the high nibble alone.
ST_FN int64_t compact(const Ref &R, const uint8_t *bytes, int64_t len, int32_t mode, int32_t *pos, uint8_t *code) {
  int64_t n = 0;
  for (int64_t r = 0; r < len; ++r) {
    const int alt = (mode == kNormal ? 15 : bytes[r]) & (bytes[r] >> 4) & 15;
    if (!alt) continue;
    if (pos) {
      const int64_t x = R.off + r;
      pos[n] = (int32_t)r;
      code[n] = (uint8_t)((((R.nt16[x >> 1] >> ((x & 1) ? 0 : 4)) & 15) << 4) | alt);
    }
    ++n;
  }
  return n;
}

}  // namespace ganon_st

#endif  // GANON_SITE_TALLY_H
