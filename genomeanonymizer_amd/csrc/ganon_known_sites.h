// ganon_known_sites.h — the panel mask of --known_sites: a read base that shows a listed ALT allele at a
// listed position becomes the reference base, where its record is decoded. One source for the host
// decoder (records_to_columns, csrc/ganon_host.cpp) and the device decoder's thread-per-record path
// (k_bam_known_mask, csrc/ganon_bam.hip): plain C++17, no HIP headers, the same bytes on both sides (as
// ganon_name_hash.h). Internal to the libraries; not part of the C ABI.
//
// Table: per BAM reference sequence tid the sites [off[tid], off[tid + 1]) of pos (0-based, strictly
// increasing) and code = ref_nt16 << 4 | alt_mask (nt16 is a bit set: A 1, C 2, G 4, T 8; ref one bit,
// alt_mask the OR of the ALT bits, never ref's).
#ifndef GANON_KNOWN_SITES_H
#define GANON_KNOWN_SITES_H

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define KS_FN __host__ __device__ __forceinline__
#else
#define KS_FN inline
#endif

namespace ganon_ks {

struct View {
  int32_t n_ref = 0;
  const int64_t *off = nullptr;    // [n_ref + 1]
  const int32_t *pos = nullptr;
  const uint8_t *code = nullptr;
  int32_t qual = -1;               // --masked_base_quality: a rewritten base's quality (-1: left alone)
};

// Is `code` a table code: one reference bit above, ALT bits below, the reference's not among them.
KS_FN bool code_ok(uint8_t code) {
  const int ref = code >> 4, alt = code & 15;
  return ref && !(ref & (ref - 1)) && alt && !(alt & ref);
}

// The first index in [lo, hi) whose position is >= key (hi: none).
KS_FN int64_t lower(const int32_t *pos, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)pos[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Is base nibble b (one of A, C, G, T) an ALT of `code`?
KS_FN bool hits(int b, uint8_t code) { return b && !(b & (b - 1)) && (b & code & 15); }

// Does the rule skip the record whole? (unmapped flag, no reference, no CIGAR, no bases, or no site list)
KS_FN bool skips(const View &S, int32_t tid, uint32_t flag, int32_t ncig, int32_t lseq) {
  return (flag & 4u) || tid < 0 || tid >= S.n_ref || ncig <= 0 || lseq <= 0;
}

// One record, by one thread: a merge walk of its CIGAR ops and the sites of its reference sequence from
// the first one at or after pos. seq / qual are the record's own packed bases and qualities (lseq of
// them; query index q is the high nibble of seq[q / 2] when q is even). Returns the bases rewritten.
KS_FN int mask_record(const View &S, int32_t tid, int32_t pos, uint32_t flag, int32_t ncig, int32_t lseq,
                      const uint32_t *cig, uint8_t *seq, uint8_t *qual) {
  if (skips(S, tid, flag, ncig, lseq)) return 0;
  const int64_t hi = S.off[tid + 1];
  int64_t j = lower(S.pos, S.off[tid], hi, pos);
  if (j >= hi) return 0;
  const bool q_on = S.qual >= 0 && qual[0] != 0xFF;   // (0xFF first: no qualities stored)
  int64_t r = pos, q = 0;
  int cnt = 0;
  for (int k = 0; k < ncig && j < hi && q < lseq; ++k) {
    const uint32_t w = cig[k];
    const int op = (int)(w & 15u);
    const int64_t len = w >> 4;
    if (op == 0 || op == 7 || op == 8) {   // M = X: the sites inside [r, r + len)
      for (; j < hi; ++j) {
        const int64_t p = S.pos[j];
        if (p >= r + len) break;
        const int64_t x = q + (p - r);
        if (x >= lseq) return cnt;   // (a CIGAR longer than the read)
        const uint8_t code = S.code[j];
        const int sh = (x & 1) ? 0 : 4;
        const uint8_t byte = seq[x >> 1];
        if (hits((byte >> sh) & 15, code)) {
          seq[x >> 1] = (uint8_t)((byte & ~(15 << sh)) | ((code >> 4) << sh));
          if (q_on) qual[x] = (uint8_t)S.qual;
          ++cnt;
        }
      }
      r += len;
      q += len;
    } else if (op == 1 || op == 4) {       // I S
      q += len;
    } else if (op == 2 || op == 3) {       // D N: the sites inside are no base of this read
      r += len;
      j = lower(S.pos, j, hi, r);
    }
  }
  return cnt;
}

}  // namespace ganon_ks

#endif  // GANON_KNOWN_SITES_H
