// ganon_bam.hip — BAM records to column arrays on MI355X (gfx950), part of libganon_hip.so; C ABI in
// include/ganon.h (ganon_bam_columns). SURVEY §8(f)4, its second half: the record walk after the
// inflate, which libganon_host.so does on the host (records_to_columns, csrc/ganon_host.cpp; the
// column view ganon_bam_view of include/ganon_host.h) and the reference gets from htslib's bam_read1
// behind AlignmentFile.fetch / pileup (pileup_io.pyx:12-17). The input is the inflated stream in
// device memory — k_inflate's output where the inflate ran on the device (ganon_inflate_device_output)
// — so the decoded records never cross PCIe.
//
// Record boundaries. Record k + 1 starts 4 + block_size(k) bytes after record k: a chain that one
// thread would walk at one dependent load per record. The stream [p, n) is cut into kChunk-byte
// chunks; chunk c holds the records that start in [p + c kChunk, p + (c + 1) kChunk). A wave per
// chunk guesses the chunk's first record start (the first offset from which kProbe chained records
// look like BAM records: sizes, reference ids, name terminator, read length against the block size)
// and one lane walks the chain to the chunk's end: its record count and exit (the first start at or past the
// chunk's end). The guesses are then proven: chunk 0 starts at p, and a chunk whose guess equals its
// predecessor's exit holds exactly the true records when its predecessor does — so by induction every
// chunk before the first failing one is exact. A failing chunk whose predecessor passed is walked
// again from that predecessor's exit, and the host repeats check and fix until no chunk fails (each
// round fixes at least the first failing run of chunks; `fixes` counts the failing chunks met).
// The exact walk checks what the host decoder checks (block_size >= 32, the record inside the
// stream), the per-record pass the rest (read length and CIGAR inside the block): same errors.
//
// Columns. Per-record sizes (name bytes kept with a NUL, CIGAR ops, packed sequence bytes, quality
// bytes, aux bytes), five exclusive scans (rocPRIM) for the blob offsets, then a wave per record:
// lanes 0-35 load the record's size and fixed fields once (broadcast by readlane), lane 0 writes the
// scalar columns, the wave copies name / CIGAR / sequence / quality / aux bytes lane-strided and sums
// the reference length of its CIGAR ops for bam_endpos. Bytes are copied as bytes: BAM fields are
// not aligned in the stream.
//
// Hashed names (--hash_read_names, ganon_ctx_set_name_key). With a key on the context every name takes
// 33 bytes (32 hex characters of its keyed BLAKE2s-128, ganon_name_hash.h, and a NUL), the scatter
// copies no name bytes, and k_bam_name_hash, a thread per record, reads each name from the stream and
// writes the name blob: a workgroup's 256 names are one contiguous 8,448-byte range, built in LDS and
// stored as coalesced dwords. Without a key nothing of this runs: the sizes and scatter kernels are
// the instantiations they were.
//
// Known sites (--known_sites, ganon_ctx_set_known_sites). With a panel table on the context
// k_bam_known_mask runs after the scatter over the columns in device memory: a base aligned to a listed
// position that shows a listed ALT becomes the reference base (ganon_known_sites.h, the host decoder's
// rule). A thread per record — almost all leave after one lower bound —, a wave per record with more
// than 48 CIGAR ops. Without a table nothing of this runs.
//
// SA clips (--mask_sa_clips, ganon_ctx_set_sa_clips). With the header's names on the context as well
// k_bam_sa_clips runs right after k_bam_known_mask: the soft-clipped bases of a record with an SA:Z tag
// are masked along the alignments the tag names (ganon_sa_clips.h, the host decoder's rule). A thread
// per record — almost all leave after their first and last CIGAR word —, the candidates compacted
// through LDS and taken a thread each. Without the names nothing of this runs.
//
// Site discovery (--discover_sites, ganon_ctx_set_site_tally). With a device tally on the context
// k_bam_site_tally runs after the scatter over the columns in device memory: the alleles the records of
// one reference sequence show against the reference are OR-ed into a byte per position
// (ganon_site_tally.h, the host decoder's rule). k_site_compact turns the bytes into the (pos, code)
// list of the positions both datasets show one allele at. Without a tally nothing of this runs.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/ganon.h"
#include "../../include/ganon_host.h"
#include "ganon_ctx.h"

using ganon_detail::check_launch;
using ganon_detail::fail;

namespace {

constexpr int kBamThreads = 256;
constexpr int64_t kChunk = 2048;     // stream bytes per chunk (~6 short-read records)
constexpr int kProbe = 2;            // chained plausible records that make a guess (4: 0.23 vs 0.18 ms per 254 MB,
                                     // 506 vs 610 wrong guesses: each one costs a re-walk of a chunk, not a result)
constexpr int64_t kGuessSpan = 2 * kChunk;   // guess search window from the chunk start

__device__ __forceinline__ uint32_t rd32(const uint8_t *__restrict__ d, int64_t o) {
  return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24);
}

// 32 bits at any byte offset o of the stream [0, n) from the two aligned dwords that hold them
// (alignbyte): half the load instructions of four byte loads — the guess and the walk are bound
// by the texture path's per-instruction cost, not by bytes. Bytes near the stream's end, where the
// second dword would pass it, are read one by one.
__device__ __forceinline__ uint32_t ld32(const uint8_t *__restrict__ d, int64_t o, int64_t n) {
  const int64_t a = o & ~(int64_t)3;
  if (a + 8 > n) return rd32(d, o);
  const uint32_t *w = reinterpret_cast<const uint32_t *>(d + a);
  return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(o & 3));
}

// Does a BAM record plausibly start at o? (guesses only: a wrong guess is caught by the check)
__device__ __forceinline__ bool plausible(const uint8_t *__restrict__ d, int64_t o, int64_t n, int64_t &next) {
  if (o + 40 > n) {   // (the stream's last bytes: byte loads)
    if (o + 36 > n) return false;
  }
  uint32_t h[9];   // block_size and the fixed fields, [o, o + 36)
  if (o + 40 <= n) {
    const int64_t a = o & ~(int64_t)3;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(d + a);
    uint32_t x[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) x[k] = w[k];
    const uint32_t sh = (uint32_t)(o & 3);
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], sh);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = rd32(d, o + 4 * k);
  }
  const int32_t bs = (int32_t)h[0];
  if (bs < 32 || o + 4 + (int64_t)bs > n) return false;
  const int32_t tid = (int32_t)h[1], pos = (int32_t)h[2];
  const int l_rn = (int)(h[3] & 0xFF);
  const int ncig = (int)(h[4] & 0xFFFF);
  const int32_t lseq = (int32_t)h[5];
  const int32_t mtid = (int32_t)h[6], mpos = (int32_t)h[7];
  if (tid < -1 || pos < -1 || mtid < -1 || mpos < -1 || l_rn < 1 || lseq < 0) return false;
  if (32 + (int64_t)l_rn + 4LL * ncig + ((int64_t)lseq + 1) / 2 + lseq > bs) return false;
  if (d[o + 4 + 32 + l_rn - 1] != 0) return false;
  next = o + 4 + bs;
  return true;
}

__device__ __forceinline__ bool chain_plausible(const uint8_t *__restrict__ d, int64_t o, int64_t n) {
  for (int k = 0; k < kProbe && o < n; ++k) {
    int64_t next;
    if (!plausible(d, o, n, next)) return false;
    o = next;
  }
  return true;
}

struct Chunks {
  int64_t *entry, *exitp, *cnt;
  int32_t *bad;     // 1: truncated size field, 2: bad block_size (the walk stopped there)
  uint8_t *flag;    // the chunk's entry is not its predecessor's exit
  unsigned long long *info;   // [failing chunks, first failing chunk, first bad chunk, first cut record]
  int64_t *tailp;   // (cut mode) the start of the record the stream's end cuts, -1 none
  bool cut;         // cut mode: the stream may end inside a record (a window of a region read); that
                    // record and the bytes after it are not records — the chain ends at its start
};

// Walk chunk c's chain from e (a record start, or < 0 for none): count and exit.
__device__ __forceinline__ void walk(const uint8_t *__restrict__ d, int64_t p, int64_t n, int64_t c, int64_t e,
                                     const Chunks &K) {
  const int64_t ce = min(n, p + (c + 1) * kChunk);
  int64_t s = e, k = 0, t = -1;
  int b = 0;
  if (s >= 0) {
    while (s < ce) {
      if (s + 4 > n) {
        if (K.cut) {   // (the chain ends here: every later chunk holds no record, entry = exit = n)
          t = s;
          s = n;
          break;
        }
        b = 1;
        break;
      }
      const int32_t bs = (int32_t)ld32(d, s, n);
      if (bs >= 32 && s + 4 + (int64_t)bs > n && K.cut) {
        t = s;
        s = n;
        break;
      }
      if (bs < 32 || s + 4 + (int64_t)bs > n) {
        b = 2;
        break;
      }
      s += 4 + (int64_t)bs;
      ++k;
    }
  }
  if (K.cut) K.tailp[c] = t;
  K.entry[c] = e;
  K.exitp[c] = b ? -2 : (e >= 0 ? s : -1);
  K.cnt[c] = k;
  K.bad[c] = b;
}

// Every chunk's guess and walk, a wave per chunk: the lanes test 64 consecutive candidate offsets at
// once (their first loads coalesced: a thread per chunk testing one offset after another made the
// byte loads of 64 lanes touch 64 cache lines apiece, 2.5 ms per 254 MB), the first plausible one
// (ballot) is the guess, and lane 0 walks the chain.
__global__ void __launch_bounds__(kBamThreads) k_bam_guess(const uint8_t *__restrict__ d, int64_t p, int64_t n,
                                                           int64_t n_chunks, Chunks K) {
  const int lane = threadIdx.x & 63;
  const int64_t c = ((int64_t)blockIdx.x * kBamThreads + threadIdx.x) >> 6;
  if (c >= n_chunks) return;   // (wave-uniform)
  int64_t e = -1;
  if (c == 0) {
    e = p;
  } else {
    const int64_t cs = p + c * kChunk, lim = min(n, cs + kGuessSpan);
    for (int64_t o0 = cs; o0 < lim; o0 += 64) {
      const int64_t o = o0 + lane;
      const unsigned long long m = __ballot(o < lim && chain_plausible(d, o, n));
      if (m) {
        e = o0 + __builtin_ctzll(m);
        break;
      }
    }
    if (e < 0 && lim == n) e = n;   // (no record starts in the rest of the stream: a guess too)
  }
  if (lane == 0) walk(d, p, n, c, e, K);
}

// A run of failing chunks whose predecessor passed, walked again from the predecessor's exit chunk
// after chunk by one thread (a long read's record covers several chunks that found no start: one
// round for the run).
__global__ void __launch_bounds__(kBamThreads) k_bam_fix(const uint8_t *__restrict__ d, int64_t p, int64_t n,
                                                         int64_t n_chunks, Chunks K) {
  const int64_t c = (int64_t)blockIdx.x * kBamThreads + threadIdx.x;
  if (c >= n_chunks || c == 0 || !K.flag[c] || K.flag[c - 1]) return;
  for (int64_t cc = c; cc < n_chunks && (cc == c || K.flag[cc]); ++cc) walk(d, p, n, cc, K.exitp[cc - 1], K);
}

__global__ void __launch_bounds__(kBamThreads) k_bam_check(int64_t n_chunks, Chunks K) {
  const int64_t c = (int64_t)blockIdx.x * kBamThreads + threadIdx.x;
  if (c >= n_chunks) return;
  const int64_t e = K.entry[c];
  const bool f = c > 0 && (e < 0 || e != K.exitp[c - 1]);
  K.flag[c] = f ? 1 : 0;
  if (f) {
    __hip_atomic_fetch_add(K.info, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(K.info + 1, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (K.bad[c]) __hip_atomic_fetch_min(K.info + 2, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // (read once no chunk fails: then every chunk is exact and at most one ends the chain at a cut)
  if (K.cut && K.tailp[c] >= 0)
    __hip_atomic_fetch_min(K.info + 3, (unsigned long long)K.tailp[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The record offsets: each chunk's chain again, from its proven entry, at its records' base index.
__global__ void __launch_bounds__(kBamThreads) k_bam_offsets(const uint8_t *__restrict__ d, int64_t p, int64_t n,
                                                             int64_t n_chunks, const int64_t *__restrict__ entry,
                                                             const int64_t *__restrict__ base,
                                                             int64_t *__restrict__ rec) {
  const int64_t c = (int64_t)blockIdx.x * kBamThreads + threadIdx.x;
  if (c >= n_chunks) return;
  const int64_t ce = min(n, p + (c + 1) * kChunk);
  int64_t s = entry[c], i = base[c];
  if (s < 0) return;
  while (s < ce) {
    if (s + 4 > n) break;   // (cut mode: the record the stream's end cuts is not one)
    const int64_t bs = (int64_t)(int32_t)ld32(d, s, n);
    if (s + 4 + bs > n) break;
    rec[i++] = s;
    s += 4 + bs;
  }
}

inline __device__ int64_t tid_order_d(int32_t t) { return t < 0 ? (int64_t)INT32_MAX : (int64_t)t; }

// A region read's records (ganon_bam_reader_region's scan_region, csrc/ganon_host.cpp): the window's
// records run from the region's first candidate; the region ends at the first record of another
// sequence or at pos >= end (info[0] = its index; info[1] = the same when that record's sequence
// comes before the region's: the index pointed before its sequence); a record before it is kept when
// bam_endpos > beg (htslib's overlap test). info[2] = the first record of the region's sequence with
// pos < end whose fields pass its block (the host walk's predicate, record_fields_fit: name, CIGAR,
// sequence and qualities; its CIGAR is not read here). The host walk reports it when it comes before
// the region's end, kept or not; a later one it never meets.
__global__ void __launch_bounds__(kBamThreads) k_region_keep(const uint8_t *__restrict__ d, int64_t n,
                                                             const int64_t *__restrict__ rec, int64_t nr, int32_t tid,
                                                             int64_t beg, int64_t end, uint8_t *__restrict__ keep,
                                                             unsigned long long *__restrict__ info) {
  const int64_t i = (int64_t)blockIdx.x * kBamThreads + threadIdx.x;
  if (i >= nr) return;
  const int64_t o = rec[i];
  const int32_t bs = (int32_t)rd32(d, o), rtid = (int32_t)rd32(d, o + 4), rpos = (int32_t)rd32(d, o + 8);
  if (rtid != tid || (int64_t)rpos >= end) {
    keep[i] = 0;
    __hip_atomic_fetch_min(info, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid_order_d(rtid) < tid_order_d(tid))
      __hip_atomic_fetch_min(info + 1, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int l_rn = d[o + 12];
  const int nc = (int)(d[o + 16] | (d[o + 17] << 8));
  const int flag = (int)(d[o + 18] | (d[o + 19] << 8));
  const int32_t lseq = (int32_t)rd32(d, o + 20);
  if (lseq < 0 || 32 + (int64_t)l_rn + 4LL * nc + ((int64_t)lseq + 1) / 2 + lseq > (int64_t)bs) {
    keep[i] = 1;
    __hip_atomic_fetch_min(info + 2, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  int64_t rl = 0;
  if (!(flag & 4))
    for (int k = 0; k < nc; ++k) {
      const uint32_t w = rd32(d, o + 36 + l_rn + 4LL * k);
      const int op = (int)(w & 0xF);
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += w >> 4;
    }
  keep[i] = (int64_t)rpos + (rl > 0 ? rl : 1) > beg ? 1 : 0;
}

struct Sizes {
  int64_t *name, *cig, *seq, *qual, *aux;   // [nr + 1] each (the last entry 0: the scan's total)
};

// Per record: the blob bytes it takes (records_to_columns' first pass), or the first bad record.
// Hashed: every name takes ganon_nh::kSlot bytes.
template <bool Hashed>
__global__ void __launch_bounds__(kBamThreads) k_bam_sizes(const uint8_t *__restrict__ d, const int64_t *__restrict__ rec,
                                                           int64_t nr, Sizes S, unsigned long long *__restrict__ first_bad) {
  const int64_t i = (int64_t)blockIdx.x * kBamThreads + threadIdx.x;
  if (i >= nr) return;
  const int64_t o = rec[i];
  const int32_t bs = (int32_t)rd32(d, o);
  const uint8_t *r = d + o + 4;
  const int l_rn = r[8];
  const int ncig = (int)(r[12] | (r[13] << 8));
  const int32_t lseq = (int32_t)rd32(r, 16);
  const int64_t need = 32 + (int64_t)l_rn + 4LL * ncig + ((int64_t)lseq + 1) / 2 + lseq;
  if (lseq < 0 || need > bs) {
    __hip_atomic_fetch_min(first_bad, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S.name[i] = S.cig[i] = S.seq[i] = S.qual[i] = S.aux[i] = 0;
    return;
  }
  S.name[i] = Hashed ? ganon_nh::kSlot : l_rn + ((l_rn == 0 || r[32 + l_rn - 1] != 0) ? 1 : 0);
  S.cig[i] = ncig;
  S.seq[i] = ((int64_t)lseq + 1) / 2;
  S.qual[i] = lseq;
  S.aux[i] = bs - need;
}

}  // namespace

struct ganon_bam_dcols {
  ganon_bam_cols v{};          // device pointers
  void *block = nullptr;        // one block for the per-record columns
  void *blobs = nullptr;        // one block for the blobs
  uint8_t *stream = nullptr;    // the device copy of a host stream (on_host)
  size_t block_bytes = 0, blobs_bytes = 0, stream_bytes = 0;   // (context cache blocks)
  int64_t blobs_used = 0;       // bytes of the blob block the carve uses
  int64_t fixes = 0;            // failing chunks met by the checks (summed over the rounds)
};

// A device site tally (include/ganon.h): one reference sequence's nt16 bases and a byte per position,
// both padded with zeros to whole compaction tiles, and after ganon_dtally_compact the site list.
struct ganon_dtally {
  int64_t len = 0, padded = 0;   // bases; bases rounded up to a multiple of kSiteTile
  uint8_t *ref = nullptr;        // padded / 2 bytes
  uint32_t *words = nullptr;     // padded bytes
  int32_t *pos = nullptr;        // (after the compaction) n_sites positions and codes
  uint8_t *code = nullptr;
  int64_t n_sites = -1;
  ganon_st::Rule rule;           // ganon_dtally_create_ex: the evidence filters and the mode (zero: none)
};

namespace {

// Record i's columns and blob bytes, by one wave; src(k) = byte k of the record (its block_size
// field first), from global memory or from the block's LDS copy.
// Hashed: the name bytes are k_bam_name_hash's (none copied here), name_len = 32.
template <bool Hashed, class Src>
__device__ __forceinline__ void scatter_record(const ganon_bam_cols &V, int64_t i, int lane, Src src) {
  uint8_t *cig8 = reinterpret_cast<uint8_t *>(V.cigar);
  const int hb = lane < 36 ? (int)src(lane) : 0;   // block_size + the fixed fields
  auto b = [&](int k) { return (uint32_t)__builtin_amdgcn_readlane(hb, k) & 0xFFu; };
  auto w32 = [&](int k) { return b(k) | (b(k + 1) << 8) | (b(k + 2) << 16) | (b(k + 3) << 24); };
  const int32_t bs = (int32_t)w32(0);
  const int l_rn = (int)b(12);
  const int ncig = (int)(b(16) | (b(17) << 8));
  const int flag = (int)(b(18) | (b(19) << 8));
  const int32_t lseq = (int32_t)w32(20);
  const int32_t pos = (int32_t)w32(8);
  const int64_t o_name = V.name_off[i], o_cig = V.cig_off[i], o_seq = V.seq_off[i], o_qual = V.qual_off[i],
                o_aux = V.aux_off[i];
  const int nseq = (int)(((int64_t)lseq + 1) / 2);
  const int e_name = l_rn, e_cig = e_name + 4 * ncig, e_seq = e_cig + nseq, e_qual = e_seq + lseq;
  const int body = bs - 32, na = body - e_qual;   // name .. aux: one byte stream, five blobs
  // each blob's destination less its first body index (wave-uniform): a byte's destination is
  // base[segment] + its body index
  uint8_t *const d_name = reinterpret_cast<uint8_t *>(V.names) + o_name, *const d_cig = cig8 + 4 * o_cig - e_name,
                 *const d_seq = V.seq + o_seq - e_cig, *const d_qual = V.qual + o_qual - e_seq,
                 *const d_aux = V.aux + o_aux - e_qual;
  // the body bytes, four loads in flight per lane before their stores
  for (int k0 = 0; k0 < body; k0 += 4 * 64) {
    uint8_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 64 * u + lane;
      v[u] = k < body ? src(36 + k) : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 64 * u + lane;
      if (k < body && !(Hashed && k < e_name)) {
        uint8_t *base = k < e_name ? d_name : k < e_cig ? d_cig : k < e_seq ? d_seq : k < e_qual ? d_qual : d_aux;
        base[k] = v[u];
      }
    }
  }
  if (!Hashed && lane == 0 && V.name_off[i + 1] - o_name > l_rn) V.names[o_name + l_rn] = 0;   // (a name without its NUL)
  // the reference length of the M / D / N / = / X ops (bam_endpos)
  unsigned long long rl = 0;
  for (int k = lane; k < ncig; k += 64) {
    const int64_t q = 36 + e_name + 4LL * k;
    const uint32_t w = (uint32_t)src(q) | ((uint32_t)src(q + 1) << 8) | ((uint32_t)src(q + 2) << 16) | ((uint32_t)src(q + 3) << 24);
    const int op = (int)(w & 0xF);
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += w >> 4;
  }
  for (int s = 32; s > 0; s >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)rl, s), hi = (uint32_t)__shfl_xor((int)(uint32_t)(rl >> 32), s);
    rl += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 0) {
    const int64_t rlen = (flag & 4) ? 0 : (int64_t)rl;
    V.tid[i] = (int32_t)w32(4);
    V.pos[i] = pos;
    V.end[i] = (int32_t)(pos + (rlen > 0 ? rlen : 1));
    V.flag[i] = flag;
    V.mapq[i] = (int)b(13);
    V.l_seq[i] = lseq;
    V.n_cigar[i] = ncig;
    V.mate_tid[i] = (int32_t)w32(24);
    V.mate_pos[i] = (int32_t)w32(28);
    V.tlen[i] = (int32_t)w32(32);
    V.name_len[i] = Hashed ? ganon_nh::kHexLen : (l_rn > 0 ? l_rn - 1 : 0);
    V.aux_len[i] = (int32_t)na;
  }
}

#ifndef GANON_SCAT_RECS
#define GANON_SCAT_RECS 32         // (profiles/r06/bam_sr: 8 0.643, 16 0.615, 32 0.598, 64 0.836 ms)
#endif
#ifndef GANON_SCAT_STAGE
#define GANON_SCAT_STAGE 16384
#endif
constexpr int kScatRecs = GANON_SCAT_RECS;    // records per workgroup (eight per wave)
constexpr int kStage = GANON_SCAT_STAGE;      // LDS bytes staged per workgroup

// A wave per record. The workgroup's run of kScatRecs records (back to back in the stream) is first
// copied to LDS with coalesced aligned dword loads, then each wave reads its record's bytes from
// there (a byte per lane per instruction from global memory, BAM fields being unaligned, cost the
// texture path as much as the stores); a run longer than the LDS copy reads global memory.
template <bool Hashed>
__global__ void __launch_bounds__(kBamThreads) k_bam_scatter(const uint8_t *__restrict__ d, int64_t n,
                                                             const int64_t *__restrict__ rec, int64_t nr,
                                                             ganon_bam_cols V) {
  __shared__ uint32_t stage[kStage / 4];
  const int64_t i0 = (int64_t)blockIdx.x * kScatRecs;
  if (i0 >= nr) return;
  const int64_t i1 = min(nr, i0 + kScatRecs);
  const int64_t s0 = rec[i0], s1 = i1 < nr ? rec[i1] : n;   // (records lie back to back up to n)
  const int64_t a0 = s0 & ~(int64_t)3;
  const bool fits = s1 - a0 <= kStage;
  if (fits) {
    const int nw = (int)((s1 - a0 + 3) >> 2);
    for (int w = threadIdx.x; w < nw; w += kBamThreads) {
      const int64_t a = a0 + 4LL * w;
      uint32_t v;
      if (a + 4 <= n) {
        v = *reinterpret_cast<const uint32_t *>(d + a);
      } else {
        v = 0;
        for (int k = 0; k < 4; ++k)
          if (a + k < n) v |= (uint32_t)d[a + k] << (8 * k);
      }
      stage[w] = v;
    }
  }
  __syncthreads();
  const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage);
  const int lane = threadIdx.x & 63;
  for (int64_t i = i0 + (threadIdx.x >> 6); i < i1; i += kBamThreads / 64) {
    const int64_t o = rec[i];
    if (fits) {
      const int base = (int)(o - a0);
      scatter_record<Hashed>(V, i, lane, [&](int64_t k) { return sb[base + k]; });
    } else {
      scatter_record<Hashed>(V, i, lane, [&](int64_t k) { return d[o + k]; });
    }
  }
}

// The name blob of hashed names, a thread per record: record i's name (the bytes the unhashed columns
// report: l_read_name - 1 of them from byte 36 of the record, its fields checked by k_bam_sizes) to
// 32 hex characters and a NUL at names[33 i]. The workgroup's kBamThreads slots are contiguous and
// start at a multiple of 4 bytes (33 * 256 i0; the blob is 256-byte aligned): they are built in LDS
// and stored as dwords, the last workgroup's odd tail as bytes.
__global__ void __launch_bounds__(kBamThreads) k_bam_name_hash(const uint8_t *__restrict__ d, int64_t n,
                                                               const int64_t *__restrict__ rec, int64_t nr,
                                                               ganon_nh::KeyState ks, char *__restrict__ names) {
  __shared__ uint32_t slots[kBamThreads * ganon_nh::kSlot / 4];
  uint8_t *sb = reinterpret_cast<uint8_t *>(slots);
  const int64_t i0 = (int64_t)blockIdx.x * kBamThreads;
  const int64_t i = i0 + threadIdx.x;
  if (i < nr) {
    const int64_t o = rec[i];
    const int l_rn = d[o + 12];
    const uint8_t *nm = d + o + 36;
    const int64_t left = n - (o + 36);   // stream bytes from the name's first on (>= l_rn)
    uint8_t *slot = sb + ganon_nh::kSlot * threadIdx.x;
    ganon_nh::hash_name(
        ks, l_rn > 0 ? l_rn - 1 : 0,
        [&](int k, int nb) {
          // the two aligned dwords that hold name bytes k .. k + 3 when the stream has them, else bytes
          const uintptr_t a = reinterpret_cast<uintptr_t>(nm + k);
          const int64_t pre = (int64_t)(a & 3);
          if (nb == 4 && k + 8 - pre <= left) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(a - pre);
            return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)pre);
          }
          uint32_t v = 0;
          for (int c = 0; c < nb; ++c) v |= (uint32_t)nm[k + c] << (8 * c);
          return v;
        },
        [&](int k, uint32_t w) {
          slot[4 * k] = (uint8_t)w;
          slot[4 * k + 1] = (uint8_t)(w >> 8);
          slot[4 * k + 2] = (uint8_t)(w >> 16);
          slot[4 * k + 3] = (uint8_t)(w >> 24);
        });
    slot[ganon_nh::kHexLen] = 0;
  }
  __syncthreads();
  const int cnt = (int)min((int64_t)kBamThreads, nr - i0);
  const int bytes = cnt * ganon_nh::kSlot;
  char *out = names + ganon_nh::kSlot * i0;
  uint32_t *out4 = reinterpret_cast<uint32_t *>(out);
  for (int w = threadIdx.x; w < bytes / 4; w += kBamThreads) out4[w] = slots[w];
  if ((int)threadIdx.x < (bytes & 3)) out[(bytes & ~3) + threadIdx.x] = (char)sb[(bytes & ~3) + threadIdx.x];
}

constexpr int kKsLongOps = 48;   // records with more CIGAR ops take a wave each (the scan's threshold)

// Inclusive prefix sum over the wave of values below 2^28 (CIGAR op lengths) without overflow: the low
// and the high 14 bits summed apart (64 x 2^14 fits an int), wave total in `total`.
__device__ __forceinline__ int64_t ks_incl_sum(uint32_t v, int64_t &total) {
  const int lo = ganon_wave::incl_sum((int)(v & 0x3FFFu)), hi = ganon_wave::incl_sum((int)(v >> 14));
  total = (int64_t)ganon_wave::last(lo) + ((int64_t)ganon_wave::last(hi) << 14);
  return (int64_t)lo + ((int64_t)hi << 14);
}

// One record with a long CIGAR, by one wave (every lane active): 64 ops at a time, their reference and
// query starts from prefix sums; a lane with an M / = / X op searches the sites inside its op's
// reference range and patches them. Two lanes can own the two nibbles of one byte (an op boundary at
// an odd query index), so a nibble is rewritten by a 32-bit atomic xor of (base ^ ref) on the aligned
// word that holds it (the blobs are 256-byte aligned and padded): no lane writes a bit it does not own.
__device__ __forceinline__ int ks_mask_wave(const ganon_ks::View &S, int lane, int32_t tid, int32_t pos, int32_t ncig,
                                            int32_t lseq, const uint32_t *__restrict__ cig, uint8_t *seq, uint8_t *qual) {
  const int64_t lo = S.off[tid], hi = S.off[tid + 1];
  if (ganon_ks::lower(S.pos, lo, hi, pos) >= hi) return 0;   // (wave-uniform)
  const bool q_on = S.qual >= 0 && qual[0] != 0xFF;
  int64_t r = pos, q = 0;
  int cnt = 0;
  for (int k0 = 0; k0 < ncig && q < lseq; k0 += 64) {
    const uint32_t w = k0 + lane < ncig ? cig[k0 + lane] : 0u;
    const int op = (int)(w & 15u);
    const uint32_t len = w >> 4;
    const bool m = op == 0 || op == 7 || op == 8;
    const uint32_t rl = (m || op == 2 || op == 3) ? len : 0u, ql = (m || op == 1 || op == 4) ? len : 0u;
    int64_t rt, qt;
    const int64_t r0 = r + ks_incl_sum(rl, rt) - rl, q0 = q + ks_incl_sum(ql, qt) - ql;
    if (m && len && q0 < lseq) {
      const int64_t rend = r0 + len;
      for (int64_t j = ganon_ks::lower(S.pos, lo, hi, r0); j < hi; ++j) {
        const int64_t p = S.pos[j];
        if (p >= rend) break;
        const int64_t x = q0 + (p - r0);
        if (x >= lseq) break;
        const uint8_t code = S.code[j];
        const int sh = (x & 1) ? 0 : 4;
        const int b = (seq[x >> 1] >> sh) & 15;
        if (ganon_ks::hits(b, code)) {
          const uintptr_t a = reinterpret_cast<uintptr_t>(seq + (x >> 1));
          __hip_atomic_fetch_xor(reinterpret_cast<uint32_t *>(a & ~(uintptr_t)3),
                                 (uint32_t)(b ^ (code >> 4)) << (8 * (int)(a & 3) + sh), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
          if (q_on) qual[x] = (uint8_t)S.qual;
          ++cnt;
        }
      }
    }
    r += rt;
    q += qt;
  }
  return cnt;
}

// The panel mask of --known_sites over the decoded columns (ganon_known_sites.h has the rule). A thread
// per record: its columns, then a lower bound of pos in its sequence's sites; no site before `end`
// (almost every short read at panel densities) and it is done, else it merge-walks its CIGAR and the
// sites (ganon_ks::mask_record; its bases are whole bytes it alone owns: plain byte stores). Records
// with more than kKsLongOps ops are listed in LDS instead and taken a wave each (ks_mask_wave). One
// atomic add per workgroup that rewrote anything.
__global__ void __launch_bounds__(kBamThreads) k_bam_known_mask(ganon_bam_cols V, int64_t nr, ganon_ks::View S,
                                                                unsigned long long *__restrict__ count) {
  __shared__ int s_long[kBamThreads];
  __shared__ int s_nlong, s_cnt;
  if (threadIdx.x == 0) s_nlong = s_cnt = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kBamThreads;
  const int64_t i = i0 + threadIdx.x;
  int cnt = 0;
  if (i < nr) {
    const int32_t tid = V.tid[i], pos = V.pos[i], end = V.end[i], flag = V.flag[i], ncig = V.n_cigar[i], lseq = V.l_seq[i];
    const int64_t o_cig = V.cig_off[i], o_seq = V.seq_off[i], o_qual = V.qual_off[i];
    if (!ganon_ks::skips(S, tid, (uint32_t)flag, ncig, lseq)) {
      const int64_t hi = S.off[tid + 1];
      const int64_t j = ganon_ks::lower(S.pos, S.off[tid], hi, pos);
      if (j < hi && S.pos[j] < end) {
        if (ncig > kKsLongOps)
          s_long[atomicAdd(&s_nlong, 1)] = (int)threadIdx.x;
        else
          cnt = ganon_ks::mask_record(S, tid, pos, (uint32_t)flag, ncig, lseq, V.cigar + o_cig, V.seq + o_seq, V.qual + o_qual);
      }
    }
  }
  __syncthreads();
  const int nlong = s_nlong, lane = threadIdx.x & 63;
  for (int k = threadIdx.x >> 6; k < nlong; k += kBamThreads / 64) {   // (wave-uniform)
    const int64_t g = i0 + s_long[k];
    const int c = ks_mask_wave(S, lane, V.tid[g], V.pos[g], V.n_cigar[g], V.l_seq[g], V.cigar + V.cig_off[g],
                               V.seq + V.seq_off[g], V.qual + V.qual_off[g]);
    cnt += c;
  }
  if (__any(cnt != 0)) {
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    if (lane == 0) atomicAdd(&s_cnt, cnt);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(count, (unsigned long long)s_cnt);
}

// The SA clip mask of --mask_sa_clips over the decoded columns, after k_bam_known_mask in stream order
// (ganon_sa_clips.h has the rule; a byte that holds an aligned and a clipped nibble is written by the
// one kernel, then by the other). A thread per record loads flag, n_cigar, cig_off and its first and
// last CIGAR word (24 bytes) and leaves unless one of them is S or H: nearly every record. The rest
// settle their clips (ganon_sa::own_clip) and scan their aux bytes for the SA:Z value; those that have
// one are listed in LDS with the value's bounds and, after the barrier, taken by the block's first
// threads, a thread per candidate: the tag is tens of bytes of decimal text that only a serial parse
// reads, and an M run holds a few sites at most, so a wave per candidate would idle 63 lanes, while
// the compaction packs a block's few candidates into one wave instead of leaving each to diverge in
// its own. One thread owns a record, whose bases are whole bytes of its own: plain byte stores. Counts:
// a shuffle sum and one LDS add per wave, one global add per count per workgroup that has any.
__global__ void __launch_bounds__(kBamThreads) k_bam_sa_clips(ganon_bam_cols V, int64_t nr, ganon_ks::View S,
                                                              ganon_sa::Names N, unsigned long long *__restrict__ count) {
  __shared__ int s_cand[kBamThreads], s_v0[kBamThreads], s_v1[kBamThreads];
  __shared__ int s_ncand, s_cnt, s_ign;
  if (threadIdx.x == 0) s_ncand = s_cnt = s_ign = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kBamThreads;
  const int64_t i = i0 + threadIdx.x;
  if (i < nr) {
    const int32_t flag = V.flag[i], ncig = V.n_cigar[i];
    if (!(flag & 4) && ncig > 0) {
      const uint32_t *cg = V.cigar + V.cig_off[i];
      const uint32_t o0 = cg[0] & 15u, o1 = cg[ncig - 1] & 15u;
      if (o0 == 4u || o0 == 5u || o1 == 4u || o1 == 5u) {
        const int32_t tid = V.tid[i], lseq = V.l_seq[i], alen = V.aux_len[i];
        ganon_sa::Clip c;
        int64_t v0, v1;
        if (!ganon_ks::skips(S, tid, (uint32_t)flag, ncig, lseq) && alen > 3 && ganon_sa::own_clip(ncig, lseq, cg, &c) &&
            ganon_sa::find_sa(V.aux + V.aux_off[i], alen, &v0, &v1)) {
          const int k = atomicAdd(&s_ncand, 1);
          s_cand[k] = (int)threadIdx.x;
          s_v0[k] = (int)v0;
          s_v1[k] = (int)v1;
        }
      }
    }
  }
  __syncthreads();
  const int ncand = s_ncand, lane = threadIdx.x & 63;
  int cnt = 0, ign = 0;
  if ((int)threadIdx.x < ncand) {
    const int64_t g = i0 + s_cand[threadIdx.x];
    const int32_t ncig = V.n_cigar[g], lseq = V.l_seq[g];
    const uint32_t *cg = V.cigar + V.cig_off[g];
    ganon_sa::Clip c;
    ganon_sa::own_clip(ncig, lseq, cg, &c);
    cnt = ganon_sa::mask_tag(S, N, c, (uint32_t)V.flag[g], lseq, V.seq + V.seq_off[g], V.qual + V.qual_off[g],
                             V.aux + V.aux_off[g], s_v0[threadIdx.x], s_v1[threadIdx.x], &ign);
  }
  if (__any(cnt != 0 || ign != 0)) {
    for (int s = 32; s > 0; s >>= 1) {
      cnt += __shfl_xor(cnt, s);
      ign += __shfl_xor(ign, s);
    }
    if (lane == 0) {
      if (cnt) atomicAdd(&s_cnt, cnt);
      if (ign) atomicAdd(&s_ign, ign);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_cnt) atomicAdd(count, (unsigned long long)s_cnt);
    if (s_ign) atomicAdd(count + 1, (unsigned long long)s_ign);
  }
}

// ---- --discover_sites: the evidence tally and its compaction ---------------------------------------------

struct StView {
  const uint8_t *ref;   // the sequence's nt16 bases from nibble 0 on
  uint32_t *words;      // its tally bytes as dwords
  int64_t len;
  int32_t tid;          // the BAM sequence id whose records are evidence
  int32_t dataset;
  ganon_st::Rule rule;  // (read by the filtered instantiation alone)
};

// ganon_st's store on the device: one relaxed agent-scope atomic OR on the aligned word that holds the
// position's byte (four positions share a word, records of other workgroups write them).
struct StStore {
  uint32_t *words;
  __device__ __forceinline__ void operator()(int64_t r, uint8_t bits) {
    __hip_atomic_fetch_or(words + (r >> 2), (uint32_t)bits << (8 * (int)(r & 3)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// One record with a long CIGAR, by one wave (every lane active): 64 ops at a time, their reference and
// query starts from prefix sums (ks_incl_sum: the lengths in two 14-bit halves); a lane with an M / = /
// X op tallies its op's bases (ganon_st::tally_span clips them to the read and the sequence). Filtered:
// qual is the record's quality bytes, which each lane's q0 indexes as it does the bases.
template <bool Filtered>
__device__ __forceinline__ void st_tally_wave(const StView &T, int lane, int32_t pos, int32_t ncig, int32_t lseq,
                                              const uint32_t *__restrict__ cig, const uint8_t *__restrict__ seq,
                                              const uint8_t *__restrict__ qual) {
  const ganon_st::Ref R{T.ref, 0, T.len};
  StStore st{T.words};
  int64_t r = pos, q = 0;
  for (int k0 = 0; k0 < ncig && q < lseq && r < T.len; k0 += 64) {   // (wave-uniform)
    const uint32_t w = k0 + lane < ncig ? cig[k0 + lane] : 0u;
    const int op = (int)(w & 15u);
    const uint32_t len = w >> 4;
    const bool m = op == 0 || op == 7 || op == 8;
    const uint32_t rl = (m || op == 2 || op == 3) ? len : 0u, ql = (m || op == 1 || op == 4) ? len : 0u;
    int64_t rt, qt;
    const int64_t r0 = r + ks_incl_sum(rl, rt) - rl, q0 = q + ks_incl_sum(ql, qt) - ql;
    if (m && len)
      ganon_st::tally_span<Filtered>(R, seq, qual, Filtered ? T.rule.min_base_quality : 0, lseq, r0, q0, (int64_t)len,
                                     4 * T.dataset, st);
    r += rt;
    q += qt;
  }
}

// The tally of --discover_sites over the decoded columns (ganon_site_tally.h has the rule). A thread per
// record of sequence T.tid that the rule does not skip: it walks its CIGAR and compares eight bases a
// step, a dword of read nibbles XOR a dword of reference nibbles (ganon_st::nib8), and goes nibble by
// nibble only inside a word that differs: mismatches are about 0.1-1 % of the bases, the atomic ORs are
// rare. Records with more than kKsLongOps ops are listed in LDS and taken a wave each after the
// barrier (st_tally_wave), as k_bam_known_mask does and for the same reason: one thread on a
// thousand-op CIGAR would hold its wave. Filtered (a rule with an evidence filter; false is the kernel
// without one, which reads neither mapq nor a quality byte): a record also leaves when its mapq is below
// the rule's or its flag has an excluded bit, and a differing base counts only with its own quality byte
// at or above the rule's: a byte load per mismatch.
template <bool Filtered>
__global__ void __launch_bounds__(kBamThreads) k_bam_site_tally(ganon_bam_cols V, int64_t nr, StView T) {
  __shared__ int s_long[kBamThreads];
  __shared__ int s_nlong;
  if (threadIdx.x == 0) s_nlong = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kBamThreads;
  const int64_t i = i0 + threadIdx.x;
  if (i < nr && V.tid[i] == T.tid) {
    const int32_t flag = V.flag[i], ncig = V.n_cigar[i], lseq = V.l_seq[i];
    if (!(flag & 4) && ncig > 0 && lseq > 0 && (!Filtered || ganon_st::passes(T.rule, (uint32_t)flag, V.mapq[i]))) {
      if (ncig > kKsLongOps) {
        s_long[atomicAdd(&s_nlong, 1)] = (int)threadIdx.x;
      } else {
        const ganon_st::Ref R{T.ref, 0, T.len};
        StStore st{T.words};
        ganon_st::tally_record<Filtered>(R, V.pos[i], ncig, lseq, V.cigar + V.cig_off[i], V.seq + V.seq_off[i],
                                         Filtered ? V.qual + V.qual_off[i] : nullptr, Filtered ? T.rule.min_base_quality : 0,
                                         T.dataset, st);
      }
    }
  }
  __syncthreads();
  const int nlong = s_nlong, lane = threadIdx.x & 63;
  for (int k = threadIdx.x >> 6; k < nlong; k += kBamThreads / 64) {   // (wave-uniform)
    const int64_t g = i0 + s_long[k];
    st_tally_wave<Filtered>(T, lane, V.pos[g], V.n_cigar[g], V.l_seq[g], V.cigar + V.cig_off[g], V.seq + V.seq_off[g],
                            Filtered ? V.qual + V.qual_off[g] : nullptr);
  }
}

constexpr int kSiteTile = 8 * kBamThreads;   // positions per workgroup of k_site_compact: eight a thread

// The sites of a tally: a thread takes eight positions (two dwords of tally bytes, OR-ed with the host
// tally's where the host side touched the sequence), alt = low & high nibble per byte, or with Normal
// (the rule's mode `normal`) the high nibble alone: the low one is not consulted. Write false:
// the tile's site count to count[tile]. Write true: the sites at base[tile] (the scanned counts) plus
// the block's exclusive prefix, in position order, the reference nibble from the sequence's nt16.
template <bool Write, bool Normal>
__global__ void __launch_bounds__(kBamThreads) k_site_compact(const uint32_t *__restrict__ words,
                                                              const uint32_t *__restrict__ host_words,
                                                              const uint8_t *__restrict__ ref, int64_t *__restrict__ count,
                                                              const int64_t *__restrict__ base, int32_t *__restrict__ pos,
                                                              uint8_t *__restrict__ code) {
  __shared__ int s_wave[kBamThreads / 64];
  const int64_t p0 = (int64_t)blockIdx.x * kSiteTile + 8 * (int64_t)threadIdx.x;
  uint2 w = *reinterpret_cast<const uint2 *>(words + (p0 >> 2));
  if (host_words) {
    const uint2 h = *reinterpret_cast<const uint2 *>(host_words + (p0 >> 2));
    w.x |= h.x;
    w.y |= h.y;
  }
  const uint32_t a0 = (Normal ? ~0u : w.x) & (w.x >> 4) & 0x0F0F0F0Fu, a1 = (Normal ? ~0u : w.y) & (w.y >> 4) & 0x0F0F0F0Fu;
  int cnt = 0;
  for (int j = 0; j < 4; ++j) cnt += ((a0 >> (8 * j)) & 15u ? 1 : 0) + ((a1 >> (8 * j)) & 15u ? 1 : 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = ganon_wave::incl_sum(cnt);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int before = 0, total = 0;
  for (int k = 0; k < kBamThreads / 64; ++k) {
    if (k < wave) before += s_wave[k];
    total += s_wave[k];
  }
  if (!Write) {
    if (threadIdx.x == 0) count[blockIdx.x] = total;
    return;
  }
  if (!cnt) return;
  int64_t o = base[blockIdx.x] + before + incl - cnt;
  const uint32_t rf = __builtin_bswap32(*reinterpret_cast<const uint32_t *>(ref + (p0 >> 1)));   // base j: bits 31 - 4j ..
  for (int j = 0; j < 8; ++j) {
    const uint32_t alt = ((j < 4 ? a0 : a1) >> (8 * (j & 3))) & 15u;
    if (!alt) continue;
    pos[o] = (int32_t)(p0 + j);
    code[o] = (uint8_t)((((rf >> (28 - 4 * j)) & 15u) << 4) | alt);
    ++o;
  }
}

unsigned grid_of(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kBamThreads - 1) / kBamThreads); }

template <typename T>
T *carve(uint8_t *&at, int64_t count) {
  T *p = reinterpret_cast<T *>(at);
  at += ((count * (int64_t)sizeof(T) + 255) / 256) * 256;
  return p;
}

// A region read's request (ganon_region_decode): the records of sequence tid overlapping [beg, end)
// from the window's first record on. status out: 1 the region ends inside the window (the columns
// are its records'), 0 it goes on past the window, 2 declined — a malformed record before the region's
// end or the index pointed before the sequence: the host's walk reports those.
struct RegionReq {
  int32_t tid;
  int64_t beg, end;
  bool at_eof;   // the window ends at the end of the file
  int status;
};

int columns(ganon_ctx *ctx, const uint8_t *d, int64_t p, int64_t n, ganon_bam_dcols *H, RegionReq *rg = nullptr) {
  hipStream_t s = ctx->stream;
  const int64_t n_chunks = n > p ? (n - p + kChunk - 1) / kChunk : 0;
  int rc;
  // chunk arrays and the scans' temporary space from the context's block cache (stream-ordered
  // reuse: no hipMalloc / hipFree, which synchronize, once a call of this size has run)
  std::vector<std::pair<void *, size_t>> tmp;
  auto dalloc = [&](size_t bytes) -> void * {
    void *q = nullptr;
    size_t got = 0;
    if (ctx_dmalloc(ctx, &q, std::max<size_t>(bytes, 256), &got) != hipSuccess) return nullptr;
    tmp.emplace_back(q, got);
    return q;
  };
  struct Free {
    ganon_ctx *ctx;
    std::vector<std::pair<void *, size_t>> &t;
    ~Free() {
      for (auto &q : t) ctx_dfree(ctx, q.first, q.second);
    }
  } free_tmp{ctx, tmp};
  Chunks K{};
  int64_t *base = nullptr;
  unsigned long long tail = ~0ull;   // (cut mode) the record the window's end cuts
  if (n_chunks) {
    const int64_t nc = n_chunks;
    K.entry = static_cast<int64_t *>(dalloc(nc * 8));
    K.exitp = static_cast<int64_t *>(dalloc(nc * 8));
    K.cnt = static_cast<int64_t *>(dalloc((nc + 1) * 8));
    base = static_cast<int64_t *>(dalloc((nc + 1) * 8));
    K.bad = static_cast<int32_t *>(dalloc(nc * 4));
    K.flag = static_cast<uint8_t *>(dalloc(nc));
    K.info = static_cast<unsigned long long *>(dalloc(4 * 8));
    K.cut = rg != nullptr;
    K.tailp = rg ? static_cast<int64_t *>(dalloc(nc * 8)) : nullptr;
    if (!K.entry || !K.exitp || !K.cnt || !base || !K.bad || !K.flag || !K.info || (rg && !K.tailp))
      return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation failed");
    {
      ganon_detail::KernelScope ks(ctx, "k_bam_guess");
      hipLaunchKernelGGL(k_bam_guess, dim3(grid_of(64 * nc)), dim3(kBamThreads), 0, s, d, p, n, nc, K);
    }
    if ((rc = check_launch(ctx, "k_bam_guess"))) return rc;
    for (int64_t round = 0;; ++round) {
      const unsigned long long init[4] = {0ull, ~0ull, ~0ull, ~0ull};
      unsigned long long info[4];
      HIP_OR_FAIL(hipMemcpyAsync(K.info, init, sizeof init, hipMemcpyHostToDevice, s));
      {
        ganon_detail::KernelScope ks(ctx, "k_bam_check");
        hipLaunchKernelGGL(k_bam_check, dim3(grid_of(nc)), dim3(kBamThreads), 0, s, nc, K);
      }
      if ((rc = check_launch(ctx, "k_bam_check"))) return rc;
      HIP_OR_FAIL(ganon_detail::readback(info, K.info, sizeof info, s));
      HIP_OR_FAIL(ganon_detail::sync_stream(s));
      // every chunk before the first failing one is exact: a bad walk there is the stream's error
      if (info[2] != ~0ull && info[2] < info[1]) {
        if (rg) {
          rg->status = 2;
          return GANON_OK;
        }
        return fail(ctx, GANON_E_ARG, "ganon_bam_columns: bad record size (chunk %lld)", (long long)info[2]);
      }
      if (info[0] == 0) {
        tail = info[3];
        break;
      }
      if (round > nc) return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: record chain did not settle");
      H->fixes += (int64_t)info[0];
      {
        ganon_detail::KernelScope ks(ctx, "k_bam_fix");
        hipLaunchKernelGGL(k_bam_fix, dim3(grid_of(nc)), dim3(kBamThreads), 0, s, d, p, n, nc, K);
      }
      if ((rc = check_launch(ctx, "k_bam_fix"))) return rc;
    }
    HIP_OR_FAIL(hipMemsetAsync(K.cnt + nc, 0, 8, s));
    size_t tb = 0;
    HIP_OR_FAIL(rocprim::exclusive_scan(nullptr, tb, K.cnt, base, (int64_t)0, (size_t)(nc + 1), rocprim::plus<int64_t>(), s));
    void *tsc = dalloc(tb);
    if (!tsc) return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation failed");
    HIP_OR_FAIL(rocprim::exclusive_scan(tsc, tb, K.cnt, base, (int64_t)0, (size_t)(nc + 1), rocprim::plus<int64_t>(), s));
  }
  int64_t nr = 0;
  if (n_chunks) {
    HIP_OR_FAIL(ganon_detail::readback(&nr, base + n_chunks, 8, s));
    HIP_OR_FAIL(ganon_detail::sync_stream(s));
  }
  // A region read: the window's records up to the region's end, those overlapping [beg, end) kept
  // (a stream compaction of their offsets); the columns below are built for those alone.
  int64_t *sel = nullptr;
  if (rg) {
    if (rg->at_eof && tail != ~0ull) {   // the file ends inside a record: the host's error
      rg->status = 2;
      return GANON_OK;
    }
    int64_t *all = static_cast<int64_t *>(dalloc((size_t)(nr + 1) * 8));
    uint8_t *keep = static_cast<uint8_t *>(dalloc((size_t)nr + 1));
    unsigned long long *ri = static_cast<unsigned long long *>(dalloc(3 * 8));
    sel = static_cast<int64_t *>(dalloc((size_t)(nr + 1) * 8));
    int64_t *cnt = static_cast<int64_t *>(dalloc(8));
    if (!all || !keep || !ri || !sel || !cnt) return fail(ctx, GANON_E_DEVICE, "ganon_region_decode: device allocation failed");
    const unsigned long long init[3] = {~0ull, ~0ull, ~0ull};
    unsigned long long info[3] = {~0ull, ~0ull, ~0ull};
    HIP_OR_FAIL(hipMemcpyAsync(ri, init, sizeof init, hipMemcpyHostToDevice, s));
    if (nr) {
      {
        ganon_detail::KernelScope ks(ctx, "k_bam_offsets");
        hipLaunchKernelGGL(k_bam_offsets, dim3(grid_of(n_chunks)), dim3(kBamThreads), 0, s, d, p, n, n_chunks, K.entry,
                           base, all);
      }
      if ((rc = check_launch(ctx, "k_bam_offsets"))) return rc;
      {
        ganon_detail::KernelScope ks(ctx, "k_region_keep");
        hipLaunchKernelGGL(k_region_keep, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, d, n, all, nr, rg->tid, rg->beg,
                           rg->end, keep, ri);
      }
      if ((rc = check_launch(ctx, "k_region_keep"))) return rc;
      HIP_OR_FAIL(ganon_detail::readback(info, ri, sizeof info, s));
      HIP_OR_FAIL(ganon_detail::sync_stream(s));
    }
    // declined: a malformed record before the region's end (before nr when the region ends with the
    // window's records: one after the region's end the host walk never reads), or an index that
    // pointed before its sequence
    if ((info[2] != ~0ull && (info[0] == ~0ull || info[2] < info[0])) || (info[1] != ~0ull && info[1] == info[0])) {
      rg->status = 2;
      return GANON_OK;
    }
    if (info[0] == ~0ull && (!rg->at_eof || tail != ~0ull)) {   // the region goes on past the window
      rg->status = 0;
      return GANON_OK;
    }
    const int64_t cut = info[0] == ~0ull ? nr : (int64_t)info[0];
    int64_t nk = 0;
    if (cut > 0) {
      size_t tb = 0;
      HIP_OR_FAIL(rocprim::select(nullptr, tb, all, keep, sel, cnt, (size_t)cut, s));
      void *tsel = dalloc(tb);
      if (!tsel) return fail(ctx, GANON_E_DEVICE, "ganon_region_decode: device allocation failed");
      HIP_OR_FAIL(rocprim::select(tsel, tb, all, keep, sel, cnt, (size_t)cut, s));
      HIP_OR_FAIL(ganon_detail::readback(&nk, cnt, 8, s));
      HIP_OR_FAIL(ganon_detail::sync_stream(s));
    }
    nr = nk;
    rg->status = 1;
  }
  // per-record columns: 12 int32 + 6 int64 (5 offsets of nr + 1, the record offsets) + the sizes
  ganon_bam_cols &V = H->v;
  V.n_records = nr;
  {
    const int64_t m = nr + 1;
    const int64_t bytes = 12 * (((m * 4) + 255) / 256 * 256) + 11 * (((m * 8) + 255) / 256 * 256);
    if (ctx_dmalloc(ctx, &H->block, (size_t)std::max<int64_t>(bytes, 256), &H->block_bytes) != hipSuccess)
      return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation of %lld bytes failed", (long long)bytes);
    uint8_t *at = static_cast<uint8_t *>(H->block);
    for (int32_t **f : {&V.tid, &V.pos, &V.end, &V.flag, &V.mapq, &V.l_seq, &V.n_cigar, &V.mate_tid, &V.mate_pos, &V.tlen,
                        &V.name_len, &V.aux_len})
      *f = carve<int32_t>(at, m);
    for (int64_t **f : {&V.name_off, &V.cig_off, &V.seq_off, &V.qual_off, &V.aux_off, &V.rec_off}) *f = carve<int64_t>(at, m);
    Sizes S{carve<int64_t>(at, m), carve<int64_t>(at, m), carve<int64_t>(at, m), carve<int64_t>(at, m),
            carve<int64_t>(at, m)};
    unsigned long long *first_bad = static_cast<unsigned long long *>(dalloc(8));
    if (!first_bad) return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation failed");
    const unsigned long long none = ~0ull;
    HIP_OR_FAIL(hipMemcpyAsync(first_bad, &none, 8, hipMemcpyHostToDevice, s));
    if (sel) {
      if (nr) HIP_OR_FAIL(hipMemcpyAsync(V.rec_off, sel, (size_t)nr * 8, hipMemcpyDeviceToDevice, s));
    } else {
      if (nr) {
        ganon_detail::KernelScope ks(ctx, "k_bam_offsets");
        hipLaunchKernelGGL(k_bam_offsets, dim3(grid_of(n_chunks)), dim3(kBamThreads), 0, s, d, p, n, n_chunks, K.entry,
                           base, V.rec_off);
      }
      if ((rc = check_launch(ctx, "k_bam_offsets"))) return rc;
    }
    for (int64_t *z : {S.name, S.cig, S.seq, S.qual, S.aux}) HIP_OR_FAIL(hipMemsetAsync(z + nr, 0, 8, s));
    if (nr) {
      ganon_detail::KernelScope ks(ctx, "k_bam_sizes");
      if (ctx->name_hash)
        hipLaunchKernelGGL(k_bam_sizes<true>, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, d, V.rec_off, nr, S, first_bad);
      else
        hipLaunchKernelGGL(k_bam_sizes<false>, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, d, V.rec_off, nr, S, first_bad);
    }
    if ((rc = check_launch(ctx, "k_bam_sizes"))) return rc;
    size_t tb = 0;
    HIP_OR_FAIL(rocprim::exclusive_scan(nullptr, tb, S.name, V.name_off, (int64_t)0, (size_t)m, rocprim::plus<int64_t>(), s));
    void *tsc = dalloc(tb);
    if (!tsc) return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation failed");
    {
      ganon_detail::KernelScope ks(ctx, "bam_scans");
      const std::pair<int64_t *, int64_t *> io[5] = {{S.name, V.name_off}, {S.cig, V.cig_off}, {S.seq, V.seq_off},
                                                     {S.qual, V.qual_off}, {S.aux, V.aux_off}};
      for (const auto &x : io)
        HIP_OR_FAIL(rocprim::exclusive_scan(tsc, tb, x.first, x.second, (int64_t)0, (size_t)m, rocprim::plus<int64_t>(), s));
    }
    unsigned long long bad_rec = ~0ull;
    int64_t tot[5];
    HIP_OR_FAIL(ganon_detail::readback(&bad_rec, first_bad, 8, s));
    int64_t *offs[5] = {V.name_off, V.cig_off, V.seq_off, V.qual_off, V.aux_off};
    for (int k = 0; k < 5; ++k) HIP_OR_FAIL(ganon_detail::readback(&tot[k], offs[k] + nr, 8, s));
    HIP_OR_FAIL(ganon_detail::sync_stream(s));
    if (bad_rec != ~0ull) {
      if (rg) {
        rg->status = 2;
        return GANON_OK;
      }
      return fail(ctx, GANON_E_ARG, "ganon_bam_columns: record %lld: fields exceed block size", (long long)bad_rec);
    }
    V.names_bytes = tot[0];
    V.cigar_ops = tot[1];
    V.seq_bytes = tot[2];
    V.qual_bytes = tot[3];
    V.aux_bytes = tot[4];
  }
  {
    const int64_t rb = ((V.names_bytes + 255) / 256 + (4 * V.cigar_ops + 255) / 256 + (V.seq_bytes + 255) / 256 +
                        (V.qual_bytes + 255) / 256 + (V.aux_bytes + 255) / 256) * 256;
    if (ctx_dmalloc(ctx, &H->blobs, (size_t)std::max<int64_t>(rb, 256), &H->blobs_bytes) != hipSuccess)
      return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation of %lld bytes failed", (long long)rb);
    uint8_t *at = static_cast<uint8_t *>(H->blobs);
    V.names = carve<char>(at, V.names_bytes);
    V.cigar = carve<uint32_t>(at, V.cigar_ops);
    V.seq = carve<uint8_t>(at, V.seq_bytes);
    V.qual = carve<uint8_t>(at, V.qual_bytes);
    V.aux = carve<uint8_t>(at, V.aux_bytes);
    H->blobs_used = rb;
  }
  if (nr) {
    ganon_detail::KernelScope ks(ctx, "k_bam_scatter");
    const unsigned grid = (unsigned)((nr + kScatRecs - 1) / kScatRecs);
    if (ctx->name_hash)
      hipLaunchKernelGGL(k_bam_scatter<true>, dim3(grid), dim3(kBamThreads), 0, s, d, n, V.rec_off, nr, V);
    else
      hipLaunchKernelGGL(k_bam_scatter<false>, dim3(grid), dim3(kBamThreads), 0, s, d, n, V.rec_off, nr, V);
  }
  if ((rc = check_launch(ctx, "k_bam_scatter"))) return rc;
  if (nr && ctx->name_hash) {   // (names_bytes = 33 nr: k_bam_sizes<true>)
    {
      ganon_detail::KernelScope ks(ctx, "k_bam_name_hash");
      hipLaunchKernelGGL(k_bam_name_hash, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, d, n, V.rec_off, nr, ctx->name_key,
                         V.names);
    }
    if ((rc = check_launch(ctx, "k_bam_name_hash"))) return rc;
  }
  if (nr && ctx->ks_block) {   // --known_sites: the panel mask over the columns just written
    {
      ganon_detail::KernelScope ks(ctx, "k_bam_known_mask");
      hipLaunchKernelGGL(k_bam_known_mask, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, V, nr, ctx->ks_view, ctx->ks_count);
    }
    if ((rc = check_launch(ctx, "k_bam_known_mask"))) return rc;
  }
  if (nr && ctx->ks_block && ctx->sa_block) {   // --mask_sa_clips: the clips of the columns just masked
    {
      ganon_detail::KernelScope ks(ctx, "k_bam_sa_clips");
      hipLaunchKernelGGL(k_bam_sa_clips, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, V, nr, ctx->ks_view, ctx->sa_names,
                         ctx->sa_count);
    }
    if ((rc = check_launch(ctx, "k_bam_sa_clips"))) return rc;
  }
  if (nr && ctx->st_tally) {   // --discover_sites: the evidence of the columns just written
    const ganon_dtally *D = ctx->st_tally;
    const StView T{D->ref, D->words, D->len, ctx->st_tid, ctx->st_dataset, D->rule};
    {
      ganon_detail::KernelScope ks(ctx, "k_bam_site_tally");
      if (ganon_st::filtered(D->rule))
        hipLaunchKernelGGL(k_bam_site_tally<true>, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, V, nr, T);
      else
        hipLaunchKernelGGL(k_bam_site_tally<false>, dim3(grid_of(nr)), dim3(kBamThreads), 0, s, V, nr, T);
    }
    if ((rc = check_launch(ctx, "k_bam_site_tally"))) return rc;
  }
  return ganon_batch_sync(ctx);   // (collects the kernel times when profiling)
}

void release(ganon_ctx *ctx, ganon_bam_dcols *H) {
  if (!H) return;
  ctx_dfree(ctx, H->block, H->block_bytes);
  ctx_dfree(ctx, H->blobs, H->blobs_bytes);
  ctx_dfree(ctx, H->stream, H->stream_bytes);
  delete H;
}

}  // namespace

GANON_API int ganon_bam_columns(ganon_ctx *ctx, const uint8_t *stream, int64_t p, int64_t n, int on_host,
                                ganon_bam_dcols **out) {
  if (!ctx || !out || p < 0 || n < p || (n > 0 && !stream))
    return fail(ctx, GANON_E_ARG, "ganon_bam_columns: bad arguments");
  if (!on_host && (reinterpret_cast<uintptr_t>(stream) & 3))   // (the walks read aligned dwords)
    return fail(ctx, GANON_E_ARG, "ganon_bam_columns: a device stream must be 4-byte aligned");
  *out = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  if (ctx->profiling) {   // a profiled call: ganon_last_kernel_times reports this call's kernels alone
    ganon_detail::sync_stream(ctx->stream);
    for (auto &r : ctx->recs) {
      ctx->pool.push_back(r.e0);
      ctx->pool.push_back(r.e1);
    }
    ctx->recs.clear();
  }
  auto *H = new ganon_bam_dcols();
  const uint8_t *d = stream;
  if (on_host && n > 0) {
    if (ctx_dmalloc(ctx, reinterpret_cast<void **>(&H->stream), (size_t)n, &H->stream_bytes) != hipSuccess) {
      release(ctx, H);
      return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: device allocation of %lld bytes failed", (long long)n);
    }
    // (waited for: the kernel events that follow time the record walk, not the copy)
    if (hipMemcpyAsync(H->stream, stream, (size_t)n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        ganon_detail::sync_stream(ctx->stream) != hipSuccess) {
      ganon_detail::sync_stream(ctx->stream);
      release(ctx, H);
      return fail(ctx, GANON_E_DEVICE, "ganon_bam_columns: stream copy failed");
    }
    d = H->stream;
  }
  const int rc = columns(ctx, d, p, n, H);
  if (rc) {
    ganon_detail::sync_stream(ctx->stream);
    release(ctx, H);
    return rc;
  }
  *out = H;
  return GANON_OK;
}

GANON_API int ganon_bam_walk_params(int64_t out[5]) {
  if (!out) return GANON_E_ARG;
  out[0] = kChunk;
  out[1] = kProbe;
  out[2] = kGuessSpan;
  out[3] = kStage;
  out[4] = kScatRecs;
  return GANON_OK;
}

GANON_API int ganon_ctx_set_name_key(ganon_ctx *ctx, const uint8_t *key, int32_t key_len) {
  if (!ctx) return GANON_E_ARG;
  if (key_len < 0 || key_len > ganon_nh::kMaxKey || (key_len > 0 && !key))
    return fail(ctx, GANON_E_ARG, "ganon_ctx_set_name_key: a key of 1..32 bytes, or length 0 for none");
  ctx->name_hash = key_len > 0;
  if (ctx->name_hash) ganon_nh::key_state(key, key_len, &ctx->name_key);
  return GANON_OK;
}

// The running count of the table in place, added to ks_total; the device counter is left as it is.
static int ks_collect(ganon_ctx *ctx, int64_t *sum) {
  *sum = ctx->ks_total;
  if (!ctx->ks_block) return GANON_OK;
  unsigned long long c = 0;
  HIP_OR_FAIL(ganon_detail::readback(&c, ctx->ks_count, 8, ctx->stream));
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  *sum += (int64_t)c;
  return GANON_OK;
}

GANON_API int ganon_ctx_set_known_sites(ganon_ctx *ctx, int32_t n_ref, const int64_t *site_off, const int32_t *site_pos,
                                        const uint8_t *site_code, int64_t n, int32_t quality) {
  if (!ctx) return GANON_E_ARG;
  if (n < 0 || quality < -1 || quality > 93 || (n > 0 && (n_ref <= 0 || !site_off || !site_pos || !site_code)))
    return fail(ctx, GANON_E_ARG, "ganon_ctx_set_known_sites: bad arguments");
  if (n > 0) {   // (the kernel trusts the table: what ganon_sites_create checks)
    if (site_off[0] != 0 || site_off[n_ref] != n)
      return fail(ctx, GANON_E_ARG, "ganon_ctx_set_known_sites: site_off must run from 0 to n");
    for (int32_t t = 0; t < n_ref; ++t) {
      if (site_off[t + 1] < site_off[t] || site_off[t + 1] > n)
        return fail(ctx, GANON_E_ARG, "ganon_ctx_set_known_sites: site_off must not decrease");
      for (int64_t j = site_off[t]; j < site_off[t + 1]; ++j)
        if (site_pos[j] < 0 || (j > site_off[t] && site_pos[j] <= site_pos[j - 1]) || !ganon_ks::code_ok(site_code[j]))
          return fail(ctx, GANON_E_ARG, "ganon_ctx_set_known_sites: site %lld: positions strictly increasing per sequence, "
                      "codes ref_nt16 << 4 | alt_mask", (long long)j);
    }
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  if (ctx->ks_block) {   // the table in place goes: its count stays in the total
    int64_t sum = 0;
    const int rc = ks_collect(ctx, &sum);
    if (rc) return rc;
    ctx->ks_total = sum;
    HIP_OR_FAIL(hipFree(ctx->ks_block));   // (waits for the device: no kernel reads it any more)
    ctx->ks_block = nullptr;
    ctx->ks_count = nullptr;
    ctx->ks_view = ganon_ks::View{};
  }
  if (n == 0) return GANON_OK;
  const int64_t b_off = ((int64_t)(n_ref + 1) * 8 + 255) / 256 * 256, b_pos = (n * 4 + 255) / 256 * 256,
                b_code = (n + 255) / 256 * 256;
  void *blk = nullptr;
  HIP_OR_FAIL(hipMalloc(&blk, (size_t)(b_off + b_pos + b_code + 256)));
  uint8_t *at = static_cast<uint8_t *>(blk);
  hipStream_t s = ctx->stream;
  const unsigned long long zero = 0;
  if (hipMemcpyAsync(at, site_off, (size_t)(n_ref + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(at + b_off, site_pos, (size_t)n * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(at + b_off + b_pos, site_code, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(at + b_off + b_pos + b_code, &zero, 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      ganon_detail::sync_stream(s) != hipSuccess) {
    ganon_detail::sync_stream(s);
    hipFree(blk);
    return fail(ctx, GANON_E_DEVICE, "ganon_ctx_set_known_sites: upload failed");
  }
  ctx->ks_block = blk;
  ctx->ks_view.n_ref = n_ref;
  ctx->ks_view.off = reinterpret_cast<const int64_t *>(at);
  ctx->ks_view.pos = reinterpret_cast<const int32_t *>(at + b_off);
  ctx->ks_view.code = at + b_off + b_pos;
  ctx->ks_view.qual = quality;
  ctx->ks_count = reinterpret_cast<unsigned long long *>(at + b_off + b_pos + b_code);
  return GANON_OK;
}

GANON_API int ganon_ctx_known_sites_masked(ganon_ctx *ctx, int64_t *masked) {
  if (!ctx || !masked) return fail(ctx, GANON_E_ARG, "ganon_ctx_known_sites_masked: bad arguments");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  return ks_collect(ctx, masked);
}

// The running counts of the names in place, added to sa_total; the device counters are left as they are.
static int sa_collect(ganon_ctx *ctx, int64_t sum[2]) {
  sum[0] = ctx->sa_total[0];
  sum[1] = ctx->sa_total[1];
  if (!ctx->sa_block) return GANON_OK;
  unsigned long long c[2] = {0, 0};
  HIP_OR_FAIL(ganon_detail::readback(c, ctx->sa_count, 16, ctx->stream));
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  sum[0] += (int64_t)c[0];
  sum[1] += (int64_t)c[1];
  return GANON_OK;
}

GANON_API int ganon_ctx_set_sa_clips(ganon_ctx *ctx, int32_t n_names, const char *names, const int64_t *name_off,
                                     const int32_t *name_tid) {
  if (!ctx) return GANON_E_ARG;
  if (n_names < 0 || (n_names > 0 && (!names || !name_off || !name_tid)))
    return fail(ctx, GANON_E_ARG, "ganon_ctx_set_sa_clips: bad arguments");
  if (n_names > 0) {   // (the kernel trusts the names: what ganon_sites_set_sa_clips checks)
    if (name_off[0] != 0) return fail(ctx, GANON_E_ARG, "ganon_ctx_set_sa_clips: name_off[0] must be 0");
    for (int32_t i = 0; i < n_names; ++i) {
      if (name_off[i + 1] < name_off[i] || name_tid[i] < 0)
        return fail(ctx, GANON_E_ARG, "ganon_ctx_set_sa_clips: name_off must not decrease, sequence ids >= 0");
      if (i > 0) {
        const int64_t la = name_off[i] - name_off[i - 1], lb = name_off[i + 1] - name_off[i];
        const int c = std::memcmp(names + name_off[i - 1], names + name_off[i], (size_t)std::min(la, lb));
        if (c > 0 || (c == 0 && la >= lb))
          return fail(ctx, GANON_E_ARG, "ganon_ctx_set_sa_clips: the names must be sorted bytewise and distinct");
      }
    }
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  if (ctx->sa_block) {   // the names in place go: their counts stay in the totals
    int64_t sum[2];
    const int rc = sa_collect(ctx, sum);
    if (rc) return rc;
    ctx->sa_total[0] = sum[0];
    ctx->sa_total[1] = sum[1];
    HIP_OR_FAIL(hipFree(ctx->sa_block));   // (waits for the device: no kernel reads it any more)
    ctx->sa_block = nullptr;
    ctx->sa_count = nullptr;
    ctx->sa_names = ganon_sa::Names{};
  }
  if (n_names == 0) return GANON_OK;
  const int64_t nb = name_off[n_names];
  const int64_t b_off = ((int64_t)(n_names + 1) * 8 + 255) / 256 * 256, b_tid = ((int64_t)n_names * 4 + 255) / 256 * 256,
                b_blob = (nb + 255) / 256 * 256;
  void *blk = nullptr;
  HIP_OR_FAIL(hipMalloc(&blk, (size_t)(b_off + b_tid + b_blob + 256)));
  uint8_t *at = static_cast<uint8_t *>(blk);
  hipStream_t s = ctx->stream;
  const unsigned long long zero[2] = {0, 0};
  if (hipMemcpyAsync(at, name_off, (size_t)(n_names + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(at + b_off, name_tid, (size_t)n_names * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
      (nb > 0 && hipMemcpyAsync(at + b_off + b_tid, names, (size_t)nb, hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(at + b_off + b_tid + b_blob, zero, 16, hipMemcpyHostToDevice, s) != hipSuccess ||
      ganon_detail::sync_stream(s) != hipSuccess) {
    ganon_detail::sync_stream(s);
    hipFree(blk);
    return fail(ctx, GANON_E_DEVICE, "ganon_ctx_set_sa_clips: upload failed");
  }
  ctx->sa_block = blk;
  ctx->sa_names.n = n_names;
  ctx->sa_names.off = reinterpret_cast<const int64_t *>(at);
  ctx->sa_names.tid = reinterpret_cast<const int32_t *>(at + b_off);
  ctx->sa_names.blob = reinterpret_cast<const char *>(at + b_off + b_tid);
  ctx->sa_count = reinterpret_cast<unsigned long long *>(at + b_off + b_tid + b_blob);
  return GANON_OK;
}

GANON_API int ganon_ctx_sa_clips_counts(ganon_ctx *ctx, int64_t *masked, int64_t *ignored) {
  if (!ctx || !masked || !ignored) return fail(ctx, GANON_E_ARG, "ganon_ctx_sa_clips_counts: bad arguments");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  int64_t sum[2];
  const int rc = sa_collect(ctx, sum);
  if (rc) return rc;
  *masked = sum[0];
  *ignored = sum[1];
  return GANON_OK;
}

GANON_API int ganon_site_compact_tile(void) { return kSiteTile; }

static void dtally_release(ganon_dtally *D) {
  if (!D) return;
  hipFree(D->ref);   // (hipFree waits for the device: no kernel reads them any more)
  hipFree(D->words);
  hipFree(D->pos);
  hipFree(D->code);
  delete D;
}

GANON_API int ganon_dtally_create_ex(ganon_ctx *ctx, const uint8_t *ref_nt16, int64_t len, int32_t min_base_quality,
                                     int32_t min_mapq, uint32_t exclude_flags, int32_t mode, ganon_dtally **out) {
  if (!ctx || !out || len < 0 || len > INT32_MAX || (len > 0 && !ref_nt16))
    return fail(ctx, GANON_E_ARG, "ganon_dtally_create: bad arguments");
  *out = nullptr;
  const ganon_st::Rule rule{min_base_quality, min_mapq, exclude_flags, mode};
  if (!ganon_st::rule_valid(rule))
    return fail(ctx, GANON_E_ARG,
                "ganon_dtally_create_ex: base quality 0..93, mapq 0..255, flags 0..65535, mode 0 (both) or 1 (normal)");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  auto *D = new ganon_dtally();
  D->len = len;
  D->rule = rule;
  D->padded = std::max<int64_t>(1, (len + kSiteTile - 1) / kSiteTile) * kSiteTile;
  hipStream_t s = ctx->stream;
  if (hipMalloc(reinterpret_cast<void **>(&D->ref), (size_t)D->padded / 2) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&D->words), (size_t)D->padded) != hipSuccess ||
      hipMemsetAsync(D->ref, 0, (size_t)D->padded / 2, s) != hipSuccess ||
      hipMemsetAsync(D->words, 0, (size_t)D->padded, s) != hipSuccess ||
      (len > 0 && hipMemcpyAsync(D->ref, ref_nt16, (size_t)((len + 1) / 2), hipMemcpyHostToDevice, s) != hipSuccess) ||
      ganon_detail::sync_stream(s) != hipSuccess) {
    ganon_detail::sync_stream(s);
    dtally_release(D);
    return fail(ctx, GANON_E_DEVICE, "ganon_dtally_create: device allocation or upload of %lld bases failed", (long long)len);
  }
  *out = D;
  return GANON_OK;
}

GANON_API int ganon_dtally_create(ganon_ctx *ctx, const uint8_t *ref_nt16, int64_t len, ganon_dtally **out) {
  return ganon_dtally_create_ex(ctx, ref_nt16, len, 0, 0, 0u, ganon_st::kBoth, out);
}

GANON_API int ganon_ctx_set_site_tally(ganon_ctx *ctx, ganon_dtally *tally, int32_t dataset, int32_t tid) {
  if (!ctx) return GANON_E_ARG;
  if (tally && (dataset < 0 || dataset > 1 || tid < 0))
    return fail(ctx, GANON_E_ARG, "ganon_ctx_set_site_tally: dataset is 0 (tumor) or 1 (normal), tid a BAM sequence id");
  if (tally && tally->n_sites >= 0) return fail(ctx, GANON_E_STATE, "ganon_ctx_set_site_tally: the tally is compacted already");
  ctx->st_tally = tally;
  ctx->st_dataset = tally ? dataset : 0;
  ctx->st_tid = tally ? tid : -1;
  return GANON_OK;
}

GANON_API int ganon_dtally_compact(ganon_ctx *ctx, ganon_dtally *D, const uint8_t *host_bytes, int64_t *n) {
  if (!ctx || !D || !n) return fail(ctx, GANON_E_ARG, "ganon_dtally_compact: bad arguments");
  if (D->n_sites >= 0) return fail(ctx, GANON_E_STATE, "ganon_dtally_compact: compacted already");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  hipStream_t s = ctx->stream;
  if (ctx->profiling) {   // a profiled call: ganon_last_kernel_times reports this call's kernels alone
    ganon_detail::sync_stream(s);
    for (auto &r : ctx->recs) {
      ctx->pool.push_back(r.e0);
      ctx->pool.push_back(r.e1);
    }
    ctx->recs.clear();
  }
  const int64_t tiles = D->padded / kSiteTile;
  const bool normal = D->rule.mode == ganon_st::kNormal;
  std::vector<std::pair<void *, size_t>> tmp;
  auto dalloc = [&](size_t bytes) -> void * {
    void *q = nullptr;
    size_t got = 0;
    if (ctx_dmalloc(ctx, &q, std::max<size_t>(bytes, 256), &got) != hipSuccess) return nullptr;
    tmp.emplace_back(q, got);
    return q;
  };
  struct Free {
    ganon_ctx *ctx;
    hipStream_t s;
    std::vector<std::pair<void *, size_t>> &t;
    ~Free() {
      ganon_detail::sync_stream(s);
      for (auto &q : t) ctx_dfree(ctx, q.first, q.second);
    }
  } free_tmp{ctx, s, tmp};
  int rc;
  uint32_t *hw = nullptr;
  if (host_bytes && D->len > 0) {
    hw = static_cast<uint32_t *>(dalloc((size_t)D->padded));
    if (!hw) return fail(ctx, GANON_E_DEVICE, "ganon_dtally_compact: device allocation failed");
    HIP_OR_FAIL(hipMemsetAsync(hw, 0, (size_t)D->padded, s));
    HIP_OR_FAIL(hipMemcpyAsync(hw, host_bytes, (size_t)D->len, hipMemcpyHostToDevice, s));
    HIP_OR_FAIL(ganon_detail::sync_stream(s));   // (the kernel events time the compaction, not the copy)
  }
  int64_t *count = static_cast<int64_t *>(dalloc((size_t)(tiles + 1) * 8));
  int64_t *base = static_cast<int64_t *>(dalloc((size_t)(tiles + 1) * 8));
  size_t tb = 0;
  HIP_OR_FAIL(rocprim::exclusive_scan(nullptr, tb, count, base, (int64_t)0, (size_t)(tiles + 1), rocprim::plus<int64_t>(), s));
  void *tsc = dalloc(tb);
  if (!count || !base || !tsc) return fail(ctx, GANON_E_DEVICE, "ganon_dtally_compact: device allocation failed");
  HIP_OR_FAIL(hipMemsetAsync(count + tiles, 0, 8, s));
  {
    ganon_detail::KernelScope ks(ctx, "k_site_compact");
    if (normal)
      hipLaunchKernelGGL((k_site_compact<false, true>), dim3((unsigned)tiles), dim3(kBamThreads), 0, s, D->words, hw, D->ref,
                         count, base, nullptr, nullptr);
    else
      hipLaunchKernelGGL((k_site_compact<false, false>), dim3((unsigned)tiles), dim3(kBamThreads), 0, s, D->words, hw, D->ref,
                         count, base, nullptr, nullptr);
  }
  if ((rc = check_launch(ctx, "k_site_compact"))) return rc;
  {
    ganon_detail::KernelScope ks(ctx, "site_scan");
    HIP_OR_FAIL(rocprim::exclusive_scan(tsc, tb, count, base, (int64_t)0, (size_t)(tiles + 1), rocprim::plus<int64_t>(), s));
  }
  int64_t total = 0;
  HIP_OR_FAIL(ganon_detail::readback(&total, base + tiles, 8, s));
  HIP_OR_FAIL(ganon_detail::sync_stream(s));
  if (total < 0 || total > D->len) return fail(ctx, GANON_E_STATE, "ganon_dtally_compact: site count out of range");
  if (total) {
    HIP_OR_FAIL(hipMalloc(reinterpret_cast<void **>(&D->pos), (size_t)total * 4));
    HIP_OR_FAIL(hipMalloc(reinterpret_cast<void **>(&D->code), (size_t)total));
    {
      ganon_detail::KernelScope ks(ctx, "k_site_compact");
      if (normal)
        hipLaunchKernelGGL((k_site_compact<true, true>), dim3((unsigned)tiles), dim3(kBamThreads), 0, s, D->words, hw, D->ref,
                           count, base, D->pos, D->code);
      else
        hipLaunchKernelGGL((k_site_compact<true, false>), dim3((unsigned)tiles), dim3(kBamThreads), 0, s, D->words, hw, D->ref,
                           count, base, D->pos, D->code);
    }
    if ((rc = check_launch(ctx, "k_site_compact"))) return rc;
  }
  if ((rc = ganon_batch_sync(ctx))) return rc;   // (collects the kernel times when profiling)
  D->n_sites = total;
  *n = total;
  return GANON_OK;
}

GANON_API int ganon_dtally_sites(ganon_ctx *ctx, ganon_dtally *D, int32_t *pos, uint8_t *code) {
  if (!ctx || !D) return fail(ctx, GANON_E_ARG, "ganon_dtally_sites: bad arguments");
  if (D->n_sites < 0) return fail(ctx, GANON_E_STATE, "ganon_dtally_sites: before ganon_dtally_compact");
  if (D->n_sites == 0) return GANON_OK;
  if (!pos || !code) return fail(ctx, GANON_E_ARG, "ganon_dtally_sites: bad arguments");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  HIP_OR_FAIL(hipMemcpyAsync(pos, D->pos, (size_t)D->n_sites * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_OR_FAIL(hipMemcpyAsync(code, D->code, (size_t)D->n_sites, hipMemcpyDeviceToHost, ctx->stream));
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  return GANON_OK;
}

GANON_API int ganon_dtally_free(ganon_ctx *ctx, ganon_dtally *D) {
  if (!D) return GANON_OK;
  if (ctx) {
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
    if (ctx->st_tally == D) {
      ctx->st_tally = nullptr;
      ctx->st_tid = -1;
    }
    ganon_detail::sync_stream(ctx->stream);
  }
  dtally_release(D);
  return GANON_OK;
}

GANON_API int ganon_bam_dcols_get(const ganon_bam_dcols *c, ganon_bam_cols *device_view, int64_t *fixes) {
  if (!c || !device_view) return GANON_E_ARG;
  *device_view = c->v;
  if (fixes) *fixes = c->fixes;
  return GANON_OK;
}

GANON_API int ganon_bam_dcols_download(ganon_ctx *ctx, const ganon_bam_dcols *c, const ganon_bam_cols *host) {
  if (!ctx || !c || !host) return fail(ctx, GANON_E_ARG, "ganon_bam_dcols_download: bad arguments");
  const ganon_bam_cols &V = c->v;
  const int64_t nr = V.n_records;
  hipStream_t s = ctx->stream;
  auto cp = [&](void *dst, const void *src, int64_t bytes) {
    return !dst || bytes <= 0 || hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  };
  bool ok = true;
  const std::pair<int32_t *, const int32_t *> i32[12] = {
      {host->tid, V.tid}, {host->pos, V.pos}, {host->end, V.end}, {host->flag, V.flag}, {host->mapq, V.mapq},
      {host->l_seq, V.l_seq}, {host->n_cigar, V.n_cigar}, {host->mate_tid, V.mate_tid}, {host->mate_pos, V.mate_pos},
      {host->tlen, V.tlen}, {host->name_len, V.name_len}, {host->aux_len, V.aux_len}};
  for (const auto &x : i32) ok = ok && cp(x.first, x.second, nr * 4);
  const std::pair<int64_t *, const int64_t *> i64[6] = {{host->name_off, V.name_off}, {host->cig_off, V.cig_off},
                                                        {host->seq_off, V.seq_off},   {host->qual_off, V.qual_off},
                                                        {host->aux_off, V.aux_off},   {host->rec_off, V.rec_off}};
  for (const auto &x : i64) ok = ok && cp(x.first, x.second, nr * 8);
  ok = ok && cp(host->names, V.names, V.names_bytes) && cp(host->cigar, V.cigar, 4 * V.cigar_ops) &&
       cp(host->seq, V.seq, V.seq_bytes) && cp(host->qual, V.qual, V.qual_bytes) && cp(host->aux, V.aux, V.aux_bytes);
  if (!ok || ganon_detail::sync_stream(s) != hipSuccess) {
    ganon_detail::sync_stream(s);
    return fail(ctx, GANON_E_DEVICE, "ganon_bam_dcols_download: copy failed");
  }
  return GANON_OK;
}

GANON_API int ganon_bam_dcols_free(ganon_ctx *ctx, ganon_bam_dcols *c) {
  if (ctx) ganon_detail::sync_stream(ctx->stream);
  release(ctx, c);
  return GANON_OK;
}

// ---- a region read decoded on the device (the reader's region decoder, ganon_bam_reader_region) ----
GANON_API int ganon_region_decode(void *user, const uint8_t *comp, int64_t comp_len, const int64_t *in_off,
                                  const int32_t *in_len, const int64_t *out_off, const int32_t *out_len,
                                  int64_t n_blocks, uint8_t *out, int64_t out_total, int64_t p0, int32_t tid,
                                  int64_t beg, int64_t end, int at_eof, ganon_bam_view *cols, void **block) {
  ganon_ctx *ctx = static_cast<ganon_ctx *>(user);
  if (!ctx || !cols || !block || (out_total > 0 && !out) || p0 < 0) return -1;
  *block = nullptr;
  if (ganon_inflate_impl(ctx, comp, comp_len, in_off, in_len, out_off, out_len, n_blocks, nullptr, out_total, nullptr))
    return -1;   // (the inflate failed: ctx->err)
  const uint8_t *dout = nullptr;
  int64_t bytes = 0;
  if (ganon_inflate_device_output(ctx, &dout, &bytes) || bytes != out_total) return -1;
  hipStream_t s = ctx->stream;
  // the host's walk goes on from the inflated window: its bytes to `out`
  auto raw = [&]() -> int {
    if (out_total > 0 && (hipMemcpyAsync(out, dout, (size_t)out_total, hipMemcpyDeviceToHost, s) != hipSuccess ||
                          ganon_detail::sync_stream(s) != hipSuccess)) {
      ganon_detail::sync_stream(s);
      return fail(ctx, -1, "ganon_region_decode: copy failed");
    }
    return 0;
  };
  if (p0 > out_total) return raw();
  auto *H = new ganon_bam_dcols();
  RegionReq rq{tid, beg, end, at_eof != 0, 0};
  const int rc = columns(ctx, dout, p0, out_total, H, &rq);
  if (rc || rq.status != 1) {   // (a device failure, too, leaves the window to the host)
    ganon_detail::sync_stream(s);
    release(ctx, H);
    return raw();
  }
  // the columns to one page-locked block, laid out as the device block's first 17 columns and the
  // blob block: two copies by DMA
  const ganon_bam_cols &V = H->v;
  const int64_t m = V.n_records + 1;
  const int64_t prefix = 12 * (((m * 4) + 255) / 256 * 256) + 5 * (((m * 8) + 255) / 256 * 256);
  void *hb = nullptr;
  if (ganon_pinned_alloc(prefix + H->blobs_used + 256, &hb) != 0 || !hb) {
    release(ctx, H);
    return raw();
  }
  uint8_t *h8 = static_cast<uint8_t *>(hb);
  if (hipMemcpyAsync(h8, H->block, (size_t)prefix, hipMemcpyDeviceToHost, s) != hipSuccess ||
      (H->blobs_used > 0 &&
       hipMemcpyAsync(h8 + prefix, H->blobs, (size_t)H->blobs_used, hipMemcpyDeviceToHost, s) != hipSuccess) ||
      ganon_detail::sync_stream(s) != hipSuccess) {
    ganon_detail::sync_stream(s);
    release(ctx, H);
    ganon_pinned_free(hb);
    return raw();
  }
  ganon_bam_cols hv{};
  uint8_t *at = h8;
  for (int32_t **f : {&hv.tid, &hv.pos, &hv.end, &hv.flag, &hv.mapq, &hv.l_seq, &hv.n_cigar, &hv.mate_tid, &hv.mate_pos,
                      &hv.tlen, &hv.name_len, &hv.aux_len})
    *f = carve<int32_t>(at, m);
  for (int64_t **f : {&hv.name_off, &hv.cig_off, &hv.seq_off, &hv.qual_off, &hv.aux_off}) *f = carve<int64_t>(at, m);
  at = h8 + prefix;
  hv.names = carve<char>(at, V.names_bytes);
  hv.cigar = carve<uint32_t>(at, V.cigar_ops);
  hv.seq = carve<uint8_t>(at, V.seq_bytes);
  hv.qual = carve<uint8_t>(at, V.qual_bytes);
  hv.aux = carve<uint8_t>(at, V.aux_bytes);
  *cols = ganon_bam_view{};
  cols->n_records = V.n_records;
  cols->tid = hv.tid, cols->pos = hv.pos, cols->end = hv.end, cols->flag = hv.flag, cols->mapq = hv.mapq;
  cols->l_seq = hv.l_seq, cols->n_cigar = hv.n_cigar, cols->mate_tid = hv.mate_tid, cols->mate_pos = hv.mate_pos;
  cols->tlen = hv.tlen, cols->name_len = hv.name_len, cols->aux_len = hv.aux_len;
  cols->name_off = hv.name_off, cols->cig_off = hv.cig_off, cols->seq_off = hv.seq_off, cols->qual_off = hv.qual_off;
  cols->aux_off = hv.aux_off;
  cols->names = hv.names, cols->names_bytes = V.names_bytes;
  cols->cigar = hv.cigar, cols->cigar_ops = V.cigar_ops;
  cols->seq = hv.seq, cols->seq_bytes = V.seq_bytes;
  cols->qual = hv.qual, cols->qual_bytes = V.qual_bytes;
  cols->aux = hv.aux, cols->aux_bytes = V.aux_bytes;
  release(ctx, H);
  *block = hb;
  return 1;
}
