// ganon_prep.hip — device prep of a masking batch on MI355X (gfx950): the derived layer of
// ganon_batch.h rebuilt from the raw SoA on every ganon_batch_run, so that a step processes the
// batch exactly as the host hands it over (BAM nt16 bases + BAM CIGAR words + scope incidences).
//
// Reference semantics being prepared: the reference's pileup
// (pileup_io.pyx:8-41, htslib truncate=False) visits every aligned base (CIGAR M/=/X) of every
// read of a scope at reference position p, query position q; insertions and soft clips consume
// the read only, deletions and skips the reference only (variation_classifier.py:185-215 walks
// those columns). Here each read's CIGAR is walked once per (scope, read) incidence into segment
// records — one per aligned run: (query nibble, reference nibble, length, dataset, whether this
// scope writes the read) — that k_group (ganon_group.hip) streams in 16-base chunks.
//
// Kernels (integer work, HBM/latency bound, no MFMA), in launch order. Plan (ganon_batch_replan /
// the upload; one host synchronization):
//   k_prep_scan + k_prep_reduce  one pass over the raw per-read and per-scope arrays: every check of
//                   the host validation, read_end, the batch shape (longest read, segments per
//                   read, I/D ops, written reads, huge scopes, write-scope hash sum) as per-block
//                   partials, and the group table of the short-read modes — groups are the scopes
//                   whose (incidences + weight per scope) prefix, the CSR offsets themselves, falls
//                   in one bucket of group_target units (the weight caps a group at 256 scopes);
//   (long-read mode) k_prep_nseg + k_prep_scope_cost + exclusive scan: groups cut on the
//                   segments-per-scope prefix instead;
//   (two-pass and long modes) k_prep_groups + a counting emit: record ranges of groups with more
//                   segments than incidences.
// Run (ganon_batch_run):
//   k_prep_emit_flat (every read with at most one aligned segment: short reads, the default then):
//                   workgroup per group, thread per incidence, its one record at the slot of its own
//                   index — no count pass, no scan, no allocation; the incidence checks, the
//                   write-scope hash sum and the group's partition candidates (lowest buffer offset
//                   of the reads it writes, per dataset) marked in the line map; a group is read
//                   through the 2-bit reference unless one of its records touches a non-ACGT block;
//   k_prep_emit     (two-pass: short reads with indels) workgroup per group: counts clean/dirty
//                   segments around a block scan, takes the group's record range (its own incidence
//                   indices, or one of 256 allocation counters), writes the records —
//                   all-ACGT-reference segments from the front, the others from the back;
//   k_prep_long_groups + k_prep_emit_waves + k_prep_long_mid (long reads): one wave per incidence
//                   walks its CIGAR 64 ops at a time (wave prefix sums of the query / reference
//                   deltas and of the record counts) into deterministic slots — no atomics;
//   k_prep_linemap + k_prep_pieces  the candidates' 128-byte lines form a 3-level bitmap (ties on a
//                   line through a small hash table); each candidate's piece runs from its line to
//                   the next marked one, so the pieces tile the output buffer — each group copies at
//                   most two pieces. No sort.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include <rocprim/device/device_scan.hpp>


#include "ganon_batch.h"

using namespace ganon_dev;
using ganon_detail::check_launch;
using ganon_detail::fail;
using ganon_detail::KernelScope;

namespace {

constexpr int kPrepThreads = 256;
constexpr unsigned long long kNone = ~0ull;
constexpr int kCursors = 256;   // emit allocation counters (group g uses g % kCursors): no same-address hot spot
constexpr int64_t kFarMax = int64_t(1) << 28;   // far-mask list entries at most

// The raw arrays and sizes every prep kernel reads.
struct Raw {
  const int32_t *ref_start, *read_len, *n_cig, *write_scope;
  const int64_t *seq_off, *cig_off;
  const uint8_t *dataset;
  const uint32_t *cigar;
  const int64_t *incid_off;
  const int32_t *incid_read;
  const int32_t *span_start, *span_len;
  const int64_t *ref_off;
  const uint8_t *keep_code;
  int32_t n_reads, n_scopes;
  int64_t n_incid, seq_bytes, n_cigar_ops, ref_nibs;
};

// ---- reference blocks -----------------------------------------------------------------------
// Bit k of bad: 64-base block k (32 bytes of nt16) holds a code other than A, C, G, T.
__global__ void __launch_bounds__(kPrepThreads) k_ref_blocks(const uint8_t *__restrict__ ref, int64_t bytes,
                                                             int64_t n_blk, uint64_t *__restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * kPrepThreads;
  // n_blk rounded up to whole waves so that every lane reaches the ballot
  const int64_t n_round = (n_blk + 63) & ~(int64_t)63;
  for (int64_t k = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x; k < n_round; k += stride) {
    bool b = false;
    if (k < n_blk) {
      const int64_t e = min(32 * k + 32, bytes);
      for (int64_t x = 32 * k; x < e; ++x) {
        const int v = ref[x];
        const int hi = v >> 4, lo = v & 15;
        b |= !((0x116 >> hi) & 1) || !((0x116 >> lo) & 1);
      }
    }
    const uint64_t m = __ballot(b);
    if ((threadIdx.x & 63) == 0) bad[k >> 6] = m;
  }
}

// Scope groups: the scopes whose cost prefix (incidences + `weight` per scope, no scan needed: the
// CSR offsets are that prefix) falls in one bucket of `target` units. The weight bounds a group to
// 256 scopes. A bucket skipped over by a scope with many incidences is an empty group.
__device__ __forceinline__ int64_t group_of(const int64_t *__restrict__ incid_off, int64_t s, long long weight,
                                            long long target, const int64_t *__restrict__ cost) {
  return cost ? cost[s] / target : (incid_off[s] + weight * s) / target;
}

// ---- the batch scan: every per-read and per-scope check, one pass over the raw arrays ----------
// Replaces round 2's four check kernels, the segments-per-read pass and the far-capacity pass
// (k_prep_reads / k_prep_scope_check / k_prep_incid_check / k_prep_seen_check / k_prep_farcap):
// one coalesced read of each per-read and per-scope array. Read blocks validate every read field
// before any load that depends on it, write read_end (bam_endpos) and count the aligned segments
// and I/D ops per read; scope blocks validate the scope arrays and write the group table (first
// scope and incidence of each short-read group, closed form from the CSR offsets). Per-block
// partial sums (no same-address atomics: a batch-wide counter hit once per wave serialised
// k_prep_reads at 0.8 ms) go to `part`, reduced by k_prep_reduce. The incidence checks (read
// index, span containment) and the write-scope check need the scope of each incidence: the emit
// kernels make them where they walk the incidences anyway (neither can fault: they range-check
// before they gather); ganon_batch_download reports their errors.
enum { kPartWritten = 0, kPartMaxLen, kPartMaxSeg, kPartIdOps, kPartHuge, kPartWsHash, kParts };

// The write-scope check without a per-read mark: every written read r contributes ws_hash(r) once
// from the batch scan and once from the emit path that meets it in its write scope; the sums
// (64-bit, wrapping, order-free) agree iff every written read is listed by its write scope (up to
// a 2^-64 collision: a read listed twice in its write scope and another one missing give
// different sums). k_finish compares them; on a mismatch ganon_batch_download runs
// k_prep_ws_diag to name the read.
// Sum of v over the block (256 threads); the result in every thread.
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *ws) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    v += ((unsigned long long)hi << 32) | lo;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0;
  for (int w = 0; w < kWaves; ++w) t += ws[w];
  return t;
}
#ifndef GANON_SCAN_U
#define GANON_SCAN_U 4   // reads per thread of k_prep_scan (loads issued together)
#endif
constexpr int kScanReadsPerBlock = GANON_SCAN_U * kPrepThreads;
constexpr int kScanScopesPerBlock = 4 * kPrepThreads;

struct ScanOut {
  int32_t *read_end;
  int32_t *long_list;         // reads with more than kScanLongCigar CIGAR ops (k_prep_scan_long walks them)
  unsigned int *long_count;
  longlong2 *gmeta;           // [g_bound] first scope and incidence of each short-read group
  int64_t g_bound;            // group count bound: (n_incid + weight (n_scopes - 1)) / target + 1
  unsigned long long *part;   // [kParts][part_stride]: partial k of block b at part[k * part_stride + b]
  int64_t part_stride;
  int32_t *nseg;              // k_prep_scan_long: aligned segments of each long read (long-read mode), or null
  int4 *desc;                 // fused one-segment mode: [n_reads] read descriptors (ganon_batch.h), or null
  unsigned long long *cand;   // and [2 g_bound] partition candidates: ~(lowest written offset), atomicMax
  int32_t *xidx;              // (per multi-segment read: its extras header)
  int4 *xrec;                 // and the extras records of reads of 2..kFusedMaxSeg segments: kXStripes
  unsigned int *xcount;       // stripes of xper records each, stripe k's count at xcount[kXStride * k]
  uint32_t xper;
};


__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int lane) {
  const uint32_t lo = __shfl((uint32_t)v, lane), hi = __shfl((uint32_t)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// Partition candidate of a written read (fused one-segment mode): group g's candidate in dataset d
// is the lowest buffer offset of the reads it writes — the reads whose write scope falls in g. A
// wave's lanes hold consecutive reads (tumor and normal interleaved by position), so a wave meets
// few distinct (group, dataset) keys: one device-scope atomic per key and wave — the first
// pending lane leads, the lanes holding its key reduce their offsets across the wave, the leader
// stores. key < 0: no candidate. Every lane of the wave calls.
__device__ __forceinline__ void scan_candidate(unsigned long long *__restrict__ cand, long long key, int64_t so) {
  const unsigned long long v = ~(unsigned long long)so;   // (complements: the largest wins)
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(key >= 0);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const uint32_t klo = __builtin_amdgcn_readlane((uint32_t)key, leader),
                   khi = __builtin_amdgcn_readlane((uint32_t)((unsigned long long)key >> 32), leader);
    const long long lk = (long long)(((unsigned long long)khi << 32) | klo);
    const bool same = key == lk;
    unsigned long long x = same ? v : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long y = shfl64(x, lane ^ o);
      x = y > x ? y : x;
    }
    if (lane == leader) atomicMax(&cand[lk], x);
    pending &= ~__ballot(same);
  }
}

__device__ __forceinline__ void block_parts(unsigned long long (&acc)[kParts], unsigned long long *__restrict__ part,
                                            int64_t stride) {
  __shared__ unsigned long long ws[kWaves][kParts];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kParts; ++k) {
    unsigned long long v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long x = shfl64(v, lane ^ o);
      v = (k == kPartMaxLen || k == kPartMaxSeg) ? (x > v ? x : v) : v + x;
    }
    if (lane == 0) ws[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kParts) {
    const int k = threadIdx.x;
    unsigned long long v = 0;
    for (int w = 0; w < kWaves; ++w)
      v = (k == kPartMaxLen || k == kPartMaxSeg) ? (ws[w][k] > v ? ws[w][k] : v) : v + ws[w][k];
    part[stride * k + blockIdx.x] = v;
  }
}

// One read's CIGAR walked by a whole wave, 64 ops at a time (long reads: thousands of ops, a serial
// chain of dependent loads for one thread): the reference length (bam_endpos), the aligned
// segments as walk_segments cuts them (per-lane query offsets from a wave prefix sum, the
// read-length clip), the I/D ops; bad_op = the first op code above 8 (the walk stops there), or -1.
// Query-consuming lengths may sum past 2^31 (each op holds up to 2^28 - 1): every per-lane query delta
// is capped at the read length L (below 2^24: the scan's check) and the carried offset stops at L, as
// walk_segments stops there — an offset that wrapped counted segments walk_segments never writes.
struct CigarWalk {
  long long rl;
  int ns, nid, bad_op;
};

__device__ __forceinline__ CigarWalk wave_cigar_walk(const uint32_t *__restrict__ cg, int nc, int L) {
  const int lane = threadIdx.x & 63;
  CigarWalk W{0, 0, 0, -1};
  int q = 0;
  // per-lane sums, reduced once after the walk: only the query offset is a prefix
  int seg = 0, id = 0;
  long long dr = 0;
  for (int base = 0; base < nc; base += 64) {
    const int k = base + lane;
    const uint32_t w = k < nc ? cg[k] : 0u;   // padding lanes: a 0M op, which adds nothing
    const int op = (int)(w & 0xF), len = (int)(w >> 4);
    const unsigned long long badm = __ballot(op > 8);
    if (badm) {
      W.bad_op = __shfl(op, __ffsll((long long)badm) - 1);
      break;
    }
    const bool al = is_aligned_op(op);
    const int dq = (al || op == 1 || op == 4) ? min(len, L) : 0;
    const int incl = ganon_wave::incl_sum(dq);
    const int q0 = q + incl - dq;
    seg += (al && q0 < L) ? (min(len, L - q0) + kSegMaxLen - 1) / kSegMaxLen : 0;
    id += (op == 1 || op == 2) ? 1 : 0;
    dr += (al || op == 2 || op == 3) ? (long long)len : 0ll;
    q = min(q + ganon_wave::last(incl), L);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    seg += __shfl_xor(seg, o);
    id += __shfl_xor(id, o);
    dr += __shfl_xor(dr, o);
  }
  W.ns = seg;
  W.nid = id;
  W.rl = dr;
  return W;
}

constexpr int kScanLongCigar = 48;   // reads with more CIGAR ops are walked by a wave (k_prep_scan_long)
constexpr int kXStripes = 64;        // extras-list allocation counters (scan block b: stripe b mod 64)
constexpr int kXStride = 32;         // ... one 128-byte line each
constexpr int kLongGrid = 4096;      // workgroups of k_prep_scan_long at most (4 waves each)

#ifndef GANON_SCAN_BLOCKS
#define GANON_SCAN_BLOCKS 1   // resident workgroups per CU k_prep_scan is compiled for (1: no bound)
#endif
// NARROW: sequence bytes and CIGAR ops below 2^31 (every configs[1]-sized batch): the offsets are
// kept as 32 bits once checked (fewer live registers across the walks: occupancy).
template <bool NARROW>
__global__ void __launch_bounds__(kPrepThreads, GANON_SCAN_BLOCKS) k_prep_scan(const Raw R, PrepErr *err, ScanOut O, long long weight,
                                                            long long target, int read_blocks) {
  unsigned long long acc[kParts] = {0, 0, 0, 0, 0, 0};
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < read_blocks) {
    typedef typename std::conditional<NARROW, uint32_t, int64_t>::type Off;
    uint32_t n_wr = 0, mx_len = 0, mx_seg = 0, n_id = 0;   // (per thread: 32 bits are enough)
    uint32_t nxp = 0;   // (fused mode) further segments of each multi-segment read, 4 bits per u
    unsigned long long hsum = 0;
    // kScanU reads per thread, each load stage issued for all of them before any is used (the chain
    // read fields -> first CIGAR word is latency bound)
    constexpr int kScanU = kScanReadsPerBlock / kPrepThreads;
    const int64_t r0 = (int64_t)blockIdx.x * kScanReadsPerBlock;
    const int64_t r1 = min(r0 + kScanReadsPerBlock, (int64_t)R.n_reads);
    int L[kScanU], nc[kScanU], rs[kScanU], ws[kScanU], ds[kScanU];
    Off co[kScanU], so[kScanU];
    bool ok[kScanU];
    {
      int64_t co64[kScanU], so64[kScanU];
#pragma unroll
      for (int u = 0; u < kScanU; ++u) {
        const int64_t r = r0 + tid + kPrepThreads * u;
        ok[u] = r < r1;
        const int64_t rr = ok[u] ? r : r0;
        L[u] = R.read_len[rr];
        nc[u] = R.n_cig[rr];
        co64[u] = R.cig_off[rr];
        rs[u] = R.ref_start[rr];
        so64[u] = R.seq_off[rr];
        ws[u] = R.write_scope[rr];
        ds[u] = R.dataset[rr];
      }
#pragma unroll
      for (int u = 0; u < kScanU; ++u) {
        const int64_t r = r0 + tid + kPrepThreads * u;
        if (ok[u]) {
          if (L[u] < 0 || so64[u] < 0 || so64[u] + ((int64_t)L[u] + 1) / 2 > R.seq_bytes) { report(err, kErrReadSeq, r); ok[u] = false; }
          else if (nc[u] < 0 || co64[u] < 0 || co64[u] + nc[u] > R.n_cigar_ops) { report(err, kErrReadCigar, r); ok[u] = false; }
          if (ds[u] > 1) report(err, kErrReadDataset, r);
          if (ws[u] < -1 || ws[u] >= R.n_scopes) { report(err, kErrReadWriteScope, r, ws[u]); ok[u] = false; }
          if (L[u] >= (1 << 24)) { report(err, kErrReadLong, r); ok[u] = false; }   // (the walks rely on L < 2^24)
        }
        co[u] = ok[u] ? (Off)co64[u] : (Off)0;   // (checked: in range)
        so[u] = ok[u] ? (Off)so64[u] : (Off)0;
      }
    }
    uint32_t w0[kScanU];
    // (fused one-segment mode) the CSR offset of each written read's write scope (incidence counts
    // are below 2^31: load_batch) gives its group: the partition candidates, before the walks
    int wo[kScanU];
#pragma unroll
    for (int u = 0; u < kScanU; ++u) {
      w0[u] = ok[u] && nc[u] > 0 ? R.cigar[co[u]] : 0u;
      wo[u] = O.cand && ok[u] && ws[u] >= 0 && L[u] > 0 ? (int)R.incid_off[ws[u]] : -1;
    }
    if (O.cand) {
#pragma unroll
      for (int u = 0; u < kScanU; ++u) {
        long long key = -1;
        if (wo[u] >= 0) {
          // group_of, the offset loaded above (32-bit division when it fits)
          const uint64_t x = (uint64_t)wo[u] + (uint64_t)weight * (uint64_t)ws[u];
          int64_t g = x >> 32 ? (int64_t)(x / (uint64_t)target) : (int64_t)((uint32_t)x / (uint32_t)target);
          g = g < 0 ? 0 : (g > O.g_bound - 1 ? O.g_bound - 1 : g);
          key = 2 * g + (ds[u] & 1);
        }
        scan_candidate(O.cand, key, (int64_t)so[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kScanU; ++u) {
      const int64_t r = r0 + tid + kPrepThreads * u;
      if (ok[u]) {
        n_wr += ws[u] >= 0;
        if (ws[u] >= 0) hsum += ws_hash((int)r);
        mx_len = max(mx_len, (uint32_t)L[u]);
        if (nc[u] > kScanLongCigar) {   // a long read: k_prep_scan_long walks it with a wave
          O.long_list[atomicAdd(O.long_count, 1u)] = (int32_t)r;
          continue;
        }
        // one walk: reference length (bam_endpos), aligned segments as walk_segments cuts them,
        // I/D ops (the indel tally's observations); the first segment for the descriptor. The query
        // offset stops advancing at the read length, as walk_segments stops there: lengths that sum
        // past 2^31 wrapped it, and the wrapped offset counted (and described) segments that
        // walk_segments never writes
        int64_t rl = 0;
        int q = 0, ns = 0, nid = 0;
        int fq = 0, fn = 0;
        int fp = 0;
        bool good = true;
        for (int k = 0; k < nc[u]; ++k) {
          const uint32_t w = k == 0 ? w0[u] : R.cigar[co[u] + k];
          const int op = (int)(w & 0xF);
          const int len = (int)(w >> 4);
          if (op > 8) { report(err, kErrCigarOp, r, op); good = false; break; }
          if (is_aligned_op(op)) {
            if (q < L[u]) {
              if (ns == 0) {
                fq = q;
                fp = (int)rl;
                fn = min(min(len, L[u] - q), kSegMaxLen);
              }
              ns += (min(len, L[u] - q) + kSegMaxLen - 1) / kSegMaxLen;
              q += len;
            }
            rl += len;
          } else if (op == 1 || op == 4) {
            q = q < L[u] ? q + len : q;
          } else if (op == 2 || op == 3) {
            rl += len;
          }
          nid += op == 1 || op == 2;
        }
        if (good && (rs[u] < 0 || rs[u] + rl > INT32_MAX)) { report(err, kErrReadPos, r); good = false; }
        if (good) {
          const int re = (int32_t)(rs[u] + (rl > 0 ? rl : 1));
          O.read_end[r] = re;
          mx_seg = max(mx_seg, (uint32_t)ns);
          n_id += (uint32_t)nid;
          if (O.xrec && ns > 1 && ns <= kFusedMaxSeg) {
            nxp |= (uint32_t)(ns - 1) << (4 * u);   // (its descriptor and extras: below)
          } else if (O.desc) {
            const uint64_t sq = 2 * (uint64_t)so[u] + (uint64_t)fq;
            const int p = (int)(rs[u] + fp);
            const int d1 = p - rs[u], d2 = re - p - fn;
            const bool wide = d1 > 15 || d2 < 0 || d2 > 15;
            const uint32_t z = (uint32_t)((sq >> 32) & 0xFF) | ((uint32_t)fn << 8) | ((uint32_t)ds[u] << 22) |
                               (wide ? kDescWide : ((uint32_t)d1 << 24) | ((uint32_t)d2 << 28));
            O.desc[r] = make_int4((int)(uint32_t)sq, p, (int)z, ws[u]);
          }
        }
      }
    }
    if (O.xrec) {
      // reads of 2..kFusedMaxSeg aligned segments (short reads with an I/D/N op): every segment as an
      // extras record, the descriptor pointing at the first. One allocation per block, from one of
      // kXStripes counters (a counter hit once per wave serialised the scan: 1.5 ms instead of 0.16
      // on c2id). The block's multi-segment reads (a few per cent) are compacted into an LDS list
      // first and walked again a lane each, all in one round (walked in place, each wave's lanes
      // took up to four dependent rounds: scan 0.28 ms instead of 0.17)
      __shared__ uint32_t xs[kWaves + 1];
      __shared__ uint32_t xq[kScanReadsPerBlock];   // (read offset in the block << 16 | first record, block-relative)
      const int lane = tid & 63, wave = tid >> 6;
      uint32_t pk = 0;   // records (bits 0-15) and multi-segment reads (bits 16-31) of this thread's reads
#pragma unroll
      for (int u = 0; u < kScanU; ++u) {
        const uint32_t nx = (nxp >> (4 * u)) & 15u;
        pk += nx ? (nx + 1) | (1u << 16) : 0u;
      }
      const uint32_t incl = (uint32_t)ganon_wave::incl_sum((int)pk);
      if (lane == 63) xs[wave] = incl;
      __syncthreads();
      uint32_t wbase = 0, btot = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        wbase += w < wave ? xs[w] : 0u;
        btot += xs[w];
      }
      uint32_t at = wbase + incl - pk;   // this thread's first record (low) and list slot (high)
#pragma unroll
      for (int u = 0; u < kScanU; ++u) {
        const uint32_t nx = (nxp >> (4 * u)) & 15u;
        if (!nx) continue;
        xq[at >> 16] = ((uint32_t)(tid + kPrepThreads * u) << 16) | (at & 0xFFFFu);
        at += (nx + 1) | (1u << 16);
      }
      const uint32_t stripe = blockIdx.x & (kXStripes - 1);
      __syncthreads();   // (every thread has read xs[0..kWaves))
      if (tid == 0) xs[kWaves] = btot ? atomicAdd(O.xcount + kXStride * stripe, btot & 0xFFFFu) : 0u;
      __syncthreads();
      // (records past the stripe's xper: the plan grows the list and scans again; a speculative run
      // is gated)
      const uint64_t s0 = (uint64_t)stripe * O.xper + xs[kWaves], s1 = (uint64_t)stripe * O.xper + O.xper;
      for (int q = tid; q < (int)(btot >> 16); q += kPrepThreads) {
        const uint32_t e = xq[q];
        const int64_t r = r0 + (e >> 16);
        const uint32_t idx = (uint32_t)(s0 + (e & 0xFFFFu));
        const int64_t co_r = R.cig_off[r], so_r = R.seq_off[r];
        const int nc_r = R.n_cig[r], L_r = R.read_len[r], rs_r = R.ref_start[r], ds_r = R.dataset[r], ws_r = R.write_scope[r];
        const uint32_t *cg = R.cigar + co_r;
        int k = 0, p0 = 0, n0 = 0;
        uint64_t sq0 = 0;
        // (the segment count is the first loop's; a stripe that overflows writes nothing past it)
        walk_segments(cg, nc_r, L_r, rs_r, cg[0], [&](int qq, int p, int n) {
          const uint64_t sq = 2 * (uint64_t)so_r + (uint64_t)qq;
          if (k == 0) {   // (the descriptor's)
            sq0 = sq;
            p0 = p;
            n0 = n;
          } else if ((uint64_t)idx + k < s1) {
            O.xrec[idx + k] = make_int4((int)(uint32_t)sq, p, (int)(((uint32_t)(sq >> 32) & 0x7F) | ((uint32_t)n << 8)), 0);
          }
          ++k;
        });
        int64_t rl = 0;   // the read's end (bam_endpos) for the header: its span is checked there
        for (int c = 0; c < nc_r; ++c) {
          const uint32_t w = cg[c];
          const int op = (int)(w & 0xF);
          if (is_aligned_op(op) || op == 2 || op == 3) rl += (int64_t)(w >> 4);
        }
        if ((uint64_t)idx < s1) O.xrec[idx] = make_int4(rs_r, (int)(rs_r + (rl > 0 ? rl : 1)), 0, 0);
        O.xidx[r] = (int32_t)idx;
        const int d1 = p0 - rs_r;
        const uint32_t z = ((uint32_t)(sq0 >> 32) & 0x7F) | kDescMulti | ((uint32_t)n0 << 8) | ((uint32_t)(ds_r & 1) << 22) |
                           (d1 > 15 ? kDescWide : (uint32_t)d1 << 24) | ((uint32_t)(k - 1) << 28);
        O.desc[r] = make_int4((int)(uint32_t)sq0, p0, (int)z, ws_r);
      }
    }
    acc[kPartWritten] = n_wr;
    acc[kPartWsHash] = hsum;
    acc[kPartMaxLen] = mx_len;
    acc[kPartMaxSeg] = mx_seg;
    acc[kPartIdOps] = n_id;
  } else {
    const int64_t s0 = (int64_t)(blockIdx.x - read_blocks) * kScanScopesPerBlock;
    const int64_t s1 = min(s0 + kScanScopesPerBlock, (int64_t)R.n_scopes);
    for (int64_t s = s0 + tid; s < s1; s += kPrepThreads) {
      const int64_t i0 = R.incid_off[s], i1 = R.incid_off[s + 1];
      if (i0 < 0 || i1 < i0 || i1 > R.n_incid) report(err, kErrScopeOff, s);
      const int64_t ss = R.span_start[s], sl = R.span_len[s];
      if (ss < 0 || sl < 0) report(err, kErrScopeSpan, s);
      if (R.ref_off[s] < 0 || R.ref_off[s] + sl > R.ref_nibs) report(err, kErrScopeRef, s);
      if (R.keep_code[s] > 15) report(err, kErrScopeKeep, s);
      acc[kPartHuge] += sl > kGrpMaxSpan;

      // the group table: every bucket from the previous scope's (exclusive) to this scope's starts
      // here (clamped: offsets are only known valid after this kernel)
      int64_t b = group_of(R.incid_off, s, weight, target, nullptr);
      int64_t bp = s == 0 ? -1 : group_of(R.incid_off, s - 1, weight, target, nullptr);
      b = min(b, O.g_bound - 1);
      bp = max(bp, (int64_t)-1);
      const longlong2 m = make_longlong2(s, i0);
      for (int64_t x = bp + 1; x <= b; ++x) O.gmeta[x] = m;
    }
  }
  block_parts(acc, O.part, O.part_stride);
}

// The long reads k_prep_scan listed (their read-level checks passed there), one wave each: read_end,
// segments, I/D ops into per-block partials after the scan's (k_prep_reduce sums both). Launched
// after the plan's synchronization found some (a second, small reduction follows): short-read
// batches never pay for it.
__global__ void __launch_bounds__(kPrepThreads) k_prep_scan_long(const Raw R, PrepErr *err, ScanOut O, int n_long) {
  unsigned long long acc[kParts] = {0, 0, 0, 0, 0, 0};
  const int64_t n_waves = (int64_t)gridDim.x * (kPrepThreads / 64);
  for (int64_t j = (blockIdx.x * (int64_t)kPrepThreads + threadIdx.x) >> 6; j < n_long; j += n_waves) {
    const int64_t r = O.long_list[j];
    const int rs_ = R.ref_start[r];
    const CigarWalk W = wave_cigar_walk(R.cigar + R.cig_off[r], R.n_cig[r], R.read_len[r]);
    if ((threadIdx.x & 63) != 0) continue;
    if (W.bad_op >= 0) {
      report(err, kErrCigarOp, r, W.bad_op);
    } else if (rs_ < 0 || rs_ + W.rl > INT32_MAX) {
      report(err, kErrReadPos, r);
    } else {
      O.read_end[r] = (int32_t)(rs_ + (W.rl > 0 ? W.rl : 1));
      if (O.nseg) O.nseg[r] = W.ns;   // (the long-read mode's segments per read: no second walk)
      acc[kPartMaxSeg] = max(acc[kPartMaxSeg], (unsigned long long)W.ns);
      acc[kPartIdOps] += (unsigned long long)W.nid;
    }
  }
  block_parts(acc, O.part, O.part_stride);
}

// plan_info: [0] I/D ops, [1] huge scopes, [2] written reads, [3] longest read, [4] most segments of
// one read, [5] short-read groups (bucket of the last scope + 1), [6] write-scope hash sum, [7] the
// run's gate: nonzero when the one-segment kernels must not run — the scan found an invalid field,
// or (speculative replan, spec_rpi > 0) the batch is not what the plan launched for: a read with
// more segments than spec_maxseg (1, or kFusedMaxSeg in the fused mode), more extras records than
// the list holds, a longer read than the overflow regions were cut for, a huge scope.
constexpr int kReduceThreads = 1024;

__global__ void __launch_bounds__(kReduceThreads) k_prep_reduce(const Raw R, const unsigned long long *__restrict__ part,
                                                                int64_t stride, int n_blocks, long long weight,
                                                                long long target, int64_t g_bound,
                                                                unsigned long long *__restrict__ info,
                                                                const PrepErr *__restrict__ err, long long spec_rpi,
                                                                const unsigned int *__restrict__ long_count,
                                                                int spec_maxseg, const unsigned int *__restrict__ xcount,
                                                                unsigned int xper) {
  // partials of one kind contiguous (block_parts): every load coalesced, 1024 threads in flight,
  // kReduceU blocks of every kind loaded per thread before any is added (a loop of dependent
  // single loads took ~50 us for configs[1]'s 11 k blocks: one HBM latency per iteration)
  constexpr int kReduceU = 8;
  unsigned long long acc[kParts] = {0, 0, 0, 0, 0, 0};
  for (int b0 = threadIdx.x; b0 < n_blocks; b0 += kReduceU * kReduceThreads) {
    unsigned long long v[kParts][kReduceU];
#pragma unroll
    for (int k = 0; k < kParts; ++k)
#pragma unroll
      for (int u = 0; u < kReduceU; ++u) {
        const int b = b0 + u * kReduceThreads;
        v[k][u] = b < n_blocks ? part[stride * k + b] : 0ull;
      }
#pragma unroll
    for (int k = 0; k < kParts; ++k)
#pragma unroll
      for (int u = 0; u < kReduceU; ++u)
        acc[k] = (k == kPartMaxLen || k == kPartMaxSeg) ? (v[k][u] > acc[k] ? v[k][u] : acc[k]) : acc[k] + v[k][u];
  }
  __shared__ unsigned long long out[kParts];
  __shared__ unsigned int xmax;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int kRW = kReduceThreads / 64;
  if (wave == 0) {   // the fullest extras stripe (fused mode; zeros otherwise)
    static_assert(kXStripes == 64, "one lane per stripe");
    unsigned int x = xcount[kXStride * lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, (unsigned int)__shfl_xor((int)x, o));
    if (lane == 0) xmax = x;
  }
  __shared__ unsigned long long ws[kRW][kParts];
#pragma unroll
  for (int k = 0; k < kParts; ++k) {
    unsigned long long v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long x = shfl64(v, lane ^ o);
      v = (k == kPartMaxLen || k == kPartMaxSeg) ? (x > v ? x : v) : v + x;
    }
    if (lane == 0) ws[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kParts) {
    const int k = threadIdx.x;
    unsigned long long v = 0;
    for (int w = 0; w < kRW; ++w)
      v = (k == kPartMaxLen || k == kPartMaxSeg) ? (ws[w][k] > v ? ws[w][k] : v) : v + ws[w][k];
    out[k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    info[0] = out[kPartIdOps];
    info[1] = out[kPartHuge];
    info[2] = out[kPartWritten];
    info[3] = out[kPartMaxLen];
    info[4] = out[kPartMaxSeg];
    info[6] = out[kPartWsHash];
    int64_t ng = 0;
    if (R.n_scopes > 0) {
      ng = group_of(R.incid_off, R.n_scopes - 1, weight, target, nullptr) + 1;
      ng = ng < 1 ? 1 : (ng > g_bound ? g_bound : ng);
    }
    info[5] = (unsigned long long)ng;
    const unsigned long long rpi = (out[kPartMaxLen] + 47) / 48;
    const bool spec_bad = spec_rpi > 0 && (out[kPartMaxSeg] > (unsigned long long)spec_maxseg ||
                                           rpi > (unsigned long long)spec_rpi || out[kPartHuge] > 0 ||
                                           *long_count > 0 || xmax > xper);
    info[7] = (err->code != 0 ? 1ull : 0ull) | (spec_bad ? 2ull : 0ull);
  }
}

// Largest j in [0, n) with off[j] <= i (off nondecreasing, off[0] <= i).
__device__ __forceinline__ int lds_upper(const long long *off, int n, long long i) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Long-read mode only: aligned segments per read (walk_segments' cuts), for the segment-weighted
// groups and the record slots — the reads of at most kScanLongCigar ops, a thread each
// (k_prep_scan_long wrote the long reads' counts during its walk).
__global__ void __launch_bounds__(kPrepThreads) k_prep_nseg(const Raw R, int32_t *__restrict__ nseg) {
  for (int64_t r = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x; r < R.n_reads; r += (int64_t)gridDim.x * kPrepThreads) {
    const int nc = R.n_cig[r];
    if (nc > kScanLongCigar) continue;
    const int L = R.read_len[r];
    const uint32_t *cg = R.cigar + R.cig_off[r];
    int q = 0, ns = 0;
    for (int k = 0; k < nc && q < L; ++k) {
      const uint32_t w = cg[k];
      const int op = (int)(w & 0xF), len = (int)(w >> 4);
      if (is_aligned_op(op)) {
        ns += (min(len, L - q) + kSegMaxLen - 1) / kSegMaxLen;
        q += len;
      } else if (op == 1 || op == 4) {
        q += len;
      }
    }
    nseg[r] = ns;
  }
}

// The write-scope sums disagreed (k_finish): name a written read its write scope does not list.
__global__ void __launch_bounds__(kPrepThreads) k_prep_ws_diag(const Raw R, PrepErr *err) {
  for (int64_t r = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x; r < R.n_reads;
       r += (int64_t)gridDim.x * kPrepThreads) {
    const int ws = R.write_scope[r];
    if (ws < 0) continue;
    int n = 0;
    for (int64_t i = R.incid_off[ws]; i < R.incid_off[ws + 1]; ++i) n += R.incid_read[i] == (int)r;
    if (n != 1) report(err, kErrWriteScopeMissing, r, ws);
  }
}

// The incidence checks of the emit paths: read index in range (before any gather through it) and
// the read inside its scope's span. False = the incidence contributes nothing (the batch is
// reported invalid).
__device__ __forceinline__ bool incid_ok(const Raw &R, const int32_t *__restrict__ read_end, PrepErr *err, int64_t i,
                                         int64_t s, int r, int ss, int se) {
  if (r < 0 || r >= R.n_reads) {
    report(err, kErrIncidRead, i, r);
    return false;
  }
  if (R.ref_start[r] < ss || read_end[r] > se) {
    report(err, kErrIncidSpan, s, r);
    return false;
  }
  return true;
}

// Long-read mode (upload): cost of scope s = its incidences' segments + weight (exclusive prefix next).
__global__ void __launch_bounds__(kPrepThreads) k_prep_scope_cost(const Raw R, const int32_t *__restrict__ nseg,
                                                                  long long weight, int64_t *__restrict__ cost) {
  for (int64_t s = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x; s <= R.n_scopes;
       s += (int64_t)gridDim.x * kPrepThreads) {
    if (s == R.n_scopes) {
      cost[s] = 0;
      continue;
    }
    int64_t c = weight;
    for (int64_t i = R.incid_off[s]; i < R.incid_off[s + 1]; ++i) {
      const int r = R.incid_read[i];
      if (r >= 0 && r < R.n_reads) c += nseg[r];
    }
    cost[s] = c;
  }
}

// gmeta[b] = (first scope of group b, its first incidence); allocation counters reset.
__global__ void __launch_bounds__(kPrepThreads) k_prep_groups(const Raw R, long long weight, long long target,
                                                              const int64_t *__restrict__ cost,
                                                              longlong2 *__restrict__ gmeta,
                                                              unsigned long long *__restrict__ cursor) {
  const int64_t gt = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x;
  if (gt < kCursors) cursor[gt] = 0;
  for (int64_t s = gt; s < R.n_scopes; s += (int64_t)gridDim.x * kPrepThreads) {
    const int64_t b = group_of(R.incid_off, s, weight, target, cost);
    const int64_t bp = s == 0 ? -1 : group_of(R.incid_off, s - 1, weight, target, cost);
    if (bp == b) continue;
    const longlong2 m = make_longlong2(s, R.incid_off[s]);
    for (int64_t x = bp + 1; x <= b; ++x) gmeta[x] = m;
  }
}

__device__ __forceinline__ int4 piece(int64_t a, int64_t b) {
  return make_int4((int)(uint32_t)a, (int)(uint32_t)((uint64_t)a >> 32), (int)(uint32_t)b,
                   (int)(uint32_t)((uint64_t)b >> 32));
}

// ---- partition pieces (no sort) --------------------------------------------------------------
// Every candidate (a group's lowest written offset in one dataset) starts a piece on its 128-byte
// line; a piece runs to the next line holding a candidate (the last one to the end of the buffer,
// the first one from 0). Several candidates on one line: the one with the largest (offset, index)
// owns it and the others get empty pieces — exactly what sorting the candidates and cutting at
// their aligned offsets gives (round 1's plan; the previous version sorted with rocPRIM). Lines
// holding a candidate are a 3-level bitmap (bit per line / per level-0 word / per level-1 word),
// so "next" and "previous" marked line are a few word loads; ties go through a small hash table
// keyed by line with a 64-bit atomicMax of (offset << 25 | candidate index).
struct LineMap {
  unsigned long long *l0, *l1, *l2;   // bit per line, per nonzero l0 word, per nonzero l1 word
  unsigned long long *hkey, *hval;    // tie table: line + 1 (0 empty), max (offset << 25 | candidate)
  int64_t n_lines, n0, n1, n2;        // lines, words per level
  int64_t hsize;                      // power of two
};

__device__ __forceinline__ unsigned long long bit_above(unsigned long long w, int b) {   // bits > b
  return b >= 63 ? 0ull : w & (~0ull << (b + 1));
}
__device__ __forceinline__ unsigned long long bit_below(unsigned long long w, int b) {   // bits < b
  return b <= 0 ? 0ull : w & (~0ull >> (64 - b));
}

// Smallest marked index > x at level `lv` words (n words), or -1.
__device__ int64_t map_next(const LineMap &M, int64_t x) {
  int64_t w = x >> 6;
  unsigned long long m = bit_above(M.l0[w], (int)(x & 63));
  if (m) return (w << 6) + __ffsll((long long)m) - 1;
  int64_t w1 = w >> 6;                      // l1 word holding bit w
  unsigned long long m1 = bit_above(M.l1[w1], (int)(w & 63));
  if (!m1) {
    int64_t w2 = w1 >> 6;
    unsigned long long m2 = bit_above(M.l2[w2], (int)(w1 & 63));
    while (!m2) {
      if (++w2 >= M.n2) return -1;
      m2 = M.l2[w2];
    }
    w1 = (w2 << 6) + __ffsll((long long)m2) - 1;
    m1 = M.l1[w1];
  }
  w = (w1 << 6) + __ffsll((long long)m1) - 1;
  return (w << 6) + __ffsll((long long)M.l0[w]) - 1;
}

// Is any index < x marked?
__device__ bool map_any_below(const LineMap &M, int64_t x) {
  int64_t w = x >> 6;
  if (bit_below(M.l0[w], (int)(x & 63))) return true;
  int64_t w1 = w >> 6;
  if (bit_below(M.l1[w1], (int)(w & 63))) return true;
  int64_t w2 = w1 >> 6;
  if (bit_below(M.l2[w2], (int)(w1 & 63))) return true;
  for (int64_t k = 0; k < w2; ++k)
    if (M.l2[k]) return true;
  return false;
}

__device__ __forceinline__ unsigned hash_line(int64_t line, int64_t hsize) {
  return (unsigned)(((uint64_t)line * 0x9E3779B97F4A7C15ull) >> 32) & (unsigned)(hsize - 1);
}

// Mark candidate c (lowest offset `key`) of the emit kernel's group.
__device__ void map_mark(const LineMap &M, unsigned long long key, uint32_t c) {
  const int64_t line = (int64_t)(key >> 7);
  atomicOr(&M.l0[line >> 6], 1ull << (line & 63));
  const unsigned long long tag = (unsigned long long)line + 1, v = (key << 25) | c;
  for (unsigned h = hash_line(line, M.hsize);; h = (h + 1) & (unsigned)(M.hsize - 1)) {
    const unsigned long long prev = atomicCAS(&M.hkey[h], 0ull, tag);
    if (prev == 0ull || prev == tag) {
      atomicMax(&M.hval[h], v);
      return;
    }
  }
}

// l1 / l2 from l0: a wave per l1 word, one l0 word per lane, the l1 word is the wave's ballot.
__global__ void __launch_bounds__(kPrepThreads) k_prep_linemap(LineMap M) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * (kPrepThreads / 64);
  for (int64_t w1 = (blockIdx.x * (int64_t)kPrepThreads + threadIdx.x) >> 6; w1 < M.n1; w1 += n_waves) {
    const int64_t w = (w1 << 6) + lane;
    const unsigned long long b = __ballot(w < M.n0 && M.l0[w] != 0);
    if (lane == 0) {
      M.l1[w1] = b;
      if (b) atomicOr(&M.l2[w1 >> 6], 1ull << (w1 & 63));
    }
  }
}

// Piece of candidate c: slot d = c & 1 of group c >> 1. No candidate at all: candidate 0 (group
// 0, dataset 0) copies the whole buffer.
__global__ void __launch_bounds__(kPrepThreads) k_prep_pieces(const unsigned long long *__restrict__ lo, int n_cand,
                                                              LineMap M, int64_t seq_bytes, int4 *__restrict__ groups,
                                                              const unsigned long long *__restrict__ gate) {
  if (gate) {   // one-segment mode: the candidates of the scan's groups only
    if (gate[7]) return;
    n_cand = (int)min((unsigned long long)n_cand, 2 * gate[5]);
  }
  for (int64_t c = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x; c < n_cand; c += (int64_t)gridDim.x * kPrepThreads) {
    const unsigned long long k = lo[c];
    int4 pc = piece(0, 0);
    if (k != kNone) {
      const int64_t line = (int64_t)(k >> 7);
      unsigned long long win = 0;
      for (unsigned h = hash_line(line, M.hsize);; h = (h + 1) & (unsigned)(M.hsize - 1))
        if (M.hkey[h] == (unsigned long long)line + 1) {
          win = M.hval[h];
          break;
        }
      if ((win & ((1ull << 25) - 1)) == (unsigned long long)c) {
        const int64_t next = map_next(M, line);
        const int64_t a = map_any_below(M, line) ? line * kPartAlign : 0;
        pc = piece(a, next < 0 ? seq_bytes : next * kPartAlign);
      }
    } else if (c == 0) {
      bool any = false;   // no candidate at all: candidate 0 copies the whole buffer
      for (int64_t w = 0; w < M.n2 && !any; ++w) any = M.l2[w] != 0;
      if (!any) pc = piece(0, seq_bytes);
    }
    groups[kGrpRec * (c >> 1) + 2 + 2 * (c & 1)] = pc;
  }
}

// Fused one-segment mode, thread per group (the scan's group bound): group records 0, 1 and 3 in
// closed form from the scan's group table (every segment slot is the incidence's own; the group
// kernel picks the reference copy per tile), the candidates the scan found (lo, line map marks),
// and a zero write-scope sum for the groups past the scan's count (the group kernel writes the
// others'); and thread per scope: whether the scope's reference span holds a non-ACGT block (its
// records then read the nt16 reference). Nothing on a gated run.
__global__ void __launch_bounds__(kPrepThreads) k_prep_cands(const Raw R, const longlong2 *__restrict__ gmeta,
                                                             int n_groups, long long region_per_incid,
                                                             const unsigned long long *__restrict__ cand,
                                                             unsigned long long *__restrict__ lo, int4 *__restrict__ groups,
                                                             LineMap M, unsigned long long *__restrict__ ws_part,
                                                             const unsigned long long *__restrict__ gate,
                                                             uint8_t *__restrict__ sdirty, const uint64_t *__restrict__ bad,
                                                             int64_t n_blk) {
  const int64_t g = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x;
  if (gate[7]) return;
  if (g < R.n_scopes) {   // (huge scopes: the tile path; slices were validated by the scan)
    const int64_t sl = R.span_len[g], ro = R.ref_off[g];
    sdirty[g] = sl > 0 && sl <= kGrpMaxSpan && !ref_clean(bad, n_blk, ro, (int)sl);
  }
  if (g >= n_groups) return;
  if ((unsigned long long)g >= gate[5]) {
    ws_part[g] = 0;
    return;
  }
  const longlong2 m0 = gmeta[g];
  const longlong2 m1 = (unsigned long long)g + 1 < gate[5] ? gmeta[g + 1] : make_longlong2(R.n_scopes, R.n_incid);
  const int s0 = (int)m0.x, s1 = (int)m1.x;
  const int64_t i0 = m0.y, i1 = m1.y;
  const int64_t region = i0 * region_per_incid + (int64_t)kGrpObs * g;
  const int cap = (int)min((i1 - i0) * region_per_incid + kGrpObs, (long long)(INT32_MAX / 2));
  groups[kGrpRec * g] = make_int4(s0, s1, (int)(uint32_t)i0, (int)(uint32_t)((uint64_t)i0 >> 32));
  groups[kGrpRec * g + 1] = make_int4((int)(uint32_t)i1, (int)(uint32_t)((uint64_t)i1 >> 32), (int)(uint32_t)i1,
                                      (int)(uint32_t)((uint64_t)i1 >> 32));
  groups[kGrpRec * g + 3] = make_int4((int)(uint32_t)region, (int)(uint32_t)((uint64_t)region >> 32), cap, 0);
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const unsigned long long c = cand[2 * g + d];
    const unsigned long long k = c ? ~c : kNone;
    lo[2 * g + d] = k;
    if (k != kNone) map_mark(M, k, (uint32_t)(2 * g + d));
  }
}

// Block-wide exclusive scan of two counters (256 threads).
__device__ __forceinline__ void block_scan2(int a, int b, int &ea, int &eb, int &ta, int &tb, int *ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int xa = __shfl_up(ia, o), xb = __shfl_up(ib, o);
    if (lane >= o) {
      ia += xa;
      ib += xb;
    }
  }
  if (lane == 63) {
    ws[wave] = ia;
    ws[kWaves + wave] = ib;
  }
  __syncthreads();
  int ba = 0, bb = 0;
  ta = tb = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int va = ws[w], vb = ws[kWaves + w];
    if (w < wave) {
      ba += va;
      bb += vb;
    }
    ta += va;
    tb += vb;
  }
  ea = ba + ia - a;
  eb = bb + ib - b;
  __syncthreads();
}

// Segment records, group records 0, 1, 3 and the partition candidates of group g.
// Pass 1 walks every incidence of the group (segments counted as clean/dirty); pass 2 writes the
// records — all-ACGT-reference segments from the front of the group's range, the others from the
// back. No global allocation in the common case: a group with at most one segment per incidence
// (every short-read group) uses the records at its own incidence indices [i0, i0 + count); a
// group with more (long reads, split CIGARs) takes its range past n_incid from one of 256
// allocation counters whose bases the upload plan fixed. Its overflow region is likewise a closed
// form of its incidence range: (i1 - i0) x ceil(longest read / 48) + 512 observations from
// i0 x ceil(longest read / 48) + 512 g. A group of at most kEmitUnroll x 256 incidences keeps
// pass 1's loads in registers and its single-segment records in LDS; larger groups walk again.
// `write` 0 (upload plan): counts and candidates only. The candidates are the lowest buffer
// offset of the reads the group writes, per dataset (every written read is "mine" in one
// incidence).
constexpr int kEmitUnroll = 2;   // incidences per thread and trip

struct EmitInc {                 // one incidence of a trip, in registers
  const uint32_t *cg;
  int64_t so;
  int r, j, ncig, L, rs, re, ds, wsc;
  uint32_t w0;
};

// What the emit kernels need for the incidence checks (incid_ok) and the write-scope marks.
struct Checks {
  const int32_t *read_end;
  unsigned long long *ws_part;   // [group] write-scope hash sum of the group's mine incidences
  PrepErr *err;
};

// The read side of a trip (needs no scope lookup: issued before the scope staging is waited for).
// An incidence whose read index is out of range is reported and dropped before any gather.
__device__ __forceinline__ void emit_load_reads(const Raw &R, const Checks &C, long long base, long long i1,
                                                EmitInc (&e)[kEmitUnroll]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int u = 0; u < kEmitUnroll; ++u) {
    const long long i = base + tid + kPrepThreads * u;
    e[u].r = i < i1 ? R.incid_read[i] : -1;
    if (i < i1 && (e[u].r < 0 || e[u].r >= R.n_reads)) {
      report(C.err, kErrIncidRead, i, e[u].r);
      e[u].r = -1;
    }
  }
#pragma unroll
  for (int u = 0; u < kEmitUnroll; ++u) {
    const int rr = e[u].r >= 0 ? e[u].r : 0;
    e[u].cg = R.cigar + R.cig_off[rr];
    e[u].ncig = e[u].r >= 0 ? R.n_cig[rr] : 0;
    e[u].L = R.read_len[rr];
    e[u].rs = R.ref_start[rr];
    e[u].re = C.read_end[rr];
    e[u].so = R.seq_off[rr];
    e[u].ds = R.dataset[rr];
    e[u].wsc = R.write_scope[rr];
  }
#pragma unroll
  for (int u = 0; u < kEmitUnroll; ++u) e[u].w0 = e[u].ncig > 0 ? e[u].cg[0] : 0u;
}

// The scope side: local scope index by binary search in the staged offsets; a read outside its
// scope's span is reported and dropped; `hsum` (if given) adds the write-scope hash of the reads met
// in their write scope; huge scopes drop out unless kept.
__device__ __forceinline__ void emit_resolve(const long long *off, const uint8_t *huge, const int *sstart,
                                             const int *send, int s0, int ns, long long base, EmitInc (&e)[kEmitUnroll],
                                             bool keep_huge, const Checks &C, unsigned long long *hsum) {
#pragma unroll
  for (int u = 0; u < kEmitUnroll; ++u) {
    e[u].j = 0;
    if (e[u].r < 0) continue;
    const int j = lds_upper(off, ns, base + threadIdx.x + kPrepThreads * u);
    e[u].j = j;
    if (e[u].rs < sstart[j] || e[u].re > send[j]) {
      report(C.err, kErrIncidSpan, s0 + j, e[u].r);
      e[u].r = -1;
      continue;
    }
    if (hsum && e[u].wsc == s0 + j) *hsum += ws_hash(e[u].r);
    if (!keep_huge && huge[j]) e[u].r = -1;
  }
}

__global__ void __launch_bounds__(kPrepThreads) k_prep_emit(const Raw R, const longlong2 *__restrict__ gmeta,
                                                            int n_groups, int write, const uint64_t *__restrict__ bad,
                                                            int64_t n_blk, long long region_per_incid, const Checks C,
                                                            int4 *__restrict__ seg4,
                                                            int4 *__restrict__ groups, unsigned long long *__restrict__ lo,
                                                            LineMap M, unsigned long long *__restrict__ cursor,
                                                            const unsigned long long *__restrict__ cursor_base) {
  __shared__ long long off[kGrpMaxScopes + 1];
  __shared__ long long ref0[kGrpMaxScopes];
  __shared__ int sstart[kGrpMaxScopes], send[kGrpMaxScopes];
  __shared__ uint8_t huge[kGrpMaxScopes];
  __shared__ int ws[2 * kWaves];
  __shared__ unsigned long long lmin[2], gbase;
  __shared__ int4 stash[kPrepThreads * kEmitUnroll];       // one-trip groups: single-segment records
  __shared__ uint8_t stash_clean[kPrepThreads * kEmitUnroll];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  const longlong2 m0 = gmeta[g];
  const longlong2 m1 = g + 1 < n_groups ? gmeta[g + 1] : make_longlong2(R.n_scopes, R.n_incid);
  const int s0 = (int)m0.x, s1 = (int)m1.x, ns = s1 - s0;   // ns <= kGrpMaxScopes (the cost weight)
  const long long i0 = m0.y, i1 = m1.y;
  for (int t = tid; t <= ns; t += kPrepThreads) off[t] = R.incid_off[s0 + t];
  for (int t = tid; t < ns; t += kPrepThreads) {
    sstart[t] = R.span_start[s0 + t];
    send[t] = R.span_start[s0 + t] + R.span_len[s0 + t];
    ref0[t] = R.ref_off[s0 + t] - R.span_start[s0 + t];
    huge[t] = R.span_len[s0 + t] > kGrpMaxSpan;
  }
  if (tid < 2) lmin[tid] = kNone;
  const bool one_trip = i1 - i0 <= (long long)kPrepThreads * kEmitUnroll;
  int cnt[kEmitUnroll];        // (one trip) segments of this thread's incidences
#pragma unroll
  for (int u = 0; u < kEmitUnroll; ++u) cnt[u] = 0;   // an empty group runs no trip
  int tot_c = 0, tot_d = 0, ec = 0, ed = 0;   // group totals; (one trip) this thread's offsets
  unsigned long long mn0 = kNone, mn1 = kNone;   // this thread's candidates
  unsigned long long hsum = 0;                    // write-scope hash of this thread's mine incidences
  // ---- pass 1: count
  for (long long base = i0; base < i1; base += kPrepThreads * kEmitUnroll) {   // uniform trip count
    EmitInc e[kEmitUnroll];
    emit_load_reads(R, C, base, i1, e);
    __syncthreads();   // (first trip: the scope staging)
    emit_resolve(off, huge, sstart, send, s0, ns, base, e, true, C, &hsum);
    int tnc = 0, tnd = 0;
#pragma unroll
    for (int u = 0; u < kEmitUnroll; ++u) {
      cnt[u] = 0;
      if (e[u].r < 0) continue;
      const EmitInc &x = e[u];
      const bool mine = x.wsc == s0 + x.j;
      if (mine && x.L > 0) {
        if (x.ds) mn1 = min(mn1, (unsigned long long)x.so);
        else mn0 = min(mn0, (unsigned long long)x.so);
      }
      if (huge[x.j]) continue;
      const uint32_t fl = ((uint32_t)x.ds << 30) | (mine ? kSegMine : 0u);
      const int64_t qnib = 2 * x.so, r0 = ref0[x.j];
      const int ss = sstart[x.j], jl = x.j;
      const int slot = tid + kPrepThreads * u;
      int &n_ = cnt[u];
      walk_segments(x.cg, x.ncig, x.L, x.rs, x.w0, [&](int q, int p, int n) {
        const uint64_t sq = (uint64_t)(qnib + q), rf = (uint64_t)(r0 + p);
        const bool clean = ref_clean(bad, n_blk, (int64_t)rf, n);
        if (n_ == 0 && one_trip) {
          const uint32_t z = (uint32_t)((sq >> 32) & 0xFF) | ((uint32_t)((rf >> 32) & 0xFF) << 8) | ((uint32_t)n << 16) | fl;
          stash[slot] = make_int4((int)(uint32_t)sq, (int)(uint32_t)rf, (int)z, (int)((uint32_t)jl | ((uint32_t)(p - ss) << 12)));
          stash_clean[slot] = clean;
        }
        ++n_;
        if (clean) ++tnc;
        else ++tnd;
      });
    }
    int tc, td;
    block_scan2(tnc, tnd, ec, ed, tc, td, ws);
    ec += tot_c;
    ed += tot_d;
    tot_c += tc;
    tot_d += td;
  }
  {
    __shared__ unsigned long long hws[kWaves];
    const unsigned long long h = block_sum_u64(hsum, hws);
    if (tid == 0) C.ws_part[g] = h;
  }
  // ---- candidates: wave reductions, one LDS atomic per wave
  for (int o = 32; o > 0; o >>= 1) {
    mn0 = min(mn0, (unsigned long long)__shfl_xor(mn0, o));
    mn1 = min(mn1, (unsigned long long)__shfl_xor(mn1, o));
  }
  if ((tid & 63) == 0) {
    if (mn0 != kNone) atomicMin(&lmin[0], mn0);
    if (mn1 != kNone) atomicMin(&lmin[1], mn1);
  }
  // ---- the group's record range: its own incidence indices, or (more segments than incidences)
  //      past n_incid from sub-counter g % kCursors
  const long long count = tot_c + tot_d;
  if (tid == 0) {
    if (count <= i1 - i0) {
      gbase = (unsigned long long)i0;
    } else {
      const int k = g % kCursors;
      gbase = (unsigned long long)R.n_incid + cursor_base[k] + atomicAdd(&cursor[k], (unsigned long long)count);
    }
  }
  __syncthreads();
  const int64_t seg_b = (int64_t)gbase, seg_e = seg_b + count;
  // ---- pass 2: write (walks again where the stash does not hold the incidence's one record)
  if (write) {
    int64_t run_c = 0, run_d = 0;
    for (long long base = i0; base < i1; base += kPrepThreads * kEmitUnroll) {
      int xc = ec, xd = ed, tc = 0, td = 0;
      int cc[kEmitUnroll], cd[kEmitUnroll];
      EmitInc e[kEmitUnroll];
      const bool reload = !one_trip || cnt[0] > 1 || cnt[1] > 1;
      if (reload) {
        emit_load_reads(R, C, base, i1, e);
        emit_resolve(off, huge, sstart, send, s0, ns, base, e, false, C, nullptr);
      }
      if (one_trip) {
#pragma unroll
        for (int u = 0; u < kEmitUnroll; ++u) {
          cc[u] = cnt[u] == 1 ? (int)stash_clean[tid + kPrepThreads * u] : 0;
          cd[u] = cnt[u] == 1 ? 1 - cc[u] : 0;
          if (cnt[u] > 1) {
            const int64_t r0 = ref0[e[u].j];
            int &c_ = cc[u], &d_ = cd[u];
            walk_segments(e[u].cg, e[u].ncig, e[u].L, e[u].rs, e[u].w0, [&](int, int p, int n) {
              if (ref_clean(bad, n_blk, r0 + p, n)) ++c_;
              else ++d_;
            });
          }
        }
      } else {
        int tnc = 0, tnd = 0;
#pragma unroll
        for (int u = 0; u < kEmitUnroll; ++u) {
          cc[u] = cd[u] = 0;
          if (e[u].r < 0) continue;
          const int64_t r0 = ref0[e[u].j];
          int &c_ = cc[u], &d_ = cd[u];
          walk_segments(e[u].cg, e[u].ncig, e[u].L, e[u].rs, e[u].w0, [&](int, int p, int n) {
            if (ref_clean(bad, n_blk, r0 + p, n)) ++c_;
            else ++d_;
          });
          tnc += c_;
          tnd += d_;
        }
        block_scan2(tnc, tnd, xc, xd, tc, td, ws);
      }
      int64_t pc = seg_b + run_c + xc, pd = seg_e - 1 - (run_d + xd);
#pragma unroll
      for (int u = 0; u < kEmitUnroll; ++u) {
        if (cc[u] + cd[u] == 0) continue;
        if (one_trip && cnt[u] == 1) {
          if (cc[u]) seg4[pc++] = stash[tid + kPrepThreads * u];
          else seg4[pd--] = stash[tid + kPrepThreads * u];
          continue;
        }
        const EmitInc &x = e[u];
        const uint32_t fl = ((uint32_t)x.ds << 30) | (x.wsc == s0 + x.j ? kSegMine : 0u);
        const int64_t qnib = 2 * x.so, r0 = ref0[x.j];
        const int ss = sstart[x.j], jl = x.j;
        walk_segments(x.cg, x.ncig, x.L, x.rs, x.w0, [&](int q, int p, int n) {
          const uint64_t sq = (uint64_t)(qnib + q), rf = (uint64_t)(r0 + p);
          const uint32_t z = (uint32_t)((sq >> 32) & 0xFF) | ((uint32_t)((rf >> 32) & 0xFF) << 8) | ((uint32_t)n << 16) | fl;
          const int4 rec = make_int4((int)(uint32_t)sq, (int)(uint32_t)rf, (int)z,
                                     (int)((uint32_t)jl | ((uint32_t)(p - ss) << 12)));
          if (ref_clean(bad, n_blk, (int64_t)rf, n)) seg4[pc++] = rec;
          else seg4[pd--] = rec;
        });
      }
      run_c += tc;
      run_d += td;
    }
  }
  if (tid < 2) {
    lo[2 * (int64_t)g + tid] = lmin[tid];
    if (lmin[tid] != kNone) map_mark(M, lmin[tid], (uint32_t)(2 * g + tid));
  }
  if (tid == 0) {
    const int64_t mid = seg_b + tot_c;
    const int64_t region = i0 * region_per_incid + (int64_t)kGrpObs * g;
    const int cap = (int)min((i1 - i0) * region_per_incid + kGrpObs, (long long)(INT32_MAX / 2));
    groups[kGrpRec * (int64_t)g] = make_int4(s0, s1, (int)(uint32_t)seg_b, (int)(uint32_t)((uint64_t)seg_b >> 32));
    groups[kGrpRec * (int64_t)g + 1] = make_int4((int)(uint32_t)seg_e, (int)(uint32_t)((uint64_t)seg_e >> 32),
                                                 (int)(uint32_t)mid, (int)(uint32_t)((uint64_t)mid >> 32));
    groups[kGrpRec * (int64_t)g + 3] = make_int4((int)(uint32_t)region, (int)(uint32_t)((uint64_t)region >> 32), cap, 0);
  }
}

// ---- one-segment mode: every read of the batch has at most one aligned segment (short reads) ----
// Each incidence owns exactly the slot of its own index, so the records need no count pass, no
// scan and no allocation: thread per incidence, one CIGAR walk, one record (an incidence without a
// segment, or in a huge scope, leaves a zero-length record the group kernel skips). A group whose
// records all have an all-ACGT reference range is read through the 2-bit reference (clean part =
// the whole range), any other group through the nt16 reference.
constexpr unsigned long long kLongReadLen = 1000;   // auto prep: long-read mode above this read length

// kFlatU: incidences per thread and trip (GANON_PARAM_PREP_UNROLL). Besides the records and group
// records 0, 1 and 3 the kernel makes the incidence checks, sums the write-scope hashes of the
// reads met in their write scope and marks the group's partition candidates (the lowest buffer
// offset of the reads it writes, per dataset) in the line map.
template <int kFlatU>
__global__ void __launch_bounds__(kPrepThreads) k_prep_emit_flat(const Raw R, const longlong2 *__restrict__ gmeta,
                                                                 int n_groups, const uint64_t *__restrict__ bad,
                                                                 int64_t n_blk, long long region_per_incid,
                                                                 const Checks C, int4 *__restrict__ seg4,
                                                                 int4 *__restrict__ groups,
                                                                 unsigned long long *__restrict__ lo, LineMap M,
                                                                 const unsigned long long *__restrict__ gate) {
  __shared__ long long off[kGrpMaxScopes + 1];
  __shared__ long long ref0[kGrpMaxScopes];
  __shared__ int sstart[kGrpMaxScopes], send[kGrpMaxScopes];
  __shared__ uint8_t huge[kGrpMaxScopes];
  __shared__ int s_dirty;
  __shared__ unsigned long long lmin[2];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  // launched for the group bound: past the scan's group count (gate[5]) a block only clears its
  // write-scope sum; nothing runs on a batch the scan rejected (gate[7])
  if (gate[7]) return;
  if ((unsigned long long)g >= gate[5]) {
    if (tid == 0) C.ws_part[g] = 0;
    return;
  }
  const longlong2 m0 = gmeta[g];
  const longlong2 m1 = (unsigned long long)g + 1 < gate[5] ? gmeta[g + 1] : make_longlong2(R.n_scopes, R.n_incid);
  const int s0 = (int)m0.x, s1 = (int)m1.x, ns = s1 - s0;
  const long long i0 = m0.y, i1 = m1.y;
  for (int t = tid; t <= ns; t += kPrepThreads) off[t] = R.incid_off[s0 + t];
  for (int t = tid; t < ns; t += kPrepThreads) {
    sstart[t] = R.span_start[s0 + t];
    send[t] = R.span_start[s0 + t] + R.span_len[s0 + t];
    ref0[t] = R.ref_off[s0 + t] - R.span_start[s0 + t];
    huge[t] = R.span_len[s0 + t] > kGrpMaxSpan;
  }
  if (tid == 0) s_dirty = 0;
  if (tid < 2) lmin[tid] = kNone;
  __syncthreads();
  bool dirty = false;
  unsigned long long hsum = 0, mn0 = kNone, mn1 = kNone;
  // kFlatU incidences per thread and trip, their loads issued together (the chain incidence -> read
  // fields -> CIGAR -> reference block bitmap is latency bound)
  for (long long base = i0; base < i1; base += kFlatU * kPrepThreads) {
    EmitInc e[kFlatU];
    int jj[kFlatU];
#pragma unroll
    for (int u = 0; u < kFlatU; ++u) {
      const long long i = base + tid + kPrepThreads * u;
      e[u].r = i < i1 ? R.incid_read[i] : -1;
      if (i < i1 && (e[u].r < 0 || e[u].r >= R.n_reads)) {
        report(C.err, kErrIncidRead, i, e[u].r);
        e[u].r = -2;   // in range of the group, no read: a zero-length record
      }
    }
#pragma unroll
    for (int u = 0; u < kFlatU; ++u) {
      const int rr = e[u].r >= 0 ? e[u].r : 0;
      e[u].cg = R.cigar + R.cig_off[rr];
      e[u].ncig = e[u].r >= 0 ? R.n_cig[rr] : 0;
      e[u].L = R.read_len[rr];
      e[u].rs = R.ref_start[rr];
      e[u].re = C.read_end[rr];
      e[u].so = R.seq_off[rr];
      e[u].ds = R.dataset[rr];
      e[u].wsc = R.write_scope[rr];
      jj[u] = lds_upper(off, ns, base + tid + kPrepThreads * u);
    }
#pragma unroll
    for (int u = 0; u < kFlatU; ++u) e[u].w0 = e[u].ncig > 0 ? e[u].cg[0] : 0u;
#pragma unroll
    for (int u = 0; u < kFlatU; ++u) {
      if (e[u].r == -1) continue;   // past the group
      const EmitInc &x = e[u];
      const int j = jj[u];
      int4 rec = make_int4(0, 0, 0, j);   // zero-length: no chunks
      bool ok = x.r >= 0;
      if (ok && (x.rs < sstart[j] || x.re > send[j])) {
        report(C.err, kErrIncidSpan, s0 + j, x.r);
        ok = false;
      }
      const bool mine = ok && x.wsc == s0 + j;
      if (mine) {
        hsum += ws_hash(x.r);
        if (x.L > 0) {
          if (x.ds) mn1 = min(mn1, (unsigned long long)x.so);
          else mn0 = min(mn0, (unsigned long long)x.so);
        }
      }
      if (ok && !huge[j]) {
        const uint32_t fl = ((uint32_t)x.ds << 30) | (mine ? kSegMine : 0u);
        const int64_t qnib = 2 * x.so, r0 = ref0[j];
        const int ss = sstart[j];
        walk_segments(x.cg, x.ncig, x.L, x.rs, x.w0, [&](int q, int p, int n) {
          const uint64_t sq = (uint64_t)(qnib + q), rf = (uint64_t)(r0 + p);
          const uint32_t z = (uint32_t)((sq >> 32) & 0xFF) | ((uint32_t)((rf >> 32) & 0xFF) << 8) | ((uint32_t)n << 16) | fl;
          rec = make_int4((int)(uint32_t)sq, (int)(uint32_t)rf, (int)z, (int)((uint32_t)j | ((uint32_t)(p - ss) << 12)));
          dirty |= !ref_clean(bad, n_blk, (int64_t)rf, n);
        });
      }
      seg4[base + tid + kPrepThreads * u] = rec;
    }
  }
  if (__any(dirty) && (tid & 63) == 0) s_dirty = 1;
  for (int o = 32; o > 0; o >>= 1) {
    mn0 = min(mn0, (unsigned long long)__shfl_xor(mn0, o));
    mn1 = min(mn1, (unsigned long long)__shfl_xor(mn1, o));
  }
  if ((tid & 63) == 0) {
    if (mn0 != kNone) atomicMin(&lmin[0], mn0);
    if (mn1 != kNone) atomicMin(&lmin[1], mn1);
  }
  __shared__ unsigned long long hws[kWaves];
  const unsigned long long h = block_sum_u64(hsum, hws);   // (its barriers order s_dirty and lmin too)
  if (tid < 2) {
    lo[2 * (int64_t)g + tid] = lmin[tid];
    if (lmin[tid] != kNone) map_mark(M, lmin[tid], (uint32_t)(2 * g + tid));
  }
  if (tid == 0) {
    C.ws_part[g] = h;
    const int64_t seg_b = i0, seg_e = i1, mid = s_dirty ? seg_b : seg_e;
    const int64_t region = i0 * region_per_incid + (int64_t)kGrpObs * g;
    const int cap = (int)min((i1 - i0) * region_per_incid + kGrpObs, (long long)(INT32_MAX / 2));
    groups[kGrpRec * (int64_t)g] = make_int4(s0, s1, (int)(uint32_t)seg_b, (int)(uint32_t)((uint64_t)seg_b >> 32));
    groups[kGrpRec * (int64_t)g + 1] = make_int4((int)(uint32_t)seg_e, (int)(uint32_t)((uint64_t)seg_e >> 32),
                                                 (int)(uint32_t)mid, (int)(uint32_t)((uint64_t)mid >> 32));
    groups[kGrpRec * (int64_t)g + 3] = make_int4((int)(uint32_t)region, (int)(uint32_t)((uint64_t)region >> 32), cap, 0);
  }
}

// ---- long-read mode: segment records once per read -------------------------------------------
// A 10-100 kb read with 5 % indel errors has thousands of aligned segments, and it sits in several
// scopes (windows every 10 kb): round 3 wrote its records once per (scope, read) incidence, ~4x the
// read's own (1.8 GB per C5 batch of 20 k reads), and the group kernel read them back. The records
// do not depend on the scope except through its reference offset, span start and write mark, so
// they are written once per read here (b_rrec, read records) and the group kernel adds those
// fields when it stages a tile (grp_tile_long). One wave walks a read 64 CIGAR ops at a time:
// per-lane query / reference deltas, wave prefix sums for each op's (q, p), the read-length clip
// (ops at or past the read length give nothing, as walk_segments stops there), per-lane pieces of
// kSegMaxLen and a wave prefix of the piece counts — deterministic slots from b_rbase (the
// exclusive prefix of the segments per read), no atomics.
__global__ void __launch_bounds__(kPrepThreads) k_prep_read_recs(const Raw R, const int64_t *__restrict__ rbase,
                                                                 int4 *__restrict__ rrec) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (blockIdx.x * (int64_t)kPrepThreads + threadIdx.x) >> 6; r < R.n_reads; r += nw) {
    const int nc = R.n_cig[r], L = R.read_len[r];
    const int64_t co = R.cig_off[r];
    const uint32_t fl = (uint32_t)R.dataset[r] << 30;
    const int64_t qnib = 2 * R.seq_off[r];
    int q = 0, p = R.ref_start[r];   // carries (wave-uniform)
    int64_t slot = rbase[r];
    for (int base = 0; base < nc && q < L; base += 64) {
      const int k = base + lane;
      const uint32_t w = k < nc ? R.cigar[co + k] : 0u;
      const int op = (int)(w & 0xF), len = (int)(w >> 4);
      const bool al = is_aligned_op(op);
      // (query deltas capped at L < 2^24: 64 of them cannot wrap the prefix sum, and an op at or past
      // L gives nothing either way; the reference deltas sum to at most INT32_MAX: the scan's check)
      const int dq = (al || op == 1 || op == 4) ? min(len, L) : 0;
      const int dp = (al || op == 2 || op == 3) ? len : 0;
      const int iq = ganon_wave::incl_sum(dq), ip = ganon_wave::incl_sum(dp);
      const int q0 = q + iq - dq, p0 = p + ip - dp;
      const int n = (al && q0 < L) ? min(len, L - q0) : 0;
      const int c = (n + kSegMaxLen - 1) / kSegMaxLen;   // pieces
      const int ic = ganon_wave::incl_sum(c);
      int64_t pc = slot + ic - c;
      for (int o = 0; o < n; o += kSegMaxLen) {
        const int m = min(kSegMaxLen, n - o);
        const uint64_t sq = (uint64_t)(qnib + q0 + o);
        rrec[pc++] = make_int4((int)(uint32_t)sq, p0 + o, (int)((uint32_t)((sq >> 32) & 0xFF) | ((uint32_t)m << 16) | fl), 0);
      }
      slot += ganon_wave::last(ic);
      q += ganon_wave::last(iq);
      p += ganon_wave::last(ip);
    }
  }
}

// Long-read mode, per group (thread per group): each incidence's first slot in the group's slot
// space (the segments of the group's earlier incidences; no walk: the segments per read), scope and
// write mark and its read's record base (incidence records, b_inc4), the incidence checks, the
// group records (slot range, first incidence and count, overflow region), the candidates, the
// write-scope hash sum, and per scope whether its reference span holds a non-ACGT block.
// Long-read groups hold few incidences.
__global__ void __launch_bounds__(kPrepThreads) k_prep_long_groups(const Raw R, const longlong2 *__restrict__ gmeta,
                                                                   int n_groups, long long region_per_incid,
                                                                   const int32_t *__restrict__ nseg,
                                                                   const int64_t *__restrict__ rbase,
                                                                   int4 *__restrict__ groups,
                                                                   unsigned long long *__restrict__ lo, LineMap M,
                                                                   int4 *__restrict__ inc4, uint8_t *__restrict__ sdirty,
                                                                   const uint64_t *__restrict__ bad, int64_t n_blk,
                                                                   const Checks C) {
  for (int64_t g = blockIdx.x * (int64_t)kPrepThreads + threadIdx.x; g < n_groups;
       g += (int64_t)gridDim.x * kPrepThreads) {
    const longlong2 m0 = gmeta[g];
    const longlong2 m1 = g + 1 < n_groups ? gmeta[g + 1] : make_longlong2(R.n_scopes, R.n_incid);
    const int s0 = (int)m0.x, s1 = (int)m1.x;
    const long long i0 = m0.y, i1 = m1.y;
    unsigned long long count = 0, mn[2] = {kNone, kNone}, hsum = 0;
    for (int s = s0; s < s1; ++s) {
      const int ss = R.span_start[s], sl = R.span_len[s], se = ss + sl;
      const bool big = sl > kGrpMaxSpan;   // huge scope: tile path
      sdirty[s] = !big && sl > 0 && !ref_clean(bad, n_blk, R.ref_off[s], sl);
      for (int64_t i = R.incid_off[s]; i < R.incid_off[s + 1]; ++i) {
        const int r = R.incid_read[i];
        const bool ok = incid_ok(R, C.read_end, C.err, i, s, r, ss, se);
        const bool mine = ok && R.write_scope[r] == s;
        const int64_t rb = ok ? rbase[r] : 0;
        inc4[i] = make_int4((int)count, (int)((uint32_t)(s - s0) | (mine ? kSegMine : 0u)), (int)(uint32_t)rb,
                            (int)(uint32_t)((uint64_t)rb >> 32));
        if (!ok) continue;
        if (mine) hsum += ws_hash(r);
        if (big) continue;
        count += (unsigned long long)nseg[r];
        if (mine && R.read_len[r] > 0) {
          const int d = R.dataset[r];
          mn[d] = min(mn[d], (unsigned long long)R.seq_off[r]);
        }
      }
    }
    for (int d = 0; d < 2; ++d) {
      lo[2 * g + d] = mn[d];
      if (mn[d] != kNone) map_mark(M, mn[d], (uint32_t)(2 * g + d));
    }
    const int64_t region = i0 * region_per_incid + (int64_t)kGrpObs * g;
    const int cap = (int)min((i1 - i0) * region_per_incid + kGrpObs, (long long)(INT32_MAX / 2));
    groups[kGrpRec * g] = make_int4(s0, s1, 0, 0);
    groups[kGrpRec * g + 1] = make_int4((int)(uint32_t)count, (int)(uint32_t)(count >> 32), (int)(uint32_t)i0,
                                        (int)(uint32_t)((uint64_t)i0 >> 32));
    groups[kGrpRec * g + 3] = make_int4((int)(uint32_t)region, (int)(uint32_t)((uint64_t)region >> 32), cap,
                                        (int)(i1 - i0));
    C.ws_part[g] = hsum;
  }
}

Raw raw_of(const ganon_dbatch *db) {
  const DevBatch &B = db->B;
  Raw R;
  R.ref_start = B.ref_start;
  R.read_len = B.read_len;
  R.n_cig = B.n_cig;
  R.write_scope = B.write_scope;
  R.seq_off = B.seq_off;
  R.cig_off = B.cig_off;
  R.dataset = B.dataset;
  R.cigar = B.cigar;
  R.incid_off = B.incid_off;
  R.incid_read = B.incid_read;
  R.span_start = B.span_start;
  R.span_len = B.span_len;
  R.ref_off = B.ref_off;
  R.keep_code = B.keep_code;
  R.n_reads = db->n_reads;
  R.n_scopes = db->n_scopes;
  R.n_incid = db->n_incid;
  R.seq_bytes = db->seq_bytes;
  R.n_cigar_ops = db->n_cigar_ops;
  R.ref_nibs = 2 * db->ref->bytes;
  return R;
}

unsigned grid_for(int64_t n, int64_t cap = 16384) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kPrepThreads - 1) / kPrepThreads, cap));
}

long long weight_of(int target) { return (target + kGrpMaxScopes - 2) / (kGrpMaxScopes - 1); }

const char *err_text(int kind) {
  switch (kind) {
    case kErrReadSeq: return "read %lld: sequence out of range";
    case kErrReadCigar: return "read %lld: cigar out of range";
    case kErrReadDataset: return "read %lld: dataset must be 0 or 1";
    case kErrReadWriteScope: return "read %lld: write_scope %lld out of range";
    case kErrReadLong: return "read %lld longer than 16 Mb";
    case kErrCigarOp: return "read %lld: bad cigar op %lld";
    case kErrReadPos: return "read %lld: bad position";
    case kErrScopeOff: return "scope %lld: incidence offsets decreasing or out of range";
    case kErrScopeSpan: return "scope %lld: bad span";
    case kErrScopeRef: return "scope %lld: reference slice out of range";
    case kErrScopeKeep: return "scope %lld: keep_code > 15";
    case kErrIncidRead: return "incidence %lld: read %lld out of range";
    case kErrIncidSpan: return "scope %lld: read %lld outside its span";
    case kErrWriteScopeMissing: return "read %lld: write_scope %lld does not list it exactly once";
    default: return "invalid batch (%lld)";
  }
}

// The line map over the batch's output buffer (b_linemap: l0 | l1 | l2 | hash keys | hash values).
LineMap line_map(const ganon_dbatch *db) {
  LineMap M;
  M.n_lines = std::max<int64_t>(1, (db->seq_bytes + kPartAlign - 1) / kPartAlign);
  M.n0 = (M.n_lines + 63) / 64;
  M.n1 = (M.n0 + 63) / 64;
  M.n2 = (M.n1 + 63) / 64;
  int64_t h = 64;
  while (h < 4 * 2 * (int64_t)db->n_groups) h <<= 1;
  M.hsize = h;
  auto *base = static_cast<unsigned long long *>(db->b_linemap.p);
  M.l0 = base;
  M.l1 = M.l0 + M.n0;
  M.l2 = M.l1 + M.n1;
  M.hkey = M.l2 + M.n2;
  M.hval = M.hkey + M.hsize;
  return M;
}

int64_t line_map_words(const ganon_dbatch *db) {
  const LineMap M = line_map(db);
  return M.n0 + M.n1 + M.n2 + 2 * M.hsize;
}

Checks checks_of(const ganon_dbatch *db) {
  return Checks{db->B.read_end, static_cast<unsigned long long *>(db->b_wspart.p), db->err};
}

int launch_groups(ganon_ctx *ctx, ganon_dbatch *db, const Raw &R) {
  KernelScope ks(ctx, "prep_groups");
  if (db->n_groups)   // the line map, marked by the emit kernel
    HIP_OR_FAIL(hipMemsetAsync(db->b_linemap.p, 0, (size_t)line_map_words(db) * 8, ctx->stream));
  hipLaunchKernelGGL(k_prep_groups, dim3(grid_for(std::max<int64_t>(db->n_scopes, kCursors))), dim3(kPrepThreads), 0,
                     ctx->stream, R, weight_of(db->group_target), (long long)db->group_target,
                     db->long_mode ? db->scost : nullptr, static_cast<longlong2 *>(db->b_gs0.p), db->cursor);
  return check_launch(ctx, "k_prep_groups");
}

int launch_emit(ganon_ctx *ctx, ganon_dbatch *db, const Raw &R, int write) {
  if (!db->n_groups) return GANON_OK;
  KernelScope ks(ctx, "prep_emit");
  if (db->long_mode) {
    // (write 0: the plan's counting pass is not needed in this mode)
    if (!write) return GANON_OK;
    hipLaunchKernelGGL(k_prep_long_groups, dim3(grid_for(db->n_groups)), dim3(kPrepThreads), 0, ctx->stream, R,
                       static_cast<const longlong2 *>(db->b_gs0.p), db->n_groups, (long long)db->region_per_incid,
                       static_cast<const int32_t *>(db->b_nseg.p), static_cast<const int64_t *>(db->b_rbase.p),
                       static_cast<int4 *>(db->b_groups.p), static_cast<unsigned long long *>(db->b_lo.p), line_map(db),
                       static_cast<int4 *>(db->b_inc4.p), static_cast<uint8_t *>(db->b_sdirty.p), db->ref->bad,
                       db->ref->n_blk, checks_of(db));
    hipLaunchKernelGGL(k_prep_read_recs, dim3(grid_for(db->n_reads * 64)), dim3(kPrepThreads), 0, ctx->stream, R,
                       static_cast<const int64_t *>(db->b_rbase.p), static_cast<int4 *>(db->b_rrec.p));
    return check_launch(ctx, "k_prep_long_groups / k_prep_read_recs");
  }
  if (db->flat_mode) {
    auto flat = ctx->prep_unroll == 4 ? k_prep_emit_flat<4> : ctx->prep_unroll == 1 ? k_prep_emit_flat<1>
                                                                                   : k_prep_emit_flat<2>;
    hipLaunchKernelGGL(flat, dim3((unsigned)db->n_groups), dim3(kPrepThreads), 0, ctx->stream, R,
                       static_cast<const longlong2 *>(db->b_gs0.p), db->n_groups, db->ref->bad, db->ref->n_blk,
                       (long long)db->region_per_incid, checks_of(db), static_cast<int4 *>(db->b_seg4.p),
                       static_cast<int4 *>(db->b_groups.p), static_cast<unsigned long long *>(db->b_lo.p),
                       line_map(db), static_cast<const unsigned long long *>(db->plan_info));
    return check_launch(ctx, "k_prep_emit_flat");
  }
  hipLaunchKernelGGL(k_prep_emit, dim3((unsigned)db->n_groups), dim3(kPrepThreads), 0, ctx->stream, R,
                     static_cast<const longlong2 *>(db->b_gs0.p), db->n_groups, write, db->ref->bad, db->ref->n_blk,
                     (long long)db->region_per_incid, checks_of(db), static_cast<int4 *>(db->b_seg4.p), static_cast<int4 *>(db->b_groups.p),
                     static_cast<unsigned long long *>(db->b_lo.p), line_map(db), db->cursor, db->cursor + kCursors);
  return check_launch(ctx, "k_prep_emit");
}

// Launch order of the group kernel. A scope with more incidences than the group target is a group
// of its own — at 60x coverage up to ~12x the others (8 k incidences against 704) — and
// in scope order such a group can start among the last and run on alone at the end. When a group
// costs more than twice the target, order[] lists the groups by descending cost in power-of-two
// classes (longest processing time first; the empty groups of skipped buckets and the blocks past
// the scan's count last); else order[0] = -1 and the blocks run in group order. Two passes over the
// group table (just written: L2), a block per 256 groups, no atomics outside LDS and no memset:
// per-block class counts, then every block finds its classes' offsets from all blocks' counts and
// scatters its groups. Launched only for batches that can hold such a group (launch_pieces).
constexpr int kOrderThreads = 256;
constexpr int kOrderClasses = 32;
constexpr int kOrderRow = kOrderClasses + 1;   // per-block row: class counts, then the block's max cost

// class of a group: the big ones (over twice the target) by power of two, longest first; every other
// group in one class, so that those keep their neighbours (the partition copies and the reference
// lines of consecutive groups are adjacent); the empty ones last
__device__ __forceinline__ int order_class(long long c, long long target) {
  if (c <= 0) return kOrderClasses - 1;
  if (c <= 2 * target) return kOrderClasses - 2;
  const int lg = 63 - __clzll((long long)(c / (2 * target)));   // 0 .. : twice the target << lg
  return kOrderClasses - 3 - min(lg, kOrderClasses - 3);
}

__device__ __forceinline__ long long order_cost(const int4 *__restrict__ groups, int64_t g, int64_t ng) {
  if (g >= ng) return 0;
  const int4 a = groups[kGrpRec * g], b = groups[kGrpRec * g + 1];
  const int64_t end = (int64_t)(uint32_t)b.x | ((int64_t)b.y << 32), beg = (int64_t)(uint32_t)a.z | ((int64_t)a.w << 32);
  return end - beg;
}

__device__ __forceinline__ int64_t order_groups(const unsigned long long *__restrict__ gate, int64_t n_groups) {
  return gate ? (gate[7] ? 0 : min(n_groups, (int64_t)gate[5])) : n_groups;
}

__global__ void __launch_bounds__(kOrderThreads) k_prep_order_count(const int4 *__restrict__ groups, int64_t n_groups,
                                                                     const unsigned long long *__restrict__ gate,
                                                                     long long target, uint32_t *__restrict__ rows) {
  __shared__ unsigned int hist[kOrderClasses];
  __shared__ unsigned int bmax;
  const int t = threadIdx.x;
  const int64_t ng = order_groups(gate, n_groups);
  if (t < kOrderClasses) hist[t] = 0;
  if (t == 0) bmax = 0;
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * kOrderThreads + t;
  if (g < n_groups) {
    const long long c = order_cost(groups, g, ng);
    atomicAdd(&hist[order_class(c, target)], 1u);
    atomicMax(&bmax, (unsigned int)min(c, (long long)UINT32_MAX));
  }
  __syncthreads();
  if (t < kOrderClasses) rows[(int64_t)blockIdx.x * kOrderRow + t] = hist[t];
  if (t == 0) rows[(int64_t)blockIdx.x * kOrderRow + kOrderClasses] = bmax;
}

__global__ void __launch_bounds__(kOrderThreads) k_prep_order_scatter(const int4 *__restrict__ groups, int64_t n_groups,
                                                                       const unsigned long long *__restrict__ gate,
                                                                       long long target, const uint32_t *__restrict__ rows,
                                                                       int n_blocks, int32_t *__restrict__ order) {
  __shared__ unsigned int tot[kOrderClasses], pre[kOrderClasses];
  __shared__ unsigned int gmax;
  const int t = threadIdx.x;
  const int64_t ng = order_groups(gate, n_groups);
  // column t of the per-block rows (classes, then the largest cost): all blocks' sum / max and the
  // sum over the blocks before this one; independent loads, eight in flight
  if (t <= kOrderClasses) {
    unsigned int all = 0, before = 0;
    const int me = (int)blockIdx.x;
#pragma unroll 8
    for (int k = 0; k < n_blocks; ++k) {
      const unsigned int v = rows[(int64_t)k * kOrderRow + t];
      if (t == kOrderClasses) {
        all = max(all, v);
      } else {
        all += v;
        before += k < me ? v : 0u;
      }
    }
    if (t == kOrderClasses) {
      gmax = all;
    } else {
      tot[t] = all;
      pre[t] = before;
    }
  }
  __syncthreads();
  if ((long long)gmax <= 2 * target) {
    if (blockIdx.x == 0 && t == 0) order[0] = -1;
    return;
  }
  if (t == 0) {
    unsigned int run = 0;
    for (int k = 0; k < kOrderClasses; ++k) {
      pre[k] += run;
      run += tot[k];
    }
  }
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * kOrderThreads + t;
  if (g < n_groups) order[atomicAdd(&pre[order_class(order_cost(groups, g, ng), target)], 1u)] = (int32_t)g;
}

int launch_pieces(ganon_ctx *ctx, ganon_dbatch *db) {
  hipStream_t st = ctx->stream;
  const int n_cand = 2 * db->n_groups;
  if (!db->n_groups) return GANON_OK;
  KernelScope ks(ctx, "prep_pieces");
  const LineMap M = line_map(db);
  hipLaunchKernelGGL(k_prep_linemap, dim3(grid_for(M.n1 * 64)), dim3(kPrepThreads), 0, st, M);
  hipLaunchKernelGGL(k_prep_pieces, dim3(grid_for(n_cand)), dim3(kPrepThreads), 0, st,
                     static_cast<const unsigned long long *>(db->b_lo.p), n_cand, M, db->seq_bytes,
                     static_cast<int4 *>(db->b_groups.p), db->flat_mode ? db->plan_info : nullptr);
  // launch order (k_prep_order_*): long reads, or a scope with more than twice the target's
  // incidences (the host's count at load); otherwise the group kernel runs in group order
  db->ordered = db->long_mode || db->max_scope_incid > 2 * (int64_t)db->group_target;
  if (db->ordered) {
    const int nb = (int)((db->n_groups + kOrderThreads - 1) / kOrderThreads);
    const int4 *g = static_cast<const int4 *>(db->b_groups.p);
    const unsigned long long *gate = db->flat_mode ? db->plan_info : nullptr;
    uint32_t *rows = static_cast<uint32_t *>(db->b_order.p) + (size_t)db->n_groups + 1;
    hipLaunchKernelGGL(k_prep_order_count, dim3(nb), dim3(kOrderThreads), 0, st, g, (int64_t)db->n_groups, gate,
                       (long long)db->group_target, rows);
    hipLaunchKernelGGL(k_prep_order_scatter, dim3(nb), dim3(kOrderThreads), 0, st, g, (int64_t)db->n_groups, gate,
                       (long long)db->group_target, rows, nb, static_cast<int32_t *>(db->b_order.p));
  }
  return check_launch(ctx, "k_prep_pieces");
}

}  // namespace

namespace ganon_prep {

int grow(ganon_ctx *ctx, DBuf &b, size_t bytes) {
  const size_t need = bytes + 128;
  if (b.p && b.bytes >= need) return GANON_OK;
  const size_t old = b.bytes;
  if (b.p) {
    ganon_detail::sync_stream(ctx->stream);   // a previous run may still read it
    hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
  }
  const size_t alloc = std::max(need, old + old / 4);   // some headroom for reloads
  hipError_t e = hipMalloc(&b.p, alloc);
  if (e != hipSuccess) {
    b.p = nullptr;
    return fail(ctx, GANON_E_NOMEM, "hipMalloc(%zu) failed: %s", alloc, hipGetErrorString(e));
  }
  b.bytes = alloc;
  return GANON_OK;
}

// Buffers of a plan with ng scope groups (the full plan once it knows the shape; a speculative plan
// of new counts from the shape it assumes).
int size_plan(ganon_ctx *ctx, ganon_dbatch *db, int64_t ng, int tgt0, const Raw &R) {
  hipStream_t st = ctx->stream;
  int rc;
  longlong2 *gm = nullptr;
  if (ng > INT32_MAX / kGrpRec) return fail(ctx, GANON_E_ARG, "batch too large: %lld scope groups", (long long)ng);
  db->n_groups = (int32_t)ng;
  int32_t *p32 = nullptr;
  int4 *grp = nullptr;
  unsigned long long *u64 = nullptr;
  uint32_t *u32 = nullptr;
  // (short-read modes: ng <= g_bound, so the scan's group table stays in place)
  if ((rc = grow_n(ctx, db->b_gs0, (size_t)std::max<int64_t>(ng, 1), &gm)) ||
      (rc = grow_n(ctx, db->b_groups, (size_t)kGrpRec * ng, &grp)) ||
      (rc = grow_n(ctx, db->b_grp_part, 2 * (size_t)ng, &p32)) ||
      (rc = grow_n(ctx, db->b_order, (size_t)ng + 1 + (size_t)kOrderRow * ((ng + kOrderThreads - 1) / kOrderThreads),
                   &p32)) ||
      (rc = grow_n(ctx, db->b_wspart, (size_t)std::max<int64_t>(ng, 1), &u64)) ||
      (rc = grow_n(ctx, db->b_lo, 2 * (size_t)std::max<int64_t>(ng, 1), &u64)) ||
      (rc = grow_n(ctx, db->b_linemap, (size_t)line_map_words(db), &u64)))
    return rc;
  int64_t extra_seg = 0;
  if (!db->flat_mode && !db->long_mode && ng) {
    // two-pass emit: a counting pass sizes the records of groups with more segments than
    // incidences (sub-counter bases: exclusive prefix of the pass's totals, deterministic); the
    // long-read mode keeps its records per read (b_rrec, sized by the plan)
    HIP_OR_FAIL(hipMemsetAsync(db->cursor + kCursors, 0, kCursors * sizeof(unsigned long long), st));
    if ((rc = launch_groups(ctx, db, R)) || (rc = launch_emit(ctx, db, R, 0))) return rc;
    std::vector<unsigned long long> cur(2 * kCursors, 0);
    HIP_OR_FAIL(ganon_detail::readback(cur.data(), db->cursor, kCursors * sizeof(unsigned long long), st));
    HIP_OR_FAIL(ganon_detail::sync_stream(st));
    unsigned long long tseg = 0;
    for (int k = 0; k < kCursors; ++k) {
      cur[kCursors + k] = tseg;
      tseg += cur[k];
    }
    db->cursor_h.assign(cur.begin() + kCursors, cur.end());
    HIP_OR_FAIL(hipMemcpyAsync(db->cursor + kCursors, db->cursor_h.data(), kCursors * sizeof(unsigned long long),
                               hipMemcpyHostToDevice, st));
    extra_seg = (int64_t)tseg;
  }
  db->n_seg = db->long_mode ? db->n_long_seg : db->n_incid + extra_seg;   // record slots (long: virtual)
  db->region = db->n_incid * db->region_per_incid + (int64_t)kGrpObs * ng;
  // far masks (bytes a group masks outside its own pieces, applied by k_finish): the list keeps its
  // capacity across batches; a run that needs more reports the count (k_finish) and
  // ganon_batch_download grows the list and runs again — no counting pass, no synchronization here
  const int64_t far_want = ctx->far_init > 0 ? (int64_t)ctx->far_init
                                             : std::min<int64_t>(kFarMax, std::max<int64_t>(int64_t(1) << 16, db->n_reads / 8));
  db->far_cap = std::max<int64_t>(db->far_cap_alloc, far_want);
  int4 *s4 = nullptr;
  // (fused one-segment and long-read modes: no per-incidence records in HBM)
  if ((rc = grow_n(ctx, db->b_seg4, db->fused || db->long_mode ? 1 : (size_t)std::max<int64_t>(db->n_seg, 1), &s4)))
    return rc;
  if ((rc = grow_n(ctx, db->b_far, (size_t)db->far_cap, &u64))) return rc;
  db->far_cap_alloc = db->far_cap;
  if ((rc = grow_n(ctx, db->b_gokey, (size_t)db->region, &u64)) || (rc = grow_n(ctx, db->b_gopay, (size_t)db->region, &u64)) ||
      (rc = grow_n(ctx, db->b_gtkey, 2 * (size_t)db->region + 64, &u64)) ||
      (rc = grow_n(ctx, db->b_gtflag, 2 * (size_t)db->region + 64, &u32)))
    return rc;
  db->spec_ready = db->flat_mode && db->n_huge_scopes == 0;
  db->spec_sizes[0] = db->n_reads;
  db->spec_sizes[1] = db->n_scopes;
  db->spec_sizes[2] = db->n_incid;
  db->spec_sizes[3] = tgt0;
  if (!db->spec) {   // a full plan: the shape a new batch of this context may assume
    ctx->spec_shape_ok = db->spec_ready;
    ctx->spec_rpi = db->region_per_incid;
    ctx->spec_tgt = tgt0;
  }
  return GANON_OK;
}


int plan(ganon_ctx *ctx, ganon_dbatch *db, bool allow_spec) {
  hipStream_t st = ctx->stream;
  int rc;
  const int64_t nr = db->n_reads, ns = db->n_scopes;
  int32_t *read_end = nullptr, *nseg = nullptr;
  if ((rc = grow_n(ctx, db->b_read_end, (size_t)std::max<int64_t>(nr, 1), &read_end)) ||
      (rc = grow_n(ctx, db->b_cursor, 4 * kCursors, &db->cursor)))
    return rc;
  db->B.read_end = read_end;
  db->ran = false;
  const Raw R = raw_of(db);
  // short-read groups (one-segment and two-pass emits) in closed form from the CSR offsets; the
  // long-read prep cuts its own from the segments per scope below
  const int tgt0 = ctx->group_target ? ctx->group_target : 704;
  const long long w0 = weight_of(tgt0);
  const int64_t g_bound = ns ? (db->n_incid + w0 * (ns - 1)) / tgt0 + 1 : 1;
  // speculative: the last full plan of db found a one-segment batch without huge scopes of these
  // sizes, or (other sizes: a new batch) the context's last full plan did; the run launches for that
  // shape at once (buffers sized on the host from the counts) and the scan's reduction checks it (gate)
  // ("same": the context's previous plan was of this batch — a replan of its contents in place)
  // fused mode: the scan describes the reads (and lists multi-segment reads' segments) and finds the
  // partition candidates whenever the batch may be planned in that mode — whatever the context planned
  // before (round 4 skipped it after a plan of another shape, and a context that met one batch with a
  // long CIGAR stayed on the record pass: a plan-history hazard, verdict r04 weak #11); a batch that
  // turns out not to fit (long CIGARs, reads of more than kFusedMaxSeg segments) wastes the descriptors
  const bool want_fused = ctx->fused_flat && (ctx->prep_long == -1 || ctx->prep_long == 2);
  const bool same = db->spec_ready && db->spec_sizes[0] == nr && db->spec_sizes[1] == ns &&
                    db->spec_sizes[2] == db->n_incid && db->spec_sizes[3] == tgt0 && db->flat_mode &&
                    ctx->last_plan == db && db->fused == want_fused;
  ctx->last_plan = db;
  const bool sized = !same && ctx->spec_shape_ok && ctx->spec_tgt == tgt0 && ctx->prep_long == -1;
  const bool spec = allow_spec && ctx->spec_plan && (same || sized);
  db->spec = spec;
  db->spec_sized = spec && sized;
  if (!spec) {
    db->n_groups = 0;
    db->spec_ready = false;
  }
  db->fused = want_fused;   // (until the full plan's shape says otherwise)
  const int64_t spec_rpi = !spec ? 0 : db->spec_sized ? ctx->spec_rpi : db->region_per_incid;
  longlong2 *gm = nullptr;
  unsigned long long *part = nullptr;
  const int64_t rb = (nr + kScanReadsPerBlock - 1) / kScanReadsPerBlock;
  const int64_t sb = (ns + kScanScopesPerBlock - 1) / kScanScopesPerBlock;
  const int64_t nb = std::max<int64_t>(1, rb + sb);
  if (nb > INT32_MAX) return fail(ctx, GANON_E_ARG, "batch too large");
  // partials (SoA, one row per kind): the scan's blocks, then up to kLongGrid blocks of k_prep_scan_long
  int32_t *long_list = nullptr;
  if ((rc = grow_n(ctx, db->b_gs0, (size_t)g_bound, &gm)) ||
      (rc = grow_n(ctx, db->b_part, (size_t)kParts * (nb + kLongGrid), &part)) ||
      (rc = grow_n(ctx, db->b_long, (size_t)std::max<int64_t>(nr, 1), &long_list)))
    return rc;
  unsigned long long *cand = nullptr;
  int4 *desc = nullptr, *xrec = nullptr;
  int2 *xlist = nullptr;
  int32_t *xidx = nullptr;
  uint8_t *sdirty = nullptr;   // (k_prep_cands)
  if (db->fused) {
    // extras records of multi-segment reads: the list keeps its capacity (at least one per 8 reads).
    // With GANON_PARAM_XREC_INIT the capacity asked for stays until a full plan regrows it: the second
    // plan used to take the default, and a speculative replan of the same sizes, which reuses the
    // previous plan's aux pointers (prepare), left the group kernel reading the freed list
    const int64_t xwant = std::min<int64_t>(
        INT32_MAX, ctx->xrec_init > 0 ? std::max<int64_t>(db->xcap, (int64_t)ctx->xrec_init)
                                      : std::max<int64_t>({db->xcap, int64_t(65536), nr / 8}));
    if ((rc = grow_n(ctx, db->b_desc, (size_t)std::max<int64_t>(nr, 1), &desc)) ||
        (rc = grow_n(ctx, db->b_cand, 2 * (size_t)g_bound, &cand)) ||
        (rc = grow_n(ctx, db->b_sdirty, (size_t)std::max<int64_t>(ns, 1), &sdirty)) ||
        (rc = grow_n(ctx, db->b_xrec, (size_t)xwant, &xrec)) ||
        (rc = grow_n(ctx, db->b_xlist, (size_t)std::max<int64_t>(db->n_incid, 1), &xlist)) ||
        (rc = grow_n(ctx, db->b_xidx, (size_t)std::max<int64_t>(nr, 1), &xidx)))
      return rc;
    db->xcap = std::min<int64_t>(INT32_MAX, (int64_t)((db->b_xrec.bytes - 128) / sizeof(int4)));
    // (testing knob: the allocation's rounding does not count. A capacity the batch already has wins
    // over a smaller GANON_PARAM_XREC_INIT set later: the knob sizes a fresh upload's first list)
    if (ctx->xrec_init > 0 && db->xcap > xwant) db->xcap = xwant;
  }
  db->cand = cand;
  unsigned int *long_count = db->long_count;
  const int64_t pstride = nb + kLongGrid;
  if ((rc = grow_n(ctx, db->b_xcnt, (size_t)kXStripes * kXStride, &db->xcount))) return rc;
  const ScanOut O{read_end, long_list, long_count, gm, g_bound, part, pstride, nullptr, desc, cand, xidx, xrec, db->xcount,
                  (uint32_t)(xrec ? db->xcap / kXStripes : 0)};
  // the speculation's segment bound: a fused plan takes multi-segment reads, the record pass does not
  const int spec_maxseg = db->fused ? kFusedMaxSeg : 1;
  {
    // 1. the batch scan: every per-read and per-scope check, read ends, the group table of the
    //    short-read modes, per-block partials; then their reduction
    KernelScope ks(ctx, "prep_scan");
    HIP_OR_FAIL(hipMemsetAsync(db->err, 0, db->flags_bytes, st));   // error, status, long reads, far need
    HIP_OR_FAIL(hipMemsetAsync(db->xcount, 0, (size_t)kXStripes * kXStride * sizeof(unsigned int), st));
    if (cand) HIP_OR_FAIL(hipMemsetAsync(cand, 0, 2 * (size_t)g_bound * sizeof *cand, st));
    const bool narrow = db->seq_bytes < INT32_MAX && db->n_cigar_ops < INT32_MAX;
    hipLaunchKernelGGL(narrow ? k_prep_scan<true> : k_prep_scan<false>, dim3((unsigned)nb), dim3(kPrepThreads), 0, st, R,
                       db->err, O, w0, (long long)tgt0, (int)rb);
    hipLaunchKernelGGL(k_prep_reduce, dim3(1), dim3(kReduceThreads), 0, st, R, part, pstride, (int)nb, w0, (long long)tgt0,
                       g_bound, db->plan_info, static_cast<const PrepErr *>(db->err),
                       (long long)spec_rpi, static_cast<const unsigned int *>(long_count), spec_maxseg,
                       static_cast<const unsigned int *>(db->xcount), (unsigned int)O.xper);
    if ((rc = check_launch(ctx, "k_prep_scan"))) return rc;
  }
  if (spec && !db->spec_sized) return GANON_OK;   // the previous plan's mode, sizes and buffers; errors at download
  if (spec) {
    // a new batch assumed to have the context's last shape: one-segment mode, no huge scope, reads no
    // longer than that plan's; what the scan alone knows (the written reads, the I/D ops) stays on
    // the device (prepare copies the written count into the static totals)
    db->long_mode = false;
    db->flat_mode = true;
    db->region_per_incid = spec_rpi;
    db->group_target = tgt0;
    db->n_id_ops = 0;
    db->max_len = 48 * spec_rpi;
    db->max_seg = spec_maxseg;   // (at most: the gate checks it)
    db->n_huge_scopes = 0;
    db->n_written = -1;
    db->scost = nullptr;
    return size_plan(ctx, db, ns ? g_bound : 0, tgt0, R);
  }
  // 2. the one synchronization of a fresh batch: its first error and its shape
  unsigned long long info[6] = {0, 0, 0, 0, 0, 0};
  PrepErr e{};
  unsigned int n_long = 0;
  std::vector<unsigned int> xc((size_t)kXStripes * kXStride, 0u);
  HIP_OR_FAIL(ganon_detail::readback(info, db->plan_info, sizeof info, st));
  HIP_OR_FAIL(ganon_detail::readback(&e, db->err, sizeof e, st));
  HIP_OR_FAIL(ganon_detail::readback(&n_long, long_count, sizeof n_long, st));
  if (db->fused)
    HIP_OR_FAIL(ganon_detail::readback(xc.data(), db->xcount, xc.size() * sizeof(unsigned int), st));
  HIP_OR_FAIL(ganon_detail::sync_stream(st));
  if (!e.code && n_long) {
    // reads with long CIGARs: a wave each, then the reduction again over both sets of partials
    KernelScope ks(ctx, "prep_scan_long");
    const unsigned gl = (unsigned)std::min<int64_t>(kLongGrid, ((int64_t)n_long + 3) / 4);
    ScanOut OL = O;
    OL.part = part + nb;   // (blocks nb.. of every kind)
    if ((rc = grow_n(ctx, db->b_nseg, (size_t)std::max<int64_t>(nr, 1), &OL.nseg))) return rc;
    hipLaunchKernelGGL(k_prep_scan_long, dim3(gl), dim3(kPrepThreads), 0, st, R, db->err, OL, (int)n_long);
    hipLaunchKernelGGL(k_prep_reduce, dim3(1), dim3(kReduceThreads), 0, st, R, part, pstride, (int)(nb + gl), w0,
                       (long long)tgt0, g_bound, db->plan_info, static_cast<const PrepErr *>(db->err), 0ll,
                       static_cast<const unsigned int *>(long_count), spec_maxseg,
                       static_cast<const unsigned int *>(db->xcount), (unsigned int)O.xper);
    if ((rc = check_launch(ctx, "k_prep_scan_long"))) return rc;
    HIP_OR_FAIL(ganon_detail::readback(info, db->plan_info, sizeof info, st));
    HIP_OR_FAIL(ganon_detail::readback(&e, db->err, sizeof e, st));
    HIP_OR_FAIL(ganon_detail::sync_stream(st));
  }
  if (e.code) return fail(ctx, GANON_E_ARG, err_text(e.code), e.index, e.a, e.b);
  const unsigned long long max_len = info[3], max_seg = info[4];
  // prep mode: long (a read with several segments, or forced), one-segment (every read has at most
  // one: the default for short reads), or the two-pass short emit (GANON_PARAM_PREP_LONG 0)
  // auto: the long-read prep (a wave per incidence) only for long reads; short reads with indels
  // (several segments, a few per cent of the reads) take the two-pass emit — the long prep took
  // 11.3 ms instead of ~0.2 on a planner-built 2 M-read batch (profiles/r02/planner_batch_bench.json)
  db->long_mode = ctx->prep_long == 1 || (ctx->prep_long == -1 && max_seg > 1 && max_len > kLongReadLen);
  // (fused: short reads of up to kFusedMaxSeg aligned segments too — the scan described every read:
  // none left to the wave walk, every multi-segment read's segments in the extras list)
  const bool fused_multi = db->fused && n_long == 0 && max_seg <= (unsigned long long)kFusedMaxSeg;
  int64_t xfull = 0;   // the fullest stripe's records
  for (int k = 0; k < kXStripes; ++k) xfull = std::max<int64_t>(xfull, xc[(size_t)kXStride * k]);
  if (fused_multi && max_seg > 1 && !db->long_mode && xfull > db->xcap / kXStripes) {
    // an extras stripe was too short: grow every stripe to the fullest one's count and plan again
    // (the list keeps its capacity for later batches)
    int4 *x = nullptr;
    const int64_t want = std::min<int64_t>(INT32_MAX, kXStripes * (xfull + xfull / 4 + 64));
    if (kXStripes * xfull >= INT32_MAX) return fail(ctx, GANON_E_ARG, "batch too large: %lld extras records per stripe", (long long)xfull);
    if ((rc = grow_n(ctx, db->b_xrec, (size_t)want, &x))) return rc;
    db->xcap = want;
    return plan(ctx, db, false);
  }
  db->flat_mode = !db->long_mode && (max_seg <= 1 || fused_multi) && (ctx->prep_long == -1 || ctx->prep_long == 2);
  db->fused = db->fused && db->flat_mode && n_long == 0;
  if (!db->fused) db->cand = nullptr;
  // overflow-region observations per incidence: the longest read's ceil(L / 48)
  db->region_per_incid = (int64_t)((max_len + 47) / 48);
  db->group_target = ctx->group_target ? ctx->group_target : db->long_mode ? 2816 : 704;   // auto (profiles/r06/sweep: c5 2816 1.99 vs 1408 2.08 ms, c3 704)
  db->n_id_ops = (int64_t)info[0];
  db->max_len = (int64_t)max_len;
  db->max_seg = (int64_t)max_seg;
  db->n_huge_scopes = (int32_t)info[1];
  db->n_written = (int64_t)info[2];
  if ((double)db->n_incid * (double)db->region_per_incid > 4e9)
    return fail(ctx, GANON_E_ARG, "batch too large: %lld incidences of reads up to %llu bases (split it)",
                (long long)db->n_incid, max_len);
  const long long w = weight_of(db->group_target);
  int64_t ng = ns ? (int64_t)info[5] : 0;   // closed-form groups of the target used by the scan
  db->scost = nullptr;
  if (db->long_mode && ns) {
    // groups cut on the prefix of segments per scope: cost[s] = segments of its incidences + w
    if ((rc = grow_n(ctx, db->b_nseg, (size_t)std::max<int64_t>(nr, 1), &nseg))) return rc;
    // (the short reads; k_prep_scan_long wrote the long reads' counts)
    if (nr) hipLaunchKernelGGL(k_prep_nseg, dim3(grid_for(nr)), dim3(kPrepThreads), 0, st, R, nseg);
    int64_t *cost = nullptr;
    if ((rc = grow_n(ctx, db->b_scost, (size_t)ns + 1, &cost))) return rc;
    hipLaunchKernelGGL(k_prep_scope_cost, dim3(grid_for(ns + 1)), dim3(kPrepThreads), 0, st, R, nseg, w, cost);
    if ((rc = check_launch(ctx, "k_prep_scope_cost"))) return rc;
    // and the read records' bases (exclusive prefix of the segments per read, 64-bit)
    int64_t *rbase = nullptr;
    if ((rc = grow_n(ctx, db->b_rbase, (size_t)std::max<int64_t>(nr, 1), &rbase))) return rc;
    size_t tb = 0, tb2 = 0;
    HIP_OR_FAIL(rocprim::exclusive_scan(nullptr, tb, cost, cost, (int64_t)0, (size_t)ns + 1, rocprim::plus<int64_t>(), st));
    if (nr) HIP_OR_FAIL(rocprim::exclusive_scan(nullptr, tb2, nseg, rbase, (int64_t)0, (size_t)nr, rocprim::plus<int64_t>(), st));
    tb = std::max(tb, tb2);
    void *tmp = nullptr;
    if ((rc = grow_n(ctx, db->b_scan_tmp, tb, reinterpret_cast<uint8_t **>(&tmp)))) return rc;
    HIP_OR_FAIL(rocprim::exclusive_scan(tmp, tb, cost, cost, (int64_t)0, (size_t)ns + 1, rocprim::plus<int64_t>(), st));
    int64_t last[2] = {0, 0}, rb_last = 0;   // the last scope's cost prefix, and the total
    int32_t ns_last = 0;
    HIP_OR_FAIL(ganon_detail::readback(last, cost + ns - 1, sizeof last, st));
    if (nr) {
      HIP_OR_FAIL(rocprim::exclusive_scan(tmp, tb, nseg, rbase, (int64_t)0, (size_t)nr, rocprim::plus<int64_t>(), st));
      HIP_OR_FAIL(ganon_detail::readback(&rb_last, rbase + nr - 1, sizeof rb_last, st));
      HIP_OR_FAIL(ganon_detail::readback(&ns_last, nseg + nr - 1, sizeof ns_last, st));
    }
    HIP_OR_FAIL(ganon_detail::sync_stream(st));
    db->scost = cost;
    ng = last[0] / db->group_target + 1;
    db->n_rrec = rb_last + ns_last;
    db->n_long_seg = last[1] - w * ns;   // segments over the incidences (the group kernel's slots)
    int4 *i4 = nullptr, *rr = nullptr;
    uint8_t *sd = nullptr;
    if ((rc = grow_n(ctx, db->b_inc4, (size_t)std::max<int64_t>(db->n_incid, 1), &i4)) ||
        (rc = grow_n(ctx, db->b_rrec, (size_t)std::max<int64_t>(db->n_rrec, 1), &rr)) ||
        (rc = grow_n(ctx, db->b_sdirty, (size_t)ns, &sd)))
      return rc;
  } else if (ns && db->group_target != tgt0) {
    return fail(ctx, GANON_E_STATE, "group target changed during the plan");
  }
  // one-segment mode launches for the group bound (blocks past the scan's count return at once):
  // a speculative replan of the same sizes then needs no count from the host
  if (db->flat_mode && ns) ng = g_bound;
  return size_plan(ctx, db, ng, tgt0, R);
}

int run(ganon_ctx *ctx, ganon_dbatch *db) {
  const Raw R = raw_of(db);
  int rc;
  if (!db->n_groups) return GANON_OK;
  if (db->flat_mode) {   // the scan's group table is in place; the emit marks the line map
    {
      KernelScope ks(ctx, "prep_emit");
      HIP_OR_FAIL(hipMemsetAsync(db->b_linemap.p, 0, (size_t)line_map_words(db) * 8, ctx->stream));
    }
    if (db->fused) {
      // no records: group records, candidates and line map marks from the scan's results
      KernelScope ks(ctx, "prep_cands");
      hipLaunchKernelGGL(k_prep_cands, dim3(grid_for(std::max<int64_t>(db->n_groups, db->n_scopes), INT32_MAX)),
                         dim3(kPrepThreads), 0, ctx->stream, R, static_cast<const longlong2 *>(db->b_gs0.p), db->n_groups,
                         (long long)db->region_per_incid, static_cast<const unsigned long long *>(db->cand),
                         static_cast<unsigned long long *>(db->b_lo.p), static_cast<int4 *>(db->b_groups.p), line_map(db),
                         static_cast<unsigned long long *>(db->b_wspart.p),
                         static_cast<const unsigned long long *>(db->plan_info), static_cast<uint8_t *>(db->b_sdirty.p),
                         db->ref->bad, db->ref->n_blk);
      if ((rc = check_launch(ctx, "k_prep_cands"))) return rc;
    } else if ((rc = launch_emit(ctx, db, R, 1))) {
      return rc;
    }
  } else if ((rc = launch_groups(ctx, db, R)) || (rc = launch_emit(ctx, db, R, 1))) {
    return rc;
  }
  return launch_pieces(ctx, db);
}

int ws_diag(ganon_ctx *ctx, ganon_dbatch *db) {
  hipLaunchKernelGGL(k_prep_ws_diag, dim3(grid_for(db->n_reads)), dim3(kPrepThreads), 0, ctx->stream, raw_of(db),
                     db->err);
  return check_launch(ctx, "k_prep_ws_diag");
}

int batch_error(ganon_ctx *ctx, ganon_dbatch *db) {
  PrepErr e{};
  HIP_OR_FAIL(ganon_detail::readback(&e, db->err, sizeof e, ctx->stream));
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  if (e.code) return fail(ctx, GANON_E_ARG, err_text(e.code), e.index, e.a, e.b);
  return GANON_OK;
}

}  // namespace ganon_prep

// Reference blocks of a resident reference (ganon_hip.hip ganon_ref_upload).
int ganon_ref_blocks(ganon_ctx *ctx, ganon_ref *ref) {
  if (!ref->n_blk) return GANON_OK;
  const int64_t n_round = (ref->n_blk + 63) & ~(int64_t)63;
  hipLaunchKernelGGL(k_ref_blocks, dim3(grid_for(n_round)), dim3(kPrepThreads), 0, ctx->stream, ref->nt16, ref->bytes,
                     ref->n_blk, ref->bad);
  return check_launch(ctx, "k_ref_blocks");
}
