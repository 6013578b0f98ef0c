// ganon_group.hip — k_group, the small-scope masking kernel (ganon_group, ganon_batch.h): one
// 256-thread workgroup per scope group copies its partition of the output, streams every aligned
// base of its scopes against the reference, classifies the mismatches per (scope, position,
// allele) and masks the tumor-and-normal calls. Three record sources (the record pass, the fused
// one-segment mode FLAT, the long-read mode LONG) times the unroll and observation-list sizes of
// the table at the end of the file.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ganon.h"
#include "ganon_batch.h"
#include "ganon_ctx.h"

using namespace ganon_dev;

namespace {

// ---- group kernels: scope groups, observation lists ---------------------------------------
// No per-scope table and no per-scope serialization. At upload every read of a small scope is
// cut into segments (one per aligned M/=/X run: query nibble index, reference nibble index,
// length) and consecutive scopes are packed into groups of ~kGrpTarget segments. One 256-thread
// workgroup streams all 16-base chunks of all segments of its group at once (memory-level
// parallelism across scopes instead of one scope at a time), and every base that differs from
// an ACGT reference base becomes an observation in LDS:
//   key = scope_local:12 | (pos - span_start):48 | allele:4
//   payload = nibble index:48 | ref:4 | dataset:1 | mine:1
// A set of equal keys is one call (pos, allele) of one scope, TN iff it holds a tumor and a
// normal observation — the end state of the reference's per-position state machine
// (variants.py:33-39) — and not the window's kept variant. TN calls are counted
// and their observations in reads the scope writes are masked. All 16 codes are handled
// alike (no re-run). A group whose observations overflow the LDS list (deep coverage, long
// reads) is re-scanned once into its own global observation region (sized at upload, L2-hot),
// aggregated in a global hash table of distinct keys (workgroup-scope atomics: only this
// workgroup touches it), classified, and masked from the observation region — the reads are
// not scanned again. A region that overflows too is split over halves of its key range.
//
// Output: the partition copy. Groups are launched in the order of their reads in the sequence
// buffer and each workgroup owns a 128-byte-aligned partition of the output (two pieces,
// [p0, p1) and [q0, q1)), which it copies with whole-line 16-byte stores before scanning (its
// reads' bases are then L2-hot for the scan). A mask has one of two routes (sink_patch): inside
// the partition it goes to the LDS patch list, applied after each classification as plain byte
// stores seq[b] ^ mask once the copy has drained (grp_apply_patches; the overflow-region pass
// merges its in-partition masks per byte in its hash table instead); a mask of a byte in another
// workgroup's partition (a read crossing a partition boundary) goes to the global far list,
// applied by k_finish after the kernel. Partial-line stores from different workgroups cost ~4x
// whole-line stores on MI355X (tools/membench.hip), hence partitions.
// ("Fused" is kept for the one-segment mode FLAT, db->fused: records made in the kernel.)
constexpr int kGrpThreads = 256;
#ifndef GANON_K2_BLOCKS
#define GANON_K2_BLOCKS 6   // resident workgroups per CU the K = 2 instance is compiled for
#endif
constexpr int kGrpTile = 256;        // segment records staged per tile
constexpr int kGrpStack = 80;        // key ranges pending (bisection depth <= 64)
constexpr int kGrpMap = 4096;        // chunk -> segment map entries (larger tiles binary-search)
constexpr int kGrpQuad = 256;        // lists up to this size are matched without sorting
constexpr unsigned long long kEmpty = ~0ull;
constexpr unsigned long long kNibMask = (1ull << 48) - 1;
static_assert(kGrpTile == kGrpThreads && kGrpTile <= 256, "one staged record per thread, 8-bit map");

// The few batch arrays the group kernels read (a slim kernel argument keeps SGPRs free).
struct GrpBatch {
  const uint8_t *seq, *ref, *keep_code;
  const uint32_t *ref2;
  const int32_t *keep_pos, *span_start, *span_len;
};

// OBS: observations held in LDS before a list overflows into the group's global region (512, which
// ganon_batch_run always picks on its own; 1024 only when GANON_PARAM_GROUP_OBS asks for it); the
// in-partition mask list has the same size.
template <int OBS>
struct GrpSharedT {
  static constexpr int kObs = OBS;
  int4 rec[kGrpTile];               // segment records (layout at kSegMine)
  int pre[kGrpTile];
  uint8_t cmap[kGrpMap];            // staged segment of each chunk (tiles of <= kGrpMap chunks)
  int wsum[kGrpThreads / 64];
  unsigned long long key[OBS];      // observation list
  unsigned long long pay[OBS];
  unsigned long long patch[OBS];    // nibble index << 4 | (from ^ to)
  unsigned long long stk_lo[kGrpStack], stk_hi[kGrpStack];
  int stk_mode[kGrpStack];          // (written, never read: see GrpRange::mode)
  unsigned long long kmin, kmax;
  int top, n_obs, n_patch, n_filt;
  int blk_calls, blk_bases;         // this workgroup's contribution to the totals
  int cnt_calls[kGrpMaxScopes];     // per-scope counts, written out once at the end
  int cnt_bases[kGrpMaxScopes];
  int wdirty[kGrpThreads / 64];     // fused one-segment mode: a wave's records need the nt16 reference
  unsigned long long hsum;          // ... and the write-scope hash sum of the group's mine incidences
  int n_xent, n_xrec, n_xtile;      // ... and its incidences with further segments (entries), their records, an
                                    // extras tile's records
};

struct GrpRange {
  unsigned long long lo, hi;
  int mode;   // always 0, never read (left of retired passes; removing it and stk_mode measured slower)
};

struct PatchSink {
  uint8_t *out;
  int64_t p0, p1, q0, q1;           // this workgroup's partition pieces of out (bytes)
  const GrpAux *aux;                // far-mask list
  bool part;                        // always true: masks go to the partition's two routes (below)
  bool lds;                         // in-partition masks into the LDS list (off in the overflow-region pass)
  __device__ bool inside(int64_t byte) const { return (byte >= p0 && byte < p1) || (byte >= q0 && byte < q1); }
};

__device__ __forceinline__ void patch_nibble(uint8_t *out, int64_t nib_index, int from, int to) {
  const int64_t byte = nib_index >> 1;
  const int sh = 8 * (int)(byte & 3) + ((nib_index & 1) ? 0 : 4);
  atomicXor(reinterpret_cast<uint32_t *>(out) + (byte >> 2), (uint32_t)(from ^ to) << sh);
}

// A mask (nibble index, from ^ to): out of the partition to the far list, else to the LDS patch list.
// (The flags and the atomic fall-through are what is left of the retired output paths: every
// instantiation sets both flags, so the fall-through is never reached. Taking them out was measured
// slower on the default instantiation and put back)
template <class SH>
__device__ __forceinline__ void sink_patch(SH &sh, const PatchSink &k, int64_t nib, int c, int rc) {
  const unsigned long long e = ((unsigned long long)nib << 4) | (unsigned long long)(c ^ rc);
  if (k.part) {
    const int64_t byte = nib >> 1;
    if (!k.inside(byte)) {
      const unsigned long long i = __hip_atomic_fetch_add(gp(k.aux->far_count), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (i < (unsigned long long)k.aux->far_cap) gp(k.aux->far)[i] = e;
      return;
    }
    if (k.lds) {
      const int i = atomicAdd(&sh.n_patch, 1);
      if (i < SH::kObs) sh.patch[i] = e;
      return;
    }
  }
  patch_nibble(k.out, nib, c, rc);
}

// A group's global observation region (overflow path): cap observations (key, payload) at
// obs + off, and a hash table of up to 2 * cap distinct keys (key, 2-bit tumor/normal flags)
// at tkey/tflag + 2 * off. Only the owning workgroup touches it.
struct GrpGlobal {
  const GrpAux *aux;
  int64_t off;
  int cap;
};

__device__ __forceinline__ unsigned long long ld_l2(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1: past the CU's L1
}
__device__ __forceinline__ unsigned int ld_l2(const unsigned int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_l2(const GU64 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned int ld_l2(const GU32 *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// threadIdx.x the compiler cannot hoist out of a loop: address arithmetic of the rare overflow
// paths is then recomputed where it is used instead of being kept live (spilled to scratch)
// across the whole kernel.
__device__ __forceinline__ int opaque_tid() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

__device__ __forceinline__ unsigned gtab_home(unsigned long long key, int tsize) {
  const unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  return (unsigned)(((h >> 32) * (unsigned long long)tsize) >> 32);
}

template <class SH>
__device__ __forceinline__ void grp_count(SH &sh, int s_local, int calls, int bases);

// Per-dataset Bloom bitmaps of an overflowing pass's observation keys, built from the stored
// observations in the patch list's LDS (unused until the classification): a key seen in only one
// dataset can never be a TN call, so a list that overflows the LDS list is first filtered by them
// (grp_filter) — a 60x scope's sequencing errors, almost all single-dataset, then mostly drop out
// and the rest fits in LDS. Passes that do not overflow (every configs[1] group) pay nothing.
#ifndef GANON_GRP_BLOOM
#define GANON_GRP_BLOOM 1   // 0: no Bloom filtering (A/B builds)
#endif
constexpr int kBloomBits = 16384;   // per dataset: the two take the 4 KiB of the 512-entry patch list
__device__ __forceinline__ uint32_t bloom_hash(unsigned long long key) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40);
}
template <class SH>
__device__ __forceinline__ uint32_t *bloom_of(SH &sh) {
  static_assert(sizeof(sh.patch) * 8 >= 2 * kBloomBits, "Bloom bitmaps live in the patch list");
  return reinterpret_cast<uint32_t *>(sh.patch);
}
template <class SH>
__device__ __forceinline__ bool bloom_both(SH &sh, unsigned long long key) {
  const uint32_t h = bloom_hash(key) & (kBloomBits - 1), *b = bloom_of(sh);
  return ((b[h >> 5] & b[(kBloomBits + h) >> 5]) >> (h & 31)) & 1u;
}

// payload: nibble index:48 | ref:4 | dataset:1 | mine:1
template <class SH>
__device__ __forceinline__ void grp_observe(SH &sh, const GrpRange &R, const GrpGlobal &gg,
                                            unsigned long long key, int64_t nib, int rc, int ds, uint32_t mine) {
  if (key < R.lo || key >= R.hi) return;
  const unsigned long long pay = (unsigned long long)nib | ((unsigned long long)rc << 48) |
                                 ((unsigned long long)ds << 52) | ((unsigned long long)mine << 53);
  const int k = atomicAdd(&sh.n_obs, 1);
  if (k < SH::kObs) {
    sh.key[k] = key;
    sh.pay[k] = pay;
  } else {
    // past the LDS list: straight into the group's global region (no second scan)
    if (k - SH::kObs < gg.cap - SH::kObs) {
      gp(gg.aux->okey)[gg.off + (k - SH::kObs)] = key;
      gp(gg.aux->opay)[gg.off + (k - SH::kObs)] = pay;
    }
  }
}

// Is (scope s, pos_off, allele c) the window's kept variant? (clear_keep's rule)
__device__ __forceinline__ bool grp_kept(const GrpBatch &B, int s, int64_t pos_off, int c) {
  const int kp = B.keep_pos[s];
  return kp >= 0 && B.keep_code[s] == c && (int64_t)kp - B.span_start[s] == pos_off;
}

// Partition copy: bytes [p0, p1) of src to dst in 16-byte windows (p0 16-byte aligned; a
// window may end past p1 only at the end of the buffer, which is padded), 8 windows in flight
// per thread: all loads issue before the first store waits on them.
__device__ __forceinline__ void copy_windows(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t p0,
                                             int64_t p1, int nt) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  constexpr int kCopyUnroll = 8;
  for (int64_t D0 = p0 + 16 * (int)threadIdx.x; D0 < p1; D0 += 16 * kGrpThreads * kCopyUnroll) {
    u32x4 v[kCopyUnroll];
#pragma unroll
    for (int k = 0; k < kCopyUnroll; ++k) {
      const int64_t D = D0 + 16 * kGrpThreads * k;
      if (D < p1) v[k] = *reinterpret_cast<const u32x4 *>(src + D);
    }
#pragma unroll
    for (int k = 0; k < kCopyUnroll; ++k) {
      const int64_t D = D0 + 16 * kGrpThreads * k;
      if (D >= p1) break;
      if (nt) __builtin_nontemporal_store(v[k], reinterpret_cast<u32x4 *>(dst + D));
      else *reinterpret_cast<u32x4 *>(dst + D) = v[k];
    }
  }
}

// The staged tile's chunk map: the exclusive prefix of the records' chunk counts (nck: this
// thread's record) and the chunk -> record map; returns the tile's chunk total.
template <class SH>
__device__ __forceinline__ int grp_tile_map(SH &sh, int nck) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // wave inclusive scan: DPP row_shr within each 16-lane row, then the row totals (no lane-index
  // registers: shuffle index arithmetic hoisted out of the tile loop cost 9 VGPRs and spills)
  int incl = nck;
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, false);   // row_shr:1
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, false);   // row_shr:2
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, false);   // row_shr:4
  incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, false);   // row_shr:8
  {
    const int r0 = __builtin_amdgcn_readlane(incl, 15), r1 = __builtin_amdgcn_readlane(incl, 31),
              r2 = __builtin_amdgcn_readlane(incl, 47);
    const int row = lane >> 4;
    incl += (row >= 1 ? r0 : 0) + (row >= 2 ? r1 : 0) + (row >= 3 ? r2 : 0);
  }
  if (lane == 63) sh.wsum[wave] = incl;
  __syncthreads();
  int wbase = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kGrpThreads / 64; ++w) {
    const int v = sh.wsum[w];
    wbase += w < wave ? v : 0;
    total += v;
  }
  const int pre = wbase + incl - nck;
  sh.pre[tid] = pre;
  if (total <= kGrpMap)
    for (int k = 0; k < nck; ++k) sh.cmap[pre + k] = (uint8_t)tid;
  __syncthreads();
  return total;
}

// Stage records [c0, c0 + nh) in LDS with the exclusive prefix of their chunk counts;
// returns the tile's chunk total.
template <class SH>
__device__ __forceinline__ int grp_tile(SH &sh, const int4 *__restrict__ rec4, int64_t c0, int nh, int chunk) {
  const int tid = threadIdx.x;
  const int4 r = rec4[c0 + (tid < nh ? tid : nh - 1)];
  int nck = 0;
  if (tid < nh) {
    sh.rec[tid] = r;
    nck = ((((uint32_t)r.z >> 16) & kSegMaxLen) + chunk - 1) / chunk;
  }
  return grp_tile_map(sh, nck);
}

// ---- fused one-segment mode: records made in LDS ------------------------------------------
// A one-segment batch (every read at most one aligned segment) needs no record pass over HBM:
// k_prep_scan wrote a 16-byte descriptor per read (its segment's query nibble, contig position and
// length, dataset, write scope, ganon_batch.h), and each tile here turns incidences [c0, c0 + nh)
// into the records k_prep_emit_flat used to write — scope by binary search in the staged scope
// table, the span check, the write-scope mark (and, on the group's first pass, the incidence checks
// and the write-scope hash sum). The group's scopes sit in the patch list's LDS (unused while chunks
// stream; staged again before every pass, the classification reuses it), 16 bytes each. A tile reads
// the 2-bit reference unless one of its records lies in a scope whose reference span holds a
// non-ACGT block (the record pass decided this per group; both copies give the same bases where
// the 2-bit one is read).
struct FlatScope {
  int off;                  // first incidence, relative to the group's
  int sstart;               // span start
  unsigned long long pk;    // ref_off - span_start (42-bit signed) | min(span_len, 2^20 + 1) << 42 | dirty << 63
};
static_assert(sizeof(FlatScope) * kGrpMaxScopes <= sizeof(unsigned long long) * kGrpObs,
              "the scope table fits the patch list");

template <class SH>
__device__ __forceinline__ FlatScope *flat_scopes(SH &sh) {
  return reinterpret_cast<FlatScope *>(sh.patch);
}

// Scope s of a group whose incidences start at i_begin (a thread per scope: at most kGrpMaxScopes,
// the group's workgroup size).
static_assert(kGrpMaxScopes <= kGrpThreads, "one staging thread per scope of a group");
__device__ __forceinline__ FlatScope flat_load(const GrpBatch &B, const GrpAux *__restrict__ aux, int s, int64_t i_begin) {
  const int64_t off = aux->incid_off[s], ro = aux->ref_off[s];
  const int ss = B.span_start[s], sl = B.span_len[s];
  const bool dirty = aux->sdirty[s] != 0;   // (k_prep_scan)
  FlatScope f;
  f.off = (int)(off - i_begin);
  f.sstart = ss;
  f.pk = ((unsigned long long)(ro - ss) & ((1ull << 42) - 1)) | ((unsigned long long)min(sl, kGrpMaxSpan + 1) << 42) |
         ((unsigned long long)dirty << 63);
  return f;
}

template <class SH>
__device__ __forceinline__ int blk_excl_sum(SH &sh, int v, int *total);
template <class SH>
__device__ __attribute__((noinline)) int grp_xexpand(SH &sh, const GrpAux *__restrict__ aux, int64_t i_begin, int e0, int n_e,
                                           int base, int *n_rec, int s_begin, bool first);

// r: incidence c0 + tid's read (loaded a tile ahead by grp_scan_flat). last: the group's last
// incidence tile — when the further segments of the group's multi-segment reads fit in its free
// slots, they join it (merged: no extras tile after it); nh grows by their records.
template <class SH>
__device__ __forceinline__ int grp_tile_flat(SH &sh, const GrpBatch &B, const GrpAux *__restrict__ aux, int64_t c0,
                                             int &nh, int chunk, int s_begin, int ns, int64_t i_begin, bool first,
                                             int r, bool &clean, bool last, bool &merged) {
  const int tid = threadIdx.x;
  const FlatScope *sc = flat_scopes(sh);
  int nck = 0;
  bool dirty = false;
  unsigned long long hsum = 0;
  if (tid < nh) {
    const int64_t i = c0 + tid;
    const int il = (int)(i - i_begin);
    int lo = 0, hi = ns - 1;   // the incidence's scope: largest j with off[j] <= il
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sc[mid].off <= il) lo = mid;
      else hi = mid - 1;
    }
    const int j = lo;
    int4 rec = make_int4(0, 0, 0, j);   // zero length: no chunks
    if (r < 0 || r >= aux->n_reads) {
      if (first) report(aux->err, kErrIncidRead, i, r);
    } else {
      const int4 d = aux->desc[r];
      const FlatScope S = sc[j];
      const uint32_t z = (uint32_t)d.z;
      const int n = (int)((z >> 8) & kSegMaxLen), p = d.y;
      // (a multi-segment read: the first segment's end here, the read's end when its further
      // segments are expanded)
      const bool multi = (z & kDescMulti) != 0;
      const int nx = multi ? (int)((z >> 28) & 7) : 0;
      const uint64_t sq = (uint64_t)(uint32_t)d.x | ((uint64_t)(z & 0x7F) << 32);
      int rs, re;
      if (z & kDescWide) {
        rs = aux->ref_start[r];
        re = multi ? p + n : aux->read_end[r];
      } else {
        rs = p - (int)((z >> 24) & 15);
        re = p + n + (multi ? 0 : (int)(z >> 28));
      }
      int sl = (int)((S.pk >> 42) & ((1ull << 21) - 1));
      const bool huge = sl > kGrpMaxSpan;
      if (huge) sl = B.span_len[s_begin + j];
      if (rs < S.sstart || (int64_t)re > (int64_t)S.sstart + sl) {
        if (first) report(aux->err, kErrIncidSpan, s_begin + j, r);
      } else {
        const bool mine = d.w == s_begin + j;
        if (first && mine) hsum += ws_hash(r);
        if (!huge && n > 0) {
          const int64_t r0 = (int64_t)(S.pk << 22) >> 22;
          const uint64_t rf = (uint64_t)(r0 + p);
          if (first && nx) {   // its further segments: an entry in the group's list (streamed after the incidences)
            const int k = atomicAdd(&sh.n_xent, 1);
            atomicAdd(&sh.n_xrec, nx);
            aux->xlist[i_begin + k] = make_int2(r, (int)((uint32_t)j | ((uint32_t)nx << 12) | (((z >> 22) & 1u) << 15) |
                                                        (mine ? 0x80000000u : 0u)));
          }
          const uint32_t rz = (uint32_t)((sq >> 32) & 0x7F) | ((uint32_t)((rf >> 32) & 0xFF) << 8) |
                              ((uint32_t)n << 16) | (((z >> 22) & 1u) << 30) | (mine ? kSegMine : 0u);
          rec = make_int4((int)(uint32_t)sq, (int)(uint32_t)rf, (int)rz,
                          (int)((uint32_t)j | ((uint32_t)(p - S.sstart) << 12)));
          dirty = (S.pk >> 63) != 0;
          nck = (n + chunk - 1) / chunk;
        }
      }
    }
    sh.rec[tid] = rec;
  }
  if (first) {   // the tile's write-scope hashes into the group's sum (uniform branch)
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)hsum, o), hi = __shfl_xor((uint32_t)(hsum >> 32), o);
      hsum += ((unsigned long long)hi << 32) | lo;
    }
    if ((tid & 63) == 0 && hsum) atomicAdd(&sh.hsum, hsum);
  }
  if (last) {   // (uniform) the group's further segments into this tile's free slots when they fit
    if (first) __builtin_amdgcn_s_waitcnt(0);   // (this tile's entries at L2 before the barrier)
    __syncthreads();
    const int ne = sh.n_xent, nr = sh.n_xrec;
    if (ne && nh + nr <= kGrpTile) {
      int got;
      grp_xexpand(sh, aux, i_begin, 0, ne, nh, &got, s_begin, first);   // (every entry fits: ends on a barrier)
      if (tid >= nh && tid < nh + nr) {
        const int4 x = sh.rec[tid];
        nck = ((((uint32_t)x.z >> 16) & kSegMaxLen) + chunk - 1) / chunk;
        dirty = (flat_scopes(sh)[x.w & 0xFFF].pk >> 63) != 0;
      }
      nh += nr;
      merged = true;
    }
  }
  const unsigned long long dm = __ballot(dirty);
  if ((tid & 63) == 0) sh.wdirty[tid >> 6] = dm != 0ull;
  const int total = grp_tile_map(sh, nck);
  int any = 0;
#pragma unroll
  for (int w = 0; w < kGrpThreads / 64; ++w) any |= sh.wdirty[w];
  clean = any == 0;
  return total;
}

// The staged segment owning chunk t (largest j with pre[j] <= t).
template <class SH>
__device__ __forceinline__ int grp_find(const SH &sh, int nh, int total, int t) {
  if (total <= kGrpMap) return sh.cmap[t];
  int lo = 0, hi = nh - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sh.pre[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One chunk (16 * K bases) of staged record j: each thread loads the 2K + 1 sequence dwords and
// the K + 1 (2-bit) or 2K + 1 (nt16) reference dwords covering it at once (one memory round trip
// per chunk), then takes the K 16-base windows out of registers with static indices.
template <int K, bool REF2, class SH>
__device__ __forceinline__ void grp_chunk(const GrpBatch &B, SH &sh, const GrpRange &R, const GrpGlobal &gg, int t,
                                          int j) {
  {
    {
      const int4 r = sh.rec[j];
      const uint32_t rz = (uint32_t)r.z;
      const int L = (int)((rz >> 16) & kSegMaxLen);
      const int q0 = 16 * K * (t - sh.pre[j]);
      const int64_t sn = (int64_t)((uint64_t)(uint32_t)r.x | ((uint64_t)(rz & 0xFF) << 32)) + q0;
      const int64_t rn = (int64_t)((uint64_t)(uint32_t)r.y | ((uint64_t)((rz >> 8) & 0xFF) << 32)) + q0;
      const uint32_t *ps = reinterpret_cast<const uint32_t *>(B.seq) + (sn >> 3);
      const uint32_t *pr = REF2 ? B.ref2 + (rn >> 4) : reinterpret_cast<const uint32_t *>(B.ref) + (rn >> 3);
      constexpr int NR = REF2 ? K + 1 : 2 * K + 1;   // reference words covering the chunk
      uint32_t ds[2 * K + 1], dr[NR];
#pragma unroll
      for (int i = 0; i < 2 * K + 1; ++i) ds[i] = ps[i];
#pragma unroll
      for (int i = 0; i < NR; ++i) dr[i] = pr[i];
#pragma unroll
      for (int i = 0; i < 2 * K + 1; ++i) ds[i] = nib_swap(ds[i]);
      if (!REF2) {
#pragma unroll
        for (int i = 0; i < NR; ++i) dr[i] = nib_swap(dr[i]);
      }
      const int shs = 4 * (int)(sn & 7), shr = REF2 ? 2 * (int)(rn & 15) : 4 * (int)(rn & 7);
      const int ds_ = (int)((rz >> 30) & 1);
      const unsigned long long sk = (unsigned long long)(r.w & 0xFFF) << 52;
      const int pos_seg = (int)((uint32_t)r.w >> 12);
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const int qi = q0 + 16 * i;
        if (qi >= L) break;
        const uint64_t xs0 = (uint64_t)ds[2 * i] | ((uint64_t)ds[2 * i + 1] << 32);
        const uint64_t xs1 = (uint64_t)ds[2 * i + 1] | ((uint64_t)ds[2 * i + 2] << 32);
        const uint64_t sv = (uint64_t)(uint32_t)(xs0 >> shs) | ((uint64_t)(uint32_t)(xs1 >> shs) << 32);
        uint64_t rv;
        if (REF2) {
          rv = expand2((uint32_t)((((uint64_t)dr[i]) | ((uint64_t)dr[i + 1] << 32)) >> shr));
        } else {
          const uint64_t xr0 = (uint64_t)dr[2 * i] | ((uint64_t)dr[2 * i + 1] << 32);
          const uint64_t xr1 = (uint64_t)dr[2 * i + 1] | ((uint64_t)dr[2 * i + 2] << 32);
          rv = (uint64_t)(uint32_t)(xr0 >> shr) | ((uint64_t)(uint32_t)(xr1 >> shr) << 32);
        }
        const int nb = (L - qi) < 16 ? (L - qi) : 16;
        uint64_t diff = sv ^ rv;
        diff = (diff | (diff >> 1) | (diff >> 2) | (diff >> 3)) & 0x1111111111111111ull;
        if (nb < 16) diff &= (1ull << (4 * nb)) - 1;
        while (diff) {
          const int k = __builtin_ctzll(diff) >> 2;
          diff &= diff - 1;
          const int c = (int)((sv >> (4 * k)) & 15);
          const int rc = (int)((rv >> (4 * k)) & 15);
          if (c == 15 || !is_acgt(rc)) continue;
          const unsigned long long key = sk | ((unsigned long long)(pos_seg + qi + k) << 4) | (unsigned long long)c;
          grp_observe(sh, R, gg, key, sn + 16 * i + k, rc, ds_, rz >> 31);
        }
      }
    }
  }
}

// Stream every chunk of every segment of the group, feeding observations in range R.
template <int K, bool REF2, class SH>
__device__ __forceinline__ void grp_scan(const GrpBatch &B, SH &sh, const GrpRange &R, const GrpGlobal &gg,
                                         int64_t i_begin, int64_t i_end, const int4 *__restrict__ rec4, int skip) {
  const int tid = threadIdx.x;
  for (int64_t c0 = i_begin; c0 < i_end; c0 += kGrpTile) {
    const int nh = (int)((i_end - c0) < kGrpTile ? (i_end - c0) : kGrpTile);
    int total = grp_tile(sh, rec4, c0, nh, 16 * K);
    if (skip & kSkipChunks) total = 0;
    for (int t = tid; t < total; t += kGrpThreads) {
      const int j = grp_find(sh, nh, total, t);
      grp_chunk<K, REF2>(B, sh, R, gg, t, j);
    }
    __syncthreads();
  }
}

// Long-read mode: slots [c0, c0 + nh) of a group whose incidences are [inc0, inc0 + n_inc): the
// incidence owning slot t (largest first slot <= t: incidences without records share their
// successor's first slot and lose to it), its read's record t - first slot, completed with the
// scope's fields from the staged scope table (reference offset, span start, reference flag) and
// the incidence's write mark. A tile of a 10-100 kb read's incidence reads 256 consecutive read
// records (one coalesced load). long_fetch issues a tile's loads; grp_scan_long issues the next
// tile's before it streams the current one, so their latency overlaps the chunk loads.
// itab: the group's incidence records staged in LDS after the scope table (ns + n_inc <= the
// table's 256 entries: every C5 group), else null (looked up in global memory).
struct LongFetch {
  int4 rr;   // the read record
  int iy;    // the incidence record's y: scope local | mine << 31
};

__device__ __forceinline__ LongFetch long_fetch(const GrpAux *__restrict__ aux, int64_t c0, int nh, int64_t inc0,
                                                int n_inc, const int4 *itab) {
  LongFetch f{make_int4(0, 0, 0, 0), 0};
  const int tid = threadIdx.x;
  if (tid < nh) {
    const int64_t t = c0 + tid;
    const int4 *it = itab ? itab : aux->inc4 + inc0;
    int lo = 0, hi = n_inc - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((int64_t)it[mid].x <= t) lo = mid;
      else hi = mid - 1;
    }
    const int4 I = it[lo];
    const int64_t rb = (int64_t)((uint64_t)(uint32_t)I.z | ((uint64_t)(uint32_t)I.w << 32));
    f.rr = aux->rrec[rb + (t - (int64_t)(uint32_t)I.x)];
    f.iy = I.y;
  }
  return f;
}

template <class SH>
__device__ __forceinline__ int grp_tile_long(SH &sh, const LongFetch &F, int nh, int chunk, bool &clean) {
  const int tid = threadIdx.x;
  const FlatScope *sc = flat_scopes(sh);
  int nck = 0;
  bool dirty = false;
  if (tid < nh) {
    const int j = F.iy & 0xFFF;
    const FlatScope S = sc[j];
    const uint32_t z = (uint32_t)F.rr.z;
    const int n = (int)((z >> 16) & kSegMaxLen), p = F.rr.y;
    const int64_t r0 = (int64_t)(S.pk << 22) >> 22;
    const uint64_t rf = (uint64_t)(r0 + p);
    const uint32_t rz = (z & 0xFFu) | ((uint32_t)((rf >> 32) & 0xFF) << 8) | ((uint32_t)n << 16) | (z & (1u << 30)) |
                        ((uint32_t)F.iy & kSegMine);
    sh.rec[tid] = make_int4(F.rr.x, (int)(uint32_t)rf, (int)rz, (int)((uint32_t)j | ((uint32_t)(p - S.sstart) << 12)));
    dirty = (S.pk >> 63) != 0;
    nck = (n + chunk - 1) / chunk;
  }
  const unsigned long long dm = __ballot(dirty);
  if ((tid & 63) == 0) sh.wdirty[tid >> 6] = dm != 0ull;
  const int total = grp_tile_map(sh, nck);
  int any = 0;
#pragma unroll
  for (int w = 0; w < kGrpThreads / 64; ++w) any |= sh.wdirty[w];
  clean = any == 0;
  return total;
}

template <int K, class SH>
__device__ __forceinline__ void grp_scan_long(const GrpBatch &B, SH &sh, const GrpRange &R, const GrpGlobal &gg,
                                              const GrpAux *__restrict__ aux, int64_t i_begin, int64_t i_end,
                                              int64_t inc0, int n_inc, const int4 *itab, int skip) {
  const int tid = threadIdx.x;
  const auto tile_n = [&](int64_t c0) { return (int)((i_end - c0) < kGrpTile ? (i_end - c0) : kGrpTile); };
  LongFetch next = i_begin < i_end ? long_fetch(aux, i_begin, tile_n(i_begin), inc0, n_inc, itab) : LongFetch{};
  for (int64_t c0 = i_begin; c0 < i_end; c0 += kGrpTile) {
    const int nh = tile_n(c0);
    const LongFetch cur = next;
    if (c0 + kGrpTile < i_end) next = long_fetch(aux, c0 + kGrpTile, tile_n(c0 + kGrpTile), inc0, n_inc, itab);
    bool clean;
    int total = grp_tile_long(sh, cur, nh, 16 * K, clean);
    if (skip & kSkipChunks) total = 0;
    if (clean && B.ref2) {
      for (int t = tid; t < total; t += kGrpThreads) grp_chunk<K, true>(B, sh, R, gg, t, grp_find(sh, nh, total, t));
    } else {
      for (int t = tid; t < total; t += kGrpThreads) grp_chunk<K, false>(B, sh, R, gg, t, grp_find(sh, nh, total, t));
    }
    __syncthreads();
  }
}

template <int K, class SH>
__device__ __forceinline__ void grp_scan_extra(const GrpBatch &B, SH &sh, const GrpRange &R,
                                                         const GrpGlobal &gg, const GrpAux *__restrict__ aux,
                                                         int64_t i_begin, int n_e, int skip, int s_begin, bool first);

// Fused one-segment mode: the same stream over records made from incidences [i_begin, i_end) tile
// by tile (grp_tile_flat), each tile through the 2-bit reference when all of its records allow.
template <int K, class SH>
__device__ __forceinline__ void grp_scan_flat(const GrpBatch &B, SH &sh, const GrpRange &R, const GrpGlobal &gg,
                                              const GrpAux *__restrict__ aux, int64_t i_begin, int64_t i_end,
                                              int s_begin, int ns, bool first, int skip) {
  const int tid = threadIdx.x;
  // each tile's incidence reads are loaded while the previous tile streams (one dependent load,
  // the descriptor, left per tile); the first tile's by the caller (staged in sh.rec[tid].x)
  int r_next = sh.rec[tid].x;
  bool merged = false;
  for (int64_t c0 = i_begin; c0 < i_end; c0 += kGrpTile) {
    const int nh = (int)((i_end - c0) < kGrpTile ? (i_end - c0) : kGrpTile);
    const int r = r_next;
    const int64_t in = c0 + kGrpTile + tid;
    r_next = in < i_end ? aux->incid_read[in] : -1;
    bool clean;
    int nt = nh;   // (the last tile may take the extras records too)
    int total = grp_tile_flat(sh, B, aux, c0, nt, 16 * K, s_begin, ns, i_begin, first, r, clean, c0 + kGrpTile >= i_end,
                              merged);
    if (skip & kSkipChunks) total = 0;
    if (clean && B.ref2) {
      for (int t = tid; t < total; t += kGrpThreads) grp_chunk<K, true>(B, sh, R, gg, t, grp_find(sh, nt, total, t));
    } else {
      for (int t = tid; t < total; t += kGrpThreads) grp_chunk<K, false>(B, sh, R, gg, t, grp_find(sh, nt, total, t));
    }
    __syncthreads();
  }
  // multi-segment reads (short reads with an I/D/N op): their further segments, from the entries the
  // first pass listed — a segment's observations are those of any other record of its scope, so they
  // may come after the incidences: in the last tile's free slots (merged), else in extras tiles
  if (merged) return;
  if (first) {   // (the entries' stores at L2 before any thread reads them back)
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  const int n_e = sh.n_xent;
  if (n_e) grp_scan_extra<K>(B, sh, R, gg, aux, i_begin, n_e, skip, s_begin, first);
}

// Block-wide exclusive prefix sum of v (every thread calls; ends on a barrier); *total = the sum.
template <class SH>
__device__ __forceinline__ int blk_excl_sum(SH &sh, int v, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = ganon_wave::incl_sum(v);
  if (lane == 63) sh.wsum[wave] = incl;
  __syncthreads();
  int base = 0, t = 0;
#pragma unroll
  for (int w = 0; w < kGrpThreads / 64; ++w) {
    const int x = sh.wsum[w];
    base += w < wave ? x : 0;
    t += x;
  }
  *total = t;
  __syncthreads();   // (sh.wsum is free again)
  return base + incl - v;
}

// The fused mode's extras tiles: the group's n_e entries (an incidence of a multi-segment read each:
// its read's extras index, scope, further segments, dataset, write mark) expanded into the records
// of their further segments, as many whole entries per tile as fit its kGrpTile records (an entry
// has at most kFusedMaxSeg - 1), then streamed like any tile.
// Entries [e0, e0 + min(n_e - e0, kGrpTile)) of the group's list expanded into the records of their
// further segments at sh.rec[base + ...]: as many whole entries as fit the tile (every entry has 1 to
// kFusedMaxSeg - 1 records, so the fitting ones are a prefix). Returns the entries taken; *n_rec = the
// records written. Every thread calls; ends on a barrier.
template <class SH>
__device__ __attribute__((noinline)) int grp_xexpand(SH &sh, const GrpAux *__restrict__ aux, int64_t i_begin, int e0, int n_e,
                                           int base, int *n_rec, int s_begin, bool first) {
  const int tid = opaque_tid();
  const FlatScope *sc = flat_scopes(sh);
  const unsigned long long *xl = reinterpret_cast<const unsigned long long *>(aux->xlist) + i_begin;
  const int m = min(n_e - e0, kGrpTile);
  unsigned long long ent = 0;
  if (tid < m) ent = ld_l2(xl + e0 + tid);   // (written by this workgroup's first pass: read past L1)
  const uint32_t ey = (uint32_t)(ent >> 32);
  const int nx = tid < m ? (int)((ey >> 12) & 7) : 0;
  int total;
  const int pre = base + blk_excl_sum(sh, nx, &total);
  const bool fit = tid < m && pre + nx <= kGrpTile;
  if (fit) {
    const int j = (int)(ey & 0xFFF);
    const FlatScope S = sc[j];
    const int64_t r0 = (int64_t)(S.pk << 22) >> 22;
    const int r = (int)(uint32_t)ent;
    const uint32_t xi = (uint32_t)aux->xidx[r];
    const uint32_t hi = (((ey >> 15) & 1u) << 30) | (ey & kSegMine);
    // the read's span check (the tile checked its first segment's end only): a read reaching past
    // its scope's span is the batch's error, and its further segments stream nothing
    const int4 h = aux->xrec[xi];
    const int sl = (int)((S.pk >> 42) & ((1ull << 21) - 1));   // (entries are never made in huge scopes)
    const bool in_span = h.x >= S.sstart && (int64_t)h.y <= (int64_t)S.sstart + sl;
    if (!in_span && first) report(aux->err, kErrIncidSpan, s_begin + j, r);
    for (int k = 0; k < nx; ++k) {
      const int4 e = aux->xrec[xi + 1 + k];
      const uint32_t z = (uint32_t)e.z;
      const int n = in_span ? (int)((z >> 8) & kSegMaxLen) : 0, p = e.y;
      const uint64_t rf = (uint64_t)(r0 + p);
      const uint32_t rz = (z & 0x7Fu) | ((uint32_t)((rf >> 32) & 0xFF) << 8) | ((uint32_t)n << 16) | hi;
      sh.rec[pre + k] = make_int4(e.x, (int)(uint32_t)rf, (int)rz, (int)((uint32_t)j | ((uint32_t)(p - S.sstart) << 12)));
    }
  }
  const int used = __syncthreads_count(fit);
  if (fit && tid == used - 1) sh.n_xtile = pre + nx - base;
  __syncthreads();
  *n_rec = sh.n_xtile;
  return used;
}

// The fused mode's extras tiles (the further segments that did not fit the group's last tile): the
// group's n_e entries (an incidence of a multi-segment read each: its read's extras index, scope,
// further segments, dataset, write mark) expanded tile by tile, then streamed like any tile.
template <int K, class SH>
__device__ __forceinline__ void grp_scan_extra(const GrpBatch &B, SH &sh, const GrpRange &R,
                                                         const GrpGlobal &gg, const GrpAux *__restrict__ aux,
                                                         int64_t i_begin, int n_e, int skip, int s_begin, bool first) {
  const int tid = opaque_tid();
  const FlatScope *sc = flat_scopes(sh);
  for (int e0 = 0; e0 < n_e;) {
    int nh;
    const int used = grp_xexpand(sh, aux, i_begin, e0, n_e, 0, &nh, s_begin, first);
    int nck = 0;
    bool dirty = false;
    if (tid < nh) {
      const int4 r = sh.rec[tid];
      nck = ((((uint32_t)r.z >> 16) & kSegMaxLen) + 16 * K - 1) / (16 * K);
      dirty = (sc[r.w & 0xFFF].pk >> 63) != 0;
    }
    const bool clean = !__syncthreads_or(dirty);
    int tot = grp_tile_map(sh, nck);
    if (skip & kSkipChunks) tot = 0;
    if (clean && B.ref2) {
      for (int t = tid; t < tot; t += kGrpThreads) grp_chunk<K, true>(B, sh, R, gg, t, grp_find(sh, nh, tot, t));
    } else {
      for (int t = tid; t < tot; t += kGrpThreads) grp_chunk<K, false>(B, sh, R, gg, t, grp_find(sh, nh, tot, t));
    }
    __syncthreads();
    e0 += used;
  }
}

// In-LDS bitonic sort of n keys (n <= capacity rounded to a power of two); optional payload.
__device__ __forceinline__ void lds_bitonic(unsigned long long *key, unsigned long long *pay, int n) {
  const int tid = threadIdx.x;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int i = n + tid; i < n2; i += kGrpThreads) key[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += kGrpThreads) {
        const int ixj = i ^ j;
        if (ixj <= i) continue;
        const unsigned long long a = key[i], b = key[ixj];
        if ((a > b) == ((i & k) == 0)) {
          key[i] = b;
          key[ixj] = a;
          if (pay) {
            const unsigned long long p = pay[i];
            pay[i] = pay[ixj];
            pay[ixj] = p;
          }
        }
      }
      __syncthreads();
    }
  }
}

// Calls and masked bases into the per-scope and workgroup totals.
template <class SH>
__device__ __forceinline__ void grp_count(SH &sh, int s_local, int calls, int bases) {
  if (calls) {
    atomicAdd(&sh.cnt_calls[s_local], calls);
    atomicAdd(&sh.blk_calls, calls);
  }
  if (bases) {
    atomicAdd(&sh.cnt_bases[s_local], bases);
    atomicAdd(&sh.blk_bases, bases);
  }
}

// Observation list -> calls. Up to kGrpQuad observations every thread matches its own
// observation against the whole list (no sort, no barrier); longer lists are sorted and one
// thread takes each run of equal keys.
template <class SH>
__device__ __forceinline__ void grp_classify(const GrpBatch &B, SH &sh, int n, int s_begin,
                                             const PatchSink &sink) {
  const int tid = threadIdx.x;
  if (n <= kGrpQuad) {
    if (tid >= n) return;
    const unsigned long long key = sh.key[tid];
    int seen = 0;
    bool head = true;
    for (int j = 0; j < n; ++j) {
      if (sh.key[j] != key) continue;
      seen |= 1 << ((sh.pay[j] >> 52) & 1);
      head &= j >= tid;
    }
    if (seen != 3) return;
    const int s = s_begin + (int)(key >> 52);
    const int c = (int)(key & 15);
    if (grp_kept(B, s, (int64_t)((key >> 4) & kNibMask), c)) return;
    const unsigned long long p = sh.pay[tid];
    const int mine = (int)((p >> 53) & 1);
    if (mine) sink_patch(sh, sink, (int64_t)(p & kNibMask), c, (int)((p >> 48) & 15));
    grp_count(sh, s - s_begin, head ? 1 : 0, mine);
    return;
  }
  lds_bitonic(sh.key, sh.pay, n);
  for (int i = tid; i < n; i += kGrpThreads) {
    const unsigned long long key = sh.key[i];
    if (i > 0 && sh.key[i - 1] == key) continue;
    int e = i, seen = 0;
    while (e < n && sh.key[e] == key) seen |= 1 << ((sh.pay[e++] >> 52) & 1);
    if (seen != 3) continue;
    const int s = s_begin + (int)(key >> 52);
    const int c = (int)(key & 15);
    if (grp_kept(B, s, (int64_t)((key >> 4) & kNibMask), c)) continue;
    int masked = 0;
    for (int x = i; x < e; ++x) {
      const unsigned long long p = sh.pay[x];
      if (!((p >> 53) & 1)) continue;
      sink_patch(sh, sink, (int64_t)(p & kNibMask), c, (int)((p >> 48) & 15));
      ++masked;
    }
    grp_count(sh, s - s_begin, 1, masked);
  }
}

// An overflowing list (n > OBS: OBS in LDS, the rest in the group's global region) filtered by the
// pass's Bloom bitmaps: the LDS list is compacted in place to its keys seen in both datasets (a key
// seen in one can never be a TN call; the bitmaps have no false negatives), the region's surviving
// observations are appended after it as far as OBS. Returns all survivors; sh.n_obs = the LDS
// list's. The region itself is left as it was.
template <class SH>
__device__ __attribute__((noinline)) int grp_filter(SH &sh, const GrpGlobal &gg, int n) {
  constexpr int kPer = SH::kObs / kGrpThreads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  GU64 *okey = gp(gg.aux->okey) + gg.off, *opay = gp(gg.aux->opay) + gg.off;
  uint32_t *bloom = bloom_of(sh);
  for (int i = tid; i < 2 * kBloomBits / 32; i += kGrpThreads) bloom[i] = 0u;
  __builtin_amdgcn_s_waitcnt(0);   // the scan's region stores at L2
  __syncthreads();
  // the bitmaps: every stored observation's key, by dataset (payload bit 52)
  for (int i = opaque_tid(); i < n; i += kGrpThreads) {
    const unsigned long long key = i < SH::kObs ? sh.key[i] : ld_l2(okey + (i - SH::kObs));
    const unsigned long long pay = i < SH::kObs ? sh.pay[i] : ld_l2(opay + (i - SH::kObs));
    const uint32_t h = (bloom_hash(key) & (kBloomBits - 1)) + (uint32_t)((pay >> 52) & 1) * kBloomBits;
    atomicOr(bloom + (h >> 5), 1u << (h & 31));
  }
  __syncthreads();
  unsigned long long k[kPer], p[kPer];
  bool keep[kPer];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = tid + j * kGrpThreads;
    k[j] = sh.key[i];
    p[j] = sh.pay[i];
    keep[j] = bloom_both(sh, k[j]);
    cnt += keep[j] ? 1 : 0;
  }
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int x = __shfl_up(incl, o);
    if (lane >= o) incl += x;
  }
  if (lane == 63) sh.wsum[wave] = incl;
  if (tid == 0) sh.n_filt = 0;
  __syncthreads();   // (every thread holds its entries: the list can be rewritten)
  int base = incl - cnt, total = 0;
#pragma unroll
  for (int w = 0; w < kGrpThreads / 64; ++w) {
    const int v = sh.wsum[w];
    base += w < wave ? v : 0;
    total += v;
  }
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (keep[j]) {
      sh.key[base] = k[j];
      sh.pay[base] = p[j];
      ++base;
    }
  if (tid == 0) sh.n_obs = total;
  for (int i = opaque_tid(); i < n - SH::kObs; i += kGrpThreads) {
    const unsigned long long key = ld_l2(okey + i);
    if (!bloom_both(sh, key)) continue;
    const int slot = total + atomicAdd(&sh.n_filt, 1);
    if (slot < SH::kObs) {
      sh.key[slot] = key;
      sh.pay[slot] = ld_l2(opay + i);
    }
  }
  __syncthreads();
  return total + sh.n_filt;
}

// Overflow path: n observations of one key range sit in the group's global region. Aggregate
// them in a hash table of distinct keys (workgroup-scope atomics in L2), count the TN calls
// (minus the kept variant), and mask the observations of reads the scopes write.
template <class SH>
__device__ __forceinline__ void grp_global(const GrpBatch &B, SH &sh, const GrpGlobal &gg, int n,
                                           int s_begin, const PatchSink &sink) {
  const int tid = opaque_tid();
  const int tsize = max(2 * n, 64);
  GU64 *tk = gp(gg.aux->tkey) + 2 * gg.off;
  GU32 *tf = gp(gg.aux->tflag) + 2 * gg.off;
  GU64 *okey = gp(gg.aux->okey) + gg.off, *opay = gp(gg.aux->opay) + gg.off;
  for (int i = tid; i < tsize; i += kGrpThreads) {
    tk[i] = kEmpty;
    tf[i] = 0;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int i = tid; i < n; i += kGrpThreads) {
    const unsigned long long key = ld_l2(okey + i);
    const int ds = (int)((ld_l2(opay + i) >> 52) & 1);
    unsigned slot = gtab_home(key, tsize);
    for (int probe = 0; probe < tsize; ++probe) {
      unsigned long long expected = kEmpty;
      __hip_atomic_compare_exchange_strong(tk + slot, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
      if (expected == kEmpty || expected == key) {
        __hip_atomic_fetch_or(tf + slot, 1u << ds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        break;
      }
      if (++slot == (unsigned)tsize) slot = 0;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  // calls: one per TN slot
  for (int i = tid; i < tsize; i += kGrpThreads) {
    const unsigned long long key = ld_l2(tk + i);
    if (key == kEmpty || ld_l2(tf + i) != 3) continue;
    const int c = (int)(key & 15);
    if (grp_kept(B, s_begin + (int)(key >> 52), (int64_t)((key >> 4) & kNibMask), c)) continue;
    grp_count(sh, (int)(key >> 52), 1, 0);
  }
  // masks: every observation of a read the scope writes whose key is TN
  for (int i = tid; i < n; i += kGrpThreads) {
    const unsigned long long pay = ld_l2(opay + i);
    if (!((pay >> 53) & 1)) continue;
    const unsigned long long key = ld_l2(okey + i);
    unsigned slot = gtab_home(key, tsize);
    unsigned int f = 0;
    for (int probe = 0; probe < tsize; ++probe) {
      const unsigned long long k = ld_l2(tk + slot);
      if (k == key) {
        f = ld_l2(tf + slot);
        break;
      }
      if (k == kEmpty) break;
      if (++slot == (unsigned)tsize) slot = 0;
    }
    if (f != 3) continue;
    const int c = (int)(key & 15);
    if (grp_kept(B, s_begin + (int)(key >> 52), (int64_t)((key >> 4) & kNibMask), c)) continue;
    grp_count(sh, (int)(key >> 52), 0, 1);
    const int64_t nib = (int64_t)(pay & kNibMask);
    const int rc = (int)((pay >> 48) & 15);
    if (!sink.part || !sink.inside(nib >> 1)) {
      PatchSink direct = sink;
      direct.lds = false;
      sink_patch(sh, direct, nib, c, rc);   // (to the far list)
      continue;
    }
    okey[i] = ((unsigned long long)nib << 4) | (unsigned long long)(c ^ rc);   // in-partition mask
    opay[i] = pay | (1ull << 54);
  }
  if (!sink.part) return;
  // merge the in-partition masks per byte (the table area again, keyed by byte) and apply each
  // byte once, out[b] ^= mask — only this workgroup writes its partition
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int i = tid; i < tsize; i += kGrpThreads) {
    tk[i] = kEmpty;
    tf[i] = 0;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int i = tid; i < n; i += kGrpThreads) {
    const unsigned long long e = ld_l2(okey + i);
    const unsigned long long pay = ld_l2(opay + i);
    if (!((pay >> 54) & 1)) continue;                       // no in-partition mask
    const unsigned long long byte = e >> 5;
    unsigned slot = gtab_home(byte, tsize);
    for (int probe = 0; probe < tsize; ++probe) {
      unsigned long long expected = kEmpty;
      __hip_atomic_compare_exchange_strong(tk + slot, &expected, byte, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
      if (expected == kEmpty || expected == byte) {
        __hip_atomic_fetch_xor(tf + slot, (unsigned)(e & 15) << (((e >> 4) & 1) ? 0 : 4), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        break;
      }
      if (++slot == (unsigned)tsize) slot = 0;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int i = tid; i < tsize; i += kGrpThreads) {
    const unsigned long long byte = ld_l2(tk + i);
    if (byte == kEmpty) continue;
    const unsigned w = ld_l2(reinterpret_cast<const unsigned int *>(sink.out) + (byte >> 2));
    sink.out[byte] = (uint8_t)((w >> (8 * (byte & 3))) ^ ld_l2(tf + i));
  }
  __builtin_amdgcn_s_waitcnt(0);
}

// Apply the sorted in-partition list (nibble << 4 | from ^ to) with one plain byte store per
// masked byte, out[b] ^ mask — the partition copy and earlier masks of that byte were stored by
// this workgroup and have drained (read back from L2).
template <class SH>
__device__ __forceinline__ void grp_patch_bytes(SH &sh, int np, uint8_t *out) {
  for (int i = threadIdx.x; i < np; i += kGrpThreads) {
    const unsigned long long e = sh.patch[i];
    const int64_t byte = (int64_t)(e >> 5);
    if (i > 0 && (int64_t)(sh.patch[i - 1] >> 5) == byte) continue;
    uint32_t x = 0;
    for (int k = i; k < np && (int64_t)(sh.patch[k] >> 5) == byte; ++k) {
      const unsigned long long f = sh.patch[k];
      x ^= (uint32_t)(f & 15) << (((f >> 4) & 1) ? 0 : 4);
    }
    const unsigned w = ld_l2(reinterpret_cast<const unsigned int *>(out) + (byte >> 2));
    out[byte] = (uint8_t)((w >> (8 * (byte & 3))) ^ x);
  }
}

// After a classification: the in-partition masks it listed (at most one per observation of its
// list) as byte stores, once every wave's earlier stores have drained; the list is empty again.
template <class SH>
__device__ __forceinline__ void grp_apply_patches(SH &sh, uint8_t *out) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  const int np = sh.n_patch;
  if (np) {
    lds_bitonic(sh.patch, nullptr, np);
    grp_patch_bytes(sh, np, out);
    __builtin_amdgcn_s_waitcnt(0);
  }
  if (threadIdx.x == 0) sh.n_patch = 0;
}

// groups: kGrpRec x int4 per group, in launch order: {s_begin, s_end, seg_begin lo, hi},
// {seg_end lo, hi, seg_mid lo, hi}, {partition piece A begin lo, hi, end lo, hi} (bytes),
// {global region offset lo, hi, capacity, 0}, {piece B begin lo, hi, end lo, hi};
// segments [seg_begin, seg_mid) have an all-ACGT reference range (2-bit reference).
// FLAT: fused one-segment mode (records from incidences and read descriptors, grp_tile_flat; rec4
// unused; group record 1's mid ignored). LONG: long-read mode (records from the read records and
// incidence records, grp_tile_long; rec4 unused).
template <int U, bool PART, int OBS, bool FLAT, bool LONG = false>
__global__ void __launch_bounds__(kGrpThreads, (OBS > 512 ? 4 : U == 1 ? 6 : U == 2 ? GANON_K2_BLOCKS : U == 4 ? 5 : 4)) k_group(const GrpBatch B, const int4 *__restrict__ groups,
                                                       const int4 *__restrict__ rec4,
                                                       uint8_t *__restrict__ out, const GrpAux *__restrict__ aux,
                                                       int skip, int nt_copy, const unsigned long long *__restrict__ gate,
                                                       const int32_t *__restrict__ order) {
  __shared__ GrpSharedT<OBS> sh;
  const int tid = threadIdx.x;
  // the group this block runs: order[] (k_prep_order, longest first) when the batch has groups of
  // very unequal cost, else blockIdx (order[0] = -1); partials stay at the block's own slot
  int gid = blockIdx.x;
  if (order) {
    const int o0 = order[0];
    if (o0 >= 0) gid = blockIdx.x ? order[blockIdx.x] : o0;
  }
  // one-segment mode launches for the group bound: blocks past the scan's count (gate[5]) add
  // nothing; no block runs on a batch the scan rejected (gate[7])
  if (gate && (gate[7] || (unsigned long long)gid >= gate[5])) {
    if (tid == 0) {
      gp(aux->part)[2 * blockIdx.x] = 0;
      gp(aux->part)[2 * blockIdx.x + 1] = 0;
    }
    return;
  }
  const int4 g0 = groups[kGrpRec * gid];
  const int4 g1 = groups[kGrpRec * gid + 1];
  const int4 g2 = groups[kGrpRec * gid + 2];
  const int4 g3 = groups[kGrpRec * gid + 3];
  const int4 g4 = groups[kGrpRec * gid + 4];
  const GrpGlobal gg{aux, i64_of(g3.x, g3.y), g3.z};
  const int s_begin = g0.x, s_end = g0.y;
  const int64_t i_begin = i64_of(g0.z, g0.w), i_end = i64_of(g1.x, g1.y), i_mid = i64_of(g1.z, g1.w);
  const PatchSink sink{out, i64_of(g2.x, g2.y), i64_of(g2.z, g2.w), i64_of(g4.x, g4.y), i64_of(g4.z, g4.w),
                       aux, PART, PART};
  // the partition pieces, whole 16-byte windows (the buffers are padded past seq_bytes); the
  // stores drain while the scan runs (s_waitcnt before the mask stores). (Copying tile by tile,
  // each time up to the tile's written reads so that the scan's loads hit L2, read 0.34 GB less
  // per c2 launch but took 0.55 instead of 0.54 ms in the same build: DESIGN 5. Round 4 tried it
  // again in the fused one-segment kernel, each tile first copying the piece up to its last segment
  // byte: 0.665-0.679 vs 0.618 ms per pipelined c2 step, profiles/r04/tile_copy_ab.)
  // (FLAT: the first pass's scope table and first tile's reads are loaded before the copy, which
  // hides their latency)
  FlatScope fs{};
  int r_first = -1;
  int4 inc_rec{};   // (LONG) this thread's incidence record, staged after the scope table
  const bool inc_lds = LONG && (s_end - s_begin) + g3.w <= kGrpMaxScopes;
  if constexpr (FLAT || LONG) {
    if (tid < s_end - s_begin) fs = flat_load(B, aux, s_begin + tid, i_begin);
  }
  if constexpr (LONG) {
    if (inc_lds && tid < g3.w) inc_rec = aux->inc4[i_mid + tid];
  }
  if constexpr (FLAT) {
    if (i_begin + tid < i_end) r_first = aux->incid_read[i_begin + tid];
  }
  if (PART && !(skip & kSkipCopy)) {
    copy_windows(B.seq, out, sink.p0, sink.p1, nt_copy);
    copy_windows(B.seq, out, sink.q0, sink.q1, nt_copy);
  }
  // (staged for the first pass now: registers carried into the pass loop would stay live through
  // the classification and spill)
  if constexpr (FLAT || LONG) {
    if (tid < s_end - s_begin) flat_scopes(sh)[tid] = fs;
  }
  if constexpr (LONG) {
    if (inc_lds && tid < g3.w) reinterpret_cast<int4 *>(flat_scopes(sh) + (s_end - s_begin))[tid] = inc_rec;
  }
  if constexpr (FLAT) sh.rec[tid].x = r_first;   // (read by the first tile before it writes sh.rec)
  if (tid == 0) {
    sh.top = 0;
    sh.stk_lo[0] = 0ull;
    sh.stk_hi[0] = ~0ull;
    sh.stk_mode[0] = 0;
    sh.n_patch = 0;
    sh.blk_calls = 0;
    sh.blk_bases = 0;
    sh.hsum = 0;
    sh.n_xent = 0;
    sh.n_xrec = 0;
  }
  for (int i = tid; i < kGrpMaxScopes; i += kGrpThreads) {
    sh.cnt_calls[i] = 0;
    sh.cnt_bases[i] = 0;
  }
  bool first = true;   // (FLAT) the group's first pass makes the incidence checks and the hash sum
  for (;;) {
    __syncthreads();
    const int top = sh.top;
    if (top < 0) {
      // per-scope counts (wide scopes in the id range belong to the tile path) and the
      // workgroup's partial totals (k_finish sums them)
      for (int i = opaque_tid(); i < ((skip & kSkipCounts) ? 0 : s_end - s_begin); i += kGrpThreads) {
        if (B.span_len[s_begin + i] > kGrpMaxSpan) continue;
        gp(aux->scope_calls)[s_begin + i] = sh.cnt_calls[i];
        gp(aux->scope_bases)[s_begin + i] = sh.cnt_bases[i];
      }
      if (tid == 0) {
        gp(aux->part)[2 * blockIdx.x] = sh.blk_calls;
        gp(aux->part)[2 * blockIdx.x + 1] = sh.blk_bases;
        if (FLAT) gp(aux->ws_part)[gid] = sh.hsum;
      }
      break;
    }
    const GrpRange R{sh.stk_lo[top], sh.stk_hi[top], sh.stk_mode[top]};
    __syncthreads();
    if (tid == 0) {
      sh.top = top - 1;
      sh.n_obs = 0;
      sh.kmin = ~0ull;
      sh.kmax = 0ull;
    }
    __syncthreads();
    if constexpr (FLAT) {
      // the scope table (patch list space: the previous pass's classification is done with it)
      if (!first) {   // (staged again: a pass after a key-range split)
        if (tid < s_end - s_begin) flat_scopes(sh)[tid] = flat_load(B, aux, s_begin + opaque_tid(), i_begin);
        sh.rec[tid].x = i_begin + tid < i_end ? aux->incid_read[i_begin + opaque_tid()] : -1;
      }
      __syncthreads();
      grp_scan_flat<U>(B, sh, R, gg, aux, i_begin, i_end, s_begin, s_end - s_begin, first, skip);
      first = false;
    } else if constexpr (LONG) {
      const int ns = s_end - s_begin;
      int4 *itab = reinterpret_cast<int4 *>(flat_scopes(sh) + ns);
      if (!first) {   // (staged again: a pass after a key-range split)
        if (tid < ns) flat_scopes(sh)[tid] = flat_load(B, aux, s_begin + opaque_tid(), i_begin);
        if (inc_lds && tid < g3.w) itab[tid] = aux->inc4[i_mid + opaque_tid()];
      }
      __syncthreads();
      // (i_mid: the group's first incidence, g3.w: its incidence count)
      grp_scan_long<U>(B, sh, R, gg, aux, i_begin, i_end, i_mid, g3.w, inc_lds ? itab : nullptr, skip);
      first = false;
    } else if (B.ref2) {
      grp_scan<U, true>(B, sh, R, gg, i_begin, i_mid, rec4, skip);
      grp_scan<U, false>(B, sh, R, gg, i_mid, i_end, rec4, skip);
    } else {
      grp_scan<U, false>(B, sh, R, gg, i_begin, i_end, rec4, skip);
    }
    // (grp_scan ends on a barrier)
    if (skip & kSkipClassify) continue;
    int n = sh.n_obs;
    if (tid == 0 && n > kGrpQuad)   // path counters (ganon_batch_path_counts): sorted list, region, split
      __hip_atomic_fetch_add(gp(aux->paths) + (n <= OBS ? 0 : n <= gg.cap ? 1 : 2), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n > OBS) {
      if (n <= gg.cap) {
        // drop the observations whose key was not seen in both datasets (Bloom bitmaps): when the
        // rest fits in the LDS list, it is classified there like a short list
        const int m = GANON_GRP_BLOOM ? grp_filter(sh, gg, n) : OBS + 1;
        if (m <= OBS) {
          if (tid == 0)   // (counted as a region pass above too)
            __hip_atomic_fetch_add(gp(aux->paths) + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          grp_classify(B, sh, m, s_begin, sink);
          if (sink.lds) grp_apply_patches(sh, out);
          continue;
        }
        // the list (its kept part: m - survivors of the region beyond it) joins the region's
        // tail: the region's own entries are untouched
        const int ml = GANON_GRP_BLOOM ? sh.n_obs : OBS;   // (grp_filter: the kept part of the LDS list)
        n = (n - OBS) + ml;
        for (int i = opaque_tid(); i < ml; i += kGrpThreads) {
          gp(aux->okey)[gg.off + (n - ml) + i] = sh.key[i];
          gp(aux->opay)[gg.off + (n - ml) + i] = sh.pay[i];
        }
        __builtin_amdgcn_s_waitcnt(0);   // region stores at L2 before the barrier
        __syncthreads();
        grp_global(B, sh, gg, n, s_begin, sink);
        continue;
      }
      // the region overflowed too (more than ~2 % of the bases mismatch): split [R.lo, R.hi)
      // at the middle of the stored keys' range — both halves keep stored keys, and a single key
      // never fills a region (capacity > 3 x the group's reads)
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();
      for (int i = opaque_tid(); i < gg.cap; i += kGrpThreads) {
        const unsigned long long k = i < OBS ? sh.key[i] : ld_l2(gp(aux->okey) + gg.off + (i - OBS));
        atomicMin(&sh.kmin, k);
        atomicMax(&sh.kmax, k);
      }
      __syncthreads();
      if (tid == 0) {
        const unsigned long long a = sh.kmin, b = sh.kmax, mid = a + (b - a) / 2 + 1;
        int t = sh.top;
        if (a < b && t + 2 < kGrpStack) {
          ++t;
          sh.stk_lo[t] = mid;
          sh.stk_hi[t] = R.hi;
          sh.stk_mode[t] = 0;
          ++t;
          sh.stk_lo[t] = R.lo;
          sh.stk_hi[t] = mid;
          sh.stk_mode[t] = 0;
        }
        sh.top = t;
      }
      continue;
    }
    grp_classify(B, sh, n, s_begin, sink);
    if (sink.lds) grp_apply_patches(sh, out);
  }
}

// The compiled k_group instantiations, one table for the three families (FLAT fused, LONG, record
// pass): unroll 1, 2, 4, 8 with the 512-entry observation list, 1 and 2 with the 1024-entry one.
// Null: the pair is not compiled (ganon_batch_run refuses it; no other pair runs in its place).
using GroupKernel = void (*)(const GrpBatch, const int4 *, const int4 *, uint8_t *, const GrpAux *, int, int,
                             const unsigned long long *, const int32_t *);
template <bool FLAT, bool LONG>
GroupKernel group_kernel_of(int u, int obs) {
  if (obs == 512) {
    switch (u) {
      case 1: return k_group<1, true, 512, FLAT, LONG>;
      case 2: return k_group<2, true, 512, FLAT, LONG>;
      case 4: return k_group<4, true, 512, FLAT, LONG>;
      case 8: return k_group<8, true, 512, FLAT, LONG>;
    }
  } else if (obs == 1024) {
    switch (u) {
      case 1: return k_group<1, true, 1024, FLAT, LONG>;
      case 2: return k_group<2, true, 1024, FLAT, LONG>;
    }
  }
  return nullptr;
}
GroupKernel group_kernel(bool fused, bool long_mode, int u, int obs) {
  return fused ? group_kernel_of<true, false>(u, obs)
               : long_mode ? group_kernel_of<false, true>(u, obs) : group_kernel_of<false, false>(u, obs);
}

}  // namespace

namespace ganon_group {

bool compiled(bool fused, bool long_mode, int unroll, int obs) {
  return group_kernel(fused, long_mode, unroll, obs) != nullptr;
}

int launch(ganon_ctx *ctx, ganon_dbatch *db, int unroll, int obs, const uint32_t *ref2) {
  ganon_detail::KernelScope ks(ctx, "k_group_fused");   // (the label bench.py and the tools classify by)
  const GroupKernel kern = group_kernel(db->fused, db->long_mode, unroll, obs);
  const DevBatch &B = db->B;
  const GrpBatch GB{B.seq, B.ref, B.keep_code, ref2, B.keep_pos, B.span_start, B.span_len};
  kern<<<db->n_groups, kGrpThreads, 0, ctx->stream>>>(GB, static_cast<const int4 *>(db->b_groups.p),
                                                      static_cast<const int4 *>(db->b_seg4.p), db->out, db->aux,
                                                      ctx->group_skip, ctx->nt_copy,
                                                      db->flat_mode ? db->plan_info : nullptr,
                                                      db->ordered ? static_cast<const int32_t *>(db->b_order.p) : nullptr);
  return ganon_detail::check_launch(ctx, "k_group");
}

}  // namespace ganon_group
