// ganon_huge.hip — the huge-scope tile path (ganon_huge, ganon_batch.h): scopes wider than
// kGrpMaxSpan positions, which the group kernels (ganon_group.hip) leave out. The host plans
// 16 Ki-position tiles at upload; k_tile_large tallies each tile in LDS and writes the
// tumor-and-normal table, k_mask_large writes the reads of those scopes from it. Their
// per-scope counts join the totals in k_finish (ganon_hip.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/ganon.h"
#include "ganon_batch.h"
#include "ganon_ctx.h"

using namespace ganon_dev;

namespace {

// Per-lane monotone walk over a read's CIGAR: query positions visited in increasing order.
struct CigarCursor {
  const uint32_t *cig;
  int n, k;
  int q0;        // first query position of op k
  int r0;        // first reference position of op k
  int qlen, rlen, op;

  __device__ __forceinline__ void load() {
    if (k < n) {
      const uint32_t w = cig[k];
      op = w & 0xF;
      const int len = (int)(w >> 4);
      qlen = (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? len : 0;
      rlen = (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;
    }
  }
  __device__ __forceinline__ void init(const uint32_t *c, int nc, int ref_start) {
    cig = c; n = nc; k = 0; q0 = 0; r0 = ref_start; qlen = rlen = 0; op = 0;
    load();
  }
  // Returns the reference position aligned to query position q (M/=/X), or -1 when q sits
  // in an I/S op or beyond the CIGAR. q must not decrease between calls.
  __device__ __forceinline__ int ref_of(int q) {
    while (k < n && q >= q0 + qlen) {
      q0 += qlen; r0 += rlen; ++k;
      load();
    }
    if (k >= n) return -1;
    if (op == 0 || op == 7 || op == 8) return r0 + (q - q0);
    return -1;
  }
};

__device__ __forceinline__ int block_sum(int v, int *scratch) {
  // wave reduction then LDS across waves; scratch holds kWaves ints.
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += scratch[w];
  return t;
}

// ---- tally of one read into the LDS table covering [a, b) ------------------------------
// TB = bytes per position: 1 (ACGT nibbles) or 4 (16-code masks). Returns true when a
// non-ACGTN base that would be a call was seen (only meaningful for TB == 1).
// Reference nibble of contig position p, staged in LDS (nibble 0 = position a).
struct LdsRef {
  const uint8_t *refb;
  int a;
  __device__ __forceinline__ int operator()(int p) const {
    const int off = p - a;
    return (refb[off >> 1] >> ((off & 1) ? 0 : 4)) & 0xF;
  }
};

template <int TB, typename RefFn>
__device__ __forceinline__ bool tally_read(const DevBatch &B, int r, int a, int b,
                                           uint32_t *tab, const RefFn &refn, int lane) {
  const int L = B.read_len[r];
  const int ds = B.dataset[r];
  const int64_t sq = B.seq_off[r] * 2;
  CigarCursor cur;
  cur.init(B.cigar + B.cig_off[r], B.n_cig[r], B.ref_start[r]);
  bool rare = false;
  for (int q = lane; q < L; q += 64) {
    const int p = cur.ref_of(q);
    if (p < a || p >= b) continue;
    const int c = nib_at(B.seq, sq + q);
    const int off = p - a;
    const int rc = refn(p);
    if (c == 15 || c == rc || !is_acgt(rc)) continue;
    if (TB == 1) {
      if (is_acgt(c)) atomicOr(&tab[off >> 2], (uint32_t)c << (ds * 4 + (off & 3) * 8));
      else rare = true;
    } else {
      atomicOr(&tab[off], (1u << c) << (16 * ds));
    }
  }
  return rare;
}

template <int TB>
__device__ __forceinline__ uint32_t tn_mask(const uint32_t *tab, int off) {
  if (TB == 1) {
    const uint32_t byte = (tab[off >> 2] >> ((off & 3) * 8)) & 0xFF;
    return byte & (byte >> 4) & 0xF;                  // ACGT one-hot codes
  } else {
    const uint32_t w = tab[off];
    return w & (w >> 16) & 0xFFFF;                    // bit c = code c
  }
}

template <int TB>
__device__ __forceinline__ int tn_count(uint32_t tn) { return __popc(tn); }

// Stage the reference nibbles of [a, a + span) into LDS (packed, nibble 0 = position a).
__device__ __forceinline__ void stage_ref(const DevBatch &B, int64_t nib0, int span, uint8_t *refb) {
  const int nbytes = (span + 1) >> 1;
  for (int j = threadIdx.x; j < nbytes; j += kBlock) {
    const int64_t n0 = nib0 + 2 * (int64_t)j;
    const int hi = nib_at(B.ref, n0);
    const int lo = (2 * j + 1 < span) ? nib_at(B.ref, n0 + 1) : 0;
    refb[j] = (uint8_t)((hi << 4) | lo);
  }
}

// Clear the tumor bit of the kept allele so the kept call is neither masked nor counted.
template <int TB>
__device__ __forceinline__ void clear_keep(const DevBatch &B, int s, int a, int b, uint32_t *tab) {
  if (threadIdx.x != 0) return;
  const int kp = B.keep_pos[s];
  if (kp < a || kp >= b) return;
  const int kc = B.keep_code[s];
  const int off = kp - a;
  if (TB == 1) {
    if (is_acgt(kc)) atomicAnd(&tab[off >> 2], ~((uint32_t)kc << ((off & 3) * 8)));
  } else {
    atomicAnd(&tab[off], ~(1u << kc));
  }
}

// One workgroup per 16 Ki-position tile of a large scope: tally -> TN table (global).
template <int TB>
__global__ void __launch_bounds__(kBlock) k_tile_large(const DevBatch B, const Tile *__restrict__ tiles,
                                                       const int32_t *__restrict__ tile_list, int n_static,
                                                       const int32_t *count_ptr, const int32_t *__restrict__ large_incid,
                                                       const int64_t *__restrict__ tab_off, uint16_t *__restrict__ tn_tab,
                                                       int32_t *scope_calls, int32_t *rare_list, int32_t *rare_count) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int tab_words = kTile * TB / 4;
  uint32_t *tab = smem;
  uint8_t *refb = reinterpret_cast<uint8_t *>(smem + tab_words);
  int *scratch = reinterpret_cast<int *>(refb + kTile / 2);
  const int n = count_ptr ? *count_ptr : n_static;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int li = blockIdx.x; li < n; li += gridDim.x) {
    const int ti = tile_list ? tile_list[li] : li;
    const Tile t = tiles[ti];
    const int s = t.scope;
    const int span = t.b - t.a;
    const int words = (span * TB + 3) >> 2;
    for (int w = threadIdx.x; w < words; w += kBlock) tab[w] = 0;
    stage_ref(B, B.ref_off[s] + (t.a - B.span_start[s]), span, refb);
    if (threadIdx.x == 0) scratch[kWaves] = 0;
    __syncthreads();
    bool rare = false;
    for (int64_t i = t.lo + wave; i < t.hi; i += kWaves) {
      const int r = large_incid[i];
      if (B.read_end[r] <= t.a || B.ref_start[r] >= t.b) continue;
      rare |= tally_read<TB>(B, r, t.a, t.b, tab, LdsRef{refb, t.a}, lane);
    }
    if (TB == 1 && rare) scratch[kWaves] = 1;
    __syncthreads();
    clear_keep<TB>(B, s, t.a, t.b, tab);
    __syncthreads();
    int calls = 0;
    uint16_t *dst = tn_tab + tab_off[s] + (t.a - B.span_start[s]);
    for (int off = threadIdx.x; off < span; off += kBlock) {
      const uint32_t tn = tn_mask<TB>(tab, off);
      uint32_t m16;
      if (TB == 1) m16 = ((tn & 1u) << 1) | ((tn & 2u) << 1) | ((tn & 4u) << 2) | ((tn & 8u) << 5);
      else m16 = tn;
      dst[off] = (uint16_t)m16;
      calls += tn_count<TB>(tn);
    }
    calls = block_sum(calls, scratch);
    if (threadIdx.x == 0) {
      const bool is_rare = (TB == 1) && scratch[kWaves];
      if (is_rare) rare_list[atomicAdd(rare_count, 1)] = ti;
      else if (calls) atomicAdd(&scope_calls[s], calls);
    }
    __syncthreads();
  }
}

// Reads written from large scopes: one wave per read, TN table lookups in global memory.
__global__ void __launch_bounds__(kBlock) k_mask_large(const DevBatch B, const int32_t *__restrict__ list, int n,
                                                       const int64_t *__restrict__ tab_off,
                                                       const uint16_t *__restrict__ tn_tab,
                                                       uint8_t *__restrict__ out, int32_t *scope_bases) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int nw = (gridDim.x * kBlock) >> 6;
  for (int i = gw; i < n; i += nw) {
    const int r = list[i];
    const int s = B.write_scope[r];
    const int a = B.span_start[s];
    const int64_t to = tab_off[s];
    const int64_t rnib = B.ref_off[s];
    const int L = B.read_len[r];
    const int64_t so = B.seq_off[r];
    CigarCursor cur;
    cur.init(B.cigar + B.cig_off[r], B.n_cig[r], B.ref_start[r]);
    int masked = 0;
    for (int j = lane; j < ((L + 1) >> 1); j += 64) {
      const uint8_t in = B.seq[so + j];
      int nb[2] = {in >> 4, in & 0xF};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = 2 * j + h;
        if (q >= L) break;
        const int p = cur.ref_of(q);
        if (p < 0) continue;
        const uint32_t tn = tn_tab[to + (p - a)];
        if ((tn >> nb[h]) & 1u) {
          nb[h] = nib_at(B.ref, rnib + (p - a));
          ++masked;
        }
      }
      out[so + j] = (uint8_t)((nb[0] << 4) | nb[1]);
    }
    for (int o = 32; o > 0; o >>= 1) masked += __shfl_xor(masked, o);
    if (lane == 0 && masked) atomicAdd(&scope_bases[s], masked);
  }
}

}  // namespace
// ---- host side ---------------------------------------------------------------------------

using ganon_detail::check_launch;
using ganon_detail::fail;
using ganon_detail::KernelScope;

namespace {

size_t tile_lds_bytes(int tb) { return (size_t)kTile * tb + kTile / 2 + 16 * sizeof(int); }

template <typename T>
int dmalloc(ganon_ctx *ctx, std::vector<void *> &allocs, T **p, size_t count) {
  *p = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T) + 128;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(p), bytes);
  if (e != hipSuccess) return fail(ctx, GANON_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  allocs.push_back(*p);
  return GANON_OK;
}

// bam_endpos of read r from the host batch (huge-scope planning only).
int32_t host_read_end(const ganon_batch *b, int32_t r) {
  int64_t rl = 0;
  for (int k = 0; k < b->n_cig[r]; ++k) {
    const uint32_t w = b->cigar[b->cig_off[r] + k];
    const int op = w & 0xF;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += w >> 4;
  }
  return (int32_t)(b->ref_start[r] + (rl > 0 ? rl : 1));
}

}  // namespace

namespace ganon_huge {

void init() {
  hipFuncSetAttribute(reinterpret_cast<const void *>(k_tile_large<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)tile_lds_bytes(1));
  hipFuncSetAttribute(reinterpret_cast<const void *>(k_tile_large<4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)tile_lds_bytes(4));
}

void release(ganon_dbatch *db) {
  for (void *p : db->huge_allocs) hipFree(p);
  db->huge_allocs.clear();
  db->tiles_h = nullptr;
  db->large_incid = db->large_written_h = db->large_ids = db->rare_tile_list = nullptr;
  db->tab_off = nullptr;
  db->tn_tab = nullptr;
  db->n_tiles_h = db->n_large_written_h = 0;
  db->tn_entries = 0;
}

// Scopes wider than kGrpMaxSpan (whole-contig union scopes of very deep samples; none in the
// benchmark configs): 16 Ki-position tiles planned on the host from the scopes' incidences.
int plan(ganon_ctx *ctx, ganon_dbatch *db, const ganon_batch *b) {
  release(db);
  if (!db->n_huge_scopes) return GANON_OK;
  std::vector<int32_t> large_incid, ids, written;
  std::vector<int64_t> tab_off((size_t)b->n_scopes, -1);
  std::vector<Tile> tiles;
  int64_t tn_entries = 0;
  for (int32_t s = 0; s < b->n_scopes; ++s) {
    const int32_t sl = b->scope_span_len[s];
    if (sl <= kGrpMaxSpan) continue;
    ids.push_back(s);
    tab_off[s] = tn_entries;
    tn_entries += sl;
    const int64_t base = (int64_t)large_incid.size();
    for (int64_t i = b->scope_incid_off[s]; i < b->scope_incid_off[s + 1]; ++i) large_incid.push_back(b->incid_read[i]);
    std::stable_sort(large_incid.begin() + base, large_incid.end(),
                     [&](int32_t x, int32_t y) { return b->ref_start[x] < b->ref_start[y]; });
    int32_t maxspan = 1;
    for (int64_t i = base; i < (int64_t)large_incid.size(); ++i) {
      const int32_t r = large_incid[i];
      maxspan = std::max(maxspan, host_read_end(b, r) - b->ref_start[r]);
    }
    const int32_t ss = b->scope_span_start[s];
    for (int64_t a = ss; a < (int64_t)ss + sl; a += kTile) {
      Tile t{};
      t.scope = s;
      t.a = (int32_t)a;
      t.b = (int32_t)std::min<int64_t>(a + kTile, (int64_t)ss + sl);
      auto first = large_incid.begin() + base;
      auto last = large_incid.end();
      t.lo = std::lower_bound(first, last, (int64_t)t.a - maxspan,
                              [&](int32_t r, int64_t key) { return (int64_t)b->ref_start[r] < key; }) -
             large_incid.begin();
      t.hi = std::lower_bound(first, last, (int64_t)t.b,
                              [&](int32_t r, int64_t key) { return (int64_t)b->ref_start[r] < key; }) -
             large_incid.begin();
      tiles.push_back(t);
    }
  }
  for (int32_t r = 0; r < b->n_reads; ++r) {
    const int32_t ws = b->write_scope[r];
    if (ws >= 0 && b->scope_span_len[ws] > kGrpMaxSpan) written.push_back(r);
  }
  int rc;
  auto up = [&](auto **p, const auto &v) -> int {
    using T = std::remove_const_t<std::remove_reference_t<decltype(v[0])>>;
    T *q = nullptr;
    int c = dmalloc(ctx, db->huge_allocs, &q, v.size());
    if (c) return c;
    if (!v.empty() && hipMemcpyAsync(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      return fail(ctx, GANON_E_DEVICE, "huge-scope plan copy failed");
    *p = q;
    return GANON_OK;
  };
  if ((rc = up(&db->tiles_h, tiles)) || (rc = up(&db->large_incid, large_incid)) || (rc = up(&db->tab_off, tab_off)) ||
      (rc = up(&db->large_written_h, written)) || (rc = up(&db->large_ids, ids)))
    return rc;
  if ((rc = dmalloc(ctx, db->huge_allocs, &db->rare_tile_list, tiles.size()))) return rc;
  db->n_tiles_h = (int32_t)tiles.size();
  db->n_large_written_h = (int32_t)written.size();
  db->tn_entries = tn_entries;
  return GANON_OK;
}

int run(ganon_ctx *ctx, ganon_dbatch *db) {
  if (!db->n_tiles_h) return GANON_OK;
  hipStream_t st = ctx->stream;
  const DevBatch &B = db->B;
  int rc;
  if (!db->tn_tab && (rc = dmalloc(ctx, db->huge_allocs, &db->tn_tab, (size_t)db->tn_entries))) return rc;
  {
    KernelScope ks(ctx, "k_tile_large<1>");
    k_tile_large<1><<<db->n_tiles_h, kBlock, tile_lds_bytes(1), st>>>(
        B, db->tiles_h, nullptr, db->n_tiles_h, nullptr, db->large_incid, db->tab_off, db->tn_tab, db->scope_calls,
        db->rare_tile_list, db->rare_tiles);
    if ((rc = check_launch(ctx, "k_tile_large<1>"))) return rc;
  }
  {
    // tiles that met a non-ACGTN base: re-run on the 16-code tally (count stays on the device)
    KernelScope ks(ctx, "k_tile_large<4>/rare");
    k_tile_large<4><<<std::min<int>(db->n_tiles_h, 1024), kBlock, tile_lds_bytes(4), st>>>(
        B, db->tiles_h, db->rare_tile_list, 0, db->rare_tiles, db->large_incid, db->tab_off, db->tn_tab,
        db->scope_calls, nullptr, nullptr);
    if ((rc = check_launch(ctx, "k_tile_large<4>"))) return rc;
  }
  if (db->n_large_written_h) {
    KernelScope ks(ctx, "k_mask_large");
    const int grid = std::min<int>((db->n_large_written_h + kWaves - 1) / kWaves, 8192);
    k_mask_large<<<grid, kBlock, 0, st>>>(B, db->large_written_h, db->n_large_written_h, db->tab_off, db->tn_tab,
                                          db->out, db->scope_bases);
    if ((rc = check_launch(ctx, "k_mask_large"))) return rc;
  }
  return GANON_OK;
}

}  // namespace ganon_huge
