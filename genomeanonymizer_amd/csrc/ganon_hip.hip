// ganon_hip.hip — MI355X (gfx950) germline-variant masking kernels + the C ABI of
// include/ganon.h (libganon_hip.so).
//
// Reference semantics (per scope = one CompleteGermlineAnonymizer.anonymize call,
// anonymizer_methods.py:431-535):
//   tally     process_snv for every aligned base of every scope read
//             (variation_classifier.py:144-182, :185-215): base != 'N', base != ref,
//             ref in ACGT -> observation (pos, allele, tumor|normal);
//   classify  SomaticVariationType state machine (variants.py:33-39): a call ends in
//             TUMORAL_NORMAL_VARIANT iff it was observed in >=1 tumor AND >=1 normal read;
//   mask      at the normal column: every supporting read of a TN call other than the
//             kept window variant gets the reference base (anonymizer_methods.py:537-556,
//             :170-176); the call is counted for the statistics (:555-556).
//
// Design: integer/byte work, HBM-bound — no MFMA. A run is
//   device prep (ganon_prep.hip): the raw SoA -> segment records, scope groups, partitions;
//   k_group (ganon_group.hip): one 256-thread workgroup per scope group copies its partition
//             pieces of the output and streams every aligned base of its scopes in 32-base chunks;
//             mismatches become LDS observations, classified per (scope, position, allele);
//   k_tile_large + k_mask_large (ganon_huge.hip): scopes wider than 1 Mi positions (16 Ki-position
//             LDS tiles);
//   k_finish: far masks, totals.
// The reference genome is resident (ganon_ref): nt16 + a 2-bit copy + a non-ACGT block map.
// This file: the context, the pinned pool, the reference upload (k_ref2), batch upload / reload /
// replan, the run's orchestration, k_finish, download and the ABI entry points.
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ganon.h"
#include "ganon_batch.h"
#include "ganon_ctx.h"

using namespace ganon_dev;

namespace {

// ---- 2-bit reference ----------------------------------------------------------------------
// Word w = bases [16w, 16w + 16) of ref_nt16 as 2-bit codes (A0 C1 G2 T3; base i at bits
// 2 * (i & 15)). Non-ACGT bases get code 0: only segments whose reference range is all ACGT
// (ordered first in their group at upload) read this copy — half the bytes, fewer lines.
__global__ void __launch_bounds__(kBlock) k_ref2(const uint8_t *__restrict__ ref, int64_t n_words,
                                                 uint32_t *__restrict__ ref2) {
  for (int64_t w = blockIdx.x * (int64_t)kBlock + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * kBlock) {
    const uint64_t v = load16(ref, 16 * w);
    uint32_t code = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = (int)((v >> (4 * k)) & 15);
      if (is_acgt(c)) code |= (uint32_t)__builtin_ctz(c) << (2 * k);
    }
    ref2[w] = code;
  }
}

// Last kernel of a run. (1) Far masks: masks of bytes outside the masking workgroup's
// partition (every partition is written by now). (2) Totals: the group
// workgroups' partials plus the wide scopes' counts, reduced per workgroup into acc; the last
// workgroup to finish (ticket acc[2]) writes totals = static values + sums + rare counts and
// resets acc and the rare-tile count for the next run — no memset or copy is launched per run.
// rare_tiles: tiles of huge scopes that met a non-ACGTN base (k_tile_large); far_count: far masks.
__global__ void __launch_bounds__(kBlock) k_finish(const unsigned long long *__restrict__ far, int64_t far_cap,
                                                   uint8_t *__restrict__ out, const int32_t *__restrict__ grp_part,
                                                   int n_groups, const int32_t *__restrict__ large_ids, int n_large,
                                                   const int32_t *__restrict__ scope_calls,
                                                   const int32_t *__restrict__ scope_bases,
                                                   const unsigned long long *__restrict__ static_totals,
                                                   int32_t *rare_tiles, unsigned long long *far_count,
                                                   int32_t *status, unsigned long long *acc,
                                                   unsigned long long *far_need,
                                                   unsigned long long *totals,
                                                   const unsigned long long *__restrict__ ws_part,
                                                   const unsigned long long *__restrict__ plan_info,
                                                   unsigned long long *gated) {
  const int64_t gtid = blockIdx.x * (int64_t)kBlock + threadIdx.x, gstride = (int64_t)gridDim.x * kBlock;
  const unsigned long long far_n = *far_count;
  const int64_t n_far = far_n < (unsigned long long)far_cap ? (int64_t)far_n : far_cap;
  for (int64_t i = gtid; i < n_far; i += gstride) {
    const unsigned long long e = far[i];
    const int64_t nib = (int64_t)(e >> 4);
    const int64_t byte = nib >> 1;
    const int sh = 8 * (int)(byte & 3) + ((nib & 1) ? 0 : 4);
    atomicXor(reinterpret_cast<uint32_t *>(out) + (byte >> 2), (uint32_t)(e & 15) << sh);
  }
  long long c = 0, b = 0;
  unsigned long long h = 0;   // write-scope hash sums of the emit paths (one per group)
  for (int64_t i = gtid; i < n_groups; i += gstride) {
    c += grp_part[2 * i];
    b += grp_part[2 * i + 1];
    h += ws_part[i];
  }
  for (int64_t i = gtid; i < n_large; i += gstride) {
    c += scope_calls[large_ids[i]];
    b += scope_bases[large_ids[i]];
  }
  __shared__ long long part[3][kWaves];
  __shared__ int last;
  for (int o = 32; o > 0; o >>= 1) {
    c += __shfl_xor(c, o);
    b += __shfl_xor(b, o);
    h += __shfl_xor(h, o);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = c;
    part[1][threadIdx.x >> 6] = b;
    part[2][threadIdx.x >> 6] = (long long)h;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    c = b = 0;
    h = 0;
    for (int w = 0; w < kWaves; ++w) {
      c += part[0][w];
      b += part[1][w];
      h += (unsigned long long)part[2][w];
    }
    if (c) atomicAdd(&acc[0], (unsigned long long)c);
    if (b) atomicAdd(&acc[1], (unsigned long long)b);
    if (h) atomicAdd(&acc[4], h);
    __threadfence();
    last = atomicAdd(&acc[2], 1ull) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  __threadfence();
  const unsigned long long sc = atomicExch(&acc[0], 0ull), sb = atomicExch(&acc[1], 0ull);
  atomicExch(&acc[2], 0ull);
  // every written read met once in its write scope (k_prep_scan's sum vs the emit paths'); a gated
  // run (plan_info[7]: a speculative plan the batch did not fit, or an invalid batch) ran no
  // one-segment kernel: ganon_batch_download plans and runs it again (or reports the error)
  const unsigned long long hs = atomicExch(&acc[4], 0ull);
  if (plan_info[7]) {
    atomicOr(status, 4);
    atomicAdd(gated, 1ull);   // (cumulative since upload: ganon_batch_gated_runs)
  } else if (hs != plan_info[6]) {
    atomicOr(status, 2);
  }
  for (int k = 0; k < GANON_N_TOTALS; ++k) totals[k] = static_totals[k];
  totals[GANON_T_READS_WRITTEN] = plan_info[2];
  totals[GANON_T_MASKED_SNV_CALLS] += sc;
  totals[GANON_T_MASKED_BASES] += sb;
  totals[GANON_T_RARE_SCOPES] += (unsigned long long)atomicExch(rare_tiles, 0);
  // more far masks than the list holds: the masks past it were dropped — ganon_batch_download grows
  // the list to the count kept in far_need and runs the batch again
  const unsigned long long n_far_all = atomicExch(far_count, 0ull);
  if (n_far_all > (unsigned long long)far_cap) {
    atomicOr(status, 1);
    atomicMax(far_need, n_far_all);
  }
}
}  // namespace
// ---- host side ---------------------------------------------------------------------------

using ganon_detail::check_launch;
using ganon_detail::fail;
using ganon_detail::KernelScope;

namespace {

constexpr int64_t kFarMaxEntries = int64_t(1) << 30;   // far-mask list entries at most (8 GiB)

void free_buf(DBuf &b) {
  if (b.p) hipFree(b.p);
  b = DBuf{};
}

void free_ref(ganon_ref *r) {
  if (!r) return;
  if (r->nt16) hipFree(r->nt16);
  if (r->ref2) hipFree(r->ref2);
  if (r->bad) hipFree(r->bad);
  delete r;
}

void free_batch(ganon_dbatch *db) {
  DBuf *bufs[] = {&db->b_ref_start, &db->b_read_len, &db->b_seq_off, &db->b_cig_off, &db->b_n_cig, &db->b_dataset,
                  &db->b_write_scope, &db->b_seq, &db->b_cigar, &db->b_incid_off, &db->b_incid_read,
                  &db->b_span_start, &db->b_span_len, &db->b_ref_off, &db->b_keep_pos, &db->b_keep_code,
                  &db->b_read_end, &db->b_wspart, &db->b_cursor, &db->b_gs0, &db->b_lo, &db->b_linemap, &db->b_groups,
                  &db->b_seg4, &db->b_grp_part, &db->b_far, &db->b_gokey, &db->b_gopay, &db->b_gtkey, &db->b_gtflag,
                  &db->b_out, &db->b_scope_calls, &db->b_scope_bases, &db->b_small, &db->b_part, &db->b_long, &db->b_nseg,
                  &db->b_scost, &db->b_scan_tmp, &db->b_slots, &db->b_slot0, &db->b_order, &db->b_desc, &db->b_cand,
                  &db->b_sdirty, &db->b_inc4, &db->b_rbase, &db->b_rrec, &db->b_xrec, &db->b_xlist, &db->b_xcnt, &db->b_xidx};
  for (DBuf *b : bufs) free_buf(*b);
  ganon_huge::release(db);
  free_ref(db->own_ref);
  db->own_ref = nullptr;
}

// Grow b to count elements and enqueue the copy of src (async on the stream).
template <typename T>
int h2d(ganon_ctx *ctx, DBuf &b, const T *src, size_t count, const T **field) {
  T *p = nullptr;
  int rc = ganon_prep::grow_n(ctx, b, count, &p);
  if (rc) return rc;
  if (count) {
    hipError_t e = hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipMemcpyAsync H2D failed: %s", hipGetErrorString(e));
  }
  *field = p;
  return GANON_OK;
}

int ref_create(ganon_ctx *ctx, const uint8_t *nt16, int64_t bytes, ganon_ref **out) {
  *out = nullptr;
  if (bytes < 0 || (bytes > 0 && !nt16)) return fail(ctx, GANON_E_ARG, "bad reference buffer");
  if (2 * bytes >= (int64_t(1) << 40)) return fail(ctx, GANON_E_ARG, "reference over 2^40 bases");
  ganon_ref *r = new ganon_ref();
  r->bytes = bytes;
  r->n_blk = (bytes + 31) / 32;
  const int64_t n_words = (2 * bytes + 15) / 16;
  const int64_t n_bad = (r->n_blk + 63) / 64 + 1;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&r->nt16), (size_t)bytes + 128);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&r->ref2), (size_t)(n_words + 2) * 4 + 128);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&r->bad), (size_t)n_bad * 8 + 128);
  if (e != hipSuccess) {
    free_ref(r);
    return fail(ctx, GANON_E_NOMEM, "reference allocation failed: %s", hipGetErrorString(e));
  }
  if (bytes) e = hipMemcpyAsync(r->nt16, nt16, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(r->nt16 + bytes, 0, 128, ctx->stream);
  if (e != hipSuccess) {
    free_ref(r);
    return fail(ctx, GANON_E_DEVICE, "reference copy failed: %s", hipGetErrorString(e));
  }
  int rc = GANON_OK;
  if (n_words) {
    k_ref2<<<(int)std::min<int64_t>((n_words + kBlock - 1) / kBlock, 16384), kBlock, 0, ctx->stream>>>(r->nt16, n_words,
                                                                                                    r->ref2);
    rc = check_launch(ctx, "k_ref2");
  }
  if (!rc) rc = ganon_ref_blocks(ctx, r);
  if (!rc && ganon_detail::sync_stream(ctx->stream) != hipSuccess) rc = fail(ctx, GANON_E_DEVICE, "reference upload sync failed");
  if (rc) {
    free_ref(r);
    return rc;
  }
  *out = r;
  return GANON_OK;
}


// Host copies of the arrays ganon_huge::plan reads, for a batch planned from its device arrays alone
// (ganon_batch_replan of a batch with scopes wider than the group kernels': rare).
struct HostCopy {
  std::vector<int32_t> ref_start, n_cig, write_scope, incid_read, span_start, span_len;
  std::vector<int64_t> cig_off, incid_off;
  std::vector<uint32_t> cigar;
  ganon_batch b{};
};

template <typename T>
int d2h_vec(ganon_ctx *ctx, std::vector<T> &v, const T *src, size_t n) {
  v.resize(n);
  if (n) HIP_OR_FAIL(ganon_detail::readback(v.data(), src, n * sizeof(T), ctx->stream));
  return GANON_OK;
}

int host_copy(ganon_ctx *ctx, const ganon_dbatch *db, HostCopy &h) {
  const DevBatch &B = db->B;
  int rc;
  if ((rc = d2h_vec(ctx, h.ref_start, B.ref_start, (size_t)db->n_reads)) ||
      (rc = d2h_vec(ctx, h.n_cig, B.n_cig, (size_t)db->n_reads)) ||
      (rc = d2h_vec(ctx, h.write_scope, B.write_scope, (size_t)db->n_reads)) ||
      (rc = d2h_vec(ctx, h.cig_off, B.cig_off, (size_t)db->n_reads)) ||
      (rc = d2h_vec(ctx, h.cigar, B.cigar, (size_t)db->n_cigar_ops)) ||
      (rc = d2h_vec(ctx, h.incid_off, B.incid_off, (size_t)db->n_scopes + 1)) ||
      (rc = d2h_vec(ctx, h.incid_read, B.incid_read, (size_t)db->n_incid)) ||
      (rc = d2h_vec(ctx, h.span_start, B.span_start, (size_t)db->n_scopes)) ||
      (rc = d2h_vec(ctx, h.span_len, B.span_len, (size_t)db->n_scopes)))
    return rc;
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  ganon_batch &b = h.b;
  b.n_reads = db->n_reads;
  b.n_scopes = db->n_scopes;
  b.n_incid = db->n_incid;
  b.n_cigar_ops = db->n_cigar_ops;
  b.ref_start = h.ref_start.data();
  b.n_cig = h.n_cig.data();
  b.write_scope = h.write_scope.data();
  b.cig_off = h.cig_off.data();
  b.cigar = h.cigar.data();
  b.scope_incid_off = h.incid_off.data();
  b.incid_read = h.incid_read.data();
  b.scope_span_start = h.span_start.data();
  b.scope_span_len = h.span_len.data();
  return GANON_OK;
}

// Plan a batch whose raw arrays are on the device (ganon_prep::plan: validation, prep mode, sizes),
// the huge-scope tiles (from `host`, or host copies), and upload the group kernels' aux pointers
// and the static totals (async).
// The fused mode's buffers in the host copy of the aux pointers (every plan may grow them).
void set_fused_aux(ganon_dbatch *db) {
  GrpAux &a = db->aux_h;
  a.desc = static_cast<const int4 *>(db->b_desc.p);
  a.sdirty = static_cast<const uint8_t *>(db->b_sdirty.p);
  a.xrec = static_cast<const int4 *>(db->b_xrec.p);
  a.xidx = static_cast<const int32_t *>(db->b_xidx.p);
  a.xlist = static_cast<int2 *>(db->b_xlist.p);
}

int prepare(ganon_ctx *ctx, ganon_dbatch *db, const ganon_batch *host, bool allow_spec = false) {
  int rc;
  if ((rc = ganon_prep::plan(ctx, db, allow_spec))) return rc;   // (it clears the step's flags first)
  if (db->spec && !db->spec_sized) {
    // the previous plan's tiles (none), aux pointers and static totals, unchanged on the host; copied
    // again (a reload clears the device's small state) — but for the fused mode's buffers, which the
    // plan may have grown (another GANON_PARAM_XREC_INIT since the previous plan)
    set_fused_aux(db);
    HIP_OR_FAIL(hipMemcpyAsync(db->aux, &db->aux_h, sizeof db->aux_h, hipMemcpyHostToDevice, ctx->stream));
    HIP_OR_FAIL(hipMemcpyAsync(db->static_totals, db->static_h, GANON_N_TOTALS * sizeof(unsigned long long),
                               hipMemcpyHostToDevice, ctx->stream));
    return GANON_OK;
  }
  if (db->n_huge_scopes && !host) {
    HostCopy h;
    if ((rc = host_copy(ctx, db, h)) || (rc = ganon_huge::plan(ctx, db, &h.b))) return rc;
  } else if ((rc = ganon_huge::plan(ctx, db, host))) {
    return rc;
  }
  GrpAux &a = db->aux_h;
  a = GrpAux{};
  a.scope_calls = db->scope_calls;
  a.scope_bases = db->scope_bases;
  a.part = static_cast<int32_t *>(db->b_grp_part.p);
  a.far = static_cast<unsigned long long *>(db->b_far.p);
  a.far_count = db->far_count;
  a.far_cap = db->far_cap;
  a.paths = db->paths;
  a.okey = static_cast<unsigned long long *>(db->b_gokey.p);
  a.opay = static_cast<unsigned long long *>(db->b_gopay.p);
  a.tkey = static_cast<unsigned long long *>(db->b_gtkey.p);
  a.tflag = static_cast<unsigned int *>(db->b_gtflag.p);
  a.incid_read = db->B.incid_read;
  a.ref_start = db->B.ref_start;
  a.read_end = db->B.read_end;
  a.incid_off = db->B.incid_off;
  a.ref_off = db->B.ref_off;
  a.inc4 = static_cast<const int4 *>(db->b_inc4.p);
  a.rrec = static_cast<const int4 *>(db->b_rrec.p);
  set_fused_aux(db);
  a.n_reads = db->n_reads;
  a.err = db->err;
  a.ws_part = static_cast<unsigned long long *>(db->b_wspart.p);
  unsigned long long *st = db->static_h;
  std::fill(st, st + GANON_N_TOTALS, 0ull);
  st[GANON_T_READS_IN] = (unsigned long long)db->n_reads;
  st[GANON_T_READS_WRITTEN] = (unsigned long long)db->n_written;
  st[GANON_T_SCOPES] = (unsigned long long)db->n_scopes;
  st[GANON_T_LARGE_TILES] = (unsigned long long)db->n_tiles_h;
  // (from db-resident host copies: the next plan of db synchronizes before it rewrites them)
  HIP_OR_FAIL(hipMemcpyAsync(db->aux, &db->aux_h, sizeof db->aux_h, hipMemcpyHostToDevice, ctx->stream));
  HIP_OR_FAIL(hipMemcpyAsync(db->static_totals, st, GANON_N_TOTALS * sizeof(unsigned long long), hipMemcpyHostToDevice,
                             ctx->stream));
  return GANON_OK;
}

// Copy a host batch into db (grow-only buffers), validate and plan it on the device.
int load_batch(ganon_ctx *ctx, ganon_dbatch *db, const ganon_batch *b, const ganon_ref *shared) {
  if (b->n_reads < 0 || b->n_scopes < 0 || b->n_incid < 0 || b->seq_bytes < 0 || b->n_cigar_ops < 0 || b->ref_bytes < 0)
    return fail(ctx, GANON_E_ARG, "negative size in batch");
  if (b->n_reads > 0 && (!b->ref_start || !b->read_len || !b->seq_off || !b->cig_off || !b->n_cig || !b->dataset ||
                         !b->write_scope))
    return fail(ctx, GANON_E_ARG, "null read array");
  if (b->seq_bytes > 0 && !b->seq_nt16) return fail(ctx, GANON_E_ARG, "null seq_nt16");
  if (b->n_cigar_ops > 0 && !b->cigar) return fail(ctx, GANON_E_ARG, "null cigar");
  if (!b->scope_incid_off) return fail(ctx, GANON_E_ARG, "null scope_incid_off");
  if (b->n_scopes > 0 && (!b->scope_span_start || !b->scope_span_len || !b->scope_ref_off || !b->keep_pos ||
                          !b->keep_code))
    return fail(ctx, GANON_E_ARG, "null scope array");
  if (b->n_incid > 0 && !b->incid_read) return fail(ctx, GANON_E_ARG, "null incid_read");
  if (!shared && b->ref_bytes > 0 && !b->ref_nt16) return fail(ctx, GANON_E_ARG, "null ref_nt16");
  if (b->scope_incid_off[0] != 0 || b->scope_incid_off[b->n_scopes] != b->n_incid)
    return fail(ctx, GANON_E_ARG, "scope_incid_off must start at 0 and end at n_incid");
  if (2 * b->seq_bytes >= (int64_t(1) << 39)) return fail(ctx, GANON_E_ARG, "sequence over 2^39 bases");
  int64_t max_si = 0;   // (the group kernel's launch order: ganon_prep launch_pieces)
  for (int32_t s = 0; s < b->n_scopes; ++s) max_si = std::max(max_si, b->scope_incid_off[s + 1] - b->scope_incid_off[s]);
  if (b->n_incid >= INT32_MAX) return fail(ctx, GANON_E_ARG, "more than 2^31-1 incidences");
  int rc;
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));   // a previous run of db may still read its buffers
  db->ran = false;
  db->max_scope_incid = max_si;
  if (shared) {
    db->ref = shared;
  } else {
    free_ref(db->own_ref);
    db->own_ref = nullptr;
    if ((rc = ref_create(ctx, b->ref_nt16, b->ref_bytes, &db->own_ref))) return rc;
    db->ref = db->own_ref;
  }
  db->n_reads = b->n_reads;
  db->n_scopes = b->n_scopes;
  db->n_incid = b->n_incid;
  db->seq_bytes = b->seq_bytes;
  db->n_cigar_ops = b->n_cigar_ops;
  db->group_target = ctx->group_target;
  DevBatch &D = db->B;
  if ((rc = h2d(ctx, db->b_ref_start, b->ref_start, b->n_reads, &D.ref_start)) ||
      (rc = h2d(ctx, db->b_read_len, b->read_len, b->n_reads, &D.read_len)) ||
      (rc = h2d(ctx, db->b_seq_off, b->seq_off, b->n_reads, &D.seq_off)) ||
      (rc = h2d(ctx, db->b_cig_off, b->cig_off, b->n_reads, &D.cig_off)) ||
      (rc = h2d(ctx, db->b_n_cig, b->n_cig, b->n_reads, &D.n_cig)) ||
      (rc = h2d(ctx, db->b_dataset, b->dataset, b->n_reads, &D.dataset)) ||
      (rc = h2d(ctx, db->b_write_scope, b->write_scope, b->n_reads, &D.write_scope)) ||
      (rc = h2d(ctx, db->b_seq, b->seq_nt16, b->seq_bytes, &D.seq)) ||
      (rc = h2d(ctx, db->b_cigar, b->cigar, b->n_cigar_ops, &D.cigar)) ||
      (rc = h2d(ctx, db->b_incid_off, b->scope_incid_off, (size_t)b->n_scopes + 1, &D.incid_off)) ||
      (rc = h2d(ctx, db->b_incid_read, b->incid_read, b->n_incid, &D.incid_read)) ||
      (rc = h2d(ctx, db->b_span_start, b->scope_span_start, b->n_scopes, &D.span_start)) ||
      (rc = h2d(ctx, db->b_span_len, b->scope_span_len, b->n_scopes, &D.span_len)) ||
      (rc = h2d(ctx, db->b_ref_off, b->scope_ref_off, b->n_scopes, &D.ref_off)) ||
      (rc = h2d(ctx, db->b_keep_pos, b->keep_pos, b->n_scopes, &D.keep_pos)) ||
      (rc = h2d(ctx, db->b_keep_code, b->keep_code, b->n_scopes, &D.keep_code)))
    return rc;
  D.ref = db->ref->nt16;
  D.ref2 = db->ref->ref2;
  // small device state: totals, static totals, acc, far count, plan info (u64); the rare-tile count, status;
  // the first validation error; the group kernels' aux pointers
  constexpr size_t kU64 = 8 + 8 + 5 + 1 + 8 + 4 + 1;
  // the per-plan flags (first error, status bits, long-read count, far masks needed) are adjacent:
  // one memset clears them at the start of every plan
  constexpr size_t kFlags = sizeof(PrepErr) + 16;
  constexpr size_t kSmallBytes = kU64 * 8 + 8 * 4 + kFlags + sizeof(GrpAux) + 64;
  uint8_t *sm = nullptr;
  if ((rc = ganon_prep::grow_n(ctx, db->b_small, kSmallBytes, &sm))) return rc;
  auto *u = reinterpret_cast<unsigned long long *>(sm);
  db->totals = u;
  db->static_totals = u + 8;
  db->acc = u + 16;        // [0] calls, [1] bases, [2] ticket, [3] far masks needed, [4] write-scope sum
  db->far_count = u + 21;
  db->plan_info = u + 22;
  db->paths = u + 30;
  db->gated = u + 34;      // runs a speculative plan's gate stopped (cumulative)
  db->rare_tiles = reinterpret_cast<int32_t *>(u + kU64);
  db->err = reinterpret_cast<PrepErr *>(sm + kU64 * 8 + 8 * 4);
  db->status = reinterpret_cast<int32_t *>(db->err + 1);
  db->long_count = reinterpret_cast<unsigned int *>(db->status + 1);
  db->far_need = reinterpret_cast<unsigned long long *>(db->long_count + 1);
  db->flags_bytes = kFlags;
  db->aux = reinterpret_cast<GrpAux *>(sm + kU64 * 8 + 8 * 4 + kFlags);
  HIP_OR_FAIL(hipMemsetAsync(sm, 0, kSmallBytes, ctx->stream));
  if ((rc = ganon_prep::grow_n(ctx, db->b_scope_calls, b->n_scopes, &db->scope_calls)) ||
      (rc = ganon_prep::grow_n(ctx, db->b_scope_bases, b->n_scopes, &db->scope_bases)) ||
      (rc = ganon_prep::grow_n(ctx, db->b_out, b->seq_bytes, &db->out)))
    return rc;
  // bytes outside every read are never written by the masking kernels: make them defined
  HIP_OR_FAIL(hipMemsetAsync(db->out, 0, (size_t)b->seq_bytes + 16, ctx->stream));
  if ((rc = prepare(ctx, db, b, ctx->spec_plan == 2))) return rc;   // (2: testing knob)
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  return GANON_OK;
}

int upload_common(ganon_ctx *ctx, const ganon_batch *b, const ganon_ref *ref, ganon_dbatch **out) {
  if (!ctx || !b || !out) return fail(ctx, GANON_E_ARG, "null argument");
  *out = nullptr;
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  ganon_dbatch *db = new ganon_dbatch();
  int rc = load_batch(ctx, db, b, ref);
  if (rc) {
    ganon_detail::sync_stream(ctx->stream);
    free_batch(db);
    delete db;
    return rc;
  }
  *out = db;
  return GANON_OK;
}

}  // namespace

GANON_API int ganon_abi_version(void) { return GANON_ABI_VERSION; }

GANON_API int ganon_ctx_create(int device, ganon_ctx **out) {
  if (!out) return GANON_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return GANON_E_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return GANON_E_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return GANON_E_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return GANON_E_DEVICE;
  ganon_ctx *ctx = new ganon_ctx();
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->own, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return GANON_E_DEVICE;
  }
  ctx->stream = ctx->own;
  ganon_huge::init();
  *out = ctx;
  return GANON_OK;
}

GANON_API int ganon_ctx_destroy(ganon_ctx *ctx) {
  if (!ctx) return GANON_E_ARG;
  hipSetDevice(ctx->device);
  if (ctx->own) {
    ganon_detail::sync_stream(ctx->own);
    hipStreamDestroy(ctx->own);
  }
  for (auto &r : ctx->recs) {
    hipEventDestroy(r.e0);
    hipEventDestroy(r.e1);
  }
  for (auto e : ctx->pool) hipEventDestroy(e);
  if (ctx->side) {
    ganon_detail::sync_stream(ctx->side);
    hipStreamDestroy(ctx->side);
  }
  if (ctx->fork_ev) hipEventDestroy(ctx->fork_ev);
  if (ctx->join_ev) hipEventDestroy(ctx->join_ev);
  for (auto &b : ctx->dcache) hipFree(b.second);
  if (ctx->ks_block) hipFree(ctx->ks_block);
  if (ctx->sa_block) hipFree(ctx->sa_block);
  ganon_inflate_free(ctx->inflate);
  ganon_deflate_free(ctx->deflate);
  delete ctx;
  return GANON_OK;
}

GANON_API const char *ganon_last_error(ganon_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// Page-locked blocks are cached per process (up to 8 GiB): pinning and unpinning hundreds of MB per
// reader and run (the readers' scan buffers, the FASTQ blobs) cost more than the copies they save.
namespace {
std::mutex g_pin_mu;
std::multimap<size_t, void *> g_pin_free;   // capacity -> block
std::map<void *, size_t> g_pin_cap;         // every live or cached block's capacity
size_t g_pin_cached = 0;
constexpr size_t kPinCacheMax = size_t(8) << 30;
int64_t g_pin_stats[4] = {0, 0, 0, 0};      // blocks pinned anew, their bytes, seconds in hipHostMalloc, cache hits
}  // namespace

GANON_API int ganon_pinned_alloc(int64_t bytes, void **out) {
  if (!out || bytes < 0) return GANON_E_ARG;
  *out = nullptr;
  const size_t want = (size_t)std::max<int64_t>(bytes, 1);
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pin_free.lower_bound(want);
    if (it != g_pin_free.end() && it->first <= 2 * want + (size_t(16) << 20)) {
      g_pin_stats[3] += 1;
      *out = it->second;
      g_pin_cached -= it->first;
      g_pin_free.erase(it);
      return GANON_OK;
    }
  }
  const size_t cap = (want + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
  const auto t0 = std::chrono::steady_clock::now();
  if (hipHostMalloc(out, cap, hipHostMallocDefault) != hipSuccess) {
    *out = nullptr;
    return GANON_E_NOMEM;
  }
  const int64_t ns = (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pin_cap[*out] = cap;
  g_pin_stats[0] += 1;
  g_pin_stats[1] += (int64_t)cap;
  g_pin_stats[2] += ns;
  return GANON_OK;
}

GANON_API int ganon_pinned_stats(int64_t *out4) {
  if (!out4) return GANON_E_ARG;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  for (int k = 0; k < 4; ++k) out4[k] = g_pin_stats[k];
  return GANON_OK;
}

GANON_API int ganon_pinned_free(void *p) {
  if (!p) return GANON_OK;
  std::lock_guard<std::mutex> lk(g_pin_mu);
  auto it = g_pin_cap.find(p);
  if (it == g_pin_cap.end()) return GANON_E_ARG;
  if (g_pin_cached + it->second <= kPinCacheMax) {
    g_pin_free.emplace(it->second, p);
    g_pin_cached += it->second;
  } else {
    g_pin_cap.erase(it);
    hipHostFree(p);
  }
  return GANON_OK;
}

GANON_API int ganon_ctx_set_stream(ganon_ctx *ctx, void *hip_stream) {
  if (!ctx) return GANON_E_ARG;
  ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own;
  return GANON_OK;
}

GANON_API int ganon_ctx_set_variant(ganon_ctx *ctx, int variant) {
  if (!ctx) return GANON_E_ARG;
  if (variant != GANON_VARIANT_DEFAULT && variant != GANON_VARIANT_GROUP_FUSED)
    return fail(ctx, GANON_E_ARG, "kernel variant %d was retired: the fused group kernel is the only small-scope path",
                variant);
  return GANON_OK;
}

GANON_API int ganon_ctx_set_param(ganon_ctx *ctx, int param, int value) {
  if (!ctx) return GANON_E_ARG;
  if (param == GANON_PARAM_GROUP_UNROLL) {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(ctx, GANON_E_ARG, "group unroll must be 0 (auto), 1, 2, 4 or 8 (got %d)", value);
    ctx->group_unroll = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_GROUP_TARGET) {
    if (value != 0 && (value < 16 || value > 65536))
      return fail(ctx, GANON_E_ARG, "group target must be 0 (auto) or in [16, 65536] (got %d)", value);
    ctx->group_target = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_REF2) {
    ctx->ref2 = value != 0;
    return GANON_OK;
  }
  if (param == GANON_PARAM_FASTQ_SKIP) {
    ctx->fq_skip = value & 0x3B;   // k_fq_span and k_fq_quad read bits 0, 1, 3, 4, 5; k_fq_rows 1 and 5; k_fq_dense none
    return GANON_OK;
  }
  if (param == GANON_PARAM_INDEL_SORT) {
    if (value != 0 && value != 1) return fail(ctx, GANON_E_ARG, "indel sort: 0 (segmented) or 1 (global)");
    ctx->indel_sort = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_FASTQ_KD) {
    if ((value >= 1 && value <= 6) || value == 8 || value == 10)
      return fail(ctx, GANON_E_ARG, "FASTQ kernel instance %d was retired (the round-1 dword kernel, 3 quads per lane)",
                  value);
    if (value < 0 || value > 17 || value == 7)
      return fail(ctx, GANON_E_ARG,
                  "FASTQ kernel: 0 (spans, 3 units per lane), 13 / 14 (spans, 2 per lane, 8 / 16 KiB tiles), "
                  "15 / 17 (as 0, span found by binary search / from a map entry per 8 units), "
                  "16 / 9 (quads, 2 / 1 per lane), 11 (quads, per-dword base select), 12 (record rows)");
    ctx->fq_kd = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_PREP_LONG) {
    if (value < -1 || value > 2) return fail(ctx, GANON_E_ARG, "prep mode: -1 (auto), 0 (two-pass), 1 (long), 2 (one-segment)");
    ctx->prep_long = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_PREP_UNROLL) {
    if (value != 0 && value != 1 && value != 2 && value != 4)
      return fail(ctx, GANON_E_ARG, "prep unroll: 0 (auto), 1, 2 or 4 (got %d)", value);
    ctx->prep_unroll = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_GROUP_OBS) {
    if (value != 0 && value != 512 && value != 1024)
      return fail(ctx, GANON_E_ARG, "group observation list: 0 (auto), 512 or 1024 (got %d)", value);
    ctx->group_obs = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_NT_COPY) {
    ctx->nt_copy = value != 0;
    return GANON_OK;
  }
  if (param == GANON_PARAM_SPEC_PLAN) {
    if (value < 0 || value > 2) return fail(ctx, GANON_E_ARG, "speculative plans: 0, 1 or 2 (got %d)", value);
    ctx->spec_plan = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_FUSED_FLAT) {
    if (value != 0 && value != 1) return fail(ctx, GANON_E_ARG, "fused one-segment mode: 0 or 1 (got %d)", value);
    ctx->fused_flat = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_XREC_INIT) {
    if (value < 0) return fail(ctx, GANON_E_ARG, "extras list capacity must be >= 0");
    ctx->xrec_init = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_FAR_INIT) {
    if (value < 0) return fail(ctx, GANON_E_ARG, "far-mask list capacity must be >= 0");
    ctx->far_init = value;
    return GANON_OK;
  }
  if (param == GANON_PARAM_GROUP_SKIP) {
    ctx->group_skip = value & (kSkipClassify | kSkipChunks | kSkipCopy | kSkipCounts);
    return GANON_OK;
  }
  return fail(ctx, GANON_E_ARG, "unknown parameter %d", param);
}

GANON_API int ganon_ctx_set_profiling(ganon_ctx *ctx, int enabled) {
  if (!ctx) return GANON_E_ARG;
  ctx->profiling = enabled != 0;
  return GANON_OK;
}

GANON_API int ganon_ref_upload(ganon_ctx *ctx, const uint8_t *ref_nt16, int64_t ref_bytes, ganon_ref **out) {
  if (!ctx || !out) return fail(ctx, GANON_E_ARG, "null argument");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  return ref_create(ctx, ref_nt16, ref_bytes, out);
}

GANON_API int ganon_ref_free(ganon_ctx *ctx, ganon_ref *ref) {
  if (!ref) return GANON_E_ARG;
  if (ctx) {
    hipSetDevice(ctx->device);
    ganon_detail::sync_stream(ctx->stream);
  }
  free_ref(ref);
  return GANON_OK;
}

GANON_API int ganon_batch_upload(ganon_ctx *ctx, const ganon_batch *b, ganon_dbatch **out) {
  return upload_common(ctx, b, nullptr, out);
}

GANON_API int ganon_batch_upload_ref(ganon_ctx *ctx, const ganon_batch *b, const ganon_ref *ref, ganon_dbatch **out) {
  if (!ref) return fail(ctx, GANON_E_ARG, "null reference");
  return upload_common(ctx, b, ref, out);
}

GANON_API int ganon_batch_reload(ganon_ctx *ctx, ganon_dbatch *db, const ganon_batch *b) {
  if (!ctx || !db || !b) return fail(ctx, GANON_E_ARG, "null argument");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  const ganon_ref *shared = db->own_ref ? nullptr : db->ref;
  int rc = load_batch(ctx, db, b, shared);
  if (rc) {
    // the device batch holds a partial load: only free or reload is valid now
    db->n_groups = 0;
    db->ran = false;
  }
  return rc;
}

namespace {
// A new profiled step: the event pairs of the previous one go back to the pool.
void new_step(ganon_ctx *ctx) {
  for (auto &r : ctx->recs) {
    ctx->pool.push_back(r.e0);
    ctx->pool.push_back(r.e1);
  }
  ctx->recs.clear();
}

}  // namespace

GANON_API int ganon_batch_replan(ganon_ctx *ctx, ganon_dbatch *db) {
  if (!ctx || !db) return fail(ctx, GANON_E_ARG, "null argument");
  if (!db->b_small.p) return fail(ctx, GANON_E_STATE, "replan of a batch that was never loaded");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  new_step(ctx);
  ctx->step_open = true;   // the next run's kernels join this step's timings
  // (speculative: an upload or reload plans in full — its caller reads the shape at once, e.g. the
  // I/D op count that decides the indel tally)
  int rc = prepare(ctx, db, nullptr, true);
  if (rc) {
    db->n_groups = 0;
    db->ran = false;
  }
  return rc;
}

GANON_API int ganon_batch_run(ganon_ctx *ctx, ganon_dbatch *db) {
  if (!ctx || !db) return fail(ctx, GANON_E_ARG, "null argument");
  // 16-base chunks per thread: long reads (short segments between indels) waste less with one
  // (profiles/r02/sweep_c5.jsonl); short reads run best with two (sweep_c3.jsonl)
  const int u = ctx->group_unroll ? ctx->group_unroll : db->long_mode ? 1 : 2;
  // 512 unless forced: the 1024-entry list (4 workgroups per CU instead of 6) measured slower on
  // c3 too (3.19 vs 2.84 ms, profiles/r02/sweep_c3_obs.jsonl) — occupancy outweighs the region path
  const int obs = ctx->group_obs ? ctx->group_obs : 512;
  // (before anything is launched: a pair without a compiled kernel never runs another pair's)
  if (!ganon_group::compiled(db->fused, db->long_mode, u, obs))
    return fail(ctx, GANON_E_ARG,
                "no group kernel is compiled for GANON_PARAM_GROUP_UNROLL %d with GANON_PARAM_GROUP_OBS %d "
                "(the 1024-entry list takes unroll 1 or 2)", u, obs);
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  if (!ctx->step_open) new_step(ctx);
  ctx->step_open = false;
  hipStream_t st = ctx->stream;
  int rc;
  // 1. derived layer from the raw SoA
  if ((rc = ganon_prep::run(ctx, db))) return rc;
  if (ctx->indel_fork < 0) {
    const char *v = std::getenv("GANON_INDEL_FORK");
    ctx->indel_fork = v && v[0] == '1' ? 1 : 0;
  }
  if (ctx->indel_fork) {   // (the fork point of this batch's indel tally: its inputs are final here)
    if (!ctx->fork_ev) HIP_OR_FAIL(hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming));
    HIP_OR_FAIL(hipEventRecord(ctx->fork_ev, st));
    ctx->fork_db = db;
  }
  if (db->n_huge_scopes) {
    // huge scopes are counted with atomics (tiles)
    HIP_OR_FAIL(hipMemsetAsync(db->scope_calls, 0, (size_t)db->n_scopes * sizeof(int32_t), st));
    HIP_OR_FAIL(hipMemsetAsync(db->scope_bases, 0, (size_t)db->n_scopes * sizeof(int32_t), st));
  }
  // 2. masking: the group kernel writes every byte of out (its pieces tile [0, seq_bytes))
  if (db->n_groups) {
    // (GANON_PARAM_REF2 off: the group kernels read the nt16 reference only)
    if ((rc = ganon_group::launch(ctx, db, u, obs, ctx->ref2 ? db->B.ref2 : nullptr))) return rc;
  } else if (db->seq_bytes) {
    KernelScope ks(ctx, "copy_seq");
    HIP_OR_FAIL(hipMemcpyAsync(db->out, db->B.seq, (size_t)db->seq_bytes, hipMemcpyDeviceToDevice, st));
  }
  if ((rc = ganon_huge::run(ctx, db))) return rc;
  {
    // far masks, totals from the group partials and the huge scopes, counter reset
    KernelScope ks(ctx, "k_finish");
    k_finish<<<64, kBlock, 0, st>>>(static_cast<const unsigned long long *>(db->b_far.p), db->n_groups ? db->far_cap : 0,
                                    db->out, static_cast<const int32_t *>(db->b_grp_part.p), db->n_groups,
                                    db->large_ids, db->n_huge_scopes, db->scope_calls, db->scope_bases,
                                    db->static_totals, db->rare_tiles, db->far_count, db->status, db->acc, db->far_need,
                                    db->totals,
                                    static_cast<const unsigned long long *>(db->b_wspart.p), db->plan_info, db->gated);
    if ((rc = check_launch(ctx, "k_finish"))) return rc;
  }
  db->ran = true;
  return GANON_OK;
}

GANON_API int ganon_batch_sync(ganon_ctx *ctx) {
  if (!ctx) return GANON_E_ARG;
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  if (ctx->profiling) {
    ctx->last_times.clear();
    for (auto &r : ctx->recs) {
      float ms = 0.f;
      hipEventElapsedTime(&ms, r.e0, r.e1);
      auto it = std::find_if(ctx->last_times.begin(), ctx->last_times.end(),
                             [&](const ganon_kernel_time &t) { return r.name == t.name; });
      if (it == ctx->last_times.end()) {
        ganon_kernel_time t{};
        std::snprintf(t.name, sizeof t.name, "%s", r.name.c_str());
        t.launches = 1;
        t.ms = ms;
        ctx->last_times.push_back(t);
      } else {
        it->launches += 1;
        it->ms += ms;
      }
    }
  }
  return GANON_OK;
}

GANON_API int ganon_last_kernel_times(ganon_ctx *ctx, ganon_kernel_time *out, int max_k) {
  if (!ctx) return GANON_E_ARG;
  const int n = (int)ctx->last_times.size();
  for (int i = 0; i < n && i < max_k && out; ++i) out[i] = ctx->last_times[i];
  return n;
}

GANON_API int ganon_batch_download(ganon_ctx *ctx, ganon_dbatch *db, uint8_t *seq_out, int32_t *scope_calls_out,
                                   int32_t *scope_bases_out, int64_t *totals_out) {
  if (!ctx || !db) return fail(ctx, GANON_E_ARG, "null argument");
  if (!db->ran) return fail(ctx, GANON_E_STATE, "download before run");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  // the checks made during the run (incidences, write scopes)
  if ((rc = ganon_prep::batch_error(ctx, db))) return rc;
  int32_t status = 0;
  unsigned long long far_need = 0;
  HIP_OR_FAIL(ganon_detail::readback(&status, db->status, sizeof status, st));
  HIP_OR_FAIL(ganon_detail::readback(&far_need, db->far_need, sizeof far_need, st));
  HIP_OR_FAIL(ganon_detail::sync_stream(st));
  if (status & 4) {
    // a speculative replan the batch did not fit (a read with several segments, a longer read, a
    // huge scope): plan it in full and run it again
    const int sp = ctx->spec_plan;
    const bool prof = ctx->profiling;
    ctx->spec_plan = 0;
    ctx->profiling = false;
    rc = prepare(ctx, db, nullptr);
    if (!rc) rc = ganon_batch_run(ctx, db);
    ctx->spec_plan = sp;
    ctx->profiling = prof;
    if (rc) return rc;
    if ((rc = ganon_prep::batch_error(ctx, db))) return rc;
    HIP_OR_FAIL(ganon_detail::readback(&status, db->status, sizeof status, st));
    HIP_OR_FAIL(ganon_detail::readback(&far_need, db->far_need, sizeof far_need, st));
    HIP_OR_FAIL(ganon_detail::sync_stream(st));
  }
  if (status & 2) {
    // a written read its write scope does not list (or lists twice): name it
    if ((rc = ganon_prep::ws_diag(ctx, db)) || (rc = ganon_prep::batch_error(ctx, db))) return rc;
    return fail(ctx, GANON_E_ARG, "a written read is not listed exactly once by its write scope");
  }
  if (status & 1) {
    // the far-mask list overflowed: grow it to the count the run needed and run again (the list
    // keeps its capacity for later batches)
    if ((int64_t)far_need > kFarMaxEntries)
      return fail(ctx, GANON_E_NOMEM, "far-mask list: %llu entries needed (max %lld)", far_need, (long long)kFarMaxEntries);
    unsigned long long *far = nullptr;
    const int64_t cap = std::min<int64_t>(kFarMaxEntries, (int64_t)far_need + (int64_t)far_need / 4 + 1024);
    if ((rc = ganon_prep::grow_n(ctx, db->b_far, (size_t)cap, &far))) return rc;
    db->far_cap = db->far_cap_alloc = cap;
    db->aux_h.far = far;
    db->aux_h.far_cap = cap;
    HIP_OR_FAIL(hipMemcpyAsync(db->aux, &db->aux_h, sizeof db->aux_h, hipMemcpyHostToDevice, st));
    HIP_OR_FAIL(hipMemsetAsync(db->status, 0, sizeof(int32_t), st));
    HIP_OR_FAIL(hipMemsetAsync(db->far_need, 0, sizeof(unsigned long long), st));
    const bool prof = ctx->profiling;
    ctx->profiling = false;
    rc = ganon_batch_run(ctx, db);
    ctx->profiling = prof;
    if (rc) return rc;
    HIP_OR_FAIL(ganon_detail::readback(&status, db->status, sizeof status, st));
  }
  if (seq_out && db->seq_bytes)
    HIP_OR_FAIL(hipMemcpyAsync(seq_out, db->out, (size_t)db->seq_bytes, hipMemcpyDeviceToHost, st));
  if (scope_calls_out && db->n_scopes)
    HIP_OR_FAIL(hipMemcpyAsync(scope_calls_out, db->scope_calls, (size_t)db->n_scopes * 4, hipMemcpyDeviceToHost, st));
  if (scope_bases_out && db->n_scopes)
    HIP_OR_FAIL(hipMemcpyAsync(scope_bases_out, db->scope_bases, (size_t)db->n_scopes * 4, hipMemcpyDeviceToHost, st));
  if (totals_out)
    HIP_OR_FAIL(hipMemcpyAsync(totals_out, db->totals, GANON_N_TOTALS * 8, hipMemcpyDeviceToHost, st));
  HIP_OR_FAIL(ganon_detail::sync_stream(st));
  if (status & 1) return fail(ctx, GANON_E_STATE, "far-mask list overflowed after growing: output invalid");
  return GANON_OK;
}

GANON_API int ganon_batch_free(ganon_ctx *ctx, ganon_dbatch *db) {
  if (!db) return GANON_E_ARG;
  if (ctx) {
    hipSetDevice(ctx->device);
    ganon_detail::sync_stream(ctx->stream);
  }
  free_batch(db);
  delete db;
  return GANON_OK;
}

GANON_API int ganon_batch_device_totals(ganon_dbatch *db, void **dev_ptr) {
  if (!db || !dev_ptr) return GANON_E_ARG;
  *dev_ptr = db->totals;
  return GANON_OK;
}

GANON_API int ganon_batch_copy_totals(ganon_ctx *ctx, ganon_dbatch *db, void *dev_dst) {
  if (!ctx || !db || !dev_dst) return fail(ctx, GANON_E_ARG, "null argument");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  HIP_OR_FAIL(hipMemcpyAsync(dev_dst, db->totals, GANON_N_TOTALS * sizeof(int64_t), hipMemcpyDeviceToDevice,
                             ctx->stream));
  return GANON_OK;
}

GANON_API int ganon_batch_gated_runs(ganon_ctx *ctx, ganon_dbatch *db, int64_t *out) {
  if (!ctx || !db || !out) return fail(ctx, GANON_E_ARG, "null argument");
  if (!db->gated) return fail(ctx, GANON_E_STATE, "batch never loaded");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  unsigned long long g = 0;
  HIP_OR_FAIL(ganon_detail::readback(&g, db->gated, sizeof g, ctx->stream));
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  *out = (int64_t)g;
  return GANON_OK;
}

GANON_API int ganon_batch_path_counts(ganon_ctx *ctx, ganon_dbatch *db, int64_t *out4) {
  if (!ctx || !db || !out4) return fail(ctx, GANON_E_ARG, "null argument");
  HIP_OR_FAIL(hipSetDevice(ctx->device));
  HIP_OR_FAIL(ganon_detail::readback(out4, db->paths, 4 * sizeof(int64_t), ctx->stream));
  HIP_OR_FAIL(ganon_detail::sync_stream(ctx->stream));
  return GANON_OK;
}

GANON_API int ganon_batch_info(ganon_dbatch *db, int64_t *info) {
  if (!db || !info) return GANON_E_ARG;
  info[0] = db->n_groups;
  info[1] = db->n_seg;
  info[2] = db->n_huge_scopes;
  info[3] = db->n_tiles_h;
  info[4] = db->far_cap;
  info[5] = db->n_large_written_h;
  info[6] = db->region;
  info[7] = db->n_written;
  return GANON_OK;
}

GANON_API int ganon_batch_shape(ganon_dbatch *db, int64_t *shape) {
  if (!db || !shape) return GANON_E_ARG;
  shape[0] = db->n_id_ops;
  shape[1] = db->max_len;
  shape[2] = db->max_seg;
  // (4: fused with multi-segment reads, found by a full plan; a speculative plan reports 3)
  shape[3] = db->long_mode ? 1 : db->flat_mode ? (db->fused ? (db->max_seg > 1 && !db->spec ? 4 : 3) : 2) : 0;
  return GANON_OK;
}

int ganon_dbatch_seq_buffers(const ganon_dbatch *db, const uint8_t **in, const uint8_t **out, int64_t *bytes) {
  if (!db) return GANON_E_ARG;
  *in = db->B.seq;
  *out = db->out;
  *bytes = db->seq_bytes;
  return GANON_OK;
}

int ganon_dbatch_read_view(const ganon_dbatch *db, GanonReadView *v) {
  if (!db || !v) return GANON_E_ARG;
  const DevBatch &B = db->B;
  v->ref_start = B.ref_start;
  v->read_len = B.read_len;
  v->read_end = B.read_end;
  v->n_cig = B.n_cig;
  v->write_scope = B.write_scope;
  v->seq_off = B.seq_off;
  v->cig_off = B.cig_off;
  v->seq = B.seq;
  v->dataset = B.dataset;
  v->cigar = B.cigar;
  v->incid_off = B.incid_off;
  v->incid_read = B.incid_read;
  v->span_start = B.span_start;
  v->span_len = B.span_len;
  v->n_reads = db->n_reads;
  v->n_scopes = db->n_scopes;
  return GANON_OK;
}

GANON_API int ganon_mask_batch(ganon_ctx *ctx, const ganon_batch *batch, uint8_t *seq_out, int32_t *scope_calls_out,
                               int32_t *scope_bases_out, int64_t *totals_out) {
  if (!ctx || !batch || (!seq_out && batch->seq_bytes)) return fail(ctx, GANON_E_ARG, "null argument");
  ganon_dbatch *db = nullptr;
  int rc = ganon_batch_upload(ctx, batch, &db);
  if (rc) return rc;
  rc = ganon_batch_run(ctx, db);
  if (!rc) rc = ganon_batch_sync(ctx);
  if (!rc) rc = ganon_batch_download(ctx, db, seq_out, scope_calls_out, scope_bases_out, totals_out);
  ganon_batch_free(ctx, db);
  return rc;
}
