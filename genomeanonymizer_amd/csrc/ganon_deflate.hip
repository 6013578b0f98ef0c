// ganon_deflate.hip — BGZF member encoder on MI355X (gfx950), part of libganon_hip.so; C ABI in
// include/ganon.h (ganon_deflate_bgzf). The mirror of ganon_inflate.hip: the FASTQ text the pipeline
// writes is cut into blocks of at most 0xFF00 bytes and each block becomes one complete BGZF member
// (18-byte header with the BC subfield, a raw DEFLATE payload, CRC32, ISIZE).
//
// One 256-lane workgroup per block, the block staged in LDS. The phases, each a pure function of
// the one before (the output depends on the input bytes alone: hash slots are arbitrated by
// position with a max, histograms and the bit buffer are built with commutative adds / ors, and
// every partition is a fixed count of slices, never the lane count):
//   crc      256 slices, each a table CRC from a zero register, combined with zero-shift operators
//            (x^(8k) mod P): no lane waits for another's bytes
//   match    rounds of kDefRound positions: every position looks up the latest earlier-round position
//            with the same 4-byte hash (LDS table) and the distance-1 candidate (runs; the source
//            may overlap the destination), compares 4 bytes at a time; then all positions enter
//            the table (max position wins) while wave 0 resolves the greedy parse by a scalar chain
//            through the round's advances (readlane), and the chosen lanes append their tokens
//   codes    rank sort of the used symbols, a two-queue Huffman tree, depths clamped to the limit
//            and the Kraft sum repaired on the per-length counts; canonical codes; the literal/
//            length + distance lengths run-length coded (16/17/18) under a 7-bit code
//   emit     bit length of 256 token slices, their prefix sum, every slice packed at its bit offset
//            into the LDS bit buffer (the input's space)
//   stored   whenever the dynamic block would not be smaller: BTYPE 0, n + 31 bytes in all
// The whole encoder is host-callable with one lane (tools/deflate_host_check.cpp) and gives the
// same bytes there. Written from RFC 1951, RFC 1952 and the BGZF section of the SAM specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ganon_ctx.h"
#if defined(DEF_PROF)
// (tuning build only) lane 0's cycles per phase, summed over the blocks: stage + crc, match + parse,
// codes, token bit lengths, emit + store
__device__ unsigned long long g_def_prof[5];
#endif
#include "ganon_deflate_core.h"

namespace {

using ganon_detail::check_launch;
using ganon_detail::fail;

using namespace ganon_deflate_core;

// Block b of in[0, in_len) cut every block_in bytes -> the member in slot b, its size in sizes[b].
__global__ void __launch_bounds__(kDefThreads) k_deflate(const uint8_t *__restrict__ in, int64_t in_len, int block_in,
                                                         int64_t n_blocks, uint8_t *__restrict__ slots,
                                                         uint32_t *__restrict__ tok, int32_t *__restrict__ sizes) {
  __shared__ DefShared S;
  const int t = threadIdx.x;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t lo = b * block_in;
    const int64_t left = in_len - lo;
    const int n = (int)(left < block_in ? left : block_in);
    const int sz = deflate_block<kDefThreads>(S, in + lo, n, slots + b * kDefSlot, tok + (size_t)blockIdx.x * kDefMaxIn, t);
    if (t == 0) sizes[b] = sz;
  }
}

// Exclusive scan of the member sizes (one workgroup; n_blocks is a chunk's, a few thousand at most).
__global__ void __launch_bounds__(kDefThreads) k_deflate_scan(const int32_t *__restrict__ sizes, int64_t n_blocks,
                                                              int64_t *__restrict__ off) {
  __shared__ int64_t part[kDefThreads];
  const int t = threadIdx.x;
  const int64_t per = (n_blocks + kDefThreads - 1) / kDefThreads;
  const int64_t lo = std::min<int64_t>(t * per, n_blocks), hi = std::min<int64_t>(lo + per, n_blocks);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += sizes[i];
  part[t] = s;
  __syncthreads();
  int64_t run = 0;
  for (int k = 0; k < t; ++k) run += part[k];
  for (int64_t i = lo; i < hi; ++i) {
    off[i] = run;
    run += sizes[i];
  }
  if (t == kDefThreads - 1) off[n_blocks] = run;
}

// Member b from its slot to out[off[b], + sizes[b]): the members back to back.
__global__ void __launch_bounds__(kDefThreads) k_deflate_compact(const uint8_t *__restrict__ slots,
                                                                 const int32_t *__restrict__ sizes,
                                                                 const int64_t *__restrict__ off, int64_t n_blocks,
                                                                 uint8_t *__restrict__ out, int64_t out_cap) {
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int sz = sizes[b];
    const int64_t o = off[b];
    if (sz <= 0 || sz > kDefSlot || o < 0 || o + sz > out_cap) continue;
    const uint8_t *src = slots + b * kDefSlot;
    uint8_t *dst = out + o;
    // bytes up to the destination's first 4-byte boundary, then words gathered from the (2-byte
    // aligned at best) source, then the tail
    const int head = (int)std::min<int64_t>((4 - (o & 3)) & 3, sz);
    const int words = (sz - head) >> 2;
    if ((int)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (int w = threadIdx.x; w < words; w += kDefThreads) {
      const uint8_t *p = src + head + 4 * w;
      const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = v;
    }
    const int done = head + 4 * words;
    if ((int)threadIdx.x < sz - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
  }
}

}  // namespace

struct ganon_deflate_state {
  uint8_t *in = nullptr, *slots = nullptr, *out = nullptr;
  uint32_t *tok = nullptr;
  int32_t *sizes = nullptr;
  int64_t *off = nullptr;
  size_t in_cap = 0, slots_cap = 0, out_cap = 0, tok_cap = 0, sizes_cap = 0, off_cap = 0;
};

namespace {

template <typename T>
int def_grow(ganon_ctx *ctx, T **p, size_t &cap, size_t need) {
  if (*p && cap >= need) return GANON_OK;
  if (*p) {
    ganon_detail::sync_stream(ctx->stream);
    hipFree(*p);
    *p = nullptr;
  }
  const size_t n = std::max(need, cap + cap / 2);
  if (hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
    *p = nullptr;
    cap = 0;
    return fail(ctx, GANON_E_NOMEM, "hipMalloc for the deflate buffers failed");
  }
  cap = n;
  return GANON_OK;
}

constexpr int64_t kDefChunk = 1024;   // blocks per launch (64 MiB of slots)
constexpr int kDefGrid = 512;         // workgroups (each owns a token scratch)

}  // namespace

GANON_API int64_t ganon_deflate_bound(int64_t in_len, int32_t block_in) {
  if (in_len < 0 || block_in < 0 || block_in > kDefMaxIn) return GANON_E_ARG;
  const int64_t bi = block_in ? block_in : kDefMaxIn;
  return in_len + 31 * ((in_len + bi - 1) / bi);
}

GANON_API int ganon_deflate_bgzf(ganon_ctx *ctx, const uint8_t *in, int64_t in_len, int32_t block_in, uint8_t *out,
                                 int64_t out_cap, int64_t *out_len, int32_t *member_sizes) {
  if (!ctx) return GANON_E_ARG;
  if (out_len) *out_len = 0;
  if (in_len < 0 || block_in < 0 || block_in > kDefMaxIn || out_cap < 0 || !out_len || (in_len && (!in || !out)))
    return fail(ctx, GANON_E_ARG, "ganon_deflate_bgzf: bad arguments");
  if (!in_len) return GANON_OK;
  const int bi = block_in ? block_in : kDefMaxIn;
  const int64_t n_blocks = (in_len + bi - 1) / bi;
  if (out_cap < ganon_deflate_bound(in_len, block_in))
    return fail(ctx, GANON_E_ARG, "ganon_deflate_bgzf: out_cap %lld is below ganon_deflate_bound's %lld",
                (long long)out_cap, (long long)ganon_deflate_bound(in_len, block_in));
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, GANON_E_DEVICE, "hipSetDevice failed");
  if (!ctx->deflate) ctx->deflate = new ganon_deflate_state();
  ganon_deflate_state *st = ctx->deflate;
  const int64_t cb = std::min(n_blocks, kDefChunk);
  const int grid = (int)std::min<int64_t>(cb, kDefGrid);
  int rc;
  if ((rc = def_grow(ctx, &st->in, st->in_cap, (size_t)(cb * bi))) ||
      (rc = def_grow(ctx, &st->slots, st->slots_cap, (size_t)(cb * kDefSlot))) ||
      (rc = def_grow(ctx, &st->out, st->out_cap, (size_t)(cb * kDefSlot))) ||
      (rc = def_grow(ctx, &st->tok, st->tok_cap, (size_t)grid * kDefMaxIn)) ||
      (rc = def_grow(ctx, &st->sizes, st->sizes_cap, (size_t)cb)) ||
      (rc = def_grow(ctx, &st->off, st->off_cap, (size_t)cb + 1)))
    return rc;
  hipStream_t s = ctx->stream;
  if (ctx->profiling) {   // a profiled call: ganon_last_kernel_times reports this call's kernels alone
    for (auto &r : ctx->recs) {
      ctx->pool.push_back(r.e0);
      ctx->pool.push_back(r.e1);
    }
    ctx->recs.clear();
  }
  int64_t written = 0;
  std::vector<int32_t> sz((size_t)cb);
  for (int64_t b0 = 0; b0 < n_blocks; b0 += kDefChunk) {
    const int64_t nb = std::min(n_blocks - b0, kDefChunk);
    const int64_t lo = b0 * bi, len = std::min(in_len - lo, nb * bi);
    const int64_t slots_bytes = (int64_t)st->slots_cap;
    if (len > (int64_t)st->in_cap || nb * kDefSlot > slots_bytes)
      return fail(ctx, GANON_E_STATE, "ganon_deflate_bgzf: chunk exceeds the device buffers");
    if (hipMemcpyAsync(st->in, in + lo, (size_t)len, hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(ctx, GANON_E_DEVICE, "ganon_deflate_bgzf: copy failed");
    {
      ganon_detail::KernelScope ks(ctx, "k_deflate");
      hipLaunchKernelGGL(k_deflate, dim3((unsigned)std::min<int64_t>(nb, grid)), dim3(kDefThreads), 0, s, st->in, len, bi,
                         nb, st->slots, st->tok, st->sizes);
    }
    if ((rc = check_launch(ctx, "k_deflate"))) {
      ganon_detail::sync_stream(s);
      return rc;
    }
    {
      ganon_detail::KernelScope ks(ctx, "k_deflate_compact");
      hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(kDefThreads), 0, s, st->sizes, nb, st->off);
      hipLaunchKernelGGL(k_deflate_compact, dim3((unsigned)nb), dim3(kDefThreads), 0, s, st->slots, st->sizes, st->off,
                         nb, st->out, (int64_t)st->out_cap);
    }
    if ((rc = check_launch(ctx, "k_deflate_compact"))) {
      ganon_detail::sync_stream(s);
      return rc;
    }
    if (ganon_detail::readback(sz.data(), st->sizes, (size_t)nb * 4, s) != hipSuccess ||
        ganon_detail::sync_stream(s) != hipSuccess)
      return fail(ctx, GANON_E_DEVICE, "ganon_deflate_bgzf: copy failed");
    int64_t total = 0;
    for (int64_t i = 0; i < nb; ++i) {
      const int64_t n_in = std::min<int64_t>(bi, in_len - (b0 + i) * bi);
      if (sz[i] < 26 || sz[i] > n_in + 31)
        return fail(ctx, GANON_E_DEVICE, "ganon_deflate_bgzf: member %lld has size %d", (long long)(b0 + i), sz[i]);
      total += sz[i];
    }
    if (written + total > out_cap || total > (int64_t)st->out_cap)
      return fail(ctx, GANON_E_STATE, "ganon_deflate_bgzf: the members exceed the bound");
    if (hipMemcpyAsync(out + written, st->out, (size_t)total, hipMemcpyDeviceToHost, s) != hipSuccess ||
        ganon_detail::sync_stream(s) != hipSuccess)
      return fail(ctx, GANON_E_DEVICE, "ganon_deflate_bgzf: copy failed");
    if (member_sizes) std::memcpy(member_sizes + b0, sz.data(), (size_t)nb * 4);
    written += total;
  }
  if ((rc = ganon_batch_sync(ctx))) return rc;   // (collects the kernel times when profiling)
  *out_len = written;
  return GANON_OK;
}

void ganon_deflate_free(ganon_deflate_state *st) {
  if (!st) return;
  for (void *p : {(void *)st->in, (void *)st->slots, (void *)st->out, (void *)st->tok, (void *)st->sizes, (void *)st->off})
    if (p) hipFree(p);
  delete st;
}

#if defined(DEF_PROF)
// (tuning build only) the summed phase cycles since the last call; then zeroed
GANON_API int ganon_deflate_prof_read(unsigned long long *out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_def_prof), sizeof(unsigned long long) * 5) != hipSuccess) return -1;
  unsigned long long z[5] = {0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_def_prof), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
