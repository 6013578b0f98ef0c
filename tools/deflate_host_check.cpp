// Host run of the GPU deflate's encoder (genomeanonymizer_amd/csrc/ganon_deflate_core.h,
// deflate_block with one lane and no barriers): the same source the kernel runs, checked against
// zlib on the CPU by tests/test_deflate_host.py. Plain C++17 (g++; also under ASan/UBSan). Test
// infrastructure, not part of the product.
//
//   deflate_host_check blocks in.bin meta.bin out.bin
// meta.bin: int64 n, then n x (int64 off, int64 len): the blocks of in.bin (1..0xFF00 bytes each).
// out.bin: the BGZF members back to back. Prints one member size per block (0 = refused).
//
//   deflate_host_check lengths LIMIT NSYM c0 c1 ... c(NSYM-1)
// Prints the code lengths the encoder gives the histogram (NSYM <= 288, LIMIT <= 15), one line.
#include "../genomeanonymizer_amd/csrc/ganon_deflate_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace ganon_deflate_core;

static std::vector<uint8_t> slurp(const char *p) {
  std::vector<uint8_t> v;
  FILE *f = std::fopen(p, "rb");
  if (!f) return v;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  std::fclose(f);
  return v;
}

static int run_lengths(int argc, char **argv) {
  if (argc < 4) return 2;
  const int limit = std::atoi(argv[2]), nsym = std::atoi(argv[3]);
  if (limit < 1 || limit > 15 || nsym < 2 || nsym > 288 || argc != 4 + nsym) return 2;
  std::unique_ptr<DefShared> S(new DefShared());
  std::memset(S.get(), 0, sizeof(DefShared));
  std::vector<uint32_t> freq((size_t)nsym);
  for (int i = 0; i < nsym; ++i) freq[(size_t)i] = (uint32_t)std::strtoul(argv[4 + i], nullptr, 10);
  std::vector<uint8_t> len((size_t)nsym, 0);
  def_build_lengths<1>(*S, freq.data(), nsym, limit, len.data(), 0);
  for (int i = 0; i < nsym; ++i) std::printf("%d%c", len[(size_t)i], i + 1 < nsym ? ' ' : '\n');
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "lengths")) return run_lengths(argc, argv);
  if (argc != 5 || std::strcmp(argv[1], "blocks")) return 2;
  const std::vector<uint8_t> in = slurp(argv[2]), meta = slurp(argv[3]);
  if (meta.size() < 8) return 2;
  int64_t n;
  std::memcpy(&n, meta.data(), 8);
  if (n < 0 || meta.size() != 8 + 16 * (size_t)n) return 2;
  std::unique_ptr<DefShared> S(new DefShared());
  std::memset(S.get(), 0, sizeof(DefShared));
  FILE *fo = std::fopen(argv[4], "wb");
  if (!fo) return 2;
  // (16-byte aligned, as the kernel's scratch is: the encoder reads four tokens at a time)
  std::unique_ptr<DefTok4[]> tok_mem(new DefTok4[kDefMaxIn / 4]);
  uint32_t *tok = tok_mem[0].v;
  for (int64_t i = 0; i < n; ++i) {
    int64_t m[2];
    std::memcpy(m, meta.data() + 8 + 16 * i, 16);
    int sz = 0;
    // (exactly the slot the kernel gives a member: a write past it is the sanitizer's to report)
    std::vector<uint8_t> slot((size_t)kDefSlot);
    if (m[0] >= 0 && m[1] >= 1 && m[1] <= kDefMaxIn && m[0] + m[1] <= (int64_t)in.size()) {
      // (a copy of exactly the block's length, so that a read past it is reported as well)
      std::vector<uint8_t> blk(in.begin() + m[0], in.begin() + m[0] + m[1]);
      sz = deflate_block<1>(*S, blk.data(), (int)m[1], slot.data(), tok, 0);
    }
    if (sz < 0 || sz > kDefSlot) sz = 0;
    std::fwrite(slot.data(), 1, (size_t)sz, fo);
    std::printf("%d\n", sz);
  }
  std::fclose(fo);
  return 0;
}
