// known_sites_driver.cpp — the panel mask of --known_sites under ASan/UBSan
// (tests/test_known_sites_sanitizers.py): csrc/ganon_known_sites.h inside the decoders of
// csrc/ganon_host.cpp, linked into this executable with the sanitizer runtime (nothing is preloaded,
// nothing is loaded into Python). The table's arrays live in heap blocks of exactly their size, so that
// a read past a sequence's sites is reported.
//
//   known_sites_driver file SITES Q BAM THREADS   ganon_bam_open_ex: prints "<seq hex> <qual hex>" per
//                                                 record, then "count <bases rewritten>"
//   known_sites_driver reader SITES Q BAM         the reader (needs the .bai): every sequence whole, then
//                                                 in thirds as regions, then "count <the reader's count>"
// SITES: a text file "n_ref n" then n_ref + 1 offsets, then n lines "pos code". Q: -1 or 0..93.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>

#include "../../include/ganon_host.h"

static int fail(const char *what) {
  std::fprintf(stderr, "%s: %s\n", what, ganon_host_last_error());
  return 2;
}

static void print_records(ganon_bam *b) {
  ganon_bam_view v{};
  ganon_bam_view_get(b, &v);
  for (int64_t i = 0; i < v.n_records; ++i) {
    const int64_t L = v.l_seq[i];
    for (int64_t k = 0; k < (L + 1) / 2; ++k) std::printf("%02x", v.seq[v.seq_off[i] + k]);
    std::printf(" ");
    for (int64_t k = 0; k < L; ++k) std::printf("%02x", v.qual[v.qual_off[i] + k]);
    std::printf("\n");
  }
}

int main(int argc, char **argv) {
  if (argc < 5) return 1;
  const std::string mode = argv[1];
  FILE *fh = std::fopen(argv[2], "r");
  if (!fh) return 1;
  int n_ref = 0;
  long long n = 0;
  if (std::fscanf(fh, "%d %lld", &n_ref, &n) != 2 || n_ref < 0 || n < 0) return 1;
  std::unique_ptr<int64_t[]> off(new int64_t[n_ref + 1]);
  std::unique_ptr<int32_t[]> pos(new int32_t[n ? n : 1]);
  std::unique_ptr<uint8_t[]> code(new uint8_t[n ? n : 1]);
  for (int t = 0; t <= n_ref; ++t) {
    long long o;
    if (std::fscanf(fh, "%lld", &o) != 1) return 1;
    off[t] = o;
  }
  for (long long j = 0; j < n; ++j) {
    int p, c;
    if (std::fscanf(fh, "%d %d", &p, &c) != 2) return 1;
    pos[j] = p;
    code[j] = (uint8_t)c;
  }
  std::fclose(fh);
  const int q = std::atoi(argv[3]);
  ganon_sites *S = nullptr;
  // refused, not used: a quality of 94, and (with sites) unsorted positions or a code without ALT bits
  if (ganon_sites_create(n_ref, off.get(), pos.get(), code.get(), 94, &S) == 0) return 6;
  if (n >= 2 && off[1] >= 2) {
    std::swap(pos[0], pos[1]);
    if (ganon_sites_create(n_ref, off.get(), pos.get(), code.get(), q, &S) == 0) return 6;
    std::swap(pos[0], pos[1]);
    const uint8_t keep = code[0];
    code[0] = 0x10;
    if (ganon_sites_create(n_ref, off.get(), pos.get(), code.get(), q, &S) == 0) return 6;
    code[0] = keep;
  }
  if (ganon_sites_create(n_ref, off.get(), pos.get(), code.get(), q, &S) != 0) return fail("ganon_sites_create");
  // (the handle copied the arrays: they may go before it is used)
  off.reset();
  pos.reset();
  code.reset();
  if (mode == "file" && argc >= 6) {
    ganon_bam *b = nullptr;
    if (ganon_bam_open_ex(argv[4], std::atoi(argv[5]), nullptr, 0, S, &b) != 0) return fail("ganon_bam_open_ex");
    ganon_sites_destroy(S);
    print_records(b);
    std::printf("count %lld\n", (long long)ganon_bam_known_sites_masked(b));
    ganon_bam_close(b);
    return 0;
  }
  if (mode == "reader") {
    ganon_bam_reader *R = nullptr;
    if (ganon_bam_reader_open(argv[4], 3, &R) != 0) return fail("ganon_bam_reader_open");
    if (ganon_bam_reader_set_known_sites(R, S) != 0) return fail("ganon_bam_reader_set_known_sites");
    ganon_sites_destroy(S);   // (the reader shares the table)
    ganon_bam_view h{};
    ganon_bam_reader_header(R, &h);
    for (int32_t tid = 0; tid < h.n_ref; ++tid) {
      ganon_bam *b = nullptr;
      if (ganon_bam_reader_contig(R, tid, &b) != 0) return fail("ganon_bam_reader_contig");
      print_records(b);
      ganon_bam_close(b);
      const int64_t L = h.ref_len[tid];
      for (int k = 0; k < 3; ++k) {
        if (ganon_bam_reader_region(R, tid, k * L / 3, (k + 1) * L / 3, &b) != 0) return fail("ganon_bam_reader_region");
        print_records(b);
        ganon_bam_close(b);
      }
    }
    std::printf("count %lld\n", (long long)ganon_bam_reader_known_sites_masked(R));
    ganon_bam_reader_close(R);
    return 0;
  }
  return 1;
}
