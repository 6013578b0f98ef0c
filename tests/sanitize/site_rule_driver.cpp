// site_rule_driver.cpp — the evidence filters and the rule of --discover_sites under ASan/UBSan
// (tests/test_discover_rules_sanitizers.py): ganon_site_tally_create_ex, the record and quality filters of
// csrc/ganon_site_tally.h inside the decoders of csrc/ganon_host.cpp and the host compaction in both
// modes, linked into this executable with the sanitizer runtime (nothing is preloaded, nothing is loaded
// into Python). The packed genome lives in a heap block of exactly its size.
//
//   site_rule_driver file REF THREADS TUMOR.bam NORMAL.bam Q M F MODE     ganon_bam_open_ex2 on both files
//   site_rule_driver reader REF THREADS TUMOR.bam NORMAL.bam Q M F MODE   the readers (need the .bai): every
//                                                     sequence whole, then in overlapping thirds as regions
// Q: min base quality, M: min mapq, F: excluded flags, MODE: 0 both, 1 normal.
// Both print "<sequence> <pos> <code>" per site in order, then "sites <their number>".
// REF: a text file, "n_seq" then a line per sequence: its bases, or "-" for a sequence without a reference.
// BAM sequence id t is the tally's sequence t (ids past n_seq: none).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ganon_host.h"

static int fail(const char *what) {
  std::fprintf(stderr, "%s: %s\n", what, ganon_host_last_error());
  return 2;
}

int main(int argc, char **argv) {
  if (argc < 10) return 1;
  const std::string mode = argv[1];
  FILE *fh = std::fopen(argv[2], "r");
  if (!fh) return 1;
  int n_seq = 0;
  if (std::fscanf(fh, "%d", &n_seq) != 1 || n_seq < 0) return 1;
  std::vector<std::string> seqs;
  std::vector<int64_t> off, len;
  int64_t bytes = 0;
  for (int s = 0; s < n_seq; ++s) {
    static char buf[1 << 20];
    if (std::fscanf(fh, "%1048575s", buf) != 1) return 1;
    seqs.emplace_back(buf);
    if (seqs.back() == "-") {
      off.push_back(-1);
      len.push_back(7);
    } else {
      off.push_back(2 * bytes);
      len.push_back((int64_t)seqs.back().size());
      bytes += ((int64_t)seqs.back().size() + 1) / 2;
    }
  }
  std::fclose(fh);
  std::unique_ptr<uint8_t[]> nt16(new uint8_t[bytes ? bytes : 1]);
  for (int s = 0; s < n_seq; ++s)
    if (off[s] >= 0) ganon_pack_nt16(seqs[s].data(), len[s], nt16.get() + off[s] / 2);
  const int threads = std::atoi(argv[3]);
  const int32_t q = std::atoi(argv[6]), m = std::atoi(argv[7]), rule_mode = std::atoi(argv[9]);
  const uint32_t f = (uint32_t)std::strtoul(argv[8], nullptr, 0);
  ganon_site_tally *T = nullptr;
  // refused, not used: each value one past its range
  if (ganon_site_tally_create_ex(n_seq, nt16.get(), off.data(), len.data(), 94, m, f, rule_mode, &T) == 0 || T) return 6;
  if (ganon_site_tally_create_ex(n_seq, nt16.get(), off.data(), len.data(), q, 256, f, rule_mode, &T) == 0 || T) return 6;
  if (ganon_site_tally_create_ex(n_seq, nt16.get(), off.data(), len.data(), q, m, 65536u, rule_mode, &T) == 0 || T) return 6;
  if (ganon_site_tally_create_ex(n_seq, nt16.get(), off.data(), len.data(), q, m, f, 2, &T) == 0 || T) return 6;
  if (ganon_site_tally_create_ex(n_seq, nt16.get(), off.data(), len.data(), q, m, f, rule_mode, &T) != 0)
    return fail("ganon_site_tally_create_ex");
  for (int ds = 0; ds < 2; ++ds) {
    const char *path = argv[4 + ds];
    ganon_bam_reader *R = nullptr;
    if (ganon_bam_reader_open(path, threads, &R) != 0) return fail("ganon_bam_reader_open");
    ganon_bam_view h{};
    ganon_bam_reader_header(R, &h);
    std::vector<int32_t> map((size_t)h.n_ref);
    for (int32_t t = 0; t < h.n_ref; ++t) map[(size_t)t] = t < n_seq ? t : -1;
    if (mode == "file") {
      ganon_bam *b = nullptr;
      if (ganon_bam_open_ex2(path, threads, nullptr, 0, nullptr, T, ds, map.data(), h.n_ref, &b) != 0)
        return fail("ganon_bam_open_ex2");
      ganon_bam_close(b);
    } else if (mode == "reader") {
      if (ganon_bam_reader_set_site_tally(R, T, ds, map.data(), h.n_ref) != 0) return fail("ganon_bam_reader_set_site_tally");
      for (int32_t tid = 0; tid < h.n_ref; ++tid) {
        ganon_bam *b = nullptr;
        if (ganon_bam_reader_contig(R, tid, &b) != 0) return fail("ganon_bam_reader_contig");
        ganon_bam_close(b);
        const int64_t L = h.ref_len[tid];
        for (int k = 0; k < 3; ++k) {
          const int64_t a = k * L / 3 > 5 ? k * L / 3 - 5 : 0;
          if (ganon_bam_reader_region(R, tid, a, (k + 1) * L / 3, &b) != 0) return fail("ganon_bam_reader_region");
          ganon_bam_close(b);
        }
      }
    } else {
      return 1;
    }
    ganon_bam_reader_close(R);
  }
  long long total = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int64_t n = ganon_site_tally_count(T, s);
    if (n < 0) return fail("ganon_site_tally_count");
    // (arrays of exactly n: a site too many is a reported write)
    std::unique_ptr<int32_t[]> pos(new int32_t[n ? n : 1]);
    std::unique_ptr<uint8_t[]> code(new uint8_t[n ? n : 1]);
    if (n > 0 && ganon_site_tally_finish(T, s, pos.get(), code.get(), n - 1) != -1) return 6;   // too small: refused
    if (ganon_site_tally_finish(T, s, pos.get(), code.get(), n) != n) return fail("ganon_site_tally_finish");
    if (ganon_site_tally_bytes(T, s) != nullptr) return 7;   // released
    for (int64_t j = 0; j < n; ++j) std::printf("%d %d %d\n", s, (int)pos[j], (int)code[j]);
    total += n;
  }
  std::printf("sites %lld\n", total);
  ganon_site_tally_destroy(T);
  return 0;
}
