// sa_clips_driver.cpp — the SA clip mask of --mask_sa_clips under ASan/UBSan
// (tests/test_sa_clips_sanitizers.py): csrc/ganon_sa_clips.h inside the decoder of csrc/ganon_host.cpp,
// linked into this executable with the sanitizer runtime (nothing is preloaded, nothing is loaded into
// Python). The table's and the names' arrays live in heap blocks of exactly their size, so that a read
// past them is reported; the decoder's own aux blob ends with the last record's aux bytes.
//
//   sa_clips_driver SITES NAMES Q BAM THREADS   ganon_bam_open_ex with the rule on: prints
//                                               "<seq hex> <qual hex>" per record, then
//                                               "count <panel bases> <clip bases> <entries ignored>"
// SITES: a text file "n_ref n" then n_ref + 1 offsets, then n lines "pos code". NAMES: a text file "n"
// then n lines "tid name", sorted bytewise. Q: -1 or 0..93.
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
  if (argc < 6) return 1;
  FILE *fh = std::fopen(argv[1], "r");
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
  fh = std::fopen(argv[2], "r");
  if (!fh) return 1;
  int n_names = 0;
  if (std::fscanf(fh, "%d", &n_names) != 1 || n_names < 0) return 1;
  std::vector<std::string> names;
  std::unique_ptr<int32_t[]> name_tid(new int32_t[n_names ? n_names : 1]);
  std::unique_ptr<int64_t[]> name_off(new int64_t[n_names + 1]);
  name_off[0] = 0;
  for (int i = 0; i < n_names; ++i) {
    int t;
    char buf[256];
    if (std::fscanf(fh, "%d %255s", &t, buf) != 2) return 1;
    name_tid[i] = t;
    names.emplace_back(buf);
    name_off[i + 1] = name_off[i] + (int64_t)names.back().size();
  }
  std::fclose(fh);
  std::unique_ptr<char[]> blob(new char[name_off[n_names] ? name_off[n_names] : 1]);
  for (int i = 0; i < n_names; ++i) std::memcpy(blob.get() + name_off[i], names[i].data(), names[i].size());
  const int q = std::atoi(argv[3]);
  ganon_sites *S = nullptr;
  if (ganon_sites_create(n_ref, off.get(), pos.get(), code.get(), q, &S) != 0) return fail("ganon_sites_create");
  // refused, not used: names out of order, and a sequence id the table does not have
  if (n_names >= 2) {
    std::swap(name_tid[0], name_tid[1]);
    const int32_t keep = name_tid[0];
    name_tid[0] = n_ref;
    if (ganon_sites_set_sa_clips(S, n_names, blob.get(), name_off.get(), name_tid.get(), 1) == 0) return 6;
    name_tid[0] = keep;
    std::swap(name_tid[0], name_tid[1]);
  }
  if (ganon_sites_set_sa_clips(S, n_names, blob.get(), name_off.get(), name_tid.get(), 1) != 0)
    return fail("ganon_sites_set_sa_clips");
  // (the handle copied the arrays: they may go before it is used)
  off.reset();
  pos.reset();
  code.reset();
  blob.reset();
  name_off.reset();
  name_tid.reset();
  ganon_bam *b = nullptr;
  if (ganon_bam_open_ex(argv[4], std::atoi(argv[5]), nullptr, 0, S, &b) != 0) return fail("ganon_bam_open_ex");
  ganon_sites_destroy(S);
  ganon_bam_view v{};
  ganon_bam_view_get(b, &v);
  for (int64_t i = 0; i < v.n_records; ++i) {
    const int64_t L = v.l_seq[i];
    for (int64_t k = 0; k < (L + 1) / 2; ++k) std::printf("%02x", v.seq[v.seq_off[i] + k]);
    std::printf(" ");
    for (int64_t k = 0; k < L; ++k) std::printf("%02x", v.qual[v.qual_off[i] + k]);
    std::printf("\n");
  }
  std::printf("count %lld %lld %lld\n", (long long)ganon_bam_known_sites_masked(b), (long long)ganon_bam_sa_clips_masked(b),
              (long long)ganon_bam_sa_entries_ignored(b));
  ganon_bam_close(b);
  return 0;
}
