// namehash_driver.cpp — the read-name hash under ASan/UBSan (tests/test_namehash_sanitizers.py): the
// shared core (csrc/ganon_name_hash.h) and the keyed decoders of csrc/ganon_host.cpp, linked into this
// executable with the sanitizer runtime (nothing is preloaded, nothing is loaded into Python).
//
//   namehash_driver core KEYHEX              names of every length 0..255 (each in a heap block of
//                                            exactly its length, so that a read past its end is
//                                            reported), through hash_bytes and ganon_names_hash on 1
//                                            and 3 threads: prints "<name hex> <hash>" per name
//   namehash_driver file KEYHEX BAM THREADS  ganon_bam_open_keyed: prints "<hash>" per record
//   namehash_driver reader KEYHEX BAM        the keyed reader (needs the .bai): every sequence whole,
//                                            then in thirds as regions: prints "<hash>" per record
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../genomeanonymizer_amd/csrc/ganon_name_hash.h"
#include "../../include/ganon_host.h"

static std::vector<uint8_t> unhex(const char *s) {
  std::vector<uint8_t> out;
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
    unsigned v = 0;
    std::sscanf(s + i, "%2x", &v);
    out.push_back((uint8_t)v);
  }
  return out;
}

static int fail(const char *what) {
  std::fprintf(stderr, "%s: %s\n", what, ganon_host_last_error());
  return 2;
}

static void print_names(ganon_bam *b) {
  ganon_bam_view v{};
  ganon_bam_view_get(b, &v);
  for (int64_t i = 0; i < v.n_records; ++i) {
    if (v.name_len[i] != 32 || v.name_off[i] != 33 * i || v.names[v.name_off[i] + 32] != 0) {
      std::fprintf(stderr, "record %lld: not the fixed-width layout\n", (long long)i);
      std::exit(3);
    }
    std::printf("%.32s\n", v.names + v.name_off[i]);
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  const std::string mode = argv[1];
  const std::vector<uint8_t> key = unhex(argv[2]);
  if (mode == "core") {
    ganon_nh::KeyState ks;
    ganon_nh::key_state(key.data(), (int)key.size(), &ks);
    std::vector<std::unique_ptr<uint8_t[]>> names;
    std::vector<int32_t> len;
    uint32_t x = 12345;
    for (int L = 0; L <= 255; ++L) {
      names.emplace_back(new uint8_t[L ? L : 1]);
      for (int k = 0; k < L; ++k) {
        x = x * 1664525u + 1013904223u;
        names.back()[k] = (uint8_t)(1 + (x >> 24) % 255);
      }
      len.push_back(L);
    }
    // the batch entry point reads names[off, + len): one blob of exactly their bytes
    size_t total = 0;
    for (int L : len) total += (size_t)L;
    std::unique_ptr<char[]> blob(new char[total]);
    std::vector<int64_t> off;
    size_t at = 0;
    for (size_t i = 0; i < names.size(); ++i) {
      off.push_back((int64_t)at);
      std::memcpy(blob.get() + at, names[i].get(), (size_t)len[i]);
      at += (size_t)len[i];
    }
    const int64_t n = (int64_t)names.size();
    std::unique_ptr<char[]> out1(new char[33 * n]), out3(new char[33 * n]);
    if (ganon_names_hash(blob.get(), off.data(), len.data(), n, key.data(), (int32_t)key.size(), 1, out1.get()) != 0 ||
        ganon_names_hash(blob.get(), off.data(), len.data(), n, key.data(), (int32_t)key.size(), 3, out3.get()) != 0)
      return fail("ganon_names_hash");
    if (std::memcmp(out1.get(), out3.get(), (size_t)(33 * n)) != 0) return 4;
    for (int64_t i = 0; i < n; ++i) {
      std::unique_ptr<char[]> one(new char[32]);
      ganon_nh::hash_bytes(ks, names[i].get(), len[i], one.get());
      if (std::memcmp(one.get(), out1.get() + 33 * i, 32) != 0 || out1[33 * i + 32] != 0) return 5;
      for (int k = 0; k < len[i]; ++k) std::printf("%02x", names[i][k]);
      std::printf(" %.32s\n", one.get());
    }
    // refused, not read: a key of 0 or 33 bytes, a name of 256 bytes
    const int32_t big = 256;
    const int64_t zero = 0;
    if (ganon_names_hash(blob.get(), off.data(), len.data(), n, key.data(), 0, 1, out1.get()) == 0 ||
        ganon_names_hash(blob.get(), off.data(), len.data(), n, key.data(), 33, 1, out1.get()) == 0 ||
        ganon_names_hash(blob.get(), &zero, &big, 1, key.data(), (int32_t)key.size(), 1, out1.get()) == 0)
      return 6;
    return 0;
  }
  if (mode == "file" && argc >= 5) {
    ganon_bam *b = nullptr;
    if (ganon_bam_open_keyed(argv[3], std::atoi(argv[4]), key.data(), (int32_t)key.size(), &b) != 0)
      return fail("ganon_bam_open_keyed");
    print_names(b);
    ganon_bam_close(b);
    if (ganon_bam_open_keyed(argv[3], 1, key.data(), 0, &b) == 0 || ganon_bam_open_keyed(argv[3], 1, key.data(), 33, &b) == 0)
      return 6;
    return 0;
  }
  if (mode == "reader" && argc >= 4) {
    ganon_bam_reader *R = nullptr;
    if (ganon_bam_reader_open(argv[3], 3, &R) != 0) return fail("ganon_bam_reader_open");
    if (ganon_bam_reader_set_name_key(R, key.data(), 33) == 0) return 6;
    if (ganon_bam_reader_set_name_key(R, key.data(), (int32_t)key.size()) != 0) return fail("set_name_key");
    ganon_bam_view h{};
    ganon_bam_reader_header(R, &h);
    for (int32_t tid = 0; tid < h.n_ref; ++tid) {
      ganon_bam *b = nullptr;
      if (ganon_bam_reader_contig(R, tid, &b) != 0) return fail("ganon_bam_reader_contig");
      print_names(b);
      ganon_bam_close(b);
      const int64_t L = h.ref_len[tid];
      for (int k = 0; k < 3; ++k) {
        if (ganon_bam_reader_region(R, tid, k * L / 3, (k + 1) * L / 3, &b) != 0) return fail("ganon_bam_reader_region");
        print_names(b);
        ganon_bam_close(b);
      }
    }
    ganon_bam_reader_close(R);
    return 0;
  }
  return 1;
}
