// ganon_name_hash.h — read names to hex(BLAKE2s(name, key = K, digest_size = 16)) (--hash_read_names):
// RFC 7693 keyed mode, no salt or personalisation, fanout 1 and depth 1, 32 lowercase hex characters.
// One source for the host decoder (records_to_columns, csrc/ganon_host.cpp) and the device decoder
// (k_bam_name_hash, csrc/ganon_bam.hip): plain C++17, no HIP headers, the same bytes on both sides
// (as ganon_deflate_core.h). Internal to the libraries; not part of the C ABI.
//
// A keyed BLAKE2s hashes the key, zero padded to one 64-byte block, before the message. That block's
// compression does not depend on the name, so KeyState keeps the chaining value after it: a name of
// 1..64 bytes costs one compression. The empty name is the exception — there the key block is the
// final block — so its digest is a constant of the key too, kept as its 32 characters.
#ifndef GANON_NAME_HASH_H
#define GANON_NAME_HASH_H

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define NH_FN __host__ __device__ __forceinline__
#else
#define NH_FN inline
#endif

namespace ganon_nh {

constexpr int kHexLen = 32;      // characters per hashed name
constexpr int kSlot = 33;        // ... and its NUL: name_off[i] = 33 i
constexpr int kMaxKey = 32;

struct KeyState {
  uint32_t mid[8];        // the chaining value after the key block (t = 64, not final)
  char empty_hex[32];     // the hashed empty name
};

NH_FN uint32_t rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }

// BLAKE2s compression F: h the chaining value, m the block, t the bytes hashed so far (< 2^32 here).
NH_FN void compress(uint32_t h[8], const uint32_t m[16], uint32_t t, bool last) {
  constexpr uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                              0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  constexpr uint8_t sigma[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  uint32_t v[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) {
    v[i] = h[i];
    v[i + 8] = iv[i];
  }
  v[12] ^= t;
  if (last) v[14] = ~v[14];
#define NH_G(a, b, c, d, x, y)        \
  v[a] = v[a] + v[b] + (x);           \
  v[d] = rotr(v[d] ^ v[a], 16);       \
  v[c] = v[c] + v[d];                 \
  v[b] = rotr(v[b] ^ v[c], 12);       \
  v[a] = v[a] + v[b] + (y);           \
  v[d] = rotr(v[d] ^ v[a], 8);        \
  v[c] = v[c] + v[d];                 \
  v[b] = rotr(v[b] ^ v[c], 7);
  // (unrolled on the device: sigma's rows become register names, v and m stay out of scratch memory)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint8_t *s = sigma[r];
    NH_G(0, 4, 8, 12, m[s[0]], m[s[1]])
    NH_G(1, 5, 9, 13, m[s[2]], m[s[3]])
    NH_G(2, 6, 10, 14, m[s[4]], m[s[5]])
    NH_G(3, 7, 11, 15, m[s[6]], m[s[7]])
    NH_G(0, 5, 10, 15, m[s[8]], m[s[9]])
    NH_G(1, 6, 11, 12, m[s[10]], m[s[11]])
    NH_G(2, 7, 8, 13, m[s[12]], m[s[13]])
    NH_G(3, 4, 9, 14, m[s[14]], m[s[15]])
  }
#undef NH_G
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

// The digest's 16 bytes (h[0..3], little endian) as 32 hex characters, four per call of put(k, word):
// word k of the output holds characters 4k .. 4k + 3, the first in its low byte.
template <class Put>
NH_FN void to_hex(const uint32_t h[8], Put put) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 8; ++k) {
    const uint32_t two = (h[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;   // digest bytes 2k, 2k + 1
    uint32_t w = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 4; ++c) {
      // character c: byte c / 2 of the pair, its high nibble first
      const uint32_t nib = (two >> (8 * (c >> 1) + ((c & 1) ? 0 : 4))) & 0xFu;
      w |= (nib + (nib < 10 ? 48u : 87u)) << (8 * c);
    }
    put(k, w);
  }
}

// The key's state; key_len 1..32 (checked by the callers).
NH_FN void key_state(const uint8_t *key, int key_len, KeyState *ks) {
  constexpr uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                              0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  uint32_t m[16] = {0};
  for (int i = 0; i < key_len; ++i) m[i >> 2] |= (uint32_t)key[i] << (8 * (i & 3));
  uint32_t h[8], e[8];
  for (int i = 0; i < 8; ++i) h[i] = e[i] = iv[i];
  h[0] ^= 0x01010000u ^ ((uint32_t)key_len << 8) ^ 16u;   // fanout 1, depth 1, key length, digest length 16
  e[0] = h[0];
  compress(h, m, 64, false);
  compress(e, m, 64, true);
  for (int i = 0; i < 8; ++i) ks->mid[i] = h[i];
  to_hex(e, [&](int k, uint32_t w) {
    for (int c = 0; c < 4; ++c) ks->empty_hex[4 * k + c] = (char)((w >> (8 * c)) & 0xFF);
  });
}

// One name of `len` bytes (0..255): word(o, nb) returns the name's bytes o .. o + nb - 1 (1 <= nb <= 4)
// as a little-endian word, the bytes above them zero; put(k, w) takes the hashed name four characters
// at a time (to_hex).
template <class Word, class Put>
NH_FN void hash_name(const KeyState &ks, int len, Word word, Put put) {
  if (len <= 0) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 8; ++k) {
      const char *e = ks.empty_hex + 4 * k;
      put(k, (uint32_t)(uint8_t)e[0] | ((uint32_t)(uint8_t)e[1] << 8) | ((uint32_t)(uint8_t)e[2] << 16) |
                 ((uint32_t)(uint8_t)e[3] << 24));
    }
    return;
  }
  uint32_t h[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) h[i] = ks.mid[i];
  for (int b = 0; b < len; b += 64) {   // the last block is final even when it is full
    uint32_t m[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) {
      const int o = b + 4 * j, left = len - o;
      m[j] = left > 0 ? word(o, left < 4 ? left : 4) : 0u;
    }
    const bool last = b + 64 >= len;
    compress(h, m, 64u + (uint32_t)(last ? len : b + 64), last);
  }
  to_hex(h, put);
}

// Host convenience: name[0, len) to out[0, 32).
inline void hash_bytes(const KeyState &ks, const uint8_t *name, int len, char *out) {
  hash_name(
      ks, len,
      [&](int o, int nb) {
        uint32_t w = 0;
        for (int c = 0; c < nb; ++c) w |= (uint32_t)name[o + c] << (8 * c);
        return w;
      },
      [&](int k, uint32_t w) {
        for (int c = 0; c < 4; ++c) out[4 * k + c] = (char)((w >> (8 * c)) & 0xFF);
      });
}

}  // namespace ganon_nh

#endif  // GANON_NAME_HASH_H
