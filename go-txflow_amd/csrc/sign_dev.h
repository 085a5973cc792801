// sign_dev.h — the per-lane pieces of the batch signer (kernels_sign.hip) that are plain integer
// code, as __host__ __device__ functions so tests/cpu_emu/emu_sign.hip runs the same source on the
// CPU: the tx hash (NewTxVote's TxKey = SHA-256(tx) and TxHash = its upper-case hex,
// types/tx_vote.go:38-45) and RFC 8032's S = (r + k a) mod L.
#pragma once
#include "ed25519_dev.h"

namespace txv_sign {

using namespace txv;

// big-endian word k (bytes 4k .. 4k+3) of the byte string at p, any alignment, by aligned 32-bit
// loads: reads the aligned words that cover it (up to 3 bytes before p and 3 bytes behind the word)
TXV_HD uint32_t be_word(const uint8_t* p, uint32_t k) {
  const uintptr_t a = (uintptr_t)p + 4u * (uintptr_t)k;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t s = 8u * (uint32_t)(a & 3u);
  const uint32_t lo = q[0];
  return bswap32(s ? (lo >> s) | (q[1] << (32u - s)) : lo);
}

// SHA-256 of the n bytes at p (sha2.h's block function; the padding -- 0x80, zeros, the bit length
// in the last block's words 14 and 15 -- built here); st = the 8 big-endian state words.  The buffer
// must be readable up to the aligned word that holds byte n - 1 (the staging arena is padded).
TXV_HD void tx_sha256(const uint8_t* p, uint32_t n, uint32_t st[8]) {
  sha256_init(st);
  const uint32_t nblk = (n + 9u + 63u) / 64u;
  for (uint32_t b = 0; b < nblk; ++b) {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const uint32_t k = 16u * b + (uint32_t)t, at = 4u * k;
      uint32_t v = 0;
      if (at + 4u <= n) {
        v = be_word(p, k);
      } else if (at <= n) {                  // the word that holds the 0x80 after rem message bytes
        const uint32_t rem = n - at;
        if (rem) v = be_word(p, k) & (0xFFFFFFFFu << (32u - 8u * rem));
        v |= 0x80u << (24u - 8u * rem);
      }
      w[t] = v;
    }
    if (b == nblk - 1) { w[14] = n >> 29; w[15] = n << 3; }
    sha256_block(st, w);
  }
}

// four upper-case hex characters of a 16-bit value, most significant nibble first in memory
// (as a little-endian word)
TXV_HD uint32_t hex4(uint32_t h) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t x = (h >> (12 - 4 * i)) & 15u;
    r |= (x + (x < 10u ? 0x30u : 0x37u)) << (8 * i);
  }
  return r;
}

// the digest as TxKey (8 little-endian-loaded words of its 32 bytes) and TxHash (16 words of its 64
// hex characters)
TXV_HD void tx_key_hex(const uint32_t st[8], uint32_t key[8], uint32_t hex[16]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    key[i] = bswap32(st[i]);
    hex[2 * i] = hex4(st[i] >> 16);
    hex[2 * i + 1] = hex4(st[i] & 0xFFFFu);
  }
}

// S = (r + k a) mod L: the 512-bit product k * a (a = the clamped secret scalar, < 2^255) plus r,
// reduced as the SHA-512 outputs are (txv_k_sign's expression)
TXV_HD sc sc_muladd(const uint32_t k[8], const uint32_t a[8], const uint32_t r[8]) {
  uint32_t t[16];
  uint64_t acc = 0;
  uint32_t ovf = 0;
#pragma unroll
  for (int c = 0; c < 15; ++c) {
#pragma unroll
    for (int j = (c > 7 ? c - 7 : 0); j <= (c < 7 ? c : 7); ++j) mac(acc, ovf, k[j], a[c - j]);
    t[c] = (uint32_t)acc;
    acc = (acc >> 32) | ((uint64_t)ovf << 32);
    ovf = 0;
  }
  t[15] = (uint32_t)acc;
  uint64_t cc;
  add_cc(t[0], cc, t[0], r[0]);
#pragma unroll
  for (int j = 1; j < 16; ++j) addc_cc(t[j], cc, t[j], j < 8 ? r[j] : 0u, cc);
  return sc_reduce512(t);
}

}  // namespace txv_sign
