// routepool_dev.h — the per-vote pieces of CheckTx from a route buffer (kernels_routepool.hip) that
// are plain integer code, as __host__ __device__ functions so tests/cpu_emu/emu_routepool.hip runs
// the same source on the CPU: txVoteKey = SHA-256(Signature) (txvotepool/txvotepool.go:467-469) from
// the 64-byte row of the signature column, TxVote.Size() (types/tx_vote.go:144-150) from the scalar
// columns, whether the vote reaches CheckTx at all, and the header compare that guards every read
// beyond the buffer's first 64 bytes.
#pragma once
#include "amino.hpp"
#include "route.h"
#include "sha2.h"

namespace txv_routepool {

using namespace txv;

// SHA-256 of the first len (0..64) bytes of a signature row, m = its 16 words as loaded from memory
// (little-endian); key = the digest's 32 bytes as 8 words in memory order.  The padding is
// txv_k_sig_keys's: 0x80 behind the last byte, the bit length in the last word; len <= 55 fits one
// block, 56..64 take a second one that holds no message byte.
TXV_HD void sig_key(const uint32_t m[16], uint32_t len, uint32_t key[8]) {
  uint32_t st[8], w[16];
  sha256_init(st);
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const uint32_t word = bswap32(m[t]);
    const int valid = (int)len - 4 * t;                  // message bytes inside this word
    uint32_t v = 0;
    if (valid >= 4) v = word;
    else if (valid > 0) v = word & (0xFFFFFFFFu << (8 * (4 - valid)));
    if ((uint32_t)t == len / 4) v |= 0x80000000u >> (8 * (len & 3));
    w[t] = v;
  }
  if (len <= 55) w[15] = len * 8u;
  sha256_block(st, w);
  if (len > 55) {
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = 0;
    if (len == 64) w[0] = 0x80000000u;
    w[15] = len * 8u;
    sha256_block(st, w);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) key[j] = bswap32(st[j]);
}

// TxVote.Size() as the pool takes it (pool.cpp vote_size): 0 when amino rejects the time
TXV_HD uint32_t vote_size(int64_t height, uint32_t txhash_len, int64_t sec, int32_t nanos, uint32_t addr_len,
                          uint32_t sig_len) {
  return (uint32_t)txv_host::txvote_size(height, txhash_len, sec, nanos, addr_len, sig_len);
}

// 1: the vote reaches CheckTx.  A nil *TxVote never does, and of a signature above 64 bytes the
// buffer carries only the first 64, so its key cannot be formed: both are TXV_POOL_NOT_CHECKED
TXV_HD uint8_t vote_valid(uint32_t nil, uint32_t sig_len) { return (!nil && sig_len <= 64u) ? 1 : 0; }

// the buffer's header (its first 8 words) is the one the caller's meta describes: every address the
// kernel forms from the meta then lies inside the buffer the header's writer laid out
TXV_HD bool header_ok(const uint64_t h[8], uint32_t n, uint64_t arena_bytes, uint32_t flags, uint32_t max_txhash_len,
                      uint64_t total) {
  return h[0] == txv_route::kMagic && h[1] == (uint64_t)n && h[2] == arena_bytes && h[3] == (uint64_t)flags &&
         h[4] == (uint64_t)max_txhash_len && h[5] == total;
}

}  // namespace txv_routepool

// arguments of txv_k_route_keys (kernels_routepool.hip)
struct RouteKeysArgs {
  const uint8_t* buf;                // the route buffer (16-byte aligned)
  uint32_t n, flags, max_txhash_len; // the caller's meta
  uint64_t arena_bytes, total;
  uint64_t off[txv_route::kNCols];   // txv_route::layout of the meta
  uint32_t* keys;                    // [n][8]
  uint32_t* sizes;                   // [n]
  uint8_t* valid;                    // [n]
  uint32_t* err_host;                // mapped host word: 1 when the header is not the meta's
};

#if defined(__HIPCC__)
extern "C" hipError_t txv_launch_route_keys(const RouteKeysArgs* a, hipStream_t st);
#endif
