// emu_routepool.hip — TEST-ONLY host emulation of the per-vote pieces of CheckTx from a route buffer
// (go-txflow_amd/csrc/routepool_dev.h).
//
// Compiles the very same __host__ __device__ functions txv_k_route_keys runs -- the signature key
// with its padding, TxVote.Size(), the valid flag and the header compare -- for the CPU.  It is not
// linked into libtxvote.so and the product never calls it.
#include "../../go-txflow_amd/csrc/routepool_dev.h"
#include <cstring>

// SHA-256 of the first len bytes of a 64-byte signature row (the row is loaded as the kernel loads it)
extern "C" void emu_route_key(const uint8_t* row64, uint32_t len, uint8_t* key_out) {
  uint32_t m[16], key[8];
  memcpy(m, row64, 64);
  txv_routepool::sig_key(m, len, key);
  memcpy(key_out, key, 32);
}

extern "C" uint32_t emu_route_size(int64_t height, uint32_t txhash_len, int64_t sec, int32_t nanos, uint32_t addr_len,
                                   uint32_t sig_len) {
  return txv_routepool::vote_size(height, txhash_len, sec, nanos, addr_len, sig_len);
}

extern "C" uint32_t emu_route_valid(uint32_t nil, uint32_t sig_len) { return txv_routepool::vote_valid(nil, sig_len); }

extern "C" int emu_route_header_ok(const uint64_t* h8, uint32_t n, uint64_t arena_bytes, uint32_t flags,
                                   uint32_t max_txhash_len, uint64_t total) {
  return txv_routepool::header_ok(h8, n, arena_bytes, flags, max_txhash_len, total) ? 1 : 0;
}
