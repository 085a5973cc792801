// kernels_routepool.hip — CheckTx from a route buffer in HBM: what the pool engine decides a batch
// from (PoolDevArgs keys / sizes / valid, pool_dev.h), computed straight from the buffer's columns.
//
// Reference: signTxRoutine hands every vote it signed to txVotePool.CheckTx (txvotepool/reactor.go:126
// -> txvotepool.go:180-261), which keys it by SHA-256(Signature) (:467-469) and weighs it by
// TxVote.Size().  txv_sign_txs leaves those votes as one route buffer (route.h); this kernel is the
// hop from that buffer to the engine, so the signatures never leave the device.
//
// One pass, one lane per vote, 256 threads per block.  Every lane reads the 64-byte header first and
// touches nothing beyond it unless it is the header the caller's meta describes (the submit cannot
// read the header, and a meta that overstated n would send the column reads out of bounds: the
// stride guard's idea, kernels_route.hip).  On a mismatch every vote is marked invalid -- the engine
// answers TXV_POOL_NOT_CHECKED and leaves the pool alone -- and a word in mapped host memory is set.
//
// The signature row (the column's offset is 16-byte aligned, its stride 64 bytes) is read as four
// 16-byte loads and the key leaves as two 16-byte stores; the scalar columns are read coalesced.
// The per-vote integer code is routepool_dev.h's.
#include "routepool_dev.h"

using namespace txv;

__global__ void __launch_bounds__(256) txv_k_route_keys(RouteKeysArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint4* hp = reinterpret_cast<const uint4*>(a.buf);
  uint64_t h[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 x = hp[q];
    h[2 * q] = (uint64_t)x.x | ((uint64_t)x.y << 32);
    h[2 * q + 1] = (uint64_t)x.z | ((uint64_t)x.w << 32);
  }
  const bool ok = txv_routepool::header_ok(h, a.n, a.arena_bytes, a.flags, a.max_txhash_len, a.total);
  if (!ok && i == 0) *a.err_host = 1u;
  if (i >= a.n) return;
  uint4* kp = reinterpret_cast<uint4*>(a.keys + (size_t)i * 8);
  if (!ok) {
    a.valid[i] = 0;
    a.sizes[i] = 0;
    kp[0] = make_uint4(0, 0, 0, 0);
    kp[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint8_t* b = a.buf;
  const int64_t height = reinterpret_cast<const int64_t*>(b + a.off[txv_route::kHeight])[i];
  const int64_t sec = reinterpret_cast<const int64_t*>(b + a.off[txv_route::kSec])[i];
  const int32_t nanos = reinterpret_cast<const int32_t*>(b + a.off[txv_route::kNanos])[i];
  const uint32_t th_len = reinterpret_cast<const uint32_t*>(b + a.off[txv_route::kLen])[i];
  const uint32_t addr_len = reinterpret_cast<const uint32_t*>(b + a.off[txv_route::kAddrLen])[i];
  const uint32_t sig_len = reinterpret_cast<const uint32_t*>(b + a.off[txv_route::kSigLen])[i];
  const uint32_t nil = (a.flags & txv_route::kFlagNil) ? (b + a.off[txv_route::kNil])[i] : 0u;
  const uint4* sp = reinterpret_cast<const uint4*>(b + a.off[txv_route::kSig]) + (size_t)i * 4;
  uint32_t m[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 x = sp[q];
    m[4 * q] = x.x; m[4 * q + 1] = x.y; m[4 * q + 2] = x.z; m[4 * q + 3] = x.w;
  }
  uint32_t key[8];
  txv_routepool::sig_key(m, sig_len < 64u ? sig_len : 64u, key);
  kp[0] = make_uint4(key[0], key[1], key[2], key[3]);
  kp[1] = make_uint4(key[4], key[5], key[6], key[7]);
  a.sizes[i] = txv_routepool::vote_size(height, th_len, sec, nanos, addr_len, sig_len);
  a.valid[i] = txv_routepool::vote_valid(nil, sig_len);
}

extern "C" hipError_t txv_launch_route_keys(const RouteKeysArgs* a, hipStream_t st) {
  if (!a->n) return hipSuccess;
  hipLaunchKernelGGL(txv_k_route_keys, dim3((a->n + 255) / 256), dim3(256), 0, st, *a);
  return hipGetLastError();
}
