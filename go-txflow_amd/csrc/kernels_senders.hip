// kernels_senders.hip — MempoolTxVote.Senders on the GPU for a pool with TXV_POOL_SENDERS and its
// list in HBM (senders_dev.h holds every per-element rule; pool_dev.h the list it sits beside).
//
// Per batch (txv_senders_batch, between pd_status and the launch that indexes the batch's appends):
//   sn_flag     okf[j] = the vote at sorted position j was admitted
//   (hipcub)    cpos = exclusive scan of okf
//   sn_compact  the admitted votes' slices and arrival indices, compacted in sorted order
//   sn_record   one lane per vote: an admitted vote stores (its new position, sender); an
//               ErrTxInCache vote resolves the entry txsMap holds for its key at that moment --
//               the batch's latest earlier admission of the key (resolve_hit over the compacted
//               columns: a binary search and a short step back), else the list index as it stands
//               before the appends are indexed -- and stores (that entry, sender)
// Producer and consumer are always a launch apart; the only cross-block writes are the set's
// compare-and-swaps and one add per wave on the set's word count.
#include <hipcub/hipcub.hpp>
#include "txv_device.h"
#include "pool_dev.h"
#include "senders_dev.h"
#include "../../include/txvote.h"

using txv_senders::word_t;

namespace {

// the entry txsMap indexes for key k (pool_dev.h: tag = k[3], tombstones skipped), or kNone
__device__ uint32_t list_find(const uint32_t* lk, const unsigned long long* li, uint32_t imask, uint64_t seed,
                              const uint32_t* k) {
  const uint32_t tg = k[3];
  uint32_t s = (uint32_t)txv_hash::key32(k, seed ^ kSeedList) & imask;
  for (uint32_t probe = 0; probe <= imask; ++probe, s = (s + 1) & imask) {
    const unsigned long long v = __hip_atomic_load(li + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0) return txv_senders::kNone;
    if ((uint32_t)(v >> 32) != tg || (uint32_t)v == kListTomb) continue;
    if (txv_senders::key_eq8(lk + (size_t)((uint32_t)v - 1) * 8, k)) return (uint32_t)v - 1;
  }
  return txv_senders::kNone;
}

// the wave's sum of c added to *count by its first lane
__device__ __forceinline__ void wave_count(unsigned long long* count, uint32_t c) {
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

__global__ void __launch_bounds__(256) sn_flag(SendersArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t i = a.sidx[j];
  a.okf[j] = (i >= a.n_force && a.status[i] == TXV_POOL_OK) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) sn_compact(SendersArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n || !a.okf[j]) return;
  const uint32_t c = a.cpos[j];
  a.ckey[c] = a.skey[j];
  a.cidx[c] = a.sidx[j];
}

__global__ void __launch_bounds__(256) sn_record(SendersArgs a) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  uint32_t stored = 0;
  if (j < a.n) {
    const uint32_t i = a.sidx[j];
    const uint8_t st = i >= a.n_force ? a.status[i] : (uint8_t)TXV_POOL_NOT_CHECKED;
    uint32_t entry = txv_senders::kNone;
    if (st == TXV_POOL_OK) {
      entry = *a.tail_in + a.okpos[i];                                  // :250
    } else if (st == TXV_POOL_ERR_IN_CACHE) {                           // :213-227
      const uint32_t m = a.cpos[a.n - 1] + a.okf[a.n - 1];
      const uint32_t r = txv_senders::resolve_hit(a.ckey, a.cidx, m, a.skey[j], i, a.keys);
      entry = r != txv_senders::kNone ? *a.tail_in + a.okpos[r]
                                      : list_find(a.lk, a.li, a.imask, a.seed, a.keys + (size_t)i * 8);
    }
    if (entry != txv_senders::kNone)
      stored = txv_senders::insert(a.slots, a.mask, txv_senders::pair_word(entry, a.senders[i - a.n_force]), a.seed) > 0;
  }
  wave_count(a.count, stored);
}

// a rebuild: every word of the old set whose entry is alive into the new one (cleared before), at
// the entry's position after the compaction npos describes (null: positions stay)
__global__ void __launch_bounds__(256) sn_remap(const word_t* old, uint64_t n_old, const uint8_t* alive,
                                                const uint32_t* npos, word_t* neu, uint64_t nmask, uint64_t seed,
                                                unsigned long long* count) {
  const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t stored = 0;
  if (s < n_old) {
    const word_t w = txv_senders::remap_alive(old[s], alive, npos);
    if (w) stored = txv_senders::insert(neu, nmask, w, seed) > 0;
  }
  wave_count(count, stored);
}

// txv_pool_sent_by: one wave per key.  The list probe once (every lane the same address), then
// lane p tests peers[p0 + p], a ballot, and the row's words written by lanes 0 and 1.  status (or
// null): only the rows of admitted votes are looked up (the ticket form); the others are zero.
__global__ void __launch_bounds__(256) sn_query(const uint32_t* keys, const uint8_t* status, uint32_t n,
                                                const uint16_t* peers, uint32_t n_peers, const uint32_t* lk,
                                                const unsigned long long* li, uint32_t imask, const word_t* slots,
                                                uint64_t mask, uint64_t seed, uint32_t* bits) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint32_t W = (n_peers + 31) / 32;
  uint32_t entry = txv_senders::kNone;
  if (!status || status[i] == TXV_POOL_OK) entry = list_find(lk, li, imask, seed, keys + (size_t)i * 8);
  for (uint32_t p0 = 0; p0 < n_peers; p0 += 64) {
    const uint32_t p = p0 + lane;
    const bool in = entry != txv_senders::kNone && p < n_peers &&
                    txv_senders::contains(slots, mask, txv_senders::pair_word(entry, peers[p]), seed);
    const unsigned long long b = __ballot(in);
    const uint32_t w = p0 / 32 + lane;
    if (lane < 2 && w < W) bits[(size_t)i * W + w] = (uint32_t)(b >> (32 * lane));
  }
}

}  // namespace

extern "C" size_t txv_senders_tmp_bytes(uint32_t n) {
  size_t c = 0;
  uint32_t* u = nullptr;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, u, u, (int)std::max<uint32_t>(n, 1));
  return c;
}

extern "C" hipError_t txv_senders_batch(const SendersArgs* ap, hipStream_t st) {
  const SendersArgs& a = *ap;
  if (a.n <= a.n_force) return hipSuccess;
  const dim3 g((a.n + 255) / 256), b(256);
  hipError_t e;
  size_t tb = a.tmp_bytes;
  hipLaunchKernelGGL(sn_flag, g, b, 0, st, a);
  if ((e = hipcub::DeviceScan::ExclusiveSum(a.tmp, tb, a.okf, a.cpos, (int)a.n, st))) return e;
  hipLaunchKernelGGL(sn_compact, g, b, 0, st, a);
  hipLaunchKernelGGL(sn_record, g, b, 0, st, a);
  return hipGetLastError();
}

// neu (n_new slots) = the alive entries' words of old (n_old slots), *count = how many
extern "C" hipError_t txv_senders_rebuild(const word_t* old, uint64_t n_old, const uint8_t* alive, const uint32_t* npos,
                                          word_t* neu, uint64_t n_new, uint64_t seed, unsigned long long* count,
                                          hipStream_t st) {
  hipError_t e;
  if ((e = hipMemsetAsync(neu, 0, n_new * 8, st))) return e;
  if ((e = hipMemsetAsync(count, 0, 8, st))) return e;
  hipLaunchKernelGGL(sn_remap, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, st, old, n_old, alive, npos, neu,
                     n_new - 1, seed, count);
  return hipGetLastError();
}

extern "C" hipError_t txv_senders_query(const uint32_t* keys, const uint8_t* status, uint32_t n, const uint16_t* peers,
                                        uint32_t n_peers, const uint32_t* lk, const unsigned long long* li, uint32_t imask,
                                        const word_t* slots, uint64_t mask, uint64_t seed, uint32_t* bits, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(sn_query, dim3((n + 3) / 4), dim3(256), 0, st, keys, status, n, peers, n_peers, lk, li, imask, slots,
                     mask, seed, bits);
  return hipGetLastError();
}
