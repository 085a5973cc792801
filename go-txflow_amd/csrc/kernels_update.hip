// kernels_update.hip — TxVotePool.Update's argument for one batch, built in HBM.
//
// Reference: after every fired vote the commit path runs txV.Update(height, set.GetVotes())
// (txflow/service.go:216-227 -> txvotepool/txvotepool.go:329-359).  One Update per batch with the
// "grouped" list leaves the pool exactly as that cadence does (tests/test_update_cadence.py):
//   - the sets that fired in the batch, ordered by the arrival index of their last fired vote,
//   - each set's accepted votes so far, in arrival (sequence) order, as one block.
// After the batch's tally the device state names all of it (txv_flow.h): b.stamped lists the sets
// the batch ADDED a vote to, set_cross tells which of them fired, a cell's candidate word carries
// the arrival index of its ADDED vote of this batch, its acc the arena row of its accepted vote.
//
// The chain (flow stream, behind the tally; every producer -> consumer pair is a launch apart;
// sets, count and apply are arrival_list.h's walk and scan):
//   sets    one wave per stamped set: a fired set's accepted-vote count and its id are stored at
//           the arrival index of its last fired vote (unique per set: a vote belongs to one set),
//           tagged with the batch stamp, so the columns are never cleared
//   count   per 1024 arrival indices: the fired sets and their entries
//   apply   exclusive scan over the indices: fired set k of the list and its first entry; the
//           result words (mapped host memory)
//   emit    one block per fired set: its accepted rows sorted by sequence number in LDS, then the
//           signature rows (16 lanes per 64-byte row), lengths, TxVote.Size() and set ids written
//           at first entry + rank; nothing at or past the sink's capacity
#include <algorithm>

#include "amino.hpp"
#include "arrival_list.h"

namespace {

// arrival index i is listed where a fired set's last fired vote arrived; its weight: the set's accepted votes
struct UpdValue {
  UpdateSink u;
  uint32_t stamp;
  __device__ __forceinline__ ListValue operator()(uint32_t i) const {
    const uint64_t w = u.cnt[i];
    return ListValue{(uint32_t)(w >> 32) == stamp, (uint32_t)w};
  }
};

// sets: a fired set's accepted-vote count and its id, tagged with the batch stamp
__global__ void __launch_bounds__(64) txv_k_upd_sets(FlowState fs, FlowBatch b, const uint32_t* n_stamped, UpdateSink u) {
  fired_sets_walk(
      fs, b, n_stamped, [](const TallyCell& c, uint32_t) -> uint64_t { return c.acc != 0 ? 1u : 0u; },
      [&](uint32_t i, uint32_t s, uint32_t, uint64_t cnt) {
        u.cnt[i] = ((uint64_t)b.stamp << 32) | (uint32_t)cnt;
        u.sid[i] = s;
      });
}

__global__ void __launch_bounds__(256) txv_k_upd_count(FlowBatch b, UpdateSink u) {
  list_count(b.n, u.blk, UpdValue{u, b.stamp});
}

// apply: fired set k of the list and its first entry; the batch's result words: entries written,
// fired sets, entries needed, 1 when they exceed the capacity
__global__ void __launch_bounds__(256) txv_k_upd_apply(FlowBatch b, UpdateSink u, uint32_t nb) {
  uint64_t n_sets, n_entries;
  const bool last = list_apply(
      b.n, nb, u.blk, UpdValue{u, b.stamp},
      [&](uint32_t i, uint64_t rank, uint64_t first, const ListValue&) {
        u.fired[2 * (size_t)rank] = u.sid[i];
        u.fired[2 * (size_t)rank + 1] = (uint32_t)first;
      },
      &n_sets, &n_entries);
  if (last) {
    const uint32_t need = (uint32_t)n_entries, sets = (uint32_t)n_sets;
    *reinterpret_cast<uint4*>(u.result) = make_uint4(min(need, u.cap), sets, need, need > u.cap ? 1u : 0u);
  }
}

// One block per fired set (persistent): 64 threads and a 128-entry LDS list (1.5 KB, so the blocks fit
// beside the next batch's K1b) for registries of up to 128 validators, else 256 threads and 1024
// entries (12 KB).  The set's accepted rows are listed with their sequence numbers, sorted by them
// (bitonic, in LDS: unique keys, padded to a power of two with ~0) and written out.  The kernel is
// latency bound (a C5 batch fires ~100 sets of ~1000 votes), so a thread's loads of a step are
// independent of each other (fixed trip counts, unrolled) and a set is shared by Cap / T blocks.
// The first version -- pairwise ranking, one block per set, one gather at a time -- took 265 us per
// C5 batch.
template <int T, uint32_t Cap>
__global__ void __launch_bounds__(T) txv_k_upd_emit(FlowState fs, UpdateSink u, uint32_t nb) {
  constexpr int kPer = (int)(Cap / T);                 // cells, and entries, per thread
  __shared__ uint64_t l_seq[Cap];
  __shared__ uint32_t l_row[Cap];
  __shared__ uint32_t l_k;
  const uint32_t t = threadIdx.x;
  const uint32_t n_fired = (uint32_t)u.blk[2 * (size_t)nb];
  const size_t M = fs.max_accepted;
  // kPer blocks per set: each lists and sorts the whole set (cheap) and writes T of its entries
  for (uint32_t work = blockIdx.x; work < n_fired * (uint32_t)kPer; work += gridDim.x) {
    const uint32_t j = work / (uint32_t)kPer, first = (work % (uint32_t)kPer) * T;
    const uint32_t s = u.fired[2 * (size_t)j], off = u.fired[2 * (size_t)j + 1];
    if (t == 0) l_k = 0;
    __syncthreads();
    const TallyCell* row = fs.cell + (size_t)s * fs.n_vals;
    uint32_t acc[kPer];
    uint64_t sq[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t v = t + (uint32_t)i * T;          // n_vals <= Cap = kPer * T
      acc[i] = v < fs.n_vals ? acc_of(fs, row[v].acc) : 0u;
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) sq[i] = acc[i] ? fs.arena_seq[acc[i] - 1] : 0ull;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      if (!acc[i]) continue;
      const uint32_t e = atomicAdd(&l_k, 1u);
      if (e < Cap) { l_seq[e] = sq[i]; l_row[e] = acc[i] - 1; }
    }
    __syncthreads();
    const uint32_t k = min(l_k, Cap);
    if (first >= k) {                                  // (block-uniform) no entry of this part
      __syncthreads();
      continue;
    }
    uint32_t P = 2;
    while (P < k) P <<= 1;                             // <= Cap (a power of two)
    for (uint32_t e = k + t; e < P; e += T) { l_seq[e] = ~0ull; l_row[e] = 0; }
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (uint32_t i = t; i < P / 2; i += T) {
          const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
          const uint64_t a = l_seq[lo], c = l_seq[hi];
          if ((a > c) == ((lo & size) == 0)) {
            l_seq[lo] = c; l_seq[hi] = a;
            const uint32_t ra = l_row[lo];
            l_row[lo] = l_row[hi]; l_row[hi] = ra;
          }
        }
        __syncthreads();
      }
    }
    // l_row[0 .. k): the set's rows in arrival order
    const uint32_t hl = fs.tab[fs.set_entry[s]].len;
    const uint32_t last = min(k, first + T);           // this part: entries [first, last)
    if (first + t < last && off + first + t < u.cap) {
      const uint32_t o = off + first + t, r = l_row[first + t];
      u.len[o] = 64;
      u.size[o] = (uint32_t)txv_host::txvote_size(fs.arena_height[r], hl, fs.arena_sec[r], fs.arena_nanos[r], 20, 64);
      u.set[o] = s;
    }
    // 16 lanes per 64-byte output row (the stores of a wave cover 4 consecutive rows); a thread's
    // 16 gathers are independent
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t idx = 16u * first + t + (uint32_t)q * T;
      w[q] = idx < 16u * last ? fs.arena_sig[(size_t)(idx & 15u) * M + l_row[idx >> 4]] : 0u;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const uint32_t idx = 16u * first + t + (uint32_t)q * T, o = off + (idx >> 4);
      if (idx < 16u * last && o < u.cap) u.sig[(size_t)o * 16 + (idx & 15u)] = w[q];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" hipError_t txv_flow_update_list(const FlowState* fs, const FlowBatch* b, const uint32_t* n_stamped,
                                           UpdateSink u, hipStream_t st) {
  if (fs->n_vals > TXV_UPD_MAX_VALS) return hipErrorInvalidValue;
  uint32_t nb;
  if (!list_blocks(b->n, &nb)) return hipErrorInvalidValue;
  if (b->n) {
    const uint32_t waves = std::min<uint32_t>(b->n, 4096u);
    hipLaunchKernelGGL(txv_k_upd_sets, dim3(waves), dim3(64), 0, st, *fs, *b, n_stamped, u);
    hipLaunchKernelGGL(txv_k_upd_count, dim3(nb), dim3(256), 0, st, *b, u);
  }
  hipLaunchKernelGGL(txv_k_upd_apply, dim3(nb ? nb : 1u), dim3(256), 0, st, *b, u, nb);
  if (b->n) {
    const uint32_t blocks = std::min<uint32_t>(b->n, 2048u);
    if (fs->n_vals <= 128) hipLaunchKernelGGL((txv_k_upd_emit<64, 128>), dim3(blocks), dim3(64), 0, st, *fs, u, nb);
    else hipLaunchKernelGGL((txv_k_upd_emit<256, TXV_UPD_MAX_VALS>), dim3(blocks), dim3(256), 0, st, *fs, u, nb);
  }
  return hipGetLastError();
}
