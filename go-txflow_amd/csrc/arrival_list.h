// arrival_list.h — what the per-batch sinks (kernels_update.hip, kernels_store.hip,
// kernels_gossip.hip) share on the device: the walk over the sets that fired in a batch, and the
// scan that lists a batch's arrival indices in order.  The __global__ kernels stay per sink and
// call these with what an index is worth and what is written where one is listed.
#pragma once
#include "block_scan.h"
#include "txv_flow.h"

constexpr uint32_t kListItems = 1024;      // arrival indices per scan block (256 threads x 4 consecutive)
constexpr uint32_t kListMaxBlocks = 8192;  // a block sums the block totals before its own: at most 32 per thread

// scan blocks of a batch of n votes; false when list_apply's prefix pass cannot cover them
inline bool list_blocks(uint32_t n, uint32_t* nb) {
  *nb = (n + kListItems - 1) / kListItems;
  return *nb <= kListMaxBlocks;
}

// the arena row of a cell's accepted vote + 1, or 0
__device__ __forceinline__ uint32_t acc_of(const FlowState& fs, uint32_t acc) { return acc <= fs.max_accepted ? acc : 0u; }

// One wave per set the batch ADDED a vote to (persistent one-wave blocks, as txv_k_tally_cross).
// A set fired in this batch iff the crossing step left it a crossing index; its last fired vote is
// the largest arrival index among its cells' candidates of this batch (every ADDED vote at or after
// the crossing fires, and the crossing vote itself is one of them).  cell(c, hl) is what one cell
// adds (hl: the set's TxHash length); lane 0 calls store(i, s, hl, sum) with the wave's sum at the
// arrival index i of the set's last fired vote (unique per set: a vote belongs to one set).
template <class Cell, class Store>
__device__ __forceinline__ void fired_sets_walk(const FlowState& fs, const FlowBatch& b, const uint32_t* n_stamped, Cell cell,
                                                Store store) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n_list = min(*n_stamped, b.n);
  for (uint32_t j = blockIdx.x; j < n_list; j += gridDim.x) {
    const uint32_t s = b.stamped[j];
    if (s >= fs.max_txs || fs.set_cross[s] == TXV_NO_CROSS) continue;
    const uint32_t hl = fs.tab[fs.set_entry[s]].len;
    const TallyCell* row = fs.cell + (size_t)s * fs.n_vals;
    uint64_t sum = 0;
    uint32_t last1 = 0;                          // 1 + the largest arrival index (0: none)
    for (uint32_t v = lane; v < fs.n_vals; v += 64) {
      const TallyCell c = row[v];
      sum += cell(c, hl);
      const uint32_t f = cand_of(c.cand, b.stamp);
      if (f != TXV_NONE) last1 = max(last1, f + 1u);
    }
    sum = wave_sum(sum);
    last1 = wave_max(last1);
    if (lane == 0 && last1 != 0 && last1 - 1u < b.n) store(last1 - 1u, s, hl, sum);
  }
}

// what arrival index i is worth to a list: whether it is listed, its weight (entries, bytes), and a
// word of the sink's own that travels to place()
struct ListValue {
  bool listed;
  uint64_t weight;
  uint64_t word = 0;
};

// this thread's four indices: their values, and the sums over the listed ones
template <class Value>
__device__ __forceinline__ void list_values(uint32_t n, Value value, ListValue x[4], uint64_t* items, uint64_t* weight) {
  const uint32_t base = blockIdx.x * kListItems + 4u * threadIdx.x;
  *items = *weight = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x[k] = base + k < n ? value(base + k) : ListValue{false, 0};   // (a value that is not listed weighs nothing)
    if (!x[k].listed) x[k].weight = 0;
    *items += x[k].listed ? 1u : 0u;
    *weight += x[k].weight;
  }
}

// blk[2 j], blk[2 j + 1] = the listed indices of scan block j and their weight (256 threads)
template <class Value>
__device__ __forceinline__ void list_count(uint32_t n, uint64_t* blk, Value value) {
  ListValue x[4];
  uint64_t items, weight, ti, tw;
  list_values(n, value, x, &items, &weight);
  (void)block_excl_scan64(items, &ti);
  (void)block_excl_scan64(weight, &tw);
  if (threadIdx.x == 0) {
    blk[2 * (size_t)blockIdx.x] = ti;
    blk[2 * (size_t)blockIdx.x + 1] = tw;
  }
}

// Exclusive scan over the arrival indices: place(i, rank, offset, value) for every listed index in
// order -- its rank among the listed ones, the weight listed before it and its own value.  Each block sums the
// block totals before its own itself (nb <= kListMaxBlocks), so no launch of its own computes their
// prefix.  The last block's thread 0 writes the batch's totals to blk[2 nb], blk[2 nb + 1] (no block
// reads them), hands them out and returns true: the caller writes its result words there.
// n == 0: one block, which does only that.
template <class Value, class Place>
__device__ __forceinline__ bool list_apply(uint32_t n, uint32_t nb, uint64_t* blk, Value value, Place place, uint64_t* items,
                                           uint64_t* weight) {
  uint64_t pi = 0, pw = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256) {
    pi += blk[2 * (size_t)j];
    pw += blk[2 * (size_t)j + 1];
  }
  uint64_t before_i, before_w;
  (void)block_excl_scan64(pi, &before_i);
  (void)block_excl_scan64(pw, &before_w);
  ListValue x[4];
  uint64_t mine_i, mine_w, tot_i, tot_w;
  list_values(n, value, x, &mine_i, &mine_w);
  uint64_t rank = before_i + block_excl_scan64(mine_i, &tot_i);     // < the listed indices <= n
  uint64_t off = before_w + block_excl_scan64(mine_w, &tot_w);
  const uint32_t base = blockIdx.x * kListItems + 4u * threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (x[k].listed) {
      place(base + k, rank, off, x[k]);
      ++rank;
      off += x[k].weight;
    }
  }
  if (blockIdx.x + 1 != gridDim.x || threadIdx.x != 0) return false;
  *items = blk[2 * (size_t)nb] = before_i + tot_i;
  *weight = blk[2 * (size_t)nb + 1] = before_w + tot_w;
  return true;
}
