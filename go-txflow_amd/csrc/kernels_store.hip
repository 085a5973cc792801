// kernels_store.hip — TxStore.SaveTx's records for one batch, amino-encoded in HBM.
//
// Reference: the commit block runs txStore.SaveTx(set) for every fired vote (txflow/service.go:216-218
// -> tx/store.go:83-117): db.Set("H:%X", MarshalBinaryBare(TxVoteSet)) and db.Set("C:%X",
// MarshalBinaryBare(set.MakeCommit())).  Both keys depend on the TxHash alone, so the last write
// wins: every ADDED vote of a committed set fires, the set's last fired vote of a batch is its last
// ADDED vote of that batch, and the record written there is the one built from the set's accepted
// votes as of the end of the batch.  One record per set that fired in the batch, in the order of
// each set's last fired vote, leaves a key-value store as the per-vote cadence does.  CommitSigs are
// in validator-index order (the reference lists a Go map; txv_save_tx_bytes pins the same order).
//
// A record is four parts back to back, at a 16-byte aligned offset of the sink, zero padded to the
// next one:
//   "H:%X" | [0x0a uvarint(hl) TxHash] 0x12 0x20 TxKey | "C:%X" |
//   [0x0a uvarint(hl) TxHash] { 0x12 uvarint(sz) TxVote body (amino.hpp: txvote_body) } per accepted vote
//
// The chain (flow stream, behind the tally; every producer -> consumer pair is a launch apart;
// sets, count and apply are arrival_list.h's walk and scan, the encoder is store_dev.h):
//   sets    one wave per stamped set: a fired set's id and record length are stored at the arrival
//           index of its last fired vote, tagged with the batch stamp (never cleared)
//   count   per 1024 arrival indices: fired sets and their record bytes, each rounded up to 16
//   apply   exclusive scan over the indices: record k of the batch, its set and its byte offset
//           (64 bits: what a batch needs may exceed 4 GiB whatever the sink holds)
//   emit    per record, shared by up to kParts blocks: the CommitSig lengths are scanned over the
//           validators into LDS, then the record is assembled tile by tile in LDS -- 16 lanes per
//           CommitSig, each gathering its words of the arena columns independently of the others --
//           and every tile leaves as aligned 16-byte stores, pad zeros included.  A record that ends
//           past the sink's bytes or records is not written at all.
#include <algorithm>

#include "arrival_list.h"
#include "store_dev.h"

namespace {

using namespace txv_store;

// arrival index i is listed where a fired set's last fired vote arrived; its weight: the set's
// record length rounded up to 16 (rlen[i] is read, in bounds, for the other indices too: whatever an
// earlier batch left there is dropped by list_values)
struct StValue {
  StoreSink k;
  uint32_t stamp;
  __device__ __forceinline__ ListValue operator()(uint32_t i) const {
    return ListValue{(uint32_t)(k.tag[i] >> 32) == stamp, (k.rlen[i] + 15ull) & ~15ull};
  }
};

// sets: a fired set's id, tagged with the batch stamp, and its record length
__global__ void __launch_bounds__(64) txv_k_st_sets(FlowState fs, FlowBatch b, const uint32_t* n_stamped, StoreSink k) {
  fired_sets_walk(
      fs, b, n_stamped,
      [&](const TallyCell& c, uint32_t hl) -> uint64_t {
        const uint32_t a = acc_of(fs, c.acc);
        return a ? csig_len(fs.arena_height[a - 1], hl, fs.arena_sec[a - 1], fs.arena_nanos[a - 1]) : 0u;
      },
      [&](uint32_t i, uint32_t s, uint32_t hl, uint64_t bytes) {
        k.tag[i] = ((uint64_t)b.stamp << 32) | s;
        k.rlen[i] = 2ull * (2u + 2u * hl) + 2ull * hash_field_len(hl) + 34u + bytes;
      });
}

__global__ void __launch_bounds__(256) txv_k_st_count(FlowBatch b, StoreSink k) {
  list_count(b.n, k.blk, StValue{k, b.stamp});
}

// apply: record r of the batch, its set id and byte offset; foff[records] = the bytes the batch needs
__global__ void __launch_bounds__(256) txv_k_st_apply(FlowBatch b, StoreSink k, uint32_t nb) {
  uint64_t n_recs, n_bytes;
  const bool last = list_apply(
      b.n, nb, k.blk, StValue{k, b.stamp},
      [&](uint32_t i, uint64_t r, uint64_t off, const ListValue&) {
        k.fired[r] = (uint32_t)k.tag[i];
        k.foff[r] = off;
      },
      &n_recs, &n_bytes);
  if (last) k.foff[n_recs] = n_bytes;
}

// T threads, registries of up to Cap validators (Cap / T cells per thread), tiles of TB bytes; a
// record is shared by up to kParts blocks, each of which scans the whole set (cheap) and assembles
// every kParts-th tile.  <64, 128, 4096>: 5 KB of LDS; <256, 1024, 3840>: 12 KB, so the blocks fit
// beside the next batch's K1b as txv_k_upd_emit's do.
template <int T, uint32_t Cap, uint32_t TB, uint32_t kParts>
__global__ void __launch_bounds__(T) txv_k_st_emit(FlowState fs, StoreSink k, uint32_t nb) {
  constexpr int kPer = (int)(Cap / T);
  __shared__ uint32_t l_off[Cap];                // CommitSig v starts at l_off[v] of the Commit's list
  __shared__ uint32_t l_acc[Cap];                // its arena row + 1 (0: validator v has no accepted vote)
  __shared__ __attribute__((aligned(16))) uint8_t l_tile[TB];
  static_assert(TB % 16 == 0 && Cap % T == 0 && T % 64 == 0, "tile / block shape");
  const uint32_t t = threadIdx.x;
  const uint32_t n_rec = (uint32_t)k.blk[2 * (size_t)nb];
  const size_t M = fs.max_accepted;
  if (blockIdx.x == 0 && t == 0) {
    // the records that fit are a prefix: the largest w <= min(records, cap_recs) with foff[w] <= cap_bytes
    uint32_t lo = 0, hi = min(n_rec, k.cap_recs) + 1u;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (k.foff[mid] <= k.cap_bytes) lo = mid; else hi = mid;
    }
    const uint64_t wrote = k.foff[lo], need = k.blk[2 * (size_t)nb + 1];
    uint4* res = reinterpret_cast<uint4*>(k.result);
    res[0] = make_uint4(lo, n_rec, lo < n_rec ? 1u : 0u, 0u);
    res[1] = make_uint4((uint32_t)wrote, (uint32_t)(wrote >> 32), (uint32_t)need, (uint32_t)(need >> 32));
  }
  for (uint32_t work = blockIdx.x; work < n_rec * kParts; work += gridDim.x) {
    const uint32_t j = work / kParts, part = work % kParts;
    if (j >= k.cap_recs) break;                  // (block-uniform, as every exit below)
    const uint64_t start = k.foff[j], next = k.foff[j + 1];
    if (next > k.cap_bytes) break;
    if (next - start > 0xFFFFFFF0ull) continue;  // lengths are 32 bits (txv_store_records' lens_out)
    const uint32_t len16 = (uint32_t)(next - start);
    const uint32_t ntiles = (len16 + TB - 1) / TB;
    if (part >= ntiles) continue;
    const uint32_t s = k.fired[j];
    const SetEntry e = fs.tab[fs.set_entry[s]];
    const RecCtx R = rec_ctx(fs.keys + (e.key_off - 1), e.len, fs.set_txkey + (size_t)s * 8);
    // the CommitSig lengths, scanned over the validators (thread t: validators t * kPer ...)
    const TallyCell* row = fs.cell + (size_t)s * fs.n_vals;
    uint32_t acc[kPer], cl[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t v = t * (uint32_t)kPer + (uint32_t)i;
      acc[i] = v < fs.n_vals ? acc_of(fs, row[v].acc) : 0u;
    }
    int64_t hh[kPer], ss[kPer];
    int32_t nn[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t r = acc[i] ? acc[i] - 1u : 0u;
      hh[i] = fs.arena_height[r]; ss[i] = fs.arena_sec[r]; nn[i] = fs.arena_nanos[r];
    }
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      cl[i] = acc[i] ? csig_len(hh[i], R.hl, ss[i], nn[i]) : 0u;
      sum += cl[i];
    }
    uint64_t sigs;
    uint32_t run = (uint32_t)block_excl_scan64<T / 64>(sum, &sigs);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      l_off[t * (uint32_t)kPer + (uint32_t)i] = run;
      l_acc[t * (uint32_t)kPer + (uint32_t)i] = acc[i];
      run += cl[i];
    }
    __syncthreads();
    const uint32_t s3 = head_len(R);                          // the CommitSigs start here
    const uint32_t len = s3 + (uint32_t)sigs;                 // <= len16 < len + 16
    if (part == 0 && t == 0) {
      uint4* m = reinterpret_cast<uint4*>(k.rec + j);
      m[0] = make_uint4((uint32_t)start, (uint32_t)(start >> 32), R.l0, R.hf + 34u);
      m[1] = make_uint4(R.l0, R.hf + (uint32_t)sigs, s, 0u);
    }
    for (uint32_t tile = part; tile < ntiles; tile += kParts) {
      const uint32_t t0 = tile * TB, t1 = min(t0 + TB, len16);
      const Tile tl{l_tile, t0, t1 - t0};
      for (uint32_t x = t0 + t; x < min(s3, t1); x += T) l_tile[x - t0] = head_byte(R, x);
      for (uint32_t x = max(t0, len) + t; x < t1; x += T) l_tile[x - t0] = 0;
      if (t1 > s3 && t0 < len) {
        // the CommitSigs that cover the tile
        const uint32_t v0 = csig_at(l_off, Cap, max(t0, s3) - s3), v1 = csig_at(l_off, Cap, min(t1, len) - 1u - s3);
        const uint32_t q = t & 15u;
        for (uint32_t v = v0 + (t >> 4); v <= v1; v += T / 16) {
          const uint32_t a = l_acc[v];
          if (!a) continue;
          const size_t r = a - 1u;
          // this lane's gathers, independent of each other
          const int64_t height = fs.arena_height[r], sec = fs.arena_sec[r];
          const int32_t nanos = fs.arena_nanos[r];
          const uint32_t sw = fs.arena_sig[(size_t)q * M + r];
          const uint32_t tw = fs.arena_txkey[(size_t)(q & 7u) * M + r];
          const uint32_t aw = fs.val_addr[(size_t)v * 5 + min(q, 4u)];
          put_commit_sig(tl, R, s3 + l_off[v], q, height, sec, nanos, LaneWords{sw, tw, aw});
        }
      }
      __syncthreads();
      // the tile leaves as aligned 16-byte stores (start and t0 are multiples of 16)
      uint4* dst = reinterpret_cast<uint4*>(k.buf + start + t0);
      const uint4* src = reinterpret_cast<const uint4*>(l_tile);
      for (uint32_t c = t; c < (t1 - t0) / 16u; c += T) dst[c] = src[c];
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" hipError_t txv_flow_store_records(const FlowState* fs, const FlowBatch* b, const uint32_t* n_stamped,
                                             StoreSink k, hipStream_t st) {
  if (fs->n_vals > TXV_UPD_MAX_VALS) return hipErrorInvalidValue;
  uint32_t nb;
  if (!list_blocks(b->n, &nb)) return hipErrorInvalidValue;
  if (b->n) {
    const uint32_t waves = std::min<uint32_t>(b->n, 4096u);
    hipLaunchKernelGGL(txv_k_st_sets, dim3(waves), dim3(64), 0, st, *fs, *b, n_stamped, k);
    hipLaunchKernelGGL(txv_k_st_count, dim3(nb), dim3(256), 0, st, *b, k);
  }
  hipLaunchKernelGGL(txv_k_st_apply, dim3(nb ? nb : 1u), dim3(256), 0, st, *b, k, nb);
  // (an empty batch: one block, which writes the result words)
  const uint32_t blocks = std::min<uint32_t>(std::max<uint32_t>(b->n, 1u), 2048u);
  if (fs->n_vals <= 128) hipLaunchKernelGGL((txv_k_st_emit<64, 128, 4096, 4>), dim3(blocks), dim3(64), 0, st, *fs, k, nb);
  else hipLaunchKernelGGL((txv_k_st_emit<256, TXV_UPD_MAX_VALS, 3840, 16>), dim3(blocks), dim3(256), 0, st, *fs, k, nb);
  return hipGetLastError();
}
