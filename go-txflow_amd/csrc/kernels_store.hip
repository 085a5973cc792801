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
// The chain (flow stream, behind the tally; every producer -> consumer pair is a launch apart):
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

#include "amino.hpp"
#include "block_scan.h"
#include "txv_flow.h"

namespace {

constexpr uint32_t kStItems = 1024;    // arrival indices per scan block (256 threads x 4 consecutive)

__device__ __forceinline__ uint32_t uv_len(uint64_t v) { return txv_host::put_uvarint(nullptr, v); }
// [tag uvarint(hl) TxHash]: field 1 of TxVoteSet and Commit, field 2 of a TxVote; omitted when empty
__device__ __forceinline__ uint32_t hash_field_len(uint32_t hl) { return hl ? 1u + uv_len(hl) + hl : 0u; }
// one CommitSig of a set whose TxHash has hl bytes: 0x12 uvarint(sz) + the TxVote body
__device__ __forceinline__ uint32_t csig_len(int64_t height, uint32_t hl, int64_t sec, int32_t nanos) {
  const uint32_t sz = (uint32_t)txv_host::txvote_size(height, hl, sec, nanos, 20, 64);
  return 1u + uv_len(sz) + sz;
}
// the arena row of a cell's accepted vote + 1, or 0
__device__ __forceinline__ uint32_t acc_of(const FlowState& fs, uint32_t acc) { return acc <= fs.max_accepted ? acc : 0u; }

// this index's scan value: the padded record length where a fired set's last fired vote arrived
// (a record is never empty: it holds at least the two key prefixes and the TxKey field)
__device__ __forceinline__ uint64_t st_value(const StoreSink& k, uint32_t i, uint32_t n, uint32_t stamp) {
  if (i >= n) return 0;
  return (uint32_t)(k.tag[i] >> 32) == stamp ? ((k.rlen[i] + 15ull) & ~15ull) : 0ull;
}

// One wave per set the batch ADDED a vote to, as txv_k_upd_sets: fired iff the crossing step left a
// crossing index, last fired vote = the largest candidate of this batch among its cells.
__global__ void __launch_bounds__(64) txv_k_st_sets(FlowState fs, FlowBatch b, const uint32_t* n_stamped, StoreSink k) {
  const int lane = threadIdx.x & 63;
  const uint32_t n_list = min(*n_stamped, b.n);
  for (uint32_t j = blockIdx.x; j < n_list; j += gridDim.x) {
    const uint32_t s = b.stamped[j];
    if (s >= fs.max_txs || fs.set_cross[s] == TXV_NO_CROSS) continue;
    const uint32_t hl = fs.tab[fs.set_entry[s]].len;
    const TallyCell* row = fs.cell + (size_t)s * fs.n_vals;
    uint64_t bytes = 0;
    uint32_t last1 = 0;                          // 1 + the largest arrival index (0: none)
    for (uint32_t v = lane; v < fs.n_vals; v += 64) {
      const TallyCell c = row[v];
      const uint32_t a = acc_of(fs, c.acc);
      if (a) bytes += csig_len(fs.arena_height[a - 1], hl, fs.arena_sec[a - 1], fs.arena_nanos[a - 1]);
      const uint32_t f = cand_of(c.cand, b.stamp);
      if (f != TXV_NONE) last1 = max(last1, f + 1u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      bytes += (uint64_t)__shfl_xor((long long)bytes, o, 64);
      last1 = max(last1, (uint32_t)__shfl_xor((int)last1, o, 64));
    }
    if (lane == 0 && last1 != 0 && last1 - 1u < b.n) {
      k.tag[last1 - 1u] = ((uint64_t)b.stamp << 32) | s;
      k.rlen[last1 - 1u] = 2ull * (2u + 2u * hl) + 2ull * hash_field_len(hl) + 34u + bytes;
    }
  }
}

__global__ void __launch_bounds__(256) txv_k_st_count(FlowBatch b, StoreSink k) {
  const uint32_t base = blockIdx.x * kStItems + 4u * threadIdx.x;
  uint64_t bytes = 0, recs = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint64_t x = st_value(k, base + q, b.n, b.stamp);
    bytes += x;
    recs += x ? 1u : 0u;
  }
  uint64_t tb, tr;
  (void)block_excl_scan64(bytes, &tb);
  (void)block_excl_scan64(recs, &tr);
  if (threadIdx.x == 0) {
    k.blk[2 * (size_t)blockIdx.x] = tr;
    k.blk[2 * (size_t)blockIdx.x + 1] = tb;
  }
}

// exclusive scan over the arrival indices, as txv_k_upd_apply (each block sums the block counts
// before its own): record r of the batch, its set id and byte offset; foff[records] = the bytes the
// batch needs, blk[2 nb ..] = (records, bytes).  n == 0: one block, which only writes those.
__global__ void __launch_bounds__(256) txv_k_st_apply(FlowBatch b, StoreSink k, uint32_t nb) {
  uint64_t pr = 0, pb = 0;
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256) {
    pr += k.blk[2 * (size_t)j];
    pb += k.blk[2 * (size_t)j + 1];
  }
  uint64_t before_r, before_b;
  (void)block_excl_scan64(pr, &before_r);
  (void)block_excl_scan64(pb, &before_b);
  const uint32_t base = blockIdx.x * kStItems + 4u * threadIdx.x;
  uint64_t x[4], bytes = 0, recs = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    x[q] = st_value(k, base + q, b.n, b.stamp);
    bytes += x[q];
    recs += x[q] ? 1u : 0u;
  }
  uint64_t tot_r, tot_b;
  uint64_t run_r = before_r + block_excl_scan64(recs, &tot_r);
  uint64_t run_b = before_b + block_excl_scan64(bytes, &tot_b);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (x[q]) {                                  // run_r < fired sets <= n
      k.fired[run_r] = (uint32_t)k.tag[base + q];
      k.foff[run_r] = run_b;
      ++run_r;
      run_b += x[q];
    }
  }
  if (blockIdx.x + 1 == gridDim.x && threadIdx.x == 0) {
    k.blk[2 * (size_t)nb] = before_r + tot_r;    // (no block reads index nb)
    k.blk[2 * (size_t)nb + 1] = before_b + tot_b;
    k.foff[before_r + tot_r] = before_b + tot_b;
  }
}

// what the emit kernel knows of the record it assembles
struct RecCtx {
  const uint8_t* key;      // TxHash bytes
  const uint32_t* txkey;   // the set's TxKey (8 words)
  uint32_t hl, l0, hf;     // TxHash length; "H:%X" length; [0x0a uvarint(hl) TxHash] length
};

__device__ __forceinline__ uint8_t hex_key_byte(const RecCtx& R, uint8_t tag, uint32_t x) {
  if (x == 0) return tag;
  if (x == 1) return (uint8_t)':';
  const uint32_t nib = (R.key[(x - 2u) >> 1] >> ((x & 1u) ? 0 : 4)) & 15u;
  return (uint8_t)(nib < 10 ? '0' + nib : 'A' + nib - 10);
}
__device__ __forceinline__ uint8_t hash_field_byte(const RecCtx& R, uint32_t x) {
  if (x == 0) return 0x0a;
  const uint32_t ul = uv_len(R.hl);
  if (x <= ul) return (uint8_t)(((R.hl >> (7u * (x - 1u))) & 0x7fu) | (x < ul ? 0x80u : 0u));
  return R.key[x - 1u - ul];
}
// byte x of the record's fixed front: the two keys, the TxVoteSet bytes and the Commit's TxHash field
__device__ __forceinline__ uint8_t head_byte(const RecCtx& R, uint32_t x) {
  if (x < R.l0) return hex_key_byte(R, (uint8_t)'H', x);
  x -= R.l0;
  if (x < R.hf) return hash_field_byte(R, x);
  x -= R.hf;
  if (x < 34u) return x == 0 ? 0x12 : x == 1 ? 0x20 : (uint8_t)(R.txkey[(x - 2u) >> 2] >> (8u * ((x - 2u) & 3u)));
  x -= 34u;
  if (x < R.l0) return hex_key_byte(R, (uint8_t)'C', x);
  return hash_field_byte(R, x - R.l0);
}

// the LDS tile holding record bytes [t0, t0 + n): stores outside it are dropped
struct Tile {
  uint8_t* p;
  uint32_t t0, n;
  __device__ __forceinline__ void put(uint32_t x, uint32_t byte) const {
    const uint32_t o = x - t0;
    if (o < n) p[o] = (uint8_t)byte;
  }
  __device__ __forceinline__ void put32(uint32_t x, uint32_t w) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) put(x + i, w >> (8 * i));
  }
  __device__ __forceinline__ uint32_t put_uv(uint32_t x, uint64_t v) const {
    uint32_t k = 0;
    for (; v >= 0x80; v >>= 7, ++k) put(x + k, (uint32_t)v | 0x80u);
    put(x + k, (uint32_t)v);
    return k + 1;
  }
};

// Lane q of the 16 that share the CommitSig starting at record byte p_hdr writes its part of it
// into the tile: signature word q, TxKey word q & 7, address word min(q, 4) (sw, tw, aw: gathered
// by the caller), the tags and varints (lanes 8 - 10) and every 16th TxHash byte.
__device__ __forceinline__ void put_commit_sig(const Tile& tl, const RecCtx& R, uint32_t p_hdr, uint32_t q, int64_t height,
                                               int64_t sec, int32_t nanos, uint32_t sw, uint32_t tw, uint32_t aw) {
  const uint32_t sz = (uint32_t)txv_host::txvote_size(height, R.hl, sec, nanos, 20, 64);
  const int tlen = txv_host::time_body(nullptr, sec, nanos);              // 0 .. 17: one length byte
  const uint32_t p_h = p_hdr + 1u + uv_len(sz);
  const uint32_t p_th = p_h + (height != 0 ? 1u + uv_len((uint64_t)height) : 0u);
  const uint32_t p_tk = p_th + R.hf;
  const uint32_t p_tm = p_tk + 34u;
  const uint32_t p_ad = p_tm + (tlen > 0 ? 2u + (uint32_t)tlen : 0u);
  const uint32_t p_sg = p_ad + 22u;
  tl.put32(p_sg + 2u + 4u * q, sw);
  if (q < 8) tl.put32(p_tk + 2u + 4u * q, tw);
  if (q < 5) tl.put32(p_ad + 2u + 4u * q, aw);
  if (q == 8) {
    tl.put(p_hdr, 0x12);
    tl.put_uv(p_hdr + 1u, sz);
    if (height != 0) { tl.put(p_h, 0x08); tl.put_uv(p_h + 1u, (uint64_t)height); }
  } else if (q == 9) {
    if (R.hl) { tl.put(p_th, 0x12); tl.put_uv(p_th + 1u, R.hl); }
    tl.put(p_tk, 0x1a); tl.put(p_tk + 1u, 0x20);
    tl.put(p_ad, 0x2a); tl.put(p_ad + 1u, 0x14);
    tl.put(p_sg, 0x32); tl.put(p_sg + 1u, 0x40);
  } else if (q == 10 && tlen > 0) {
    tl.put(p_tm, 0x22); tl.put(p_tm + 1u, (uint32_t)tlen);
    uint32_t p = p_tm + 2u;
    if (sec != 0) { tl.put(p, 0x08); p += 1u + tl.put_uv(p + 1u, (uint64_t)sec); }
    if (nanos != 0) { tl.put(p, 0x10); tl.put_uv(p + 1u, (uint64_t)(uint32_t)nanos); }
  }
  const uint32_t p_key = p_th + 1u + uv_len(R.hl);
  for (uint32_t i = q; i < R.hl; i += 16) tl.put(p_key + i, R.key[i]);
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
    RecCtx R;
    R.key = fs.keys + (e.key_off - 1);
    R.txkey = fs.set_txkey + (size_t)s * 8;
    R.hl = e.len;
    R.l0 = 2u + 2u * R.hl;
    R.hf = hash_field_len(R.hl);
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
    const uint32_t s3 = 2u * R.l0 + 2u * R.hf + 34u;          // the CommitSigs start here
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
        // the CommitSigs that cover the tile: the largest v with l_off[v] <= y (validators without a
        // vote, and the entries past the registry, start where the next CommitSig does)
        uint32_t vb[2];
        const uint32_t yb[2] = {max(t0, s3) - s3, min(t1, len) - 1u - s3};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint32_t lo = 0, hi = Cap;
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (l_off[mid] <= yb[h]) lo = mid; else hi = mid;
          }
          vb[h] = lo;
        }
        const uint32_t q = t & 15u;
        for (uint32_t v = vb[0] + (t >> 4); v <= vb[1]; v += T / 16) {
          const uint32_t a = l_acc[v];
          if (!a) continue;
          const size_t r = a - 1u;
          // this lane's gathers, independent of each other
          const int64_t height = fs.arena_height[r], sec = fs.arena_sec[r];
          const int32_t nanos = fs.arena_nanos[r];
          const uint32_t sw = fs.arena_sig[(size_t)q * M + r];
          const uint32_t tw = fs.arena_txkey[(size_t)(q & 7u) * M + r];
          const uint32_t aw = fs.val_addr[(size_t)v * 5 + min(q, 4u)];
          put_commit_sig(tl, R, s3 + l_off[v], q, height, sec, nanos, sw, tw, aw);
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
  const uint32_t nb = (b->n + kStItems - 1) / kStItems;
  if (nb > 8192) return hipErrorInvalidValue;
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
