// kernels_gossip.hip — the gossip sink: a batch's TxVoteMessages, amino-encoded in HBM.
//
// Reference: broadcastTxRoutine (txvotepool/reactor.go:198-265) walks the pool list in order and
// sends cdc.MustMarshalBinaryBare(&TxVoteMessage{Tx}) (:247-248) for every entry to every peer but
// the one that sent the vote (:245).  The pool list is the admitted votes in arrival order, so a
// batch's messages are those of its non-nil entries in arrival order (for txv_submit_checked the
// nil column is the pool's decisions: exactly the admitted votes).
//
// A message sits at a 16-byte aligned offset of the sink, zero padded to the next one; its bytes
// are those of txv_host::txvote_msg (amino.hpp; the device encoder is gossip_dev.h).
//
// The chain reads only the slot's raw columns (height, ts_sec, ts_nanos, th_off, th_len, th, addr,
// addr_len, sig_raw, sig_len, nil, txkey) and no TxFlow state; every producer -> consumer pair is a
// launch apart (len and apply are arrival_list.h's scan):
//   len     one lane per entry: flag, message length and the packed field lengths the layout
//           follows from (nil: not listed), and per 1024 arrival indices the listed entries and
//           their bytes, each rounded up to 16
//   apply   exclusive scan over the indices: entry k of the batch gets its descriptor (offset,
//           length, arrival index, flag); the result words (entries, overflow, bytes needed)
//   emit    16 lanes per message, four messages per wave: the lanes gather their words of the
//           columns independently, assemble the message in an LDS tile (field boundaries are
//           byte-granular) and the tile leaves as aligned 16-byte stores, pad zeros included.  A
//           message longer than a tile loops over tiles; one that would end past the sink's bytes
//           or entries is not written at all.
#include <algorithm>

#include "arrival_list.h"
#include "gossip_dev.h"

namespace {

constexpr uint32_t kGsTile = 512;      // LDS tile bytes per message
constexpr uint64_t kGsListed = 1ull << 63;

// entry i's scratch word: listed << 63 | flag << 32 | length (0: a nil entry)
// (*lay: the field lengths of an encodable message, gossip_dev.h msg_measure)
__device__ __forceinline__ uint64_t gs_entry(const FlowBatch& b, uint32_t i, uint64_t* lay) {
  *lay = 0;
  if (b.nil && b.nil[i]) return 0;
  uint32_t len;
  const uint32_t flag = txv_gossip::msg_measure(b.height[i], b.th_len[i], b.ts_sec[i], b.ts_nanos[i], b.addr_len[i],
                                                b.sig_len[i], &len, lay);
  return kGsListed | ((uint64_t)flag << 32) | len;
}
// a non-nil entry is listed; its weight: the message length rounded up to 16; its word: the entry's
__device__ __forceinline__ ListValue gs_value(uint64_t e) { return ListValue{(e >> 63) != 0, ((e & 0xFFFFFFFFull) + 15ull) & ~15ull, e}; }

// len: measures every entry on the way
__global__ void __launch_bounds__(256) txv_k_gs_len(FlowBatch b, GossipSink k) {
  list_count(b.n, k.blk, [&](uint32_t i) {
    uint64_t lay;
    const uint64_t e = gs_entry(b, i, &lay);
    k.ent[i] = e;
    k.lay[i] = lay;
    return gs_value(e);
  });
}

// apply: the descriptor of entry r of the batch; the result words
__global__ void __launch_bounds__(256) txv_k_gs_apply(FlowBatch b, GossipSink k, uint32_t nb) {
  uint64_t n_e, n_b;
  const bool last = list_apply(
      b.n, nb, k.blk, [&](uint32_t i) { return gs_value(k.ent[i]); },
      [&](uint32_t i, uint64_t r, uint64_t off, const ListValue& x) {
        if (r >= k.cap_msgs) return;
        const uint64_t e = x.word;
        GossipDesc d;
        d.off_lo = (uint32_t)off | ((uint32_t)(e >> 32) & 15u);
        d.off_hi = (uint32_t)(off >> 32);
        d.len = (uint32_t)e;
        d.idx = i;
        *reinterpret_cast<uint4*>(k.desc + r) = make_uint4(d.off_lo, d.off_hi, d.len, d.idx);
      },
      &n_e, &n_b);
  if (last) {
    uint4* res = reinterpret_cast<uint4*>(k.result);
    res[0] = make_uint4((uint32_t)n_e, (n_e > k.cap_msgs || n_b > k.cap_bytes) ? 1u : 0u, 0u, 0u);
    res[1] = make_uint4((uint32_t)n_b, (uint32_t)(n_b >> 32), 0u, 0u);
  }
}

// One wave per block: lanes 16 g .. 16 g + 15 share message 4 * pass + g.  The loop bounds are
// wave-uniform (the tile count is the largest of the four messages'), so the barriers are too.
// Left alone the compiler takes 130 VGPRs (3 waves per SIMD) to keep every clipped store's address
// and byte in flight; held to 5 waves it needs 96 and still no scratch (6 waves would spill), and
// waves in flight are this kernel's only latency hiding.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) txv_k_gs_emit(FlowBatch b, GossipSink k, uint32_t nb) {
  __shared__ __attribute__((aligned(16))) uint8_t l_tile[4][kGsTile];
  static_assert(kGsTile % 16 == 0, "tile shape");
  const uint32_t g = threadIdx.x >> 4, q = threadIdx.x & 15u;
  const uint32_t n_ent = (uint32_t)min(k.blk[2 * (size_t)nb], (uint64_t)k.cap_msgs);
  for (uint32_t base = blockIdx.x * 4u; base < n_ent; base += gridDim.x * 4u) {
    const uint32_t j = base + g;
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    if (j < n_ent) d = *reinterpret_cast<const uint4*>(k.desc + j);
    const uint64_t start = ((uint64_t)d.y << 32) | (d.x & ~15u);
    const uint32_t len = d.z, i = d.w;
    uint32_t len16 = (len + 15u) & ~15u;          // 0: flagged, or no message for this group
    if (start + len16 > k.cap_bytes) len16 = 0;   // the messages that fit are a prefix
    uint32_t ntiles = (len16 + kGsTile - 1) / kGsTile;
    ntiles = max(ntiles, (uint32_t)__shfl_xor((int)ntiles, 16, 64));
    ntiles = max(ntiles, (uint32_t)__shfl_xor((int)ntiles, 32, 64));
    int64_t height = 0, sec = 0;
    int32_t nanos = 0;
    uint64_t lay = 0;
    const uint8_t* th = b.th;
    txv_gossip::LaneWords w{0u, 0u, 0u};
    if (len16) {                                   // this lane's gathers, independent of each other
      lay = k.lay[i];                              // the field lengths, measured by the length pass
      height = b.height[i]; sec = b.ts_sec[i]; nanos = b.ts_nanos[i];
      th = b.th + b.th_off[i];
      w = txv_gossip::lane_words(q, b.sig_raw + (size_t)i * 64, b.txkey ? b.txkey + (size_t)i * 32 : nullptr,
                                 b.addr + (size_t)i * 20);
    }
    uint32_t hl, al, sl;
    const txv_gossip::MsgLayout L = txv_gossip::msg_layout(lay, len, &hl, &al, &sl);
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
      const uint32_t t0 = tile * kGsTile;
      const bool mine = t0 < len16;
      const uint32_t t1 = mine ? min(t0 + kGsTile, len16) : t0;
      if (mine) {
        const txv_gossip::Tile tl{l_tile[g], t0, t1 - t0};
        txv_gossip::put_msg(tl, L, q, k.prefix, height, sec, nanos, th, hl, al, sl, w);
      }
      __syncthreads();
      if (mine) {                                  // aligned 16-byte stores (start and t0 are multiples of 16)
        uint4* dst = reinterpret_cast<uint4*>(k.buf + start + t0);
        const uint4* src = reinterpret_cast<const uint4*>(l_tile[g]);
        for (uint32_t c = q; c < (t1 - t0) / 16u; c += txv_gossip::kLanes) dst[c] = src[c];
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" hipError_t txv_flow_gossip_msgs(const FlowBatch* b, GossipSink k, hipStream_t st) {
  uint32_t nb;
  if (!list_blocks(b->n, &nb)) return hipErrorInvalidValue;
  if (b->n) hipLaunchKernelGGL(txv_k_gs_len, dim3(nb), dim3(256), 0, st, *b, k);
  hipLaunchKernelGGL(txv_k_gs_apply, dim3(nb ? nb : 1u), dim3(256), 0, st, *b, k, nb);
  // (an empty batch: one block, which writes the result words)
  if (b->n) {
    const uint32_t blocks = std::min<uint32_t>((std::min(b->n, k.cap_msgs) + 3u) / 4u, 8192u);
    if (blocks) hipLaunchKernelGGL(txv_k_gs_emit, dim3(blocks), dim3(64), 0, st, *b, k, nb);
  }
  return hipGetLastError();
}
