// emu_store.hip — TEST-ONLY host emulation of the store sink's encoder (go-txflow_amd/csrc/store_dev.h).
//
// Compiles the very same __host__ __device__ record front, CommitSig lookup and per-lane CommitSig
// writer that kernels_store.hip runs, and drives them the way txv_k_st_emit does: the CommitSig
// offsets scanned over the validators, then the record tile by tile -- head_byte for the fixed
// front, 16 lanes per CommitSig that covers the tile, the pad zeros --, every tile starting as
// garbage so that a byte nothing writes shows.  It is not linked into libtxvote.so and the product
// never calls it.
#include "../../go-txflow_amd/csrc/store_dev.h"
#include <cstring>
#include <vector>

using namespace txv_store;

constexpr uint32_t kCap = 128;   // validators of a registry (txv_k_st_emit<64, 128, ...>'s Cap)

// One record of a set with TxHash th[hl] and TxKey set_txkey[32] over n_vals <= kCap validators;
// validator v has an accepted vote iff present[v], with height[v], sec[v], nanos[v] and the rows
// sig[v][64], txkey[v][32], addr[v][20].  out receives the record and its zero padding up to the
// next multiple of 16; lens = the four parts' lengths.  Returns the padded length, -1: bad shape or
// out_cap too small.
extern "C" int64_t emu_store_record(const uint8_t* th, uint32_t hl, const uint8_t* set_txkey, uint32_t n_vals,
                                    const uint8_t* present, const int64_t* height, const int64_t* sec, const int32_t* nanos,
                                    const uint8_t* sig, const uint8_t* txkey, const uint8_t* addr, uint32_t tile_bytes,
                                    uint8_t* out, uint32_t out_cap, uint32_t* lens) {
  if (n_vals > kCap || tile_bytes % 16 || !tile_bytes) return -1;
  alignas(4) uint8_t sk[32];
  memcpy(sk, set_txkey, 32);
  const RecCtx R = rec_ctx(th, hl, reinterpret_cast<const uint32_t*>(sk));
  // CommitSig v starts at l_off[v] of the Commit's list; l_acc[v]: its row + 1, 0 without a vote
  uint32_t l_off[kCap], l_acc[kCap], run = 0;
  for (uint32_t v = 0; v < kCap; ++v) {
    l_acc[v] = v < n_vals && present[v] ? v + 1u : 0u;
    l_off[v] = run;
    if (l_acc[v]) run += csig_len(height[v], hl, sec[v], nanos[v]);
  }
  const uint32_t s3 = head_len(R), len = s3 + run, len16 = (len + 15u) & ~15u;
  lens[0] = R.l0; lens[1] = R.hf + 34u; lens[2] = R.l0; lens[3] = R.hf + run;
  if (len16 > out_cap) return -1;
  std::vector<uint8_t> tile(tile_bytes);
  for (uint32_t t0 = 0; t0 < len16; t0 += tile_bytes) {
    const uint32_t t1 = t0 + tile_bytes < len16 ? t0 + tile_bytes : len16;
    memset(tile.data(), 0xCD, tile_bytes);
    const Tile tl{tile.data(), t0, t1 - t0};
    for (uint32_t x = t0; x < (s3 < t1 ? s3 : t1); ++x) tile[x - t0] = head_byte(R, x);
    for (uint32_t x = t0 > len ? t0 : len; x < t1; ++x) tile[x - t0] = 0;
    if (t1 > s3 && t0 < len) {
      const uint32_t v0 = csig_at(l_off, kCap, (t0 > s3 ? t0 : s3) - s3);
      const uint32_t v1 = csig_at(l_off, kCap, (t1 < len ? t1 : len) - 1u - s3);
      for (uint32_t v = v0; v <= v1; ++v) {
        if (!l_acc[v]) continue;
        const size_t r = l_acc[v] - 1u;
        alignas(4) uint8_t s[64], k[32], a[20];
        memcpy(s, sig + r * 64, 64);
        memcpy(k, txkey + r * 32, 32);
        memcpy(a, addr + r * 20, 20);
        for (uint32_t q = 0; q < kLanes; ++q)
          put_commit_sig(tl, R, s3 + l_off[v], q, height[r], sec[r], nanos[r], lane_words(q, s, k, a));
      }
    }
    memcpy(out + t0, tile.data(), t1 - t0);
  }
  return len16;
}
