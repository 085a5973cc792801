// emu_gossip.hip — TEST-ONLY host emulation of the gossip sink's encoder (go-txflow_amd/csrc/gossip_dev.h).
//
// Compiles the very same __host__ __device__ length / flag rule and per-lane field encoder that
// kernels_gossip.hip runs, and drives them the way txv_k_gs_emit does: 16 lanes per message, tile by
// tile, every tile starting as garbage so that a byte no lane writes shows.  It is not linked into
// libtxvote.so and the product never calls it.
#include "../../go-txflow_amd/csrc/gossip_dev.h"
#include <cstring>
#include <vector>

using namespace txv_gossip;

// One batch entry through the device rule and encoder.  addr / sig / txkey are the columns' rows
// (20 / 64 / 32 bytes, the first bytes of longer fields; txkey may be null).  Returns the flag;
// *len_out = the message length (0 when flagged); out receives the message and its zero padding up
// to the next multiple of 16 (out_cap >= that).  -1: out_cap too small.
extern "C" int emu_gossip_encode(int64_t height, const uint8_t* th, uint32_t hl, int64_t sec, int32_t nanos,
                                 const uint8_t* addr, uint32_t al, const uint8_t* sig, uint32_t sl, const uint8_t* txkey,
                                 uint32_t prefix, uint32_t tile_bytes, uint8_t* out, uint32_t out_cap, uint32_t* len_out) {
  uint32_t len = 0;
  uint64_t lay = 0;
  const uint32_t flag = msg_measure(height, hl, sec, nanos, al, sl, &len, &lay);
  *len_out = len;
  if (flag != TXV_GOSSIP_OK) return (int)flag;
  const uint32_t len16 = (len + 15u) & ~15u;
  if (len16 > out_cap || tile_bytes % 16 || !tile_bytes) return -1;
  alignas(16) uint8_t a[20], s[64], k[32];
  memcpy(a, addr, 20);
  memcpy(s, sig, 64);
  if (txkey) memcpy(k, txkey, 32);
  uint32_t hl2, al2, sl2;                          // the emit kernel knows the lengths from the packed word only
  const MsgLayout L = msg_layout(lay, len, &hl2, &al2, &sl2);
  if (hl2 != hl || al2 != al || sl2 != sl) return -2;
  std::vector<uint8_t> tile(tile_bytes);
  for (uint32_t t0 = 0; t0 < len16; t0 += tile_bytes) {
    const uint32_t t1 = t0 + tile_bytes < len16 ? t0 + tile_bytes : len16;
    memset(tile.data(), 0xCD, tile_bytes);
    const Tile tl{tile.data(), t0, t1 - t0};
    for (uint32_t q = 0; q < kLanes; ++q) {
      const LaneWords w = lane_words(q, s, txkey ? k : nullptr, a);
      put_msg(tl, L, q, prefix, height, sec, nanos, th, hl2, al2, sl2, w);
    }
    memcpy(out + t0, tile.data(), t1 - t0);
  }
  return (int)flag;
}
