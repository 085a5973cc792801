// txvote_lanes.h — one TxVote bare body written by 16 lanes into a byte tile: what the gossip
// sink's messages (gossip_dev.h) and the store sink's CommitSigs (store_dev.h) share, written so
// that the host compiles it too (tests/cpu_emu/emu_gossip.hip, emu_store.hip).
//
// The body is cdc.MarshalBinaryBare(TxVote) (amino.hpp: txvote_body): Height 0x08 varint, TxHash
// 0x12, TxKey 0x1a 0x20 + 32 bytes, Timestamp 0x22, ValidatorAddress 0x2a, Signature 0x32; empty
// fields omitted.
#pragma once
#include <stdint.h>

#include "amino.hpp"

namespace txv_lanes {

constexpr uint32_t kLanes = 16;     // lanes that share one TxVote

TXV_AHD uint32_t uv_len(uint64_t v) { return txv_host::put_uvarint(nullptr, v); }

// the tile holding bytes [t0, t0 + n) of a message or record: stores outside it are dropped
struct Tile {
  uint8_t* p;
  uint32_t t0, n;
  TXV_AHD void put(uint32_t x, uint32_t byte) const {
    const uint32_t o = x - t0;
    if (o < n) p[o] = (uint8_t)byte;
  }
  // the first `nb` (<= 4) bytes of the little-endian word w
  TXV_AHD void put_word(uint32_t x, uint32_t w, uint32_t nb) const {
    for (uint32_t i = 0; i < 4; ++i)
      if (i < nb) put(x + i, w >> (8 * i));
  }
  TXV_AHD uint32_t put_uv(uint32_t x, uint64_t v) const {
    uint32_t k = 0;
#pragma clang loop unroll(disable)
    for (; v >= 0x80; v >>= 7, ++k) put(x + k, (uint32_t)v | 0x80u);
    put(x + k, (uint32_t)v);
    return k + 1;
  }
};

// the words lane q gathers for its vote before it writes (independent loads): signature word q,
// TxKey word q & 7, address word min(q, 4)
struct LaneWords { uint32_t sw, tw, aw; };
// ... out of 4-byte aligned rows of 64 / 32 / 20 bytes (TxKey word zero without a TxKey row)
TXV_AHD LaneWords lane_words(uint32_t q, const uint8_t* sig, const uint8_t* txkey, const uint8_t* addr) {
  LaneWords w;
  w.sw = reinterpret_cast<const uint32_t*>(sig)[q];
  w.tw = txkey ? reinterpret_cast<const uint32_t*>(txkey)[q & 7u] : 0u;
  w.aw = reinterpret_cast<const uint32_t*>(addr)[q < 4u ? q : 4u];
  return w;
}

// where the fields of one body start, as byte offsets from its first byte (the Height field's, when
// there is one), for al <= 20 and sl <= 64: one-byte length prefixes
struct VoteLayout {
  uint32_t p_th, p_key, p_tk, p_tm, p_ad, p_sg;   // TxHash field, TxHash bytes, TxKey, Timestamp, address, signature
  uint32_t tlen;                                  // time body length (0: no Timestamp field)
  uint32_t size;                                  // the whole body (= txvote_size)
};
// f_h: the Height field's bytes (0 or 1 + uvarint), tl: the time body's
TXV_AHD VoteLayout vote_layout(uint32_t f_h, uint32_t hl, uint32_t tl, uint32_t al, uint32_t sl) {
  VoteLayout L;
  L.tlen = tl;
  L.p_th = f_h;
  L.p_key = L.p_th + (hl ? 1u + uv_len(hl) : 0u);
  L.p_tk = L.p_key + hl;
  L.p_tm = L.p_tk + 34u;
  L.p_ad = L.p_tm + (tl ? 2u + tl : 0u);
  L.p_sg = L.p_ad + (al ? 2u + al : 0u);
  L.size = L.p_sg + (sl ? 2u + sl : 0u);
  return L;
}

// Lane q of the kLanes that share the body starting at byte `base` writes its part of it into the
// tile: its signature word, TxKey word (lanes 0 - 7), address word (lanes 0 - 4), the tags and
// varints (lanes 8 - 10) and every 16th TxHash byte of the tile's range.
TXV_AHD void put_vote(const Tile& tl, uint32_t base, const VoteLayout& L, uint32_t q, int64_t height, int64_t sec,
                      int32_t nanos, const uint8_t* th, uint32_t hl, uint32_t al, uint32_t sl, const LaneWords& w) {
  const uint32_t p_th = base + L.p_th, p_tk = base + L.p_tk, p_tm = base + L.p_tm, p_ad = base + L.p_ad, p_sg = base + L.p_sg;
  if (4u * q < sl) tl.put_word(p_sg + 2u + 4u * q, w.sw, sl - 4u * q);
  if (q < 8) tl.put_word(p_tk + 2u + 4u * q, w.tw, 4);
  if (q < 5 && 4u * q < al) tl.put_word(p_ad + 2u + 4u * q, w.aw, al - 4u * q);
  if (q == 8) {
    if (height != 0) { tl.put(base, 0x08); tl.put_uv(base + 1u, (uint64_t)height); }
  } else if (q == 9) {
    if (hl) { tl.put(p_th, 0x12); tl.put_uv(p_th + 1u, hl); }
    tl.put(p_tk, 0x1a); tl.put(p_tk + 1u, 0x20);
    if (al) { tl.put(p_ad, 0x2a); tl.put(p_ad + 1u, al); }
    if (sl) { tl.put(p_sg, 0x32); tl.put(p_sg + 1u, sl); }
  } else if (q == 10 && L.tlen > 0) {
    tl.put(p_tm, 0x22); tl.put(p_tm + 1u, L.tlen);
    uint32_t p = p_tm + 2u;
    if (sec != 0) { tl.put(p, 0x08); p += 1u + tl.put_uv(p + 1u, (uint64_t)sec); }
    if (nanos != 0) { tl.put(p, 0x10); tl.put_uv(p + 1u, (uint64_t)(uint32_t)nanos); }
  }
  // the TxHash bytes that fall into the tile
  const uint32_t p_key = base + L.p_key, t1 = tl.t0 + tl.n;
  const uint32_t lo = tl.t0 > p_key ? tl.t0 - p_key : 0u;
  const uint32_t hi = t1 > p_key ? (t1 - p_key < hl ? t1 - p_key : hl) : 0u;
#pragma clang loop unroll_count(4)
  for (uint32_t i = lo + q; i < hi; i += kLanes) tl.put(p_key + i, th[i]);
}

}  // namespace txv_lanes
