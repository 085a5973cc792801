// gossip_dev.h — the TxVoteMessage encoder of the gossip sink (kernels_gossip.hip), written so
// that the host compiles it too (tests/cpu_emu/emu_gossip.hip): the length / flag rule of one batch
// entry, and the share of a message's bytes that lane q of the 16 lanes of a message writes.
//
// cdc.MustMarshalBinaryBare(&TxVoteMessage{Tx}) (txvotepool/reactor.go:247-248), the bytes of
// txv_host::txvote_msg (amino.hpp): 4 prefix bytes | 0x0a uvarint(body) | the TxVote bare body
// (Height 0x08 varint, TxHash 0x12, TxKey 0x1a 0x20 + 32 bytes, Timestamp 0x22, ValidatorAddress
// 0x2a, Signature 0x32; empty fields omitted).
#pragma once
#include <stdint.h>

#include "amino.hpp"

#ifndef TXV_GOSSIP_OK               // (include/txvote.h)
#define TXV_GOSSIP_OK 0
#define TXV_GOSSIP_HOST 1           // sig_len > 64 or addr_len > 20: the columns hold only the first bytes
#define TXV_GOSSIP_UNENCODABLE 2    // amino rejects the time (MustMarshalBinaryBare panics)
#endif

namespace txv_gossip {

constexpr uint32_t kLanes = 16;     // lanes that share one message

// where the fields of one encodable message (flag TXV_GOSSIP_OK: every length fits 32 bits) start,
// as byte offsets from the message's first byte
struct MsgLayout {
  uint32_t body;                    // TxVote bare body length (= txvote_size)
  uint32_t len;                     // whole message
  uint32_t p_h, p_th, p_key, p_tk, p_tm, p_ad, p_sg;   // Height, TxHash field, TxHash bytes, TxKey, Timestamp, address, signature
  uint32_t tlen;                    // time body length (0: no Timestamp field)
};

// The length pass measures a non-nil batch entry once: its flag, the bytes its message takes in
// the sink (0 when flagged) and, for the emit kernel, the field lengths the layout follows from,
// packed into one word: TxHash length | uvarint(body) bytes << 32 | Height field bytes << 35 |
// time body bytes << 39 | addr_len << 44 | sig_len << 49.  A message of 4 GiB or more (lengths are
// 32 bits) is left to the host encoder, as a signature above 64 or an address above 20 bytes is.
TXV_AHD uint32_t msg_measure(int64_t height, uint32_t hl, int64_t sec, int32_t nanos, uint32_t al, uint32_t sl,
                             uint32_t* len, uint64_t* lay) {
  *len = 0;
  *lay = 0;
  const int tlen = txv_host::time_body(nullptr, sec, nanos);
  if (tlen < 0) return TXV_GOSSIP_UNENCODABLE;
  const uint32_t tl = (uint32_t)tlen;                      // at most 17 bytes
  const uint32_t f_h = height != 0 ? 1u + txv_host::put_uvarint(nullptr, (uint64_t)height) : 0u;
  const uint64_t f_th = hl ? 1ull + txv_host::put_uvarint(nullptr, hl) + hl : 0ull;
  const uint64_t f_ad = al ? 1ull + txv_host::put_uvarint(nullptr, al) + al : 0ull;
  const uint64_t f_sg = sl ? 1ull + txv_host::put_uvarint(nullptr, sl) + sl : 0ull;
  const uint64_t body = f_h + f_th + 34u + (tl ? 2u + tl : 0u) + f_ad + f_sg;
  const uint32_t ub = txv_host::put_uvarint(nullptr, body);
  const uint64_t total = 5ull + ub + body;
  if (sl > 64 || al > 20 || total > 0xFFFFFFF0ull) return TXV_GOSSIP_HOST;
  *len = (uint32_t)total;
  *lay = (uint64_t)hl | (uint64_t)ub << 32 | (uint64_t)f_h << 35 | (uint64_t)tl << 39 | (uint64_t)al << 44 |
         (uint64_t)sl << 49;
  return TXV_GOSSIP_OK;
}

// the layout of an encodable message from msg_measure's word and length (al <= 20 and sl <= 64:
// one-byte length prefixes)
TXV_AHD MsgLayout msg_layout(uint64_t lay, uint32_t len, uint32_t* hl_out, uint32_t* al_out, uint32_t* sl_out) {
  const uint32_t hl = (uint32_t)lay, w = (uint32_t)(lay >> 32);
  const uint32_t ub = w & 7u, f_h = (w >> 3) & 15u, tl = (w >> 7) & 31u, al = (w >> 12) & 31u, sl = (w >> 17) & 127u;
  uint32_t uh = 0;                                         // uvarint(hl) bytes
  for (uint32_t v = hl; v; v >>= 7) ++uh;
  MsgLayout L;
  L.len = len;
  L.body = len - 5u - ub;
  L.tlen = tl;
  L.p_h = 5u + ub;
  L.p_th = L.p_h + f_h;
  L.p_key = L.p_th + (hl ? 1u + uh : 0u);
  L.p_tk = L.p_key + hl;
  L.p_tm = L.p_tk + 34u;
  L.p_ad = L.p_tm + (tl ? 2u + tl : 0u);
  L.p_sg = L.p_ad + (al ? 2u + al : 0u);
  *hl_out = hl; *al_out = al; *sl_out = sl;
  return L;
}

// the tile holding message bytes [t0, t0 + n): stores outside it are dropped
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

// the words lane q gathers for its message before it writes (independent loads): signature word q,
// TxKey word q & 7 (zero without a TxKey column), address word min(q, 4).  The columns are 4-byte
// aligned rows of 64 / 32 / 20 bytes.
struct LaneWords { uint32_t sw, tw, aw; };
TXV_AHD LaneWords lane_words(uint32_t q, const uint8_t* sig, const uint8_t* txkey, const uint8_t* addr) {
  LaneWords w;
  w.sw = reinterpret_cast<const uint32_t*>(sig)[q];
  w.tw = txkey ? reinterpret_cast<const uint32_t*>(txkey)[q & 7u] : 0u;
  w.aw = reinterpret_cast<const uint32_t*>(addr)[q < 4u ? q : 4u];
  return w;
}

// Lane q of the kLanes that share a message (flag TXV_GOSSIP_OK, layout L, len16 = its length
// rounded up to 16) writes its part of the bytes into the tile: its signature word, TxKey word
// (lanes 0 - 7), address word (lanes 0 - 4), the prefix, tags and varints (lanes 8 - 10), every
// 16th TxHash byte of the tile's range, and one byte of the zero padding.
TXV_AHD void put_msg(const Tile& tl, const MsgLayout& L, uint32_t q, uint32_t prefix, int64_t height, int64_t sec,
                     int32_t nanos, const uint8_t* th, uint32_t hl, uint32_t al, uint32_t sl, const LaneWords& w) {
  const uint32_t len = L.len;
  if (4u * q < sl) tl.put_word(L.p_sg + 2u + 4u * q, w.sw, sl - 4u * q);
  if (q < 8) tl.put_word(L.p_tk + 2u + 4u * q, w.tw, 4);
  if (q < 5 && 4u * q < al) tl.put_word(L.p_ad + 2u + 4u * q, w.aw, al - 4u * q);
  if (q == 8) {
    tl.put_word(0, prefix, 4);
    tl.put(4, 0x0a);
    tl.put_uv(5, L.body);
    if (height != 0) { tl.put(L.p_h, 0x08); tl.put_uv(L.p_h + 1u, (uint64_t)height); }
  } else if (q == 9) {
    if (hl) { tl.put(L.p_th, 0x12); tl.put_uv(L.p_th + 1u, hl); }
    tl.put(L.p_tk, 0x1a); tl.put(L.p_tk + 1u, 0x20);
    if (al) { tl.put(L.p_ad, 0x2a); tl.put(L.p_ad + 1u, al); }
    if (sl) { tl.put(L.p_sg, 0x32); tl.put(L.p_sg + 1u, sl); }
  } else if (q == 10 && L.tlen > 0) {
    tl.put(L.p_tm, 0x22); tl.put(L.p_tm + 1u, L.tlen);
    uint32_t p = L.p_tm + 2u;
    if (sec != 0) { tl.put(p, 0x08); p += 1u + tl.put_uv(p + 1u, (uint64_t)sec); }
    if (nanos != 0) { tl.put(p, 0x10); tl.put_uv(p + 1u, (uint64_t)(uint32_t)nanos); }
  }
  // the TxHash bytes that fall into the tile
  const uint32_t t1 = tl.t0 + tl.n;
  const uint32_t lo = tl.t0 > L.p_key ? tl.t0 - L.p_key : 0u;
  const uint32_t hi = t1 > L.p_key ? (t1 - L.p_key < hl ? t1 - L.p_key : hl) : 0u;
#pragma clang loop unroll_count(4)
  for (uint32_t i = lo + q; i < hi; i += kLanes) tl.put(L.p_key + i, th[i]);
  tl.put(len + q, 0);               // pad: fewer than 16 bytes, and the tile ends at len16 at the latest
}

}  // namespace txv_gossip
