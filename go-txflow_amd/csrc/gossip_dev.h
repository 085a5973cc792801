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

#include "txvote_lanes.h"

#ifndef TXV_GOSSIP_OK               // (include/txvote.h)
#define TXV_GOSSIP_OK 0
#define TXV_GOSSIP_HOST 1           // sig_len > 64 or addr_len > 20: the columns hold only the first bytes
#define TXV_GOSSIP_UNENCODABLE 2    // amino rejects the time (MustMarshalBinaryBare panics)
#endif

namespace txv_gossip {

using txv_lanes::kLanes, txv_lanes::LaneWords, txv_lanes::lane_words, txv_lanes::Tile, txv_lanes::VoteLayout;

// where the bytes of one encodable message (flag TXV_GOSSIP_OK: every length fits 32 bits) are
struct MsgLayout {
  uint32_t len;                     // whole message
  uint32_t base;                    // the TxVote bare body starts here: behind 4 prefix bytes, 0x0a, uvarint(body)
  VoteLayout v;                     // the body's fields, from there
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
  MsgLayout L;
  L.len = len;
  L.base = 5u + ub;
  L.v = txv_lanes::vote_layout(f_h, hl, tl, al, sl);
  *hl_out = hl; *al_out = al; *sl_out = sl;
  return L;
}

// Lane q of the kLanes that share a message (flag TXV_GOSSIP_OK, layout L, len16 = its length
// rounded up to 16) writes its part of the bytes into the tile: the message header (lane 8), its
// part of the TxVote body (txvote_lanes.h: put_vote) and one byte of the zero padding.
TXV_AHD void put_msg(const Tile& tl, const MsgLayout& L, uint32_t q, uint32_t prefix, int64_t height, int64_t sec,
                     int32_t nanos, const uint8_t* th, uint32_t hl, uint32_t al, uint32_t sl, const LaneWords& w) {
  if (q == 8) {
    tl.put_word(0, prefix, 4);
    tl.put(4, 0x0a);
    tl.put_uv(5, L.v.size);
  }
  txv_lanes::put_vote(tl, L.base, L.v, q, height, sec, nanos, th, hl, al, sl, w);
  tl.put(L.len + q, 0);             // pad: fewer than 16 bytes, and the tile ends at len16 at the latest
}

}  // namespace txv_gossip
