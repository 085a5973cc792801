// store_dev.h — the SaveTx record encoder of the store sink (kernels_store.hip), written so that
// the host compiles it too (tests/cpu_emu/emu_store.hip): the lengths of a record's parts, byte x
// of its fixed front, and the share of a CommitSig that lane q of its 16 lanes writes.  The four
// parts of a record: kernels_store.hip's header (amino.hpp: store_key, txvoteset_bytes, commit_bytes).
#pragma once
#include <stdint.h>

#include "txvote_lanes.h"

namespace txv_store {

using txv_lanes::kLanes, txv_lanes::LaneWords, txv_lanes::lane_words, txv_lanes::Tile, txv_lanes::uv_len;

// [tag uvarint(hl) TxHash]: field 1 of TxVoteSet and Commit, field 2 of a TxVote; omitted when empty
TXV_AHD uint32_t hash_field_len(uint32_t hl) { return hl ? 1u + uv_len(hl) + hl : 0u; }
// one CommitSig of a set whose TxHash has hl bytes: 0x12 uvarint(sz) + the TxVote body
TXV_AHD uint32_t csig_len(int64_t height, uint32_t hl, int64_t sec, int32_t nanos) {
  const uint32_t sz = (uint32_t)txv_host::txvote_size(height, hl, sec, nanos, 20, 64);
  return 1u + uv_len(sz) + sz;
}

// what the emit kernel knows of the record it assembles
struct RecCtx {
  const uint8_t* key;      // TxHash bytes
  const uint32_t* txkey;   // the set's TxKey (8 words)
  uint32_t hl, l0, hf;     // TxHash length; "H:%X" length; [0x0a uvarint(hl) TxHash] length
};
TXV_AHD RecCtx rec_ctx(const uint8_t* key, uint32_t hl, const uint32_t* txkey) {
  return RecCtx{key, txkey, hl, 2u + 2u * hl, hash_field_len(hl)};
}
// the fixed front's length: the CommitSigs start here
TXV_AHD uint32_t head_len(const RecCtx& R) { return 2u * R.l0 + 2u * R.hf + 34u; }

TXV_AHD uint8_t hex_key_byte(const RecCtx& R, uint8_t tag, uint32_t x) {
  if (x == 0) return tag;
  if (x == 1) return (uint8_t)':';
  const uint32_t nib = (R.key[(x - 2u) >> 1] >> ((x & 1u) ? 0 : 4)) & 15u;
  return (uint8_t)(nib < 10 ? '0' + nib : 'A' + nib - 10);
}
TXV_AHD uint8_t hash_field_byte(const RecCtx& R, uint32_t x) {
  if (x == 0) return 0x0a;
  const uint32_t ul = uv_len(R.hl);
  if (x <= ul) return (uint8_t)(((R.hl >> (7u * (x - 1u))) & 0x7fu) | (x < ul ? 0x80u : 0u));
  return R.key[x - 1u - ul];
}
// byte x of the record's fixed front: the two keys, the TxVoteSet bytes and the Commit's TxHash field
TXV_AHD uint8_t head_byte(const RecCtx& R, uint32_t x) {
  if (x < R.l0) return hex_key_byte(R, (uint8_t)'H', x);
  x -= R.l0;
  if (x < R.hf) return hash_field_byte(R, x);
  x -= R.hf;
  if (x < 34u) return x == 0 ? 0x12 : x == 1 ? 0x20 : (uint8_t)(R.txkey[(x - 2u) >> 2] >> (8u * ((x - 2u) & 3u)));
  x -= 34u;
  if (x < R.l0) return hex_key_byte(R, (uint8_t)'C', x);
  return hash_field_byte(R, x - R.l0);
}

// the CommitSig that covers byte y of the Commit's list: the largest v < cap (a power of two) with
// off[v] <= y, where CommitSig v starts at off[v] (validators without a vote, and the entries past
// the registry, start where the next CommitSig does)
TXV_AHD uint32_t csig_at(const uint32_t* off, uint32_t cap, uint32_t y) {
  uint32_t lo = 0, hi = cap;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= y) lo = mid; else hi = mid;
  }
  return lo;
}

// Lane q of the 16 that share the CommitSig starting at record byte p_hdr writes its part of it
// into the tile: the CommitSig header (lane 8) and its part of the TxVote body (txvote_lanes.h:
// put_vote; w: gathered by the caller)
TXV_AHD void put_commit_sig(const Tile& tl, const RecCtx& R, uint32_t p_hdr, uint32_t q, int64_t height, int64_t sec,
                            int32_t nanos, const LaneWords& w) {
  const uint32_t f_h = height != 0 ? 1u + uv_len((uint64_t)height) : 0u;
  const int tlen = txv_host::time_body(nullptr, sec, nanos);              // 0 .. 17: one length byte
  const txv_lanes::VoteLayout L = txv_lanes::vote_layout(f_h, R.hl, tlen > 0 ? (uint32_t)tlen : 0u, 20, 64);
  if (q == 8) {
    tl.put(p_hdr, 0x12);
    tl.put_uv(p_hdr + 1u, L.size);
  }
  txv_lanes::put_vote(tl, p_hdr + 1u + uv_len(L.size), L, q, height, sec, nanos, R.key, R.hl, 20, 64, w);
}

}  // namespace txv_store
