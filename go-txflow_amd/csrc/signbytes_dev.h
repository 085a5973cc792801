// signbytes_dev.h — the challenge hash SHA-512(R || A || SignBytes) of a TxVote straight from its
// field columns: the 128-byte blocks are assembled in registers, so K1a needs no message buffer
// (no txv_k_signbytes launch, no msg[msg_words][n_pad] write and read-back).
//
// The byte layout is kernels_signbytes.hip's (types/tx_vote.go:83-89, 177-192; SURVEY.md
// Appendix B):
//   uvarint(len(body)) || body,  body =
//     [0x09 Height as 8 LE bytes]                       (omitted when Height == 0)
//     [0x12 uvarint(len) TxHash]                        (omitted when empty)
//      0x1a 0x20 + 32 zero bytes
//     [0x22 uvarint(len) [0x08 uvarint(sec)] [0x10 uvarint(nanos)]]   (omitted at the Unix epoch)
//     [0x2a uvarint(len) ChainID]                       (omitted when empty)
//
// The ChainID field is the same for every vote of a context, so the runtime keeps it in HBM once,
// already followed by SHA-512's 0x80 pad byte (the field is the last of the message):
//   chain field = [0x2a uvarint(len) ChainID] 0x80, kChainFieldPad zero bytes before and behind it.
// A lane reads it at its own byte offset, which places it -- and the pad byte -- for free.
//
// Two builders, chosen per wave by the caller (both compile for the host: tests/cpu_emu):
//   fields_blocks_fast<HL>  Height != 0, a TxHash of HL bytes, 2^28 <= sec < 2^35 (the years 1978
//                           to 3058), nanos >= 0, at most two blocks: every byte up to the nanos
//                           sits at a compile-time position of the body; the chain field follows
//                           by address; one per-lane byte shift moves the body behind its 1- or
//                           2-byte length prefix
//   sha512_fields_generic   every other shape: each 64-bit word is gathered from the message's
//                           five segments (header, TxHash, TxKey, time, chain field); slow, rare
// No register array is indexed dynamically (none ends in scratch).
#pragma once
#include "sha2.h"

namespace txv {

constexpr uint32_t kChainFieldPad = 32;   // zero bytes before and behind the chain field in HBM

// one vote's SignBytes fields.  th: readable up to th + hl + 11 (the arena's padding, as for
// txv_k_signbytes); cf / cf_len: the chain field with its 0x80 (cf_len >= 1)
struct VoteFields {
  int64_t height, sec;
  int32_t nanos;
  uint32_t hl;
  const uint8_t* th;
  const uint8_t* cf;
  uint32_t cf_len;
};

TXV_HD uint32_t fields_uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80u) { v >>= 7; ++n; }
  return n;
}

// ({hi, lo} >> 8 s) & 0xffffffff, s in 0..3
TXV_HD uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * s));
#endif
}

// p rounded down to a 4-byte boundary (sh: the bytes dropped).  Pointer arithmetic, no integer
// round trip: the loads stay global loads
TXV_HD const uint32_t* align_down4(const uint8_t* p, uint32_t& sh) {
  sh = (uint32_t)((uintptr_t)p & 3u);
  return reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(p - sh, 4));
}

// N + 1 aligned words from q, each loaded once; then out[j] = bytes [4 j + sh, 4 j + sh + 4) behind q
// as a big-endian word
template <int N>
TXV_HD void be32_run(uint32_t out[N], const uint32_t* q, uint32_t sh) {
  uint32_t t[N + 1];
#pragma unroll
  for (int j = 0; j <= N; ++j) t[j] = q[j];
#pragma unroll
  for (int j = 0; j < N; ++j) out[j] = bswap32(align_bytes(t[j + 1], t[j], sh));
}

// 8 bytes at any address as one big-endian word (reads 12 bytes from p rounded down to 4)
TXV_HD uint64_t be64_at(const uint8_t* p) {
  uint32_t sh, o[2];
  const uint32_t* q = align_down4(p, sh);
  be32_run<2>(o, q, sh);
  return ((uint64_t)o[0] << 32) | o[1];
}

// length of SignBytes (prefix included) and of its body
TXV_HD uint32_t fields_len(const VoteFields& f, uint32_t& body) {
  const uint32_t tl = (f.sec != 0 ? 1u + fields_uvarint_len((uint64_t)f.sec) : 0u) +
                      (f.nanos != 0 ? 1u + fields_uvarint_len((uint64_t)(uint32_t)f.nanos) : 0u);
  body = (f.height != 0 ? 9u : 0u) + (f.hl ? 1u + fields_uvarint_len(f.hl) + f.hl : 0u) + 34u + (tl ? 2u + tl : 0u) +
         (f.cf_len - 1u);
  return fields_uvarint_len(body) + body;
}

// ---------------------------------------------------------------- the fast builder
template <uint32_t HL>
TXV_HD bool fields_fast_ok(const VoteFields& f) {
  static_assert(HL % 4 == 0 && HL >= 32 && HL < 128, "one-byte TxHash length, two blocks");
  // R || A, a 2-byte prefix (any body of this shape that nears the bound has >= 128 bytes), the
  // body: two blocks hold 239 bytes before the pad byte and the length
  const uint32_t v = (uint32_t)f.nanos;
  const uint32_t d = 8u + (v ? 2u + ((v >> 7) ? 1u : 0u) + ((v >> 14) ? 1u : 0u) + ((v >> 21) ? 1u : 0u) + ((v >> 28) ? 1u : 0u) : 0u);
  const uint32_t total = 64u + 2u + 11u + HL + 34u + d + (f.cf_len - 1u);
  return f.height != 0 && f.hl == HL && f.sec >= ((int64_t)1 << 28) && f.sec < ((int64_t)1 << 35) && f.nanos >= 0 &&
         total <= 239u;
}

// w[32]: the two padded blocks of pre[8] || SignBytes.  Returns the hashed length in bytes.
template <uint32_t HL>
TXV_HD uint32_t fields_blocks_fast(uint64_t w[32], const uint64_t pre[8], const VoteFields& f) {
  constexpr int NBD = 46;               // body words (4 bytes each) that can reach the blocks
  constexpr int TB = 11 + (int)HL / 4;  // the word of body byte 44 + HL: TxKey's last zero, then the time field
  uint32_t bd[NBD];
#pragma unroll
  for (int m = 0; m < NBD; ++m) bd[m] = 0;
  // 09 h0 h1 h2 | h3 h4 h5 h6 | h7 12 HL t0
  const uint32_t hlo = bswap32((uint32_t)(uint64_t)f.height), hhi = bswap32((uint32_t)((uint64_t)f.height >> 32));
  bd[0] = 0x09000000u | (hlo >> 8);
  bd[1] = (hlo << 24) | (hhi >> 8);
  bd[2] = (hhi << 24) | 0x00120000u | (HL << 8) | f.th[0];
  {   // TxHash bytes 1.. at body byte 12
    uint32_t sh;
    const uint32_t* q = align_down4(f.th + 1, sh);
    be32_run<(int)HL / 4>(bd + 3, q, sh);
  }
  bd[2 + HL / 4] = (bd[2 + HL / 4] & 0xFFFFFF00u) | 0x1Au;   // the last TxHash bytes, then 1a | 20 + 32 zeros
  bd[3 + HL / 4] = 0x20000000u;
  // 00 22 tl 08 | s0 s1 s2 s3 | s4 [10 n0 n1 | n2 n3 n4] from body byte 44 + HL
  const uint64_t s = (uint64_t)f.sec;
  const uint32_t v = (uint32_t)f.nanos;
  const uint32_t c1 = (v >> 7) ? 1u : 0u, c2 = (v >> 14) ? 1u : 0u, c3 = (v >> 21) ? 1u : 0u, c4 = (v >> 28) ? 1u : 0u;
  const uint32_t tl = 6u + (v ? 2u + c1 + c2 + c3 + c4 : 0u);
  const uint32_t d = 2u + tl;
  bd[TB] = 0x00220008u | (tl << 8);
  bd[TB + 1] = (((uint32_t)s & 0x7Fu) << 24) | (((uint32_t)(s >> 7) & 0x7Fu) << 16) | (((uint32_t)(s >> 14) & 0x7Fu) << 8) |
               ((uint32_t)(s >> 21) & 0x7Fu) | 0x80808080u;
  bd[TB + 2] = (uint32_t)(s >> 28) << 24;
  if (v) {
    bd[TB + 2] |= 0x00100000u | (((v & 0x7Fu) | (c1 << 7)) << 8) | ((v >> 7) & 0x7Fu) | (c2 << 7);
    bd[TB + 3] = ((((v >> 14) & 0x7Fu) | (c3 << 7)) << 24) | ((((v >> 21) & 0x7Fu) | (c4 << 7)) << 16) | ((v >> 28) << 8);
  }
  {   // the chain field and the pad byte from body byte 45 + HL + d: zeros before and behind them
    // (d <= 14: word j can hold field bytes while 4 j < 15 + cf_len; the words are loaded four at a
    // time, each once, as far as the field reaches: the bound is the same for the whole wave)
    constexpr int NCF = NBD - TB;
    uint32_t sh;
    const uint32_t* q = align_down4(f.cf - 1 - d, sh);
    uint32_t t[NCF + 1];
#pragma unroll
    for (int j = 0; j <= NCF; ++j) t[j] = 0;
#pragma unroll
    for (int g = 0; 4 * g <= NCF; ++g)
      if (16u * (uint32_t)g < 19u + f.cf_len) {
#pragma unroll
        for (int j = 4 * g; j < 4 * g + 4 && j <= NCF; ++j) t[j] = q[j];
      }
#pragma unroll
    for (int j = 0; j < NCF; ++j)
      if (4u * (uint32_t)j < 15u + f.cf_len) bd[TB + j] |= bswap32(align_bytes(t[j + 1], t[j], sh));
  }
  const uint32_t body = 11u + HL + 34u + d + (f.cf_len - 1u);
  const uint32_t p = body >= 128u ? 2u : 1u;
  const uint32_t prefix = p == 1u ? body : ((((body & 0x7Fu) | 0x80u) << 8) | (body >> 7));
  // behind the prefix: stream word 16 + m takes the last p bytes of body word m - 1
#pragma unroll
  for (int t = 0; t < 8; ++t) w[t] = pre[t];
#pragma unroll
  for (int u = 0; u < NBD / 2; ++u) {
    // (body words 4 + HL/4 .. 10 + HL/4 are TxKey's zeros: their stream words are constants)
    const bool z0 = 2 * u - 1 >= 4 + (int)HL / 4 && 2 * u <= 10 + (int)HL / 4;
    const bool z1 = 2 * u >= 4 + (int)HL / 4 && 2 * u + 1 <= 10 + (int)HL / 4;
    const uint32_t hi = z0 ? 0u : align_bytes(u ? bd[2 * u - 1] : prefix, bd[2 * u], p);
    const uint32_t lo = z1 ? 0u : align_bytes(bd[2 * u], bd[2 * u + 1], p);
    w[8 + u] = ((uint64_t)hi << 32) | lo;
  }
  const uint32_t total = 64u + p + body;
  w[31] = (uint64_t)total * 8u;
  return total;
}

// ---------------------------------------------------------------- the generic builder
// a byte string of at most 32 bytes, left-aligned big-endian in s[4], zero beyond its end
TXV_HD void seg_put(uint64_t s[4], uint32_t& pos, uint64_t be, uint32_t k) {   // k (1..8) bytes, right-aligned in be
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sh = 64 * (j + 1) - 8 * (int)(pos + k);   // left shift that places be in word j
    if (sh >= 0 && sh < 64) s[j] |= be << sh;
    else if (sh < 0 && sh > -64) s[j] |= be >> (-sh);
  }
  pos += k;
}
TXV_HD void seg_put_uvarint(uint64_t s[4], uint32_t& pos, uint64_t v) {
  while (v >= 0x80u) {
    seg_put(s, pos, (v & 0x7Fu) | 0x80u, 1);
    v >>= 7;
  }
  seg_put(s, pos, v, 1);
}
// the 8 bytes at offset rel (any sign) of such a string, zeros outside it
TXV_HD uint64_t seg_word(const uint64_t s[4], int32_t rel) {
  if (rel <= -8 || rel >= 32) return 0;
  const int32_t q = rel >> 3;          // -1 .. 3
  const uint32_t r = (uint32_t)rel & 7u;
  uint64_t hi = 0, lo = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (q == j) hi = s[j];
    if (q + 1 == j) lo = s[j];
  }
  return r ? (hi << (8u * r)) | (lo >> (64u - 8u * r)) : hi;
}
// the 8 bytes at offset rel of the n bytes at p, zeros outside them
TXV_HD uint64_t mem_word(const uint8_t* p, uint32_t n, int32_t rel) {
  if (rel <= -8 || rel >= (int32_t)n) return 0;
  const uint32_t from = rel > 0 ? (uint32_t)rel : 0u;
  const uint32_t keep = n - from;     // bytes of the string in the loaded word
  uint64_t v = be64_at(p + from);
  if (keep < 8) v &= ~0ull << (8u * (8u - keep));
  return rel < 0 ? v >> (8u * (uint32_t)(-rel)) : v;
}

struct FieldSegs {
  uint64_t head[4], time[4];   // prefix + Height + TxHash tag and length; the time field
  uint32_t head_len, time_len;
  uint32_t len;                // SignBytes length
};

TXV_HD FieldSegs fields_segs(const VoteFields& f) {
  FieldSegs g;
#pragma unroll
  for (int j = 0; j < 4; ++j) g.head[j] = g.time[j] = 0;
  uint32_t body;
  g.len = fields_len(f, body);
  uint32_t pos = 0;
  seg_put_uvarint(g.head, pos, body);
  if (f.height != 0) {
    seg_put(g.head, pos, 0x09, 1);
    seg_put(g.head, pos, ((uint64_t)bswap32((uint32_t)(uint64_t)f.height) << 32) | bswap32((uint32_t)((uint64_t)f.height >> 32)), 8);
  }
  if (f.hl) {
    seg_put(g.head, pos, 0x12, 1);
    seg_put_uvarint(g.head, pos, f.hl);
  }
  g.head_len = pos;
  pos = 0;
  if (f.sec != 0 || f.nanos != 0) {
    const uint32_t tl = (f.sec != 0 ? 1u + fields_uvarint_len((uint64_t)f.sec) : 0u) +
                        (f.nanos != 0 ? 1u + fields_uvarint_len((uint64_t)(uint32_t)f.nanos) : 0u);
    seg_put(g.time, pos, 0x2200u | tl, 2);
    if (f.sec != 0) { seg_put(g.time, pos, 0x08, 1); seg_put_uvarint(g.time, pos, (uint64_t)f.sec); }
    if (f.nanos != 0) { seg_put(g.time, pos, 0x10, 1); seg_put_uvarint(g.time, pos, (uint64_t)(uint32_t)f.nanos); }
  }
  g.time_len = pos;
  return g;
}

// stream word gw >= 8 of pre[8] || SignBytes || 0x80 (the length word is the caller's)
TXV_HD uint64_t fields_word(const VoteFields& f, const FieldSegs& g, uint32_t gw) {
  const int32_t o = (int32_t)(8u * (gw - 8u));
  const int32_t key = o - (int32_t)(g.head_len + f.hl);   // 1a 20, then 32 zeros
  uint64_t v = seg_word(g.head, o) | seg_word(g.time, key - 34) |
               mem_word(f.cf, f.cf_len, key - 34 - (int32_t)g.time_len);
  if (f.hl) v |= mem_word(f.th, f.hl, o - (int32_t)g.head_len);
  if (key > -8 && key < 2) v |= key >= 0 ? 0x1A20000000000000ull << (8u * (uint32_t)key) : 0x1A20000000000000ull >> (8u * (uint32_t)(-key));
  return v;
}

// SHA-512(pre[8] || SignBytes) for any shape; returns the hashed length in bytes.  blocks (or
// null): the padded blocks as they go to the compression, 16 words each (the host emulation)
TXV_HD uint32_t sha512_fields_generic(uint64_t st[8], const uint64_t pre[8], const VoteFields& f, uint64_t* blocks) {
  const FieldSegs g = fields_segs(f);
  const uint32_t total = 64u + g.len;
  const uint32_t nblk = (total + 17u + 127u) / 128u;
  const uint32_t last = 16u * nblk - 1u;
  {   // the first block on its own: R || A are dead behind it
    uint64_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      uint64_t v = t < 8 ? pre[t] : fields_word(f, g, (uint32_t)t);
      if ((uint32_t)t == last) v = (uint64_t)total * 8u;
      w[t] = v;
    }
    if (blocks) {
#pragma unroll
      for (int t = 0; t < 16; ++t) blocks[t] = w[t];
    }
    sha512_block(st, w);
  }
  for (uint32_t b = 1; b < nblk; ++b) {
    uint64_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const uint32_t gw = 16u * b + (uint32_t)t;
      uint64_t v = fields_word(f, g, gw);
      if (gw == last) v = (uint64_t)total * 8u;
      w[t] = v;
    }
    if (blocks) {
#pragma unroll
      for (int t = 0; t < 16; ++t) blocks[16u * b + (uint32_t)t] = w[t];
    }
    sha512_block(st, w);
  }
  return total;
}

// the two blocks of a fast shape through one copy of the compression's code
// (only the second block's words stay live beside the schedule ring)
TXV_HD void sha512_two_blocks(uint64_t st[8], const uint64_t w[32]) {
  uint64_t x[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) x[t] = w[t];
#pragma unroll 1
  for (int b = 0; b < 2; ++b) {
    sha512_block(st, x);
#pragma unroll
    for (int t = 0; t < 16; ++t) x[t] = w[16 + t];
  }
}

TXV_HD void sha512_digest_le(uint32_t digest_le[16], const uint64_t st[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    digest_le[2 * k] = bswap32((uint32_t)(st[k] >> 32));
    digest_le[2 * k + 1] = bswap32((uint32_t)st[k]);
  }
}

}  // namespace txv
