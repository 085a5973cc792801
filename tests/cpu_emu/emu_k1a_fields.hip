// emu_k1a_fields.hip — TEST-ONLY host emulation of K1a's field builder
// (go-txflow_amd/csrc/signbytes_dev.h).
//
// Compiles the very same __host__ __device__ functions txv_k_challenge runs when it gets no message
// buffer -- the compile-time layout of the common shapes and the per-lane gather of every other --
// for the CPU: the padded 128-byte blocks they hand to SHA-512 and the challenge k.  It is not
// linked into libtxvote.so and the product never calls it.
#include "../../go-txflow_amd/csrc/signbytes_dev.h"
#include "../../go-txflow_amd/csrc/sc.h"
#include <cstring>
#include <vector>

using namespace txv;

// mode 0: the gather; 32 / 64: the compile-time layout for that TxHash length (returns -1 when the
// vote does not have that shape); -1: what a wave of this one vote would take.
// ra64: R || A.  The TxHash is placed `shift` (0..3) bytes past a 4-byte boundary with 0xA5 before
// it and 16 bytes of padding behind, the chain field as the runtime uploads it.
// blocks_out: 128 bytes per block (room for 8); k_out: 32 bytes.  Returns the number of blocks.
extern "C" int emu_k1a_fields(int mode, const uint8_t* ra64, int64_t height, const uint8_t* txhash, uint32_t hl,
                              uint32_t shift, int64_t sec, int32_t nanos, const uint8_t* chain, uint32_t chain_len,
                              uint8_t* blocks_out, uint32_t max_blocks, uint8_t* k_out) {
  std::vector<uint32_t> arena((hl + 3) / 4 + 8, 0xA5A5A5A5u);
  uint8_t* th = reinterpret_cast<uint8_t*>(arena.data()) + 4 + (shift & 3u);
  if (hl) memcpy(th, txhash, hl);
  memset(th + hl, 0x5A, 16);
  std::vector<uint8_t> cfv(kChainFieldPad, 0);
  if (chain_len) {
    cfv.push_back(0x2a);
    uint32_t v = chain_len;
    while (v >= 0x80u) { cfv.push_back((uint8_t)(v | 0x80u)); v >>= 7; }
    cfv.push_back((uint8_t)v);
    cfv.insert(cfv.end(), chain, chain + chain_len);
  }
  cfv.push_back(0x80);
  const uint32_t cf_len = (uint32_t)cfv.size() - kChainFieldPad;
  cfv.resize(cfv.size() + kChainFieldPad, 0);
  std::vector<uint32_t> cfa(cfv.size() / 4 + 2, 0);   // 4-byte aligned storage
  memcpy(cfa.data(), cfv.data(), cfv.size());
  const VoteFields f{height, sec, nanos, hl, th, reinterpret_cast<const uint8_t*>(cfa.data()) + kChainFieldPad, cf_len};

  uint64_t pre[8];
  for (int j = 0; j < 8; ++j) {
    uint32_t lo, hi;
    memcpy(&lo, ra64 + 8 * j, 4);
    memcpy(&hi, ra64 + 8 * j + 4, 4);
    pre[j] = be64_from_le32(lo, hi);
  }
  uint32_t body;
  const uint32_t total = 64u + fields_len(f, body);
  const uint32_t nblk = (total + 17u + 127u) / 128u;
  if (nblk > max_blocks) return -2;
  std::vector<uint64_t> blocks(16u * nblk, 0);
  uint64_t st[8];
  sha512_init(st);
  if (mode == -1) mode = fields_fast_ok<64>(f) ? 64 : fields_fast_ok<32>(f) ? 32 : 0;
  if (mode == 0) {
    if (sha512_fields_generic(st, pre, f, blocks.data()) != total) return -3;
  } else {
    uint64_t w[32];
    uint32_t t;
    if (mode == 64 && fields_fast_ok<64>(f)) t = fields_blocks_fast<64>(w, pre, f);
    else if (mode == 32 && fields_fast_ok<32>(f)) t = fields_blocks_fast<32>(w, pre, f);
    else return -1;
    if (t != total || nblk != 2) return -3;
    memcpy(blocks.data(), w, sizeof w);
    sha512_two_blocks(st, w);
  }
  for (uint32_t i = 0; i < 16u * nblk; ++i)
    for (int b = 0; b < 8; ++b) blocks_out[8 * i + b] = (uint8_t)(blocks[i] >> (56 - 8 * b));
  uint32_t dig[16];
  sha512_digest_le(dig, st);
  const sc k = sc_reduce512(dig);
  memcpy(k_out, k.v, 32);
  return (int)nblk;
}
