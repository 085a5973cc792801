// emu_sign.hip — TEST-ONLY host emulation of the batch signer's integer pieces
// (go-txflow_amd/csrc/sign_dev.h, ed25519_dev.h next_digit).
//
// Compiles the very same __host__ __device__ functions kernels_sign.hip runs -- the tx hash with its
// padding and aligned word loads, the TxKey / hex TxHash words, S = (r + k a) mod L, and the signed
// digits the base-point walk takes -- for the CPU.  It is not linked into libtxvote.so and the
// product never calls it.
#include "../../go-txflow_amd/csrc/sign_dev.h"
#include <cstring>
#include <vector>

using namespace txv;

// SHA-256(tx) as the TxKey column's 32 bytes and the arena's 64 hex characters.  The tx is placed
// `shift` (0..3) bytes past a 4-byte boundary, with garbage around it, as in the staged arena.
extern "C" void emu_tx_hash(const uint8_t* tx, uint32_t n, uint32_t shift, uint8_t* key_out, uint8_t* hex_out) {
  std::vector<uint32_t> store((n + 3) / 4 + 8, 0xA5A5A5A5u);
  uint8_t* p = reinterpret_cast<uint8_t*>(store.data()) + 4 + (shift & 3u);
  if (n) memcpy(p, tx, n);
  uint32_t st[8], key[8], hex[16];
  txv_sign::tx_sha256(p, n, st);
  txv_sign::tx_key_hex(st, key, hex);
  memcpy(key_out, key, 32);
  memcpy(hex_out, hex, 64);
}

static void words(const uint8_t* b, uint32_t w[8]) { memcpy(w, b, 32); }

extern "C" void emu_sc_muladd(const uint8_t* k32, const uint8_t* a32, const uint8_t* r32, uint8_t* out32) {
  uint32_t k[8], a[8], r[8];
  words(k32, k); words(a32, a); words(r32, r);
  const sc s = txv_sign::sc_muladd(k, a, r);
  memcpy(out32, s.v, 32);
}

template <int W>
static int digits(const uint8_t* s32, int32_t* out) {
  uint32_t s[8], carry = 0;
  words(s32, s);
  for (int t = 0; t < Tab<W>::kPositions; ++t) out[t] = next_digit<W>(s, carry);
  return Tab<W>::kPositions;
}

// the walk's signed digits of a scalar for base window w (out: >= 64 entries); returns their
// count (Tab<w>::kPositions), -1 for a window the walk does not take
extern "C" int emu_base_digits(int w, const uint8_t* s32, int32_t* out) {
  switch (w) {
    case 4: return digits<4>(s32, out);
    case 8: return digits<8>(s32, out);
    case 10: return digits<10>(s32, out);
    case 12: return digits<12>(s32, out);
    case 14: return digits<14>(s32, out);
    case 16: return digits<16>(s32, out);
    case 20: return digits<20>(s32, out);
    case 22: return digits<22>(s32, out);
    case 24: return digits<24>(s32, out);
    case 26: return digits<26>(s32, out);
    default: return -1;
  }
}
