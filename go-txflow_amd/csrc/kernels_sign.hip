// kernels_sign.hip — Reactor.signTxRoutine's body (txvotepool/reactor.go:108-126) for a batch of
// mempool txs and ONE validator: NewTxVote + MockPV.SignTxVote, the votes written straight into a
// route buffer (route.h) in HBM.  RFC 8032 deterministic Ed25519, byte-identical to x/crypto's
// ed25519.Sign.  Not constant-time: the walk's table lines and the variable-time inverse depend
// on the nonce (MockPV-grade signing).
//
//   txv_k_sign_addr     per signer slot: address = SHA-256(pub)[:20], once per txv_keygen
//   txv_k_sign_build    per tx: TxKey = SHA-256(tx), TxHash = its hex, the uniform columns, the
//                       offsets, the signer's address, the SignBytes length; one lane also writes
//                       the header, the pads between the columns and the arena's 16 zero bytes
//   (txv_k_signbytes)   the verifier's encoder, pointed at those columns
//   txv_k_sign_nonce    r = SHA-512(prefix || M) mod L
//   txv_k_base_walk     R' = [r]B over the context's base-point table in fe10: one mixed addition
//                       per table position after the starting entry (10 at radix 2^24, 9 at 2^26),
//                       entries gathered cooperatively into LDS (walk_lds.h), the next entry issued
//                       behind the current addition, the last addition's T skipped.  No inversion:
//                       R' = (X, Y, Z) goes to HBM
//   txv_k_base_encode   K1c's shape: G votes per lane share one inversion (Montgomery), then the
//                       canonical encoding R
//   txv_k_sign_finish   k = SHA-512(R || A || M) mod L, S = (r + k a) mod L, the 64 signature bytes
//                       into the row-major column through an LDS transpose (coalesced stores)
#include <algorithm>

#include "fe_inv_var.h"
#include "route.h"
#include "sign_dev.h"
#include "txv_device.h"
#include "walk_lds.h"

using namespace txv;

__global__ void __launch_bounds__(64) txv_k_sign_addr(const uint32_t* __restrict__ pubs_le, uint32_t n,
                                                      uint32_t* __restrict__ addr_words) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8], h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = pubs_le[i * 8 + j];
  sha256_32bytes(h, w);
#pragma unroll
  for (int j = 0; j < 5; ++j) addr_words[i * 5 + j] = bswap32(h[j]);
}

namespace {

__device__ __forceinline__ uint32_t uvarint_len(uint64_t v) {
  uint32_t n = 1;
  while (v >= 0x80u) { v >>= 7; ++n; }
  return n;
}

// the SignBytes length of a vote with a 64-byte TxHash (txv_k_signbytes' own rule; the host refused
// the times amino rejects)
__device__ __forceinline__ uint32_t signbytes_len64(int64_t height, int64_t sec, int32_t nanos, uint32_t chain_len) {
  const uint32_t tl = (sec != 0 ? 1u + uvarint_len((uint64_t)sec) : 0u) +
                      (nanos != 0 ? 1u + uvarint_len((uint64_t)(uint32_t)nanos) : 0u);
  const uint32_t body = (height != 0 ? 9u : 0u) + (1u + 1u + 64u) + 34u + (tl ? 1u + uvarint_len(tl) + tl : 0u) +
                        (chain_len ? 1u + uvarint_len(chain_len) + chain_len : 0u);
  return uvarint_len(body) + body;
}

}  // namespace

__global__ void __launch_bounds__(256) txv_k_sign_build(SignTxArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint8_t* b = a.dst;
  if (i == 0) {   // the frame: header, the pad words behind each column, the zero bytes behind the arena
    uint64_t* hd = reinterpret_cast<uint64_t*>(b);
    hd[0] = txv_route::kMagic; hd[1] = a.n; hd[2] = 64ull * a.n; hd[3] = txv_route::kFlagTxKey;
    hd[4] = a.n ? 64u : 0u; hd[5] = a.bytes; hd[6] = 0; hd[7] = 0;
    const uint32_t w[txv_route::kArena] = {8, 8, 4, 4, 4, 4, 4, 20, 64, 32, 0};
    for (int c = 0; c < txv_route::kArena; ++c)
      for (uint64_t o = a.off[c] + (uint64_t)w[c] * a.n; o < a.off[c + 1]; o += 4) *reinterpret_cast<uint32_t*>(b + o) = 0;
    for (uint64_t o = a.off[txv_route::kArena] + 64ull * a.n; o < a.bytes; o += 4) *reinterpret_cast<uint32_t*>(b + o) = 0;
  }
  if (i >= a.n) return;
  uint32_t st[8], key[8], hex[16];
  txv_sign::tx_sha256(a.tx + a.tx_off[i], a.tx_len[i], st);
  txv_sign::tx_key_hex(st, key, hex);
  uint4* kq = reinterpret_cast<uint4*>(b + a.off[txv_route::kTxKey]) + 2 * (size_t)i;
  kq[0] = make_uint4(key[0], key[1], key[2], key[3]);
  kq[1] = make_uint4(key[4], key[5], key[6], key[7]);
  uint4* hq = reinterpret_cast<uint4*>(b + a.off[txv_route::kArena]) + 4 * (size_t)i;
#pragma unroll
  for (int j = 0; j < 4; ++j) hq[j] = make_uint4(hex[4 * j], hex[4 * j + 1], hex[4 * j + 2], hex[4 * j + 3]);
  const int64_t sec = a.ts_sec[i];
  const int32_t nanos = a.ts_nanos[i];
  reinterpret_cast<int64_t*>(b + a.off[txv_route::kHeight])[i] = a.height;
  reinterpret_cast<int64_t*>(b + a.off[txv_route::kSec])[i] = sec;
  reinterpret_cast<int32_t*>(b + a.off[txv_route::kNanos])[i] = nanos;
  reinterpret_cast<uint32_t*>(b + a.off[txv_route::kOff])[i] = 64u * i;
  reinterpret_cast<uint32_t*>(b + a.off[txv_route::kLen])[i] = 64u;
  reinterpret_cast<uint32_t*>(b + a.off[txv_route::kAddrLen])[i] = 20u;
  reinterpret_cast<uint32_t*>(b + a.off[txv_route::kSigLen])[i] = 64u;
  uint32_t* ad = reinterpret_cast<uint32_t*>(b + a.off[txv_route::kAddr]) + 5 * (size_t)i;
#pragma unroll
  for (int j = 0; j < 5; ++j) ad[j] = a.addr[j];
  a.msg_len[i] = signbytes_len64(a.height, sec, nanos, a.chain_len);
}

__global__ void __launch_bounds__(256) txv_k_sign_nonce(SignTxArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  MsgView m{a.msg + i, a.n_pad, a.msg_words, a.msg_len[i]};
  uint64_t pre[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) pre[j] = be64_from_le32(a.prefix[2 * j], a.prefix[2 * j + 1]);
  uint32_t h[16];
  sha512_prefixed(h, pre, 4, m);
  const sc r = sc_reduce512(h);
#pragma unroll
  for (int j = 0; j < 8; ++j) a.rbuf[(size_t)j * a.n_pad + i] = r.v[j];
}

// ---------------------------------------------------------------- [r]B
// B alone over the radix-2^WB table: position t's signed digit by next_digit<WB>, its entry
// gathered into the wave's 8 KiB LDS buffer while addition t - 1 runs (issued as soon as that
// addition has read its own entry out of the buffer).  Every lane of the wave takes part in the
// gathers: idle lanes carry the scalar 0 and walk the digit-0 (identity) entries.
template <int WB>
__device__ __forceinline__ ge10_ext base_walk(const uint32_t* tb, const uint32_t r_in[8], uint4* buf) {
  constexpr int nT = Tab<WB>::kPositions;
  static_assert(nT >= 2, "schedule too short");
  uint32_t s[8], cs = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[i] = r_in[i];
  auto issue = [&](int t) -> bool {
    const int d = next_digit<WB>(s, cs);
    entries_to_lds(tb, (uint32_t)(t * Tab<WB>::kEntries + (d < 0 ? -d : d)), buf);
    return d < 0;
  };
  // nothing of this lane's earlier work may still be in flight: the waits below count this walk's
  // gathers alone
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  bool neg = issue(0);
  ge10_ext P;
#pragma unroll 1
  for (int t = 0; t < nT - 1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // entry t has landed in LDS
    const bool neg_t = neg;
    auto rd = [&](int role) { return entry_field_lds(buf, neg_t, role); };
    auto next = [&]() {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // read out before the next DMA lands
      neg = issue(t + 1);
    };
    if (t) {
      P = ge10_madd_rd(P, rd, neg_t, next);
    } else {
      const fe10 qp = rd(0), qm = rd(1);
      next();
      P = ge10_from_entry(qp, qm);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const bool neg_t = neg;
  // the last addition: nothing left to prefetch, and its T is never read
  return ge10_madd_rd<false>(P, [&](int role) { return entry_field_lds(buf, neg_t, role); }, neg_t, [] {});
}

__device__ __forceinline__ void store_point(uint32_t* o, size_t np, const fe& X, const fe& Y, const fe& Z) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o[(size_t)j * np] = X.v[j];
    o[(size_t)(8 + j) * np] = Y.v[j];
    o[(size_t)(16 + j) * np] = Z.v[j];
  }
}

// 3 waves per SIMD (168 VGPRs: at 4 waves' 128 the additions spilled 88 bytes per lane): one 8 KiB
// gather buffer per wave, 32 KiB per 256-thread block, three blocks per CU
#define TXV_SIGN_WALK_WAVES 3
template <int WB>
__global__ void __launch_bounds__(256, TXV_SIGN_WALK_WAVES) txv_k_base_walk(const uint32_t* __restrict__ btable,
                                                          const uint32_t* __restrict__ scal, uint32_t n, uint32_t n_pad,
                                                          uint32_t* __restrict__ rpts) {
  __shared__ uint4 pf[4][8 * 64];
  // the wave's buffer from a wave-uniform (scalar) index: the LDS-DMA destination goes to M0
  uint4* wbuf = pf[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n_waves = (n + 63u) / 64u;
  // only a wave with no work skips (w is wave-uniform)
  for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < n_waves; w += gridDim.x * 4u) {
    const uint32_t i = 64u * w + lane;
    const bool on = i < n;
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = on ? scal[(size_t)j * n_pad + i] : 0u;
    const ge10_ext P = base_walk<WB>(btable, r, wbuf);
    if (on) store_point(rpts + i, n_pad, fe_from_fe10(P.X), fe_from_fe10(P.Y), fe_from_fe10(P.Z));
  }
}

// W = 4: the 74 KB table staged in LDS (8 waves share it), the radix-16 walk over ONE scalar
__global__ void __launch_bounds__(512, 2) txv_k_base_walk_w4(const uint32_t* __restrict__ btable,
                                                             const uint32_t* __restrict__ scal, uint32_t n, uint32_t n_pad,
                                                             uint32_t* __restrict__ rpts) {
  __shared__ __attribute__((aligned(16))) uint32_t btab[Tab<4>::kWords];
  {
    const uint4* src = reinterpret_cast<const uint4*>(btable);
    uint4* dst = reinterpret_cast<uint4*>(btab);
    for (int i = threadIdx.x; i < (int)(Tab<4>::kWords / 4); i += 512) dst[i] = src[i];
  }
  __syncthreads();
  for (uint32_t i = blockIdx.x * 512 + threadIdx.x; i < n; i += gridDim.x * 512) {
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = scal[(size_t)j * n_pad + i];
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const ge_ext R = double_scalarmult_w2<4, 4>((const uint32_t*)btab, (const uint32_t*)btab, r, zero, false);
    store_point(rpts + i, n_pad, R.X, R.Y, R.Z);
  }
}

// lane t takes the points (t & ~63) G + 64 h + (t & 63), h < G (a wave reads 64 consecutive points
// per slot).  Pass 1 stores each point's exclusive prefix product of Z (words 24..31, not for the
// first); pass 2 walks back from 1 / (Z_0 ... Z_last): 1/Z_h = E_h / (E_h Z_h), then 1/E_h.
template <int G>
__global__ void __launch_bounds__(64) txv_k_base_encode(uint32_t* __restrict__ rpts, uint32_t n, uint32_t n_pad,
                                                        uint32_t* __restrict__ enc_out) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  const uint32_t base = (t & ~63u) * G + (t & 63u);
  const size_t np = n_pad;
  int cnt = 0;
  fe P;
#pragma unroll 1
  for (int h = 0; h < G; ++h) {
    const uint32_t idx = base + 64u * h;
    if (idx >= n) break;
    uint32_t* e = rpts + idx;
    fe Z;
#pragma unroll
    for (int j = 0; j < 8; ++j) Z.v[j] = e[(size_t)(16 + j) * np];
    if (h) {
#pragma unroll
      for (int j = 0; j < 8; ++j) e[(size_t)(24 + j) * np] = P.v[j];
      P = fe_mul(P, Z);
    } else {
      P = Z;
    }
    cnt = h + 1;
  }
  if (!cnt) return;
  fe inv = fe_invert_var(P);
#pragma unroll 1
  for (int h = cnt - 1; h >= 0; --h) {
    const uint32_t idx = base + 64u * h;
    const uint32_t* e = rpts + idx;
    fe X, Y, zi;
#pragma unroll
    for (int j = 0; j < 8; ++j) { X.v[j] = e[(size_t)j * np]; Y.v[j] = e[(size_t)(8 + j) * np]; }
    if (h) {
      fe Z, E;
#pragma unroll
      for (int j = 0; j < 8; ++j) { Z.v[j] = e[(size_t)(16 + j) * np]; E.v[j] = e[(size_t)(24 + j) * np]; }
      zi = fe_mul(inv, E);
      inv = fe_mul(inv, Z);
    } else {
      zi = inv;
    }
    uint32_t enc[8];
    ge_encode_zinv(enc, X, Y, zi);
#pragma unroll
    for (int j = 0; j < 8; ++j) enc_out[(size_t)j * np + idx] = enc[j];
  }
}

__global__ void __launch_bounds__(256) txv_k_sign_finish(SignTxArgs a) {
  __shared__ uint32_t tile[256 * 17];   // one vote's 16 signature words per row, padded against bank conflicts
  const uint32_t first = blockIdx.x * 256, i = first + threadIdx.x;
  if (i < a.n) {
    uint32_t Rw[8], r[8], pub[8], araw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Rw[j] = a.renc[(size_t)j * a.n_pad + i];
      r[j] = a.rbuf[(size_t)j * a.n_pad + i];
      pub[j] = a.pub[j];
      araw[j] = a.araw[j];
    }
    uint64_t pre[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pre[j] = be64_from_le32(Rw[2 * j], Rw[2 * j + 1]);
      pre[4 + j] = be64_from_le32(pub[2 * j], pub[2 * j + 1]);
    }
    MsgView m{a.msg + i, a.n_pad, a.msg_words, a.msg_len[i]};
    uint32_t h[16];
    sha512_prefixed(h, pre, 8, m);
    const sc k = sc_reduce512(h);
    const sc S = txv_sign::sc_muladd(k.v, araw, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      tile[threadIdx.x * 17 + j] = Rw[j];
      tile[threadIdx.x * 17 + 8 + j] = S.v[j];
    }
  }
  __syncthreads();
  // the block's 256 x 64 signature bytes are contiguous in the row-major column
  uint32_t* out = reinterpret_cast<uint32_t*>(a.dst + a.off[txv_route::kSig]) + (size_t)first * 16;
  const uint32_t words = (a.n - first < 256u ? a.n - first : 256u) * 16u;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const uint32_t x = q * 256 + threadIdx.x;
    if (x < words) out[x] = tile[(x >> 4) * 17 + (x & 15u)];
  }
}

// ---------------------------------------------------------------- host launchers
// votes per lane of the encode pass, by K1c's rule (kernels_verify.hip k1c_votes_per_lane): the
// largest G whose launch still gives the chip 256 waves (a quarter wave per SIMD of its 1024), so
// the inversion's share falls as the batch grows: G = 1 below 32k points, 2 from 32k, 4 from 64k
// (65536 points: 256 waves), ... 32 from 512k
static int encode_votes_per_lane(uint32_t n) {
  for (int g : {32, 16, 8, 4, 2})
    if ((uint64_t)n >= (uint64_t)g * 64 * 256) return g;
  return 1;
}

template <int WB>
static void launch_walk(const uint32_t* btable, const uint32_t* scal, uint32_t n, uint32_t n_pad, uint32_t* rpts,
                        uint32_t n_cus, hipStream_t st) {
  const uint32_t waves = (n + 63u) / 64u;
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>((waves + 3u) / 4u, std::max<uint32_t>(n_cus, 1u) * TXV_SIGN_WALK_WAVES));
  hipLaunchKernelGGL(txv_k_base_walk<WB>, dim3(grid), dim3(256), 0, st, btable, scal, n, n_pad, rpts);
}

extern "C" {

hipError_t txv_launch_sign_addr(const uint32_t* pubs_le, uint32_t n, uint32_t* addr_words, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(txv_k_sign_addr, dim3((n + 63) / 64), dim3(64), 0, st, pubs_le, n, addr_words);
  return hipGetLastError();
}

hipError_t txv_launch_sign_build(const SignTxArgs* args, hipStream_t st) {
  hipLaunchKernelGGL(txv_k_sign_build, dim3(std::max<uint32_t>(1, (args->n + 255) / 256)), dim3(256), 0, st, *args);
  return hipGetLastError();
}

hipError_t txv_launch_sign_nonce(const SignTxArgs* args, hipStream_t st) {
  if (!args->n) return hipSuccess;
  hipLaunchKernelGGL(txv_k_sign_nonce, dim3((args->n + 255) / 256), dim3(256), 0, st, *args);
  return hipGetLastError();
}

bool txv_base_walk_supported(int wb) {
  switch (wb) {
    case 4: case 8: case 10: case 12: case 14: case 16: case 20: case 22: case 24: case 26: return true;
    default: return false;
  }
}

hipError_t txv_launch_base_walk(int wb, const uint32_t* btable, const uint32_t* scal, uint32_t n, uint32_t n_pad,
                                uint32_t* rpts, uint32_t n_cus, hipStream_t st) {
  if (!n) return hipSuccess;
  switch (wb) {
    case 4: {
      const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>((n + 511u) / 512u, std::max<uint32_t>(n_cus, 1u) * 2u));
      hipLaunchKernelGGL(txv_k_base_walk_w4, dim3(grid), dim3(512), 0, st, btable, scal, n, n_pad, rpts);
      break;
    }
    case 8: launch_walk<8>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 10: launch_walk<10>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 12: launch_walk<12>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 14: launch_walk<14>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 16: launch_walk<16>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 20: launch_walk<20>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 22: launch_walk<22>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 24: launch_walk<24>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    case 26: launch_walk<26>(btable, scal, n, n_pad, rpts, n_cus, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t txv_launch_base_encode(uint32_t* rpts, uint32_t n, uint32_t n_pad, uint32_t* enc, hipStream_t st) {
  if (!n) return hipSuccess;
  const int g = encode_votes_per_lane(n);
  const uint32_t grid = (uint32_t)(((uint64_t)n + 64u * g - 1) / (64u * g));
  switch (g) {
    case 1: hipLaunchKernelGGL(txv_k_base_encode<1>, dim3(grid), dim3(64), 0, st, rpts, n, n_pad, enc); break;
    case 2: hipLaunchKernelGGL(txv_k_base_encode<2>, dim3(grid), dim3(64), 0, st, rpts, n, n_pad, enc); break;
    case 4: hipLaunchKernelGGL(txv_k_base_encode<4>, dim3(grid), dim3(64), 0, st, rpts, n, n_pad, enc); break;
    case 8: hipLaunchKernelGGL(txv_k_base_encode<8>, dim3(grid), dim3(64), 0, st, rpts, n, n_pad, enc); break;
    case 16: hipLaunchKernelGGL(txv_k_base_encode<16>, dim3(grid), dim3(64), 0, st, rpts, n, n_pad, enc); break;
    default: hipLaunchKernelGGL(txv_k_base_encode<32>, dim3(grid), dim3(64), 0, st, rpts, n, n_pad, enc); break;
  }
  return hipGetLastError();
}

hipError_t txv_launch_sign_finish(const SignTxArgs* args, hipStream_t st) {
  if (!args->n) return hipSuccess;
  hipLaunchKernelGGL(txv_k_sign_finish, dim3((args->n + 255) / 256), dim3(256), 0, st, *args);
  return hipGetLastError();
}

}  // extern "C"
