// walk_lds.h — the cooperative table-entry gather of the fixed-base walks, shared by the verify
// walk (kernels_verify.hip, K1b) and the signer's [r]B walk (kernels_sign.hip).  Device only.
//
// A walk's table entries are random 128-byte lines in tens of GB of tables: every one is an
// HBM miss, and per-lane loads of them cost the memory pipeline one line request per 16 bytes
// (8 per entry; measured, tools/microbench/gather_calib.hip: 16M entries 2.00 ms as 8 x 16-byte
// loads per lane, 0.78 ms loaded cooperatively).  So the wave loads its 64 entries together:
// load i (i < 8) fetches entries 8i .. 8i+7, 8 lanes x 16 bytes per entry (one whole line per 8
// lanes), global -> LDS (global_load_lds_dwordx4, no VGPRs; the entry's address comes from its
// lane by ds_bpermute).  The LDS image is lane-linear (load i, lane l at i * 1 KiB + 16 l); lane
// l loads piece ((l & 7) + e) & 7 of entry e = 8i + (l >> 3), which makes the pieces a reader
// lane wants land in distinct banks (8 consecutive readers -> 8 distinct 16-byte slots of a
// 256-byte row).  LDS per buffer and wave: 8 KiB.
#pragma once
#include "ed25519_dev.h"

// TXV_K1B_NO_GATHER=1 (experiment builds only, tools/microbench/walk_rate): issue no gathers, the
// walk reads whatever the LDS buffers hold -- the walk's time without its table traffic
#ifndef TXV_K1B_NO_GATHER
#define TXV_K1B_NO_GATHER 0
#endif

namespace txv {

// the wave's 64 entries (entry index e_l of lane l, 128-byte units from base) -> buf
__device__ __forceinline__ void entries_to_lds(const uint32_t* base, uint32_t e_l, uint4* buf) {
  if (TXV_K1B_NO_GATHER) return;
  const int lane = threadIdx.x & 63;
  // all 8 permutes first (one LDS round trip instead of one per load: the compiler waits for
  // outstanding LDS operations before each LDS-DMA issue)
  uint32_t e[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((8 * i + (lane >> 3)) << 2, (int)e_l);
  TXV_SCHED_FENCE();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t piece = (uint32_t)((lane & 7) + 8 * i + (lane >> 3)) & 7u;
    const uint32_t* g = base + (size_t)e[i] * kEntryWords + piece * 4u;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)(buf + 64 * i), 16, 0, 0);
  }
}

// piece j of this lane's entry in the image entries_to_lds wrote
__device__ __forceinline__ const uint4* entry_piece(const uint4* buf, int j) {
  const int e = threadIdx.x & 63;
  return buf + 64 * (e >> 3) + 8 * (e & 7) + ((j - e) & 7);
}

// one field of the lane's entry; role 0 = qp, 1 = qm (swapped for -Q by the piece choice),
// 2 = qd.  Words 0..9 = pieces 0, 1, 2.xy; 12..21 = pieces 3, 4, 5.xy; qd = 5.zw, 6, 7.
__device__ __forceinline__ fe10 entry_field_lds(const uint4* buf, bool neg, int role) {
  fe10 r;
  if (role == 2) {
    const uint2 d0 = reinterpret_cast<const uint2*>(entry_piece(buf, 5))[1];
    const uint4 d1 = *entry_piece(buf, 6), d2 = *entry_piece(buf, 7);
    r.v[0] = d0.x; r.v[1] = d0.y; r.v[2] = d1.x; r.v[3] = d1.y;
    r.v[4] = d1.z; r.v[5] = d1.w; r.v[6] = d2.x; r.v[7] = d2.y; r.v[8] = d2.z; r.v[9] = d2.w;
    return r;
  }
  const int j0 = (neg != (role == 1)) ? 3 : 0;
  const uint4 p0 = *entry_piece(buf, j0), p1 = *entry_piece(buf, j0 + 1);
  const uint2 p2 = *reinterpret_cast<const uint2*>(entry_piece(buf, j0 + 2));
  r.v[0] = p0.x; r.v[1] = p0.y; r.v[2] = p0.z; r.v[3] = p0.w;
  r.v[4] = p1.x; r.v[5] = p1.y; r.v[6] = p1.z; r.v[7] = p1.w; r.v[8] = p2.x; r.v[9] = p2.y;
  return r;
}

}  // namespace txv
