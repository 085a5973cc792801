// kernels_load.hip — TxStore.LoadTxCommit for a batch of stored Commit records on the GPU
// (tx/store.go:67-80, reached from TxFlow.LoadCommit, txflow/service.go:115-120): Commit bytes in,
// ONE route buffer out (route.h, flags TXV_ROUTE_TXKEY | TXV_ROUTE_NIL), record k's CommitSigs as
// consecutive votes in the order the record lists them.  The decode rules are load_dev.h's.
//
// A record is a chain of length-prefix hops (key -> count -> next key) whose positions depend on each
// other, and a vote's place in the buffer depends on every record before it.  Three launches on
// one stream, no hand-off between workgroups inside a launch, no atomics, no spin:
//
//   txv_k_load_count  one wave (= one block) per record.  The wave keeps a TXV_LOAD_WINDOW byte
//                     window of the record in LDS, filled with coalesced 16-byte loads, and every
//                     lane makes the same hops out of it: one 8-byte LDS read per hop in the
//                     common case (load::hop_fast), the general walk otherwise (load::Window
//                     refills where a read leaves it).  load::next_group hands out up to 64
//                     elements that lie whole in the window; the lanes parse one element each out
//                     of LDS with wire::txvote_body (an element larger than the window: out of
//                     memory).  One bad element or a bad envelope makes the record CORRUPT, so a
//                     record's status is final BEFORE any vote is numbered: nothing is compacted
//                     later and no per-vote scratch exists (scratch is per record).
//                     Out: status, votes, TxHash bytes and longest TxHash of the record.
//   txv_k_load_scan   one block: exclusive scans of the votes and the TxHash bytes over the
//                     records (first_vote, the records' arena bases), the totals, the layout, the
//                     cap guard -- the decision is made here, on the device --, the meta (mapped
//                     host memory) and, when the buffer fits, its header and the zero bytes between
//                     and behind the columns.
//   txv_k_load_emit   one wave per OK record, only when the buffer fits: the same groups again,
//                     parsed again, a wave scan of their TxHash lengths for the arena offsets, and
//                     every lane writes its vote's columns: sig / addr / TxKey rows with
//                     wire::copy_row (alignbit, unaligned source) and the TxHash bytes, both out
//                     of the window.
#include "block_scan.h"
#include "load_dev.h"
#include "route.h"

using namespace txv::wire;
using namespace txv::load;

namespace {

constexpr uint32_t kWin = TXV_LOAD_WINDOW;
static_assert(kWin % 1024 == 0, "the window is filled by 64 lanes of 16-byte loads");

// the wave's window fill: bytes [lo, lo + kWin) of the records into LDS.  One wave per block, so
// __syncthreads is the wave's own barrier; every lane comes here together (the hops are uniform)
struct LdsFill {
  uint4* lds;
  const uint8_t* recs;
  uint64_t alloc;
  __device__ __forceinline__ void operator()(uint64_t lo) const {
    __syncthreads();                       // the old window's reads are done
    const uint4* src = reinterpret_cast<const uint4*>(recs + lo);
    const uint64_t nv = (alloc - lo) >> 4;   // 16-byte vectors readable from lo (lo < alloc)
#pragma unroll
    for (uint32_t j = 0; j < kWin / 1024; ++j) {
      const uint32_t v = threadIdx.x + 64 * j;
      if (v < nv) lds[v] = src[v];
    }
    __syncthreads();
  }
};
using Win = Window<LdsFill>;

// a record's bytes read out of the window: byte p of the record is at lds[p + d] (d = the
// record's start less the window's, modulo 2^32)
struct LdsBytes {
  const uint8_t* lds;
  uint32_t d;
  __device__ __forceinline__ uint32_t operator[](uint32_t p) const { return lds[(uint32_t)(p + d)]; }
};

constexpr uint32_t kSlack = 80;   // LDS behind the window: copy_row reads whole words past a row's end

constexpr uint32_t kFlags = TXV_ROUTE_TXKEY | TXV_ROUTE_NIL;

}  // namespace

__global__ void __launch_bounds__(64) txv_k_load_count(LoadArgs a) {
  __shared__ uint4 lds[(kWin + kSlack) / 16];
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  const uint64_t base = a.off[k];
  const uint32_t len = a.len[k];
  uint32_t st = TXV_COMMIT_OK, cnt = 0, thb = 0, mx = 0;
  Env e{};
  if (!len) {
    st = TXV_COMMIT_EMPTY;
  } else {
    const uint8_t* ldsb = reinterpret_cast<const uint8_t*>(lds);
    Win win{LdsFill{lds, a.recs, a.recs_alloc}, ldsb, base, 0, kWin, false, 0};
    const uint8_t* g = a.recs + base;
    bool ok = env_begin(WindowRef<LdsFill>{&win}, len, e);
    int r = 1;
    while (ok && r == 1) {
      uint32_t my_body = 0, my_len = 0;
      bool my_in = true, stale = false;
      const uint32_t n = next_group(win, e, r, &stale, [&](uint32_t j, uint32_t body, uint32_t blen, bool in) {
        if (lane == j) { my_body = body; my_len = blen; my_in = in; }
      });
      if (r < 0) { ok = false; break; }
      my_in = my_in && !stale;
      Parsed o{};
      bool nil = false, bad = false;
      if (lane < n) {
        if (my_in) bad = !elem_parse(LdsBytes{ldsb, (uint32_t)(base - win.lo)}, my_body, my_len, o, nil);
        else bad = !elem_parse(g, my_body, my_len, o, nil);
      }
      if (__ballot(bad)) { ok = false; break; }
      cnt += n;
      thb += wave_sum(o.th_len);
      const uint32_t m = wave_max(o.th_len);
      mx = m > mx ? m : mx;
    }
    if (!ok) { st = TXV_COMMIT_CORRUPT; cnt = 0; thb = 0; mx = 0; }
  }
  if (lane == 0) {
    const bool ok = st == TXV_COMMIT_OK;
    a.status[k] = (uint8_t)st;
    a.cnt[k] = cnt;
    a.thb[k] = thb;
    a.maxhl[k] = mx;
    a.m_status[k] = (uint8_t)st;
    a.m_thoff[k] = ok && e.th_len ? base + e.th_off : 0;
    a.m_thlen[k] = ok ? e.th_len : 0;
  }
}

__global__ void __launch_bounds__(256) txv_k_load_scan(LoadArgs a) {
  __shared__ uint32_t wmax[4];
  const uint32_t tid = threadIdx.x;
  uint64_t run_n = 0, run_b = 0;
  uint32_t mx = 0;
  for (uint32_t k0 = 0; k0 < a.n_rec; k0 += 256) {
    const uint32_t k = k0 + tid;
    const bool in = k < a.n_rec;
    const uint64_t c = in ? a.cnt[k] : 0, hb = in ? a.thb[k] : 0;
    uint64_t tn, tb;
    const uint64_t en = block_excl_scan64<4>(c, &tn);
    const uint64_t eb = block_excl_scan64<4>(hb, &tb);
    if (in) {
      a.first[k] = (uint32_t)(run_n + en);
      a.afirst[k] = (uint32_t)(run_b + eb);
      a.m_first[k] = (uint32_t)(run_n + en);
      const uint32_t m = a.maxhl[k];
      mx = m > mx ? m : mx;
    }
    run_n += tn;
    run_b += tb;
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  mx = wmax[0];
  for (int w = 1; w < 4; ++w) mx = wmax[w] > mx ? wmax[w] : mx;
  // the layout and the cap guard: nothing of the buffer is written unless all of it fits.  Offsets
  // in the buffer are 32-bit: an arena of 4 GiB or more never fits
  uint64_t off[txv_route::kNCols];
  const uint64_t total = txv_route::layout(run_n, run_b, kFlags, off);
  const bool fits = total <= a.cap && run_n < (1ull << 32) && run_b < (1ull << 32);
  if (tid == 0) {
    a.first[a.n_rec] = (uint32_t)run_n;
    a.m_first[a.n_rec] = (uint32_t)run_n;
    a.tot[0] = run_n; a.tot[1] = run_b; a.tot[2] = mx; a.tot[3] = fits ? 1 : 0;
    *a.m_meta = txv_route_meta{(uint32_t)run_n, mx, kFlags, fits ? 0u : 1u, run_b, total};
  }
  if (!fits) return;
  if (tid < 8) {
    const uint64_t hdr[8] = {txv_route::kMagic, run_n, run_b, kFlags, mx, total, 0, 0};
    reinterpret_cast<uint64_t*>(a.dst)[tid] = hdr[tid];
  }
  // the bytes between the columns and behind the arena (its 16 zero bytes and the alignment)
  if (tid < txv_route::kNCols) {
    const uint32_t kColW[txv_route::kNCols] = {8, 8, 4, 4, 4, 4, 4, 20, 64, 32, 1, 0};   // route.h layout's
    const uint64_t lo = tid < txv_route::kArena ? off[tid] + (uint64_t)kColW[tid] * run_n : off[txv_route::kArena] + run_b;
    const uint64_t hi = tid < txv_route::kArena ? off[tid + 1] : total;
    for (uint64_t p = lo; p < hi; ++p) a.dst[p] = 0;
  }
}

__global__ void __launch_bounds__(64) txv_k_load_emit(LoadArgs a) {
  __shared__ uint4 lds[(kWin + kSlack) / 16];
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  if (!a.tot[3] || a.status[k] != TXV_COMMIT_OK) return;
  const uint32_t cnt = a.cnt[k];
  if (!cnt) return;
  const uint64_t n_all = a.tot[0], ab = a.tot[1];
  uint64_t off[txv_route::kNCols];
  (void)txv_route::layout(n_all, ab, kFlags, off);
  const uint64_t base = a.off[k];
  const uint32_t len = a.len[k], first = a.first[k];
  const uint64_t a_end = (uint64_t)a.afirst[k] + a.thb[k];   // the record's arena share ends here
  const uint8_t* ldsb = reinterpret_cast<const uint8_t*>(lds);
  const uint32_t* ldsw = reinterpret_cast<const uint32_t*>(lds);
  Win win{LdsFill{lds, a.recs, a.recs_alloc}, ldsb, base, 0, kWin, false, 0};
  const uint8_t* g = a.recs + base;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(a.recs);
  uint8_t* d = a.dst;
  Env e{};
  if (!env_begin(WindowRef<LdsFill>{&win}, len, e)) return;
  int r = 1;
  uint32_t done = 0;
  uint64_t a_run = a.afirst[k];
  while (r == 1) {
    uint32_t my_body = 0, my_len = 0;
    bool my_in = true, stale = false;
    const uint32_t n = next_group(win, e, r, &stale, [&](uint32_t j, uint32_t body, uint32_t blen, bool in) {
      if (lane == j) { my_body = body; my_len = blen; my_in = in; }
    });
    if (r < 0) return;
    my_in = my_in && !stale;
    const uint32_t dl = (uint32_t)(base - win.lo);     // record byte p is LDS byte p + dl
    const LdsBytes lb{ldsb, dl};
    Parsed o{};
    bool nil = false, bad = false;
    if (lane < n) {
      if (my_in) bad = !elem_parse(lb, my_body, my_len, o, nil);
      else bad = !elem_parse(g, my_body, my_len, o, nil);
    }
    if (__ballot(bad)) return;
    uint32_t tb;
    const uint32_t ex = wave_excl_scan(o.th_len, &tb);
    const uint64_t aoff = a_run + ex;
    // what the count pass saw is what this pass sees (the records do not change in between); the
    // bounds are checked all the same, so that no store can leave the laid-out buffer
    if (lane < n && done + lane < cnt && aoff + o.th_len <= a_end) {
      const uint64_t i = (uint64_t)first + done + lane;
      const uint32_t sig_n = o.sig_len < 64 ? o.sig_len : 64u, addr_n = o.addr_len < 20 ? o.addr_len : 20u;
      uint32_t key[8] = {}, addr[5] = {}, sig[16] = {};
      uint8_t* th = d + off[txv_route::kArena] + aoff;
      if (my_in) {   // rows and TxHash out of the window (kSlack behind it for the rows' whole-word reads)
        if (o.has_key) copy_row<8>(ldsw, dl + o.key_off, 32u, key);
        if (addr_n) copy_row<5>(ldsw, dl + o.addr_off, addr_n, addr);
        if (sig_n) copy_row<16>(ldsw, dl + o.sig_off, sig_n, sig);
        for (uint32_t t = 0; t < o.th_len; ++t) th[t] = (uint8_t)lb[o.th_off + t];
      } else {       // an element larger than the window: out of memory (128 bytes behind the records)
        const uint32_t rb = (uint32_t)base;             // recs_bytes < 2^32 (host check)
        if (o.has_key) copy_row<8>(words, rb + o.key_off, 32u, key);
        if (addr_n) copy_row<5>(words, rb + o.addr_off, addr_n, addr);
        if (sig_n) copy_row<16>(words, rb + o.sig_off, sig_n, sig);
        for (uint32_t t = 0; t < o.th_len; ++t) th[t] = g[o.th_off + t];
      }
      reinterpret_cast<int64_t*>(d + off[txv_route::kHeight])[i] = o.height;
      reinterpret_cast<int64_t*>(d + off[txv_route::kSec])[i] = o.sec;
      reinterpret_cast<int32_t*>(d + off[txv_route::kNanos])[i] = o.nanos;
      reinterpret_cast<uint32_t*>(d + off[txv_route::kOff])[i] = nil ? 0u : (uint32_t)aoff;
      reinterpret_cast<uint32_t*>(d + off[txv_route::kLen])[i] = o.th_len;
      reinterpret_cast<uint32_t*>(d + off[txv_route::kAddrLen])[i] = o.addr_len;
      reinterpret_cast<uint32_t*>(d + off[txv_route::kSigLen])[i] = o.sig_len;
      uint32_t* ar = reinterpret_cast<uint32_t*>(d + off[txv_route::kAddr] + 20 * i);
#pragma unroll
      for (int q = 0; q < 5; ++q) ar[q] = addr[q];
      uint4* sg = reinterpret_cast<uint4*>(d + off[txv_route::kSig] + 64 * i);
#pragma unroll
      for (int q = 0; q < 4; ++q) sg[q] = make_uint4(sig[4 * q], sig[4 * q + 1], sig[4 * q + 2], sig[4 * q + 3]);
      uint4* tk = reinterpret_cast<uint4*>(d + off[txv_route::kTxKey] + 32 * i);
      tk[0] = make_uint4(key[0], key[1], key[2], key[3]);
      tk[1] = make_uint4(key[4], key[5], key[6], key[7]);
      d[off[txv_route::kNil] + i] = nil ? 1 : 0;
    }
    done += n;
    a_run += tb;
  }
}

extern "C" hipError_t txv_launch_load_commits(const LoadArgs* a, hipStream_t st) {
  if (a->n_rec) hipLaunchKernelGGL(txv_k_load_count, dim3(a->n_rec), dim3(64), 0, st, *a);
  hipLaunchKernelGGL(txv_k_load_scan, dim3(1), dim3(256), 0, st, *a);
  if (a->n_rec) hipLaunchKernelGGL(txv_k_load_emit, dim3(a->n_rec), dim3(64), 0, st, *a);
  return hipGetLastError();
}
