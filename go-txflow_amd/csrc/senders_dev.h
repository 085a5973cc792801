// senders_dev.h — MempoolTxVote.Senders (txvotepool/txvotepool.go:364-371) for a pool with
// TXV_POOL_SENDERS: every per-element rule, as __host__ __device__ functions, shared by the device
// engine (kernels_senders.hip), the host pool (pool.cpp) and tests/cpu_emu/emu_senders.hip.
//
// All entries' sets live in ONE open-addressing set of 64-bit words (linear probing, no deletion):
//   word = (entry + 1) << 16 | sender          0 = empty slot
// `entry` names a pool-list entry: its list position in HBM (a position is not reused before a
// compaction, which rebuilds the set through the position map), its node's serial number on the
// host (a recycled node gets a new serial, so it can never inherit a set).  An entry that leaves
// the list leaves its words behind; they are unreachable (txsMap no longer leads to the entry) and
// vanish at the next rebuild.  The home slot is a seeded mix of the word under a derived constant
// of its own, like kSeedIdx / kSeedList / kSeedSort (kernels_pool.hip): senders are peer ids and
// entries follow arrival order, neither may choose a probe chain.
//
// Writers use compare-and-swap only (device scope on the GPU); an equal word already present means
// done -- the LoadOrStore of :220.  Every reader runs in a later launch than any writer.
#pragma once
#include <stdint.h>
#include "txv_hash.h"

namespace txv_senders {

typedef unsigned long long word_t;

constexpr uint64_t kSeedSenders = 0x082EFA98EC4E6C89ull;
constexpr uint32_t kNone = 0xFFFFFFFFu;

TXV_HASH_HD word_t pair_word(uint64_t entry, uint32_t sender) { return ((word_t)(entry + 1) << 16) | (sender & 0xFFFFu); }
TXV_HASH_HD uint64_t word_entry(word_t w) { return (uint64_t)(w >> 16) - 1; }
TXV_HASH_HD uint32_t word_sender(word_t w) { return (uint32_t)(w & 0xFFFFu); }
TXV_HASH_HD uint64_t home(word_t w, uint64_t seed) { return txv_hash::mix64((uint64_t)w ^ seed ^ kSeedSenders); }

TXV_HASH_HD word_t slot_load(const word_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
// the slot's previous value (== expect: the swap happened)
TXV_HASH_HD word_t slot_cas(word_t* p, word_t expect, word_t want) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, want);
#else
  __atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  return expect;
#endif
}

// Senders.LoadOrStore(sender, true): 1 = stored now, 0 = present already, -1 = no free slot (the
// capacity rule -- stored words <= half the slots -- was broken by the caller).  mask = slots - 1.
TXV_HASH_HD int insert(word_t* slots, uint64_t mask, word_t w, uint64_t seed) {
  uint64_t s = home(w, seed) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
    word_t v = slot_load(slots + s);
    if (v == 0) {
      v = slot_cas(slots + s, 0, w);
      if (v == 0) return 1;
    }
    if (v == w) return 0;
  }
  return -1;
}

// Senders.Load(sender)
TXV_HASH_HD bool contains(const word_t* slots, uint64_t mask, word_t w, uint64_t seed) {
  uint64_t s = home(w, seed) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
    const word_t v = slot_load(slots + s);
    if (v == 0) return false;
    if (v == w) return true;
  }
  return false;
}

// A rebuild through a map of the entries (the list's compaction, a set that grows, a set that
// sheds its dead words): word w of the old set as it enters the new one, or 0 when its entry is
// gone.  npos[e] = the entry's new name, kNone = gone; entries >= n_entries are gone too.
TXV_HASH_HD word_t remap(word_t w, const uint32_t* npos, uint64_t n_entries) {
  if (w == 0) return 0;
  const uint64_t e = word_entry(w);
  if (e >= n_entries) return 0;
  const uint32_t q = npos[e];
  return q == kNone ? 0 : pair_word(q, word_sender(w));
}

// the same for the list in HBM, whose entries carry an alive flag: npos (or null: the positions
// stay) is the compaction's exclusive scan of the flags
TXV_HASH_HD word_t remap_alive(word_t w, const uint8_t* alive, const uint32_t* npos) {
  if (w == 0) return 0;
  const uint64_t e = word_entry(w);
  if (!alive[e]) return 0;
  return pair_word(npos ? npos[e] : e, word_sender(w));
}

TXV_HASH_HD bool key_eq8(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
  for (int k = 0; k < 8; ++k) d |= a[k] ^ b[k];
  return d == 0;
}

// Which entry txsMap holds for the key of vote i at the moment vote i (ErrTxInCache) is decided,
// as far as this batch made it: the latest vote i' < i of the batch with the same key that was
// admitted (TXV_POOL_OK), else kNone -- then it is the entry the list index held before the
// batch's appends (and after its Update's removals), which the caller probes.
//   ckey / cidx [m]: the batch's ADMITTED votes only, compacted from the batch's sorted order
//     (by sort slice; arrival order inside a slice run): their slices and arrival indices
//   h: the slice of vote i;   keys [n][8]: the batch's keys by arrival index
// A binary search finds the end of "slice h, arrival index < i"; from there back to the first
// full-key match inside the run.  Admissions of one key within a batch are at most n / C + 1 (the
// key must be evicted in between) and slice collisions are chance under the secret seed, so the
// walk is short whatever a peer sends -- a vote replayed n times is one admission and n - 1 hits
// that each stop at their first step.
TXV_HASH_HD uint32_t resolve_hit(const uint32_t* ckey, const uint32_t* cidx, uint32_t m, uint32_t h, uint32_t i,
                                 const uint32_t* keys) {
  uint32_t lo = 0, hi = m;                     // first c with (ckey, cidx)[c] >= (h, i)
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ckey[mid] < h || (ckey[mid] == h && cidx[mid] < i)) lo = mid + 1; else hi = mid;
  }
  for (uint32_t c = lo; c-- > 0 && ckey[c] == h;)
    if (key_eq8(keys + (size_t)cidx[c] * 8, keys + (size_t)i * 8)) return cidx[c];
  return kNone;
}

// slots for `words` stored words at no more than half load (a power of two, at least 1024)
TXV_HASH_HD uint64_t slots_for(uint64_t words) {
  uint64_t c = 1024;
  while (c < 2 * words) c <<= 1;
  return c;
}

}  // namespace txv_senders

// One batch's Senders pass (kernels_senders.hip txv_senders_batch), enqueued by txv_pooldev_run
// between pd_status (statuses, the appends' ranks) and the launch that indexes the appends, so the
// list index it probes is the one "before the batch's appends and after its Update's removals".
struct SendersArgs {
  uint32_t n, n_force;                 // the batch (pool_dev.h): votes [n_force, n) record a sender
  const uint32_t* keys;                // [n][8]
  const uint8_t* status;               // [n] TXV_POOL_*
  const uint32_t* okpos;               // [n] rank of an admitted vote among the batch's appends
  const uint32_t* skey;                // [n] the batch's sorted order: slices ...
  const uint32_t* sidx;                // ... and arrival indices
  const uint16_t* senders;             // [n - n_force] TxInfo.SenderID per vote
  const uint32_t* lk;                  // the pool list: entry keys,
  const unsigned long long* li;        // index (imask = slots - 1),
  uint32_t imask;
  const uint32_t* tail_in;             // and tail before the batch
  uint64_t seed;                       // the engine's secret seed
  uint32_t *okf, *cpos, *ckey, *cidx;  // scratch [n]: admitted flags by sorted position, their scan, the compacted columns
  void* tmp;                           // hipcub storage (txv_senders_tmp_bytes)
  size_t tmp_bytes;
  txv_senders::word_t* slots;          // the set
  uint64_t mask;
  unsigned long long* count;           // [1] words stored in the set
};
