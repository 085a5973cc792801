// emu_senders.hip — TEST-ONLY host emulation of the Senders set rules (go-txflow_amd/csrc/senders_dev.h).
//
// Compiles the very same __host__ __device__ functions the pool runs -- the word layout, the seeded
// home slot, insert / contains by compare-and-swap, the rebuild through an entry map, and the
// resolution of an ErrTxInCache vote to the batch's latest earlier admission of its key -- for the
// CPU.  It is not linked into libtxvote.so and the product never calls it.
//
// With -DEMU_SENDERS_MAIN the file is a stand-alone program that drives the same functions over a
// few thousand random operations against std::set, for a sanitizer run on the host:
//   hipcc -O1 -g -std=c++17 -DEMU_SENDERS_MAIN -Xarch_host -fsanitize=address,undefined \
//         tests/cpu_emu/emu_senders.hip -o emu_senders_san && ./emu_senders_san
#include "../../go-txflow_amd/csrc/senders_dev.h"
#include <cstring>

using txv_senders::word_t;

extern "C" uint64_t emu_sn_word(uint64_t entry, uint32_t sender) { return txv_senders::pair_word(entry, sender); }
extern "C" uint64_t emu_sn_word_entry(uint64_t w) { return txv_senders::word_entry(w); }
extern "C" uint32_t emu_sn_word_sender(uint64_t w) { return txv_senders::word_sender(w); }
extern "C" uint64_t emu_sn_home(uint64_t entry, uint32_t sender, uint64_t seed) {
  return txv_senders::home(txv_senders::pair_word(entry, sender), seed);
}
extern "C" uint64_t emu_sn_slots_for(uint64_t words) { return txv_senders::slots_for(words); }

// slots: n_slots words (a power of two)
extern "C" int emu_sn_insert(uint64_t* slots, uint64_t n_slots, uint64_t entry, uint32_t sender, uint64_t seed) {
  return txv_senders::insert(reinterpret_cast<word_t*>(slots), n_slots - 1, txv_senders::pair_word(entry, sender), seed);
}
extern "C" int emu_sn_contains(const uint64_t* slots, uint64_t n_slots, uint64_t entry, uint32_t sender, uint64_t seed) {
  return txv_senders::contains(reinterpret_cast<const word_t*>(slots), n_slots - 1, txv_senders::pair_word(entry, sender),
                               seed)
             ? 1
             : 0;
}

// every word of `old` through npos into `neu` (cleared first): the words stored, or -1 when one found no slot
extern "C" int64_t emu_sn_rebuild(const uint64_t* old, uint64_t n_old, const uint32_t* npos, uint64_t n_entries,
                                  uint64_t* neu, uint64_t n_new, uint64_t seed) {
  memset(neu, 0, n_new * 8);
  int64_t stored = 0;
  for (uint64_t s = 0; s < n_old; ++s) {
    const word_t w = txv_senders::remap(old[s], npos, n_entries);
    if (!w) continue;
    const int r = txv_senders::insert(reinterpret_cast<word_t*>(neu), n_new - 1, w, seed);
    if (r < 0) return -1;
    stored += r;
  }
  return stored;
}

// the same through the alive flags and the compaction's position map of the list in HBM
extern "C" int64_t emu_sn_rebuild_alive(const uint64_t* old, uint64_t n_old, const uint8_t* alive, const uint32_t* npos,
                                        uint64_t* neu, uint64_t n_new, uint64_t seed) {
  memset(neu, 0, n_new * 8);
  int64_t stored = 0;
  for (uint64_t s = 0; s < n_old; ++s) {
    const word_t w = txv_senders::remap_alive(old[s], alive, npos);
    if (!w) continue;
    const int r = txv_senders::insert(reinterpret_cast<word_t*>(neu), n_new - 1, w, seed);
    if (r < 0) return -1;
    stored += r;
  }
  return stored;
}

extern "C" uint32_t emu_sn_resolve(const uint32_t* ckey, const uint32_t* cidx, uint32_t m, uint32_t h, uint32_t i,
                                   const uint32_t* keys) {
  return txv_senders::resolve_hit(ckey, cidx, m, h, i, keys);
}

#ifdef EMU_SENDERS_MAIN
#include <cstdio>
#include <random>
#include <set>
#include <vector>

int main() {
  std::mt19937_64 rng(7);
  const uint64_t seed = rng();
  int bad = 0;
  // insert / contains against std::set, through two rebuilds (drop half the entries, then grow)
  uint64_t n_slots = 1024;
  std::vector<uint64_t> slots(n_slots, 0);
  std::set<std::pair<uint32_t, uint32_t>> ref;
  const uint32_t E = 200;
  for (int round = 0; round < 3; ++round) {
    for (int k = 0; k < 500 && ref.size() * 2 < n_slots; ++k) {
      const uint32_t e = (uint32_t)(rng() % E), s = (uint32_t)(rng() % 5 == 0 ? 65535 : rng() % 7);
      const int r = emu_sn_insert(slots.data(), n_slots, e, s, seed);
      bad += r != (ref.insert({e, s}).second ? 1 : 0);
    }
    for (uint32_t e = 0; e < E; ++e)
      for (uint32_t s : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 65535u})
        bad += emu_sn_contains(slots.data(), n_slots, e, s, seed) != (int)ref.count({e, s});
    std::vector<uint32_t> npos(E);
    std::set<std::pair<uint32_t, uint32_t>> nref;
    uint32_t q = 0;
    for (uint32_t e = 0; e < E; ++e) npos[e] = (round == 0 && (e & 1)) ? txv_senders::kNone : q++;
    for (const auto& p : ref)
      if (npos[p.first] != txv_senders::kNone) nref.insert({npos[p.first], p.second});
    const uint64_t n_new = round == 1 ? n_slots * 2 : n_slots;
    std::vector<uint64_t> neu(n_new);
    bad += emu_sn_rebuild(slots.data(), n_slots, npos.data(), E, neu.data(), n_new, seed) != (int64_t)nref.size();
    slots.swap(neu);
    n_slots = n_new;
    ref.swap(nref);
  }
  // resolve_hit on random sorted columns against a direct scan
  for (int t = 0; t < 200; ++t) {
    const uint32_t n = 1 + (uint32_t)(rng() % 64);
    std::vector<uint32_t> keys((size_t)n * 8, 0), slice(n), adm(n);
    for (uint32_t i = 0; i < n; ++i) {
      keys[(size_t)i * 8] = (uint32_t)(rng() % 6);
      slice[i] = keys[(size_t)i * 8] % 3;          // two keys share each slice
      adm[i] = rng() % 2;
    }
    std::vector<uint32_t> ckey, cidx;
    for (uint32_t h = 0; h < 3; ++h)
      for (uint32_t i = 0; i < n; ++i)
        if (slice[i] == h && adm[i]) { ckey.push_back(h); cidx.push_back(i); }
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t exp = txv_senders::kNone;
      for (uint32_t k = 0; k < i; ++k)
        if (adm[k] && keys[(size_t)k * 8] == keys[(size_t)i * 8]) exp = k;
      bad += emu_sn_resolve(ckey.data(), cidx.data(), (uint32_t)ckey.size(), slice[i], i, keys.data()) != exp;
    }
  }
  printf("emu_senders: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
#endif
