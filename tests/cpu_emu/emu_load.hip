// emu_load.hip — TEST-ONLY host emulation of the Commit loader's decode (go-txflow_amd/csrc/load_dev.h).
//
// Compiles the very same __host__ __device__ envelope walk and element parse that kernels_load.hip
// runs, and drives them the way its count and emit passes do: the walk reads through a
// load::Window (here a host buffer of `window` bytes, refilled where a read leaves it, so a small
// window puts every key and count across an edge), load::next_group hands out up to 64 elements
// that lie whole in the window, each is parsed out of the window (an element larger than the
// window: from the record's bytes), one bad element makes the record CORRUPT, and the sig / addr /
// TxKey rows come out of wire::copy_row over the window's words (or the aligned words of the
// buffer the record sits in at byte residue `shift`).  It is not linked into libtxvote.so and the
// product never calls it.
#include "../../go-txflow_amd/csrc/load_dev.h"
#include <cstring>
#include <vector>

using namespace txv::wire;
using namespace txv::load;

struct EmuVote {
  int64_t height, sec;
  int32_t nanos;
  uint32_t is_nil, th_off, th_len, addr_len, sig_len, has_key;
  uint8_t addr[20], sig[64], key[32];
};

namespace {
struct HostFill {
  uint8_t* win;
  const uint8_t* range;
  uint64_t range_bytes;
  uint32_t w;
  uint32_t* fills;
  void operator()(uint64_t lo) const {
    memset(win, 0xCD, w);                       // what a fill does not bring is garbage
    const uint64_t n = lo < range_bytes ? (range_bytes - lo < w ? range_bytes - lo : w) : 0;
    memcpy(win, range + lo, n);
    ++*fills;
  }
};
}  // namespace

// One record through the device rules.  Returns TXV_COMMIT_*; *n_out = its votes (0 unless OK),
// votes[0, *n_out) filled (at most max_votes: -1 when there are more), *th_off / *th_len =
// Commit.TxHash in the record, *fills = window refills.  window: a multiple of 16, >= 32.
extern "C" int emu_load_record(const uint8_t* rec, uint32_t len, uint32_t window, uint32_t shift, uint32_t max_votes,
                               uint32_t* th_off, uint32_t* th_len, uint32_t* n_out, EmuVote* votes, uint32_t* fills) {
  *n_out = 0; *th_off = 0; *th_len = 0; *fills = 0;
  if (window < 32 || window % 16 || shift > 4096) return -2;
  if (!len) return TXV_COMMIT_EMPTY;
  const uint64_t alloc = ((uint64_t)shift + len + 128 + 15) & ~15ull;
  std::vector<uint32_t> words(alloc / 4, 0);
  uint8_t* range = reinterpret_cast<uint8_t*>(words.data());
  memcpy(range + shift, rec, len);
  std::vector<uint8_t> wbuf(window + 80, 0xCD);       // + the slack the kernels keep behind their window
  Window<HostFill> win{HostFill{wbuf.data(), range, alloc, window, fills}, wbuf.data(), shift, 0, window, false, 0};
  const uint8_t* g = range + shift;
  const uint32_t* wwords = reinterpret_cast<const uint32_t*>(wbuf.data());
  Env e{};
  if (!env_begin(WindowRef<HostFill>{&win}, len, e)) return TXV_COMMIT_CORRUPT;
  std::vector<EmuVote> out;
  int r = 1;
  while (r == 1) {
    uint32_t body[64], blen[64];
    bool in[64], stale = false;
    const uint32_t n = next_group(win, e, r, &stale, [&](uint32_t j, uint32_t bo, uint32_t bl, bool w) {
      body[j] = bo; blen[j] = bl; in[j] = w;
    });
    if (r < 0) return TXV_COMMIT_CORRUPT;
    for (uint32_t j = 0; j < n; ++j) in[j] = in[j] && !stale;
    const uint32_t dl = (uint32_t)(shift - win.lo);    // record byte p is window byte p + dl
    for (uint32_t j = 0; j < n; ++j) {
      Parsed o;
      bool nil;
      struct WinBytes {
        const uint8_t* w; uint32_t d;
        uint32_t operator[](uint32_t p) const { return w[(uint32_t)(p + d)]; }
      } wb{wbuf.data(), dl};
      if (in[j] && !(body[j] + dl <= window && blen[j] <= window - (body[j] + dl))) return -4;   // not in the window after all
      if (!(in[j] ? elem_parse(wb, body[j], blen[j], o, nil) : elem_parse(g, body[j], blen[j], o, nil)))
        return TXV_COMMIT_CORRUPT;
      EmuVote v{};
      v.height = o.height; v.sec = o.sec; v.nanos = o.nanos;
      v.is_nil = nil; v.th_off = o.th_off; v.th_len = o.th_len; v.addr_len = o.addr_len; v.sig_len = o.sig_len;
      v.has_key = o.has_key;
      const uint32_t sig_n = o.sig_len < 64 ? o.sig_len : 64u, addr_n = o.addr_len < 20 ? o.addr_len : 20u;
      uint32_t key[8] = {}, addr[5] = {}, sig[16] = {};
      const uint32_t* words_j = in[j] ? wwords : words.data();
      const uint32_t at = in[j] ? dl : shift;
      if (o.has_key) copy_row<8>(words_j, at + o.key_off, 32u, key);
      if (addr_n) copy_row<5>(words_j, at + o.addr_off, addr_n, addr);
      if (sig_n) copy_row<16>(words_j, at + o.sig_off, sig_n, sig);
      memcpy(v.key, key, 32); memcpy(v.addr, addr, 20); memcpy(v.sig, sig, 64);
      if (in[j])
        for (uint32_t t = 0; t < o.th_len; ++t)
          if (wb[o.th_off + t] != g[o.th_off + t]) return -3;   // the TxHash as the emit pass reads it
      out.push_back(v);
    }
  }
  *th_off = e.th_off; *th_len = e.th_len;
  if (out.size() > max_votes) return -1;
  *n_out = (uint32_t)out.size();
  if (!out.empty()) memcpy(votes, out.data(), out.size() * sizeof(EmuVote));
  return TXV_COMMIT_OK;
}
