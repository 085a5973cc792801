// load_dev.h — the decode rules of TxStore.LoadTxCommit for a batch of stored Commit records
// (tx/store.go:67-80, reached from TxFlow.LoadCommit, txflow/service.go:115-120), as
// __host__ __device__ code: kernels_load.hip runs it on the GPU and tests/cpu_emu/emu_load.hip the
// same source on the host.  This comment is the spec.
//
// A record is cdc.MustMarshalBinaryBare(Commit{TxHash string; Commits []*CommitSig}) (tx/store.go:92,
// types/vote_set.go:242-287), CommitSig = TxVote.  The amino rules are go-amino v0.15.1 (external) as
// restated in oracle/wire.c's header -- struct fields in order with absent-field defaults, typ3
// checks, strictly increasing extra fields skipped by typ3, Go binary.Uvarint, length-prefixed
// counts bounded by what is left -- extended by the two rules a Commit needs and a TxVoteMessage
// does not.  Both are restated from amino's published algorithm, not run against it: PARITY
// UNPINNED, as wire.c marks its own.  What IS pinned: every record oracle.commit_bytes,
// txv_save_tx_bytes or the store sink (kernels_store.hip) writes decodes to exactly the votes it was
// written from.
//
//   envelope:   [key 1, typ3 bytes: TxHash]  only as the first key; absent -> "".
//               then zero or more CONSECUTIVE keys 2, typ3 bytes: one length-prefixed element each
//               (amino writes a list of non-byte elements as a repeated field).
//               then extra fields, numbers strictly increasing, skipped by typ3 (wire::skip_rest).
//               A key number <= the last one seen is an error, except key 2 directly after key 2.
//               A wrong typ3 on key 1 or 2, a count past the record's end, a bad uvarint: errors.
//               Every byte must be consumed.
//   element:    count 0 is a nil *CommitSig (RESTATED: amino's nil-pointer list element is an empty
//               byte slice): the vote is nil, every other column zero.
//               Any other count is a TxVote body, decoded by wire::txvote_body -- the decoder of
//               txv_k_decode_msgs, not a copy of it.
//   advance:    the parent moves by UvarintSize(count) + count behind an element's key, the minimal
//               prefix size and not the bytes read (wire.c "nested struct"; wire::parse_msg does
//               the same for the message's TxVote), so an overlong count leaves the parent at a
//               byte of the element, which then has to read as a key.
//   record:     TXV_COMMIT_EMPTY for length 0 (db.Get found nothing: LoadTxCommit returns nil);
//               TXV_COMMIT_CORRUPT when the envelope or ANY element fails (LoadTxCommit panics
//               "Error reading block commit"): such a record gives no votes at all;
//               else TXV_COMMIT_OK and one vote per element, in the record's order.
//   vote:       carries the CommitSig's own TxHash, not the envelope's (the reference compares
//               neither with the other; TxFlow routes by vote.TxHash).  sig_len > 64 and
//               addr_len > 20 keep their true lengths with the first 64 / 20 bytes, as in every
//               route buffer.
//
// All positions are byte offsets from the record's start; B is anything with b[p] -> byte.
#pragma once
#include "wire_dev.h"
#include "../../include/txvote.h"

// bytes of a record the count and emit passes keep in LDS at a time (one wave per record)
#define TXV_LOAD_WINDOW 12288

namespace txv {
namespace load {

// A window of `w` bytes over a byte range, refilled where a read leaves it: the accessor the
// envelope walk reads through.  On the GPU the window is LDS filled by the whole wave with
// 16-byte loads (every lane makes the same reads, so every lane takes a refill together); on the
// host it is a small buffer, so that the tests put keys and counts across window edges.
// fill(lo): make bytes [lo, lo + w) of the range readable at buf[0, w); lo is a multiple of 16.
template <typename Fill>
struct Window {
  Fill fill;
  const uint8_t* buf;
  uint64_t base;      // the record's offset in the range
  uint64_t lo;        // the window's
  uint32_t w;
  bool valid;
  uint32_t fills;     // refills so far: what was taken out of an earlier window is gone
  TXV_WIRE_HD uint32_t get(uint32_t p) {
    const uint64_t a = base + p;
    if (!valid || a < lo || a - lo >= w) {
      lo = a & ~15ull;
      fill(lo);
      valid = true;
      ++fills;
    }
    return buf[a - lo];
  }
  // bytes [p, p + n) of the record are in the window as it stands
  TXV_WIRE_HD bool covers(uint32_t p, uint32_t n) const {
    const uint64_t a = base + p;
    return valid && a >= lo && a - lo + n <= w;
  }
  // where byte p of the record is in buf (covers(p, 1))
  TXV_WIRE_HD uint32_t at(uint32_t p) const { return (uint32_t)(base + p - lo); }
};
template <typename Fill>
struct WindowRef {
  Window<Fill>* win;
  TXV_WIRE_HD uint32_t operator[](uint32_t p) const { return win->get(p); }
};

struct Env {
  uint32_t p, end, last;        // next byte, the record's length, the last key number seen
  uint32_t th_off, th_len;      // Commit.TxHash (length 0: absent)
};

// the record's first key: the optional TxHash.  false: an amino error
template <typename B>
TXV_WIRE_HD bool env_begin(B b, uint32_t len, Env& e) {
  e.p = 0; e.end = len; e.last = 0; e.th_off = 0; e.th_len = 0;
  if (!len) return true;
  uint32_t num = 0, typ = 0;
  const uint32_t k = wire::field_key(b, 0u, len, num, typ);
  if (!k) return false;
  if (num != 1) return true;     // the elements' or an extra field's key (0 fails there: <= last)
  if (typ != wire::TYP_BYTES) return false;
  uint32_t body, blen;
  const uint32_t a = wire::byte_slice(b, k, len, body, blen);
  if (!a) return false;
  e.th_off = body; e.th_len = blen;
  e.last = 1;
  e.p = k + a;
  return true;
}

// the next element: 1 = its body is [body, body + blen) (blen 0: nil), 0 = the record ended well
// (extra fields skipped, every byte consumed), -1 = an amino error
template <typename B>
TXV_WIRE_HD int env_next(B b, Env& e, uint32_t& body, uint32_t& blen) {
  if (e.p == e.end) return 0;
  uint32_t num = 0, typ = 0;
  const uint32_t k = wire::field_key(b, e.p, e.end, num, typ);
  if (!k) return -1;
  if (num == 2 && e.last <= 2) {
    if (typ != wire::TYP_BYTES) return -1;
    e.last = 2;
    if (!wire::byte_slice(b, e.p + k, e.end, body, blen)) return -1;
    e.p += k + wire::uvarint_size(blen) + blen;   // <= end: the bytes read were >= the minimal size
    return 1;
  }
  const bool ok = wire::skip_rest(b, e.p, e.end, e.last);
  e.p = e.end;
  return ok ? 0 : -1;
}

// env_next's common case in one window read: the one-byte key 0x12 (field 2, typ3 bytes) and a
// count that ends within 7 bytes and fits the record, read as 8 bytes at once from the window's
// words (wire::peek8 / vint, the reads of wire::fast_msg).  true: the element, with e advanced
// exactly as env_next advances it; false: nothing changed, env_next decides (every other key, a
// longer count, any error).  The caller guarantees win.covers(e.p, 12).
template <typename WP>
TXV_WIRE_HD bool hop_fast(WP words, uint32_t at, Env& e, uint32_t& body, uint32_t& blen) {
  if (e.p >= e.end || e.last > 2) return false;
  const uint64_t x = wire::peek8(words, at);
  if ((x & 0xFF) != 0x12u) return false;
  const uint32_t left = e.end - e.p - 1;
  uint64_t cnt;
  const uint32_t nb = wire::vint(x >> 8, left < 7 ? left : 7u, cnt);
  if (!nb || cnt > (uint64_t)(left - nb)) return false;
  body = e.p + 1 + nb;
  blen = (uint32_t)cnt;
  e.last = 2;
  e.p += 1 + wire::uvarint_size(cnt) + (uint32_t)cnt;
  return true;
}

// The walk's next group of elements, as both passes take it: up to 64, and only elements that lie
// whole in ONE window, so that they are parsed out of it.  Once the group has an element, the
// window must not move under it: a hop whose key and count (20 bytes at most) may leave the window,
// or an element that does not lie whole in it, ends the group, and the next group starts behind a
// refill at that key.  An element that does not fit a fresh window is a group of its own
// (in_window false: parsed from the record's bytes in memory).  keep(j, body, blen, in_window) is
// called for element j.  r = the walk's last answer (1: more).  *stale: the window moved after
// all the same (the extra fields behind the last element are skipped through it): the group's
// elements are to be read from memory.
template <typename Fill, typename Keep>
TXV_WIRE_HD uint32_t next_group(Window<Fill>& win, Env& e, int& r, bool* stale, Keep keep) {
  const WindowRef<Fill> b{&win};
  uint32_t n = 0, body = 0, blen = 0, fills0 = 0;
  r = 1;
  while (n < 64) {
    const uint32_t left = e.end - e.p;
    if (n && !win.covers(e.p, left < 20 ? left : 20u)) {
      win.valid = false;
      break;
    }
    const Env save = e;
    const bool fast = win.covers(e.p, 12) &&
                      hop_fast(reinterpret_cast<const uint32_t*>(win.buf), win.at(e.p), e, body, blen);
    if (!fast && (r = env_next(b, e, body, blen)) != 1) break;
    const bool in = win.covers(body, blen);
    if (!in && n) {
      e = save;
      win.valid = false;
      break;
    }
    if (!n) fills0 = win.fills;
    keep(n, body, blen, in);
    ++n;
    if (!in) break;
  }
  *stale = n && win.fills != fills0;
  return n;
}

// one element: false = an amino error in its TxVote body.  o is all zero for a nil element
template <typename B>
TXV_WIRE_HD bool elem_parse(B b, uint32_t body, uint32_t blen, wire::Parsed& o, bool& nil) {
  o = wire::Parsed{};
  nil = blen == 0;
  return nil || wire::txvote_body(b, body, body + blen, o);
}

}  // namespace load
}  // namespace txv

// ---- the kernels' arguments (kernels_load.hip txv_launch_load_commits) ----
struct LoadArgs {
  const uint8_t* recs;            // the records' bytes, 16-byte aligned, readable to recs_alloc
  uint64_t recs_alloc;            // >= recs_bytes + 128, a multiple of 16
  const uint64_t* off;            // [n_rec] record k at recs + off[k] (off + len <= recs_bytes: host check)
  const uint32_t* len;            // [n_rec]
  uint32_t n_rec;
  uint8_t* dst;                   // the route buffer, 16-byte aligned
  uint64_t cap;                   // nothing is written at or past dst + cap
  // per record, written by the count pass: status, elements (0 unless OK), their TxHash bytes and
  // the longest; then by the scan: the first vote (n_rec + 1 entries) and the first arena byte
  uint8_t* status;
  uint32_t* cnt;
  uint32_t* thb;
  uint32_t* maxhl;
  uint32_t* first;
  uint32_t* afirst;
  uint64_t* tot;                  // [4] votes, arena bytes, longest TxHash, 1 = fits cap (the emit pass runs)
  // mapped host memory: what txv_load_commits_wait hands out
  uint8_t* m_status;              // [n_rec]
  uint32_t* m_first;              // [n_rec + 1]
  uint64_t* m_thoff;              // [n_rec] Commit.TxHash's offset in recs
  uint32_t* m_thlen;              // [n_rec]
  txv_route_meta* m_meta;
};

#if defined(__HIPCC__)
extern "C" hipError_t txv_launch_load_commits(const LoadArgs* a, hipStream_t st);
#endif
