"""The Senders set's per-element rules (go-txflow_amd/csrc/senders_dev.h) compiled for the host by
tests/cpu_emu/emu_senders.hip: the open-addressing set of (entry + 1) << 16 | sender words
(MempoolTxVote.Senders.LoadOrStore / Load, txvotepool/txvotepool.go:220, reactor.go:245), its
rebuild through an entry map, and the resolution of an ErrTxInCache vote to the entry txsMap holds
for its key "at that moment" inside a batch (:213-227 after the :250 / :265-270 of earlier votes)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_senders.so")
SEED = 0x1234_5678_9ABC_DEF1
NONE = 0xFFFFFFFF
u64, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(EMU_DIR, "emu_senders.hip")
    deps = [src] + [os.path.join(HERE, "..", "go-txflow_amd", "csrc", f) for f in ("senders_dev.h", "txv_hash.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    E.emu_sn_word.argtypes, E.emu_sn_word.restype = [u64, u32], u64
    E.emu_sn_word_entry.argtypes, E.emu_sn_word_entry.restype = [u64], u64
    E.emu_sn_word_sender.argtypes, E.emu_sn_word_sender.restype = [u64], u32
    E.emu_sn_home.argtypes, E.emu_sn_home.restype = [u64, u32, u64], u64
    E.emu_sn_slots_for.argtypes, E.emu_sn_slots_for.restype = [u64], u64
    E.emu_sn_insert.argtypes, E.emu_sn_insert.restype = [vp, u64, u64, u32, u64], ctypes.c_int
    E.emu_sn_contains.argtypes, E.emu_sn_contains.restype = [vp, u64, u64, u32, u64], ctypes.c_int
    E.emu_sn_rebuild.argtypes, E.emu_sn_rebuild.restype = [vp, u64, vp, u64, vp, u64, u64], ctypes.c_int64
    E.emu_sn_rebuild_alive.argtypes, E.emu_sn_rebuild_alive.restype = [vp, u64, vp, vp, vp, u64, u64], ctypes.c_int64
    E.emu_sn_resolve.argtypes, E.emu_sn_resolve.restype = [vp, vp, u32, u32, u32, vp], u32
    return E


class Set:
    def __init__(self, E, n_slots):
        self.E, self.slots = E, np.zeros(n_slots, np.uint64)

    def insert(self, e, s):
        return self.E.emu_sn_insert(self.slots.ctypes.data, len(self.slots), e, s, SEED)

    def has(self, e, s):
        return bool(self.E.emu_sn_contains(self.slots.ctypes.data, len(self.slots), e, s, SEED))

    def stored(self):
        return int(np.count_nonzero(self.slots))


def test_word_layout(emu):
    assert emu.emu_sn_word(0, 0) == 1 << 16, "entry 0, sender 0 is not the empty word"
    assert emu.emu_sn_word(5, 7) == (6 << 16) | 7
    for e, s in ((0, 0), (0, 65535), (2 ** 32 - 2, 0), (2 ** 32 - 2, 65535), (12345, 9)):
        w = emu.emu_sn_word(e, s)
        assert w != 0 and emu.emu_sn_word_entry(w) == e and emu.emu_sn_word_sender(w) == s
    assert emu.emu_sn_slots_for(0) == 1024 and emu.emu_sn_slots_for(512) == 1024 and emu.emu_sn_slots_for(513) == 2048


def test_insert_is_idempotent_and_sets_do_not_mix(emu):
    S = Set(emu, 64)
    assert S.insert(3, 1) == 1 and S.insert(3, 1) == 0 and S.stored() == 1        # LoadOrStore
    assert S.insert(3, 2) == 1                                                     # two senders, one entry
    assert S.has(3, 1) and S.has(3, 2) and not S.has(3, 3) and not S.has(4, 1) and not S.has(2, 1)
    # sender 0 (UnknownPeerID) and 65535, entry 0 and the largest list position
    big = 2 ** 32 - 2
    for e, s in ((0, 0), (0, 65535), (big, 0), (big, 65535)):
        assert not S.has(e, s)
        assert S.insert(e, s) == 1 and S.has(e, s)
    assert not S.has(1, 0) and not S.has(big - 1, 65535) and not S.has(0, 1)
    assert S.stored() == 6


def test_probing_wraps_past_the_last_slot(emu):
    n = 16
    last = [(e, s) for e in range(400) for s in (1, 2) if emu.emu_sn_home(e, s, SEED) % n == n - 1][:3]
    assert len(last) == 3
    S = Set(emu, n)
    for e, s in last:
        assert S.insert(e, s) == 1
    assert S.slots[n - 1] != 0 and S.slots[0] != 0 and S.slots[1] != 0, "the second and third wrap to slots 0 and 1"
    assert all(S.has(e, s) for e, s in last) and all(S.insert(e, s) == 0 for e, s in last)
    # a full set answers instead of spinning: no free slot is -1, an absent word is absent
    T = Set(emu, 4)
    assert [T.insert(e, 1) for e in range(4)] == [1, 1, 1, 1]
    assert T.insert(9, 1) == -1 and not T.has(9, 1) and T.has(2, 1)


def test_rebuild_through_a_position_map(emu):
    rng = np.random.default_rng(5)
    S = Set(emu, 1024)
    pairs = {(int(e), int(s)) for e, s in zip(rng.integers(0, 100, 400), rng.choice([0, 1, 2, 3, 7, 65535], 400))}
    for e, s in pairs:
        S.insert(e, s)
    npos = np.full(100, NONE, np.uint32)          # odd entries are dead, the live ones close ranks
    npos[::2] = np.arange(50, dtype=np.uint32)
    for n_new in (1024, 4096):
        N = Set(emu, n_new)
        stored = emu.emu_sn_rebuild(S.slots.ctypes.data, 1024, npos.ctypes.data, 100, N.slots.ctypes.data, n_new, SEED)
        live = {(e // 2, s) for e, s in pairs if e % 2 == 0}
        assert stored == len(live) == N.stored()
        for q in range(50):
            for s in (0, 1, 2, 3, 7, 65535):
                assert N.has(q, s) == ((q, s) in live)
    # an entry beyond the map is gone too
    N = Set(emu, 1024)
    assert emu.emu_sn_rebuild(S.slots.ctypes.data, 1024, npos.ctypes.data, 10, N.slots.ctypes.data, 1024, SEED) == \
        len({(e, s) for e, s in pairs if e % 2 == 0 and e < 10})


def test_rebuild_through_alive_flags_and_a_compaction_map(emu):
    """what the list compaction in HBM does to the set: npos = exclusive scan of the alive flags;
    a live entry's words move to its new position, a dead entry's vanish; npos null keeps positions"""
    rng = np.random.default_rng(6)
    S = Set(emu, 1024)
    pairs = {(int(e), int(s)) for e, s in zip(rng.integers(0, 100, 400), rng.choice([0, 1, 2, 3, 7, 65535], 400))}
    for e, s in pairs:
        S.insert(e, s)
    alive = (rng.random(100) < 0.4).astype(np.uint8)
    alive[[0, 99]] = 1
    npos = (np.cumsum(alive) - alive).astype(np.uint32)
    N = Set(emu, 1024)
    live = {(int(npos[e]), s) for e, s in pairs if alive[e]}
    assert emu.emu_sn_rebuild_alive(S.slots.ctypes.data, 1024, alive.ctypes.data, npos.ctypes.data, N.slots.ctypes.data,
                                    1024, SEED) == len(live) == N.stored()
    for q in range(int(alive.sum())):
        for s in (0, 1, 2, 3, 7, 65535):
            assert N.has(q, s) == ((q, s) in live)
    K = Set(emu, 2048)                              # a rebuild in place: the positions stay
    kept = {(e, s) for e, s in pairs if alive[e]}
    assert emu.emu_sn_rebuild_alive(S.slots.ctypes.data, 1024, alive.ctypes.data, None, K.slots.ctypes.data, 2048,
                                    SEED) == len(kept)
    assert all(K.has(e, s) == ((e, s) in kept) for e in range(100) for s in (0, 1, 2, 3, 7, 65535))


def _columns(votes):
    """votes: [(key id, slice, admitted)] in arrival order -> (ckey, cidx, keys): the admitted votes
    compacted from the sorted order (stable by slice), the key words by arrival index"""
    keys = np.zeros((len(votes), 8), np.uint32)
    for i, (k, _, _) in enumerate(votes):
        keys[i, 5] = k
    order = sorted(range(len(votes)), key=lambda i: (votes[i][1], i))
    adm = [i for i in order if votes[i][2]]
    return (np.array([votes[i][1] for i in adm], np.uint32), np.array(adm, np.uint32), keys)


def _resolve(emu, votes, i):
    ckey, cidx, keys = _columns(votes)
    return emu.emu_sn_resolve(ckey.ctypes.data, cidx.ctypes.data, len(cidx), votes[i][1], i, keys.ctypes.data)


def test_hit_resolution_on_hand_made_columns(emu):
    A, B = 10, 11                                   # two keys that share slice 4
    # no earlier admission at all (the only other votes of the run come later or were not admitted)
    v = [(A, 4, False), (B, 9, True), (A, 4, False), (A, 4, True)]
    assert _resolve(emu, v, 0) == NONE and _resolve(emu, v, 2) == NONE
    # an earlier admission of ANOTHER key in the same slice run is not a match
    v = [(B, 4, True), (A, 4, False)]
    assert _resolve(emu, v, 1) == NONE
    v = [(A, 4, True), (B, 4, True), (A, 4, False)]
    assert _resolve(emu, v, 2) == 0, "steps back over the other key's admission to its own"
    # two admissions of one key: the later one wins only for later hits
    v = [(A, 4, True), (A, 4, False), (B, 4, True), (A, 4, True), (A, 4, False), (A, 2, False)]
    assert _resolve(emu, v, 1) == 0 and _resolve(emu, v, 4) == 3
    assert _resolve(emu, v, 3) == 0, "a vote's own admission is not earlier than itself"
    # a hit between an ErrEncoding push (cached, never admitted) and an admission of the key
    v = [(A, 4, False), (A, 4, False), (A, 4, True), (A, 4, False)]
    assert _resolve(emu, v, 1) == NONE and _resolve(emu, v, 3) == 2
    # runs before and after the hit's own never match
    v = [(A, 3, True), (A, 5, True), (A, 4, False)]
    assert _resolve(emu, v, 2) == NONE
    # no admitted vote in the whole batch
    assert _resolve(emu, [(A, 4, False), (A, 4, False)], 1) == NONE


def test_hit_resolution_random_against_a_scan(emu):
    rng = np.random.default_rng(11)
    for _ in range(50):
        n = int(rng.integers(1, 80))
        votes = [(int(k), int(k) % 3, bool(a)) for k, a in zip(rng.integers(0, 7, n), rng.integers(0, 2, n))]
        for i in range(n):
            exp = max([j for j in range(i) if votes[j][2] and votes[j][0] == votes[i][0]], default=NONE)
            assert _resolve(emu, votes, i) == exp
