"""TXV_POOL_SENDERS on the host pool: txv_pool_check_keys_from / txv_pool_sent_by with ctx = NULL
(no GPU) against a sequential model of the reference with MempoolTxVote.Senders
(tests/senders_model.py), whose statuses are asserted equal to the oracle pool's on every stream.

Reference: txvotepool/txvotepool.go:213-227 (ErrTxInCache with the key still in txsMap: the
sender joins that entry's Senders), :250 (the admitting sender), :275-284 / :329-359 (Update
removes entries, sets included), :146-159 (Flush); txvotepool/reactor.go:245 (the one reader)."""
import zlib

import numpy as np
import pytest

import oracle as O
import txflow_amd as T
from senders_model import ENCODING, IN_CACHE, NO_CACHE, OK, PEERS, Model, stream


def key(i):
    k = np.zeros(32, np.uint8)
    k[:8] = np.frombuffer(int(i).to_bytes(8, "little"), np.uint8)
    k[31] = 0xA5
    return k


def keys_of(ids):
    return np.stack([key(i) for i in ids])


def sent(pool, ids, peers):
    return [sorted(int(p) for p, b in zip(peers, row) if b) for row in pool.sent_by(keys_of(ids), peers)]


# name, cache_size, pool size, wal, zero_frac, big_frac, batch sizes (below 4096: the sequential loop;
# above: batch_check, unless a cap may bind), replay
STREAMS = [
    ("nocache", NO_CACHE, 1 << 20, False, 0.0, 0.0, [1, 37, 3000, 5000, 700, 4500], 0.30),
    ("cache2", 2, 1 << 20, False, 0.0, 0.0, [1, 2, 250, 4200, 3000, 5000], 0.30),
    ("cache8", 8, 1 << 20, False, 0.0, 0.0, [5, 1000, 4097, 2999, 6000], 0.30),
    ("cache10000", 10000, 1 << 20, False, 0.0, 0.0, [3000, 5000, 1, 4100, 2500, 6000], 0.30),
    ("cache10000_wal_zero_big", 10000, 1 << 20, True, 0.03, 0.02, [2000, 5000, 4100], 0.30),
    ("cache8_pool_fills", 8, 6000, False, 0.0, 0.0, [3000, 5000, 4500, 2000], 0.30),
]


@pytest.mark.parametrize("case", STREAMS, ids=[c[0] for c in STREAMS])
def test_streams_match_the_model(case):
    name, cache, size, wal, zero, big, batches, replay = case
    O.build()
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pool = T.TxVotePool(None, size=size, cache_size=cache, wal=wal, senders=True)
    twin = T.TxVotePool(None, size=size, cache_size=cache, wal=wal)            # no flag, the plain calls
    opool = O.Pool(size=size, cache_size=cache, wal=wal)
    model = Model(size=size, cache_size=cache, wal=wal)
    seen = np.zeros((0, 32), np.uint8)
    flushed = False
    for b, (keys, sizes, snd) in enumerate(stream(rng, batches, replay, zero, big)):
        where = f"{name} batch {b} (n={len(sizes)})"
        st = pool.check_keys(keys, sizes, senders=snd)
        mst = model.check(keys, sizes, snd)
        assert np.array_equal(mst, opool.check_keys(keys, sizes)), f"{where}: the model left the oracle"
        assert np.array_equal(st, mst), f"{where}: statuses"
        assert np.array_equal(twin.check_keys(keys, sizes), st), f"{where}: the flag changed a status"
        seen = np.unique(np.concatenate([seen, keys]), axis=0)
        got, exp = pool.sent_by(seen, PEERS), model.sent_by(seen)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, f"{where}: {bad.size} rows differ, first key {bad[0]}: {got[bad[0]]} vs {exp[bad[0]]}"
        assert pool.Size() == twin.Size() == model.n_live and pool.TxsBytes() == twin.TxsBytes() == model.txs_bytes, where
        rk, rs = pool.reap(-1)
        tk, ts = twin.reap(-1)
        assert np.array_equal(rk, tk) and np.array_equal(rs, ts), f"{where}: reap order"
        assert [k.tobytes() for k in rk] == model.reap_keys(), where
        assert np.array_equal(pool.cache_keys(), twin.cache_keys()), f"{where}: cache keys"
        # Update between batches: a third of the pool's entries and a few keys it never held
        if b % 2 == 0 and len(rk):
            pick = rng.random(len(rk)) < 0.34
            uk = np.concatenate([rk[pick], rng.integers(0, 256, size=(3, 32), dtype=np.uint8)])
            us = np.concatenate([rs[pick], np.full(3, 150, np.uint32)])
            for q in (pool, twin, opool):
                q.update_keys(b + 1, uk, us)
            model.update(uk, us)
            assert np.array_equal(pool.sent_by(seen, PEERS), model.sent_by(seen)), f"{where}: after Update"
        elif not flushed and b >= 2:
            flushed = True
            for q in (pool, twin, opool, model):
                q.flush()
            assert not pool.sent_by(seen, PEERS).any(), f"{where}: Flush empties every set"
    for q in (pool, twin):
        q.close()


def test_replay_of_a_committed_vote_records_nothing():
    pool = T.TxVotePool(None, senders=True)
    k, sz = keys_of([1]), np.array([120], np.uint32)
    assert pool.check_keys(k, sz, senders=[1])[0] == OK
    assert sent(pool, [1], [1, 2]) == [[1]]
    pool.update_keys(1, k, sz)
    assert pool.check_keys(k, sz, senders=[2])[0] == IN_CACHE     # cached by the commit, no longer pooled
    assert sent(pool, [1], [1, 2]) == [[]]
    assert pool.Size() == 0
    pool.close()


@pytest.mark.parametrize("pad", [0, 5000], ids=["sequential", "batch_check"])
def test_evicted_and_readmitted_inside_one_batch(pad):
    """CacheSize 2: K admitted by 1, hit by A = 2, evicted by X and Y, admitted again by 4, hit by B = 5,
    all in one batch: txsMap indexes the second entry, whose set is {4, 5} -- never 1 or A"""
    ids = [100, 100, 200, 300, 100, 100] + list(range(1000, 1000 + pad))
    snd = np.array([1, 2, 3, 3, 4, 5] + [7] * pad, np.uint16)
    pool = T.TxVotePool(None, size=1 << 20, cache_size=2, senders=True)
    model = Model(size=1 << 20, cache_size=2)
    k, sz = keys_of(ids), np.full(len(ids), 120, np.uint32)
    st = pool.check_keys(k, sz, senders=snd)
    assert np.array_equal(st, model.check(k, sz, snd))
    assert list(st[:6]) == [OK, IN_CACHE, OK, OK, OK, IN_CACHE]
    peers = [1, 2, 3, 4, 5, 7]
    assert sent(pool, [100, 200, 300], peers) == [[4, 5], [3], [3]]
    # Update removes the indexed (second) entry with its set; the first stays in the list, unindexed
    pool.update_keys(1, keys_of([100]), sz[:1])
    assert sent(pool, [100], peers) == [[]]
    assert pool.Size() == 3 + pad
    pool.close()


def test_a_reused_node_starts_with_an_empty_set():
    pool = T.TxVotePool(None, senders=True)
    sz = np.array([120], np.uint32)
    pool.check_keys(keys_of([1]), sz, senders=[1])
    pool.check_keys(keys_of([1]), sz, senders=[2])               # a hit: {1, 2}
    assert sent(pool, [1], [1, 2, 3]) == [[1, 2]]
    pool.update_keys(1, keys_of([1]), sz)                         # the node goes to the free list ...
    pool.check_keys(keys_of([2]), sz, senders=[3])               # ... and is handed out again
    assert sent(pool, [1, 2], [1, 2, 3]) == [[], [3]]
    pool.close()


def test_wal_and_size_zero_records_nothing():
    pool = T.TxVotePool(None, wal=True, senders=True)
    k, sz = keys_of([1]), np.array([0], np.uint32)
    assert pool.check_keys(k, sz, senders=[1])[0] == ENCODING     # pushed to the cache, never added
    assert pool.check_keys(k, sz, senders=[2])[0] == IN_CACHE     # no entry to join
    assert sent(pool, [1], [1, 2]) == [[]] and pool.Size() == 0
    pool.close()


def test_paths_without_a_sender_record_unknown_peer():
    pool = T.TxVotePool(None, senders=True)
    k, sz = keys_of([1, 2]), np.full(2, 120, np.uint32)
    pool.check_keys(k, sz)                                        # CheckTx: TxInfo{SenderID: UnknownPeerID}
    pool.check_keys(k[:1], sz[:1], senders=[9])
    assert sent(pool, [1, 2], [0, 9]) == [[0, 9], [0]]
    pool.close()


def test_the_set_sheds_dead_entries_and_grows_without_losing_a_pair():
    """a small pool (the set starts at 1024 slots): admit / Update cycles fill it with dead entries'
    words (rebuilt at the same size), then 200 live entries x 30 senders outgrow it (rebuilt larger)"""
    pool = T.TxVotePool(None, size=256, senders=True)
    sz = np.full(200, 120, np.uint32)
    w0, slots0, rb0, _, in_hbm = pool.senders_stats()
    assert (w0, slots0, rb0, in_hbm) == (0, 1024, 0, 0)
    for c in range(8):                                            # 1600 words through a 1024-slot set
        ids = list(range(c * 200, c * 200 + 200))
        pool.check_keys(keys_of(ids), sz, senders=np.full(200, 1 + c, np.uint16))
        assert all(s == [1 + c] for s in sent(pool, ids, [1 + c, 2 + c]))
        pool.update_keys(c + 1, keys_of(ids), sz)
    words, slots, rebuilds, _, _ = pool.senders_stats()
    assert slots == 1024 and rebuilds >= 2 and words <= 512, "dead entries' words must be dropped, not kept"
    ids = list(range(5000, 5200))
    for s in range(30):
        pool.check_keys(keys_of(ids), sz, senders=np.full(200, 100 + s, np.uint16))
    words, slots, rebuilds2, _, _ = pool.senders_stats()
    assert words == 200 * 30 and slots >= 2 * words and rebuilds2 > rebuilds
    peers = list(range(99, 131))
    assert all(s == list(range(100, 130)) for s in sent(pool, ids, peers))
    pool.close()
