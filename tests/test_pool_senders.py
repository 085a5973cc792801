"""TXV_POOL_SENDERS with the pool list in HBM (TXV_POOL_DEVICE_CACHE; kernels_senders.hip,
senders_dev.h): the engine's Senders against the sequential model of the reference
(tests/senders_model.py, anchored to the oracle pool's statuses) and against the host pool as a twin.

Reference: txvotepool/txvotepool.go:213-227, :250, :275-284, :329-359, :146-159; reactor.go:245."""
import ctypes
import hashlib
import random
import zlib

import numpy as np
import pytest

import oracle as O
import txflow_amd as T
from senders_model import ENCODING, IN_CACHE, NO_CACHE, OK, PEERS, Model, stream
from test_pool import _batch, vote
from test_pool_senders_host import keys_of, sent

pytestmark = pytest.mark.gpu
ESTATE = -1


@pytest.fixture(scope="module")
def ctx():
    c = T.Context(max_batch=1 << 13, max_txs=1024, max_validators=8)
    yield c
    c.close()


def _same_sets(pool, model, keys, where, peers=PEERS):
    got, exp = pool.sent_by(keys, peers), model.sent_by(keys, peers)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"{where}: {bad.size} rows differ, first key {bad[0]}: {got[bad[0]]} vs {exp[bad[0]]}"


# ---- the engine sweep: keys given, decided on the device -------------------------------------------
# name, cache_size, wal, zero_frac, big_frac (the host file's streams, through the engine)
SWEEP = [("nocache", NO_CACHE, False, 0.0, 0.0), ("cache2", 2, False, 0.0, 0.0), ("cache8", 8, False, 0.0, 0.0),
         ("cache10000", 10000, False, 0.0, 0.0), ("cache10000_wal_zero_big", 10000, True, 0.03, 0.02)]


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_engine_sweep_against_model_and_host_twin(ctx, case):
    """batches of 1, 1023, 1025 and 2500 votes (the 1024-vote tiles crossed), 30 % replays, Updates
    on the host between them (the list and its sets go home and come back) and one Flush; the last
    case with a WAL, Size() == 0 votes (ErrEncoding after the cache push: no entry) and oversize ones"""
    name, cache, wal, zero, big = case
    O.build()
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cfg = dict(size=1 << 20, cache_size=cache, wal=wal)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True, senders=True)
    twin = T.TxVotePool(None, **cfg, senders=True)                    # the host pool of test_pool_senders_host
    opool, model = O.Pool(**cfg), Model(**cfg)
    seen = np.zeros((0, 32), np.uint8)
    try:
        for b, (keys, sizes, snd) in enumerate(stream(rng, [1, 1023, 1025, 2500, 1, 2500, 1025], 0.30, zero, big)):
            where = f"{name} batch {b} (n={len(sizes)})"
            st = pool.check_keys(keys, sizes, senders=snd)
            mst = model.check(keys, sizes, snd)
            assert np.array_equal(mst, opool.check_keys(keys, sizes)), f"{where}: the model left the oracle"
            assert np.array_equal(st, mst), f"{where}: statuses"
            assert np.array_equal(twin.check_keys(keys, sizes, senders=snd), st), where
            seen = np.unique(np.concatenate([seen, keys]), axis=0)
            assert pool.senders_stats()[4] == 1, f"{where}: ran on the host"
            _same_sets(pool, model, seen, where)
            assert np.array_equal(pool.sent_by(seen, PEERS), twin.sent_by(seen, PEERS)), f"{where}: host twin"
            if wal and b in (2, 3, 5):
                assert (st == ENCODING).any() and (st == 2).any(), f"{where}: the stream lost its WAL cases"
            if b in (2, 5):
                rk, rs = pool.reap(-1)
                pick = rng.random(len(rk)) < 0.34
                for q in (pool, twin, opool):
                    q.update_keys(b + 1, rk[pick], rs[pick])
                model.update(rk[pick], rs[pick])
                _same_sets(pool, model, seen, f"{where}: after Update")
            if b == 3:
                for q in (pool, twin, opool, model):
                    q.flush()
                assert not pool.sent_by(seen, PEERS).any(), f"{where}: Flush empties every set"
        assert pool.Size() == model.n_live
    finally:
        pool.close()
        twin.close()


# ---- batches of votes (keys hashed on the GPU), submitted ------------------------------------------
def _votes(rnd, n, hist, replay=0.30):
    out = []
    for _ in range(n):
        if hist and rnd.random() < replay:
            out.append(dict(hist[rnd.randrange(len(hist))] if rnd.random() < 0.5 else hist[-1 - rnd.randrange(min(8, len(hist)))]))
        else:
            out.append(vote(rnd.randbytes(64), ts=(1_700_000_000, 1 + len(hist))))
        hist.append(out[-1])
    return out


def _ks(votes):
    keys = np.stack([np.frombuffer(hashlib.sha256(v["sig"]).digest(), np.uint8) for v in votes])
    sizes = np.array([T.txvote_size(v["height"], len(v["txhash"]), v["ts_sec"], v["ts_nanos"], len(v["addr"]),
                                    len(v["sig"])) for v in votes], np.uint32)
    return keys, sizes


@pytest.mark.parametrize("cache", [8, 10000])
def test_check_submit_with_fused_update(ctx, cache):
    """check_submit(senders=) with two tickets in flight and txv_pool_update_submit fused ahead of
    the next batch, which replays the committed votes: they are removed first, so nothing is recorded"""
    O.build()
    rnd = random.Random(cache)
    cfg = dict(size=1 << 20, cache_size=cache)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True, senders=True)
    opool, model = O.Pool(**cfg), Model(**cfg)
    hist, seen, committed, ck = [], [], [], None
    try:
        pend = []
        for b, n in enumerate([1025, 1, 2500, 1023]):
            votes = [dict(v) for v in committed] + _votes(rnd, n, hist)         # the committed votes replayed first
            keys, sizes = _ks(votes)
            snd = PEERS[[rnd.randrange(len(PEERS)) for _ in votes]]
            bt, _ = _batch(T, votes)
            pend.append((pool.check_submit(bt, senders=snd), keys, sizes, snd))
            if len(pend) == 2 or b == 3:
                for t, k, s, sd in pend:
                    st = pool.check_wait(t)
                    mst = model.check(k, s, sd)
                    assert np.array_equal(mst, opool.check_keys(k, s)) and np.array_equal(st, mst), f"batch {b}"
                    seen.append(k)
                pend = []
                allk = np.unique(np.concatenate(seen), axis=0)
                _same_sets(pool, model, allk, f"cache {cache} batch {b}")
                if ck is not None and cache == 10000:   # the replays of the committed votes were hits of cached,
                    assert not pool.sent_by(ck, PEERS).any(), f"batch {b}"   # no longer pooled keys: nothing recorded
                if b < 3:                                                       # commit a fifth of the pool, device Update
                    committed = rnd.sample(hist, len(hist) // 5)
                    ck, cs = _ks(committed)
                    cb, _ = _batch(T, committed)
                    pool.update_submit(b + 1, cb)
                    opool.update_keys(b + 1, ck, cs)
                    model.update(ck, cs)
        assert pool.Size() == model.n_live
    finally:
        pool.close()


def test_replay_chain_of_one_vote(ctx):
    """one batch of 4096 votes that is a single vote sent by peers cycling 1..5: one admission, 4095
    ErrTxInCache, and the entry holds all five"""
    pool = T.TxVotePool(ctx, size=1 << 20, device_cache=True, senders=True)
    try:
        keys, sizes = np.repeat(keys_of([77]), 4096, axis=0), np.full(4096, 130, np.uint32)
        st = pool.check_keys(keys, sizes, senders=(np.arange(4096) % 5 + 1).astype(np.uint16))
        assert st[0] == OK and (st[1:] == IN_CACHE).all()
        assert sent(pool, [77], [0, 1, 2, 3, 4, 5, 6]) == [[1, 2, 3, 4, 5]]
        assert pool.senders_stats()[0] == 5 and pool.senders_stats()[4] == 1 and pool.Size() == 1
    finally:
        pool.close()


def test_evicted_and_readmitted_inside_one_device_batch(ctx):
    """test_pool_senders_host's named case on the engine, across a tile boundary: the index as
    pd_newcache leaves it points at the later entry; its set is {4, 5}, never 1 or 2"""
    pad = 1100
    ids = [100, 100, 200, 300] + list(range(1000, 1000 + pad)) + [100, 100]
    snd = np.array([1, 2, 3, 3] + [7] * pad + [4, 5], np.uint16)
    pool = T.TxVotePool(ctx, size=1 << 20, cache_size=2, device_cache=True, senders=True)
    model = Model(size=1 << 20, cache_size=2)
    try:
        k, sz = keys_of(ids), np.full(len(ids), 120, np.uint32)
        st = pool.check_keys(k, sz, senders=snd)
        assert np.array_equal(st, model.check(k, sz, snd))
        assert list(st[:4]) + list(st[-2:]) == [OK, IN_CACHE, OK, OK, OK, IN_CACHE]
        assert sent(pool, [100, 200], [1, 2, 3, 4, 5, 7]) == [[4, 5], [3]]
        assert pool.senders_stats()[4] == 1, "the batch ran on the host"
    finally:
        pool.close()


def test_wal_and_size_zero_records_nothing_on_the_engine(ctx):
    """the named case of test_pool_senders_host on the device pool: with a WAL a Size() == 0 vote is
    ErrEncoding after its cache push, so no entry exists, and the ErrTxInCache replays of its key --
    in the same batch and in the next -- find neither an admission in the batch nor the key in the index"""
    pool = T.TxVotePool(ctx, size=1 << 20, wal=True, device_cache=True, senders=True)
    try:
        k = keys_of([1, 1, 2, 1, 2])
        st = pool.check_keys(k, np.array([0, 0, 120, 0, 120], np.uint32), senders=[1, 2, 3, 4, 5])
        assert list(st) == [ENCODING, IN_CACHE, OK, IN_CACHE, IN_CACHE]
        assert pool.senders_stats()[4] == 1, "the batch ran on the host"
        assert sent(pool, [1, 2], [1, 2, 3, 4, 5, 6]) == [[], [3, 5]]
        st = pool.check_keys(keys_of([1]), np.array([0], np.uint32), senders=[6])
        assert list(st) == [IN_CACHE] and sent(pool, [1], [1, 2, 3, 4, 5, 6]) == [[]] and pool.Size() == 1
    finally:
        pool.close()


def test_compaction_moves_the_sets(ctx):
    """Size 64, CacheSize 256 (the residents, pushed again every cycle, are never evicted; a round's
    fresh keys are, long before the round returns).  Four resident votes are admitted first and never committed; every
    cycle replays them from changing peers (so they stay cached and their sets keep growing), admits
    fresh votes, replays some of those, and commits the fresh ones on the device.  The 64k-position
    list compacts about every 1100 cycles, always with the residents alive: their words must arrive
    at their new positions (sn_remap through npos).  Phase 1 (52 admitted + 7 replays per cycle) puts
    the first compaction on an admitting batch; phase 2 (8 admitted + 50 replays) puts the second on
    an ErrTxInCache batch, whose hits then resolve through the compacted list.  The residents' and
    the cycle's sets are compared with the model right after every compaction (and on the way)."""
    rnd = random.Random(3)
    cfg = dict(size=64, cache_size=256)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True, senders=True)
    model = Model(**cfg)
    res = [vote(rnd.randbytes(64), ts=(1_700_000_000, 900_000 + i)) for i in range(4)]
    res_keys, res_sizes = _ks(res)
    res_bt = _batch(T, res)[0]
    rounds = []
    for r in range(40):                     # a round's keys left the cache long before the round returns
        votes = [vote(rnd.randbytes(64), ts=(1_700_000_000, r * 60 + i + 1)) for i in range(52)]
        hit1, hit2 = res + votes[:3], [(res + votes[:8])[i % 12] for i in range(50)]
        rounds.append((_ks(votes), _batch(T, votes)[0], _batch(T, votes[:8])[0], _ks(hit1), _batch(T, hit1)[0],
                       _ks(hit2), _batch(T, hit2)[0]))
    peers = np.arange(0, 19, dtype=np.uint16)

    def run(bt, ks, snd, expect):
        st = pool.check_batch(bt, senders=snd)
        assert np.array_equal(st, model.check(ks[0], ks[1], snd)) and (st == expect).all()

    try:
        for s_ in (1, 2, 3):                # the residents: admitted by 1, replayed by 2 and 3
            run(res_bt, (res_keys, res_sizes), np.full(4, s_, np.uint16), OK if s_ == 1 else IN_CACHE)
        compactions, fell_on, c = 0, [], 0
        while compactions < 2 and c < 2600:
            (keys, sizes), bt52, bt8, ks1, bth1, ks2, bth2 = rounds[c % 40]
            phase2 = compactions >= 1
            steps = [("admit", bt8 if phase2 else bt52, (keys[:8], sizes[:8]) if phase2 else (keys, sizes), OK),
                     ("hit", bth2 if phase2 else bth1, ks2 if phase2 else ks1, IN_CACHE)]
            for kind, bt, ks, expect in steps:
                n = len(ks[1])
                run(bt, ks, (1 + (c + np.arange(n)) % 17).astype(np.uint16), expect)
                n_comp = pool.senders_stats()[3]
                if n_comp != compactions:                       # this batch's enqueue compacted the list
                    compactions = n_comp
                    fell_on.append(kind)
                    assert pool.senders_stats()[4] == 1
                    where = f"cycle {c}: compaction {n_comp} on the {kind} batch"
                    got = pool.sent_by(res_keys, peers)
                    assert (got.sum(axis=1) >= 3).all(), f"{where}: the residents lost their senders"
                    _same_sets(pool, model, np.concatenate([res_keys, keys]), where, peers=peers)
            if c % 400 == 0:
                _same_sets(pool, model, np.concatenate([res_keys, keys]), f"cycle {c}", peers=peers)
            pool.update_submit(c + 1, bt8 if phase2 else bt52)  # the fresh votes leave, decided on the device, alone
            pool.sync()                                         # (Size must be back under the cap for the next batch)
            model.update(*((keys[:8], sizes[:8]) if phase2 else (keys, sizes)))
            c += 1
        assert compactions >= 2 and "hit" in fell_on and "admit" in fell_on, f"{fell_on} after {c} cycles"
        _same_sets(pool, model, res_keys, "at the end", peers=peers)
        assert pool.Size() == 4 == model.n_live
    finally:
        pool.close()


def test_migration_between_host_and_device(ctx):
    """a batch with one 65-byte signature runs on the host, the next on the device: the sets are
    continuous across both moves; sent_by without a ctx after device batches agrees too"""
    rnd = random.Random(9)
    cfg = dict(size=1 << 20, cache_size=10000)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True, senders=True)
    model = Model(**cfg)
    hist, seen = [], []
    try:
        for b in range(4):
            votes = _votes(rnd, 600, hist)
            if b == 1:
                votes[17] = vote(rnd.randbytes(65), ts=(1_700_000_000, 99))       # > 64 bytes: the host path
            keys, sizes = _ks(votes)
            snd = PEERS[[rnd.randrange(len(PEERS)) for _ in votes]]
            bt, long_sigs = _batch(T, votes)
            st = pool.check_batch(bt, long_sigs, senders=snd)
            assert np.array_equal(st, model.check(keys, sizes, snd)), b
            seen.append(keys)
            allk = np.unique(np.concatenate(seen), axis=0)
            if b != 2:
                _same_sets(pool, model, allk, f"batch {b}")
        # after device batches (0, 2 and 3 ran there), with no context: the list comes home first
        bits = np.zeros((len(allk), 1), np.uint32)
        assert T.lib().txv_pool_sent_by(pool._h, None, allk.ctypes.data, len(allk), PEERS.ctypes.data, len(PEERS),
                                        bits.ctypes.data) == 0
        exp = model.sent_by(allk)
        got = (bits[:, 0][:, None] >> np.arange(len(PEERS))[None, :]) & 1
        assert np.array_equal(got.astype(bool), exp)
        votes = _votes(rnd, 600, hist)                                          # and goes up again
        keys, sizes = _ks(votes)
        snd = PEERS[[rnd.randrange(len(PEERS)) for _ in votes]]
        assert np.array_equal(pool.check_batch(_batch(T, votes)[0], senders=snd), model.check(keys, sizes, snd))
        _same_sets(pool, model, np.unique(np.concatenate(seen + [keys]), axis=0), "after the round trip")
    finally:
        pool.close()


def test_the_set_grows_without_losing_a_pair(ctx):
    """a small pool (the set starts at 2048 slots): 200 live entries x 300 distinct sender ids"""
    pool = T.TxVotePool(ctx, size=512, device_cache=True, senders=True)
    try:
        ids = list(range(200))
        keys, sizes = keys_of(ids), np.full(200, 120, np.uint32)
        for s in range(300):
            st = pool.check_keys(keys, sizes, senders=np.full(200, 1000 + s, np.uint16))
            assert (st == (OK if s == 0 else IN_CACHE)).all()
        words, slots, rebuilds, _, in_hbm = pool.senders_stats()
        assert in_hbm == 1, "the batches ran on the host"
        assert words == 200 * 300 and slots >= 2 * words and rebuilds >= 5
        peers = np.arange(990, 1310, dtype=np.uint16)
        got = pool.sent_by(keys, peers)
        assert got[:, 10:310].all() and not got[:, :10].any() and not got[:, 310:].any()
    finally:
        pool.close()


def test_ticket_form(ctx):
    rnd = random.Random(21)
    pool = T.TxVotePool(ctx, size=1 << 20, device_cache=True, senders=True)
    try:
        hist = []
        votes = _votes(rnd, 700, hist)
        keys, _ = _ks(votes)
        snd = PEERS[[rnd.randrange(len(PEERS)) for _ in votes]]
        t = pool.check_submit(_batch(T, votes)[0], senders=snd)
        rows = pool.ticket_sent_by(t, PEERS)                     # finishes the ticket itself
        st = pool.check_wait(t)
        by_key = pool.sent_by(keys, PEERS)
        assert (st == IN_CACHE).any() and rows[st == OK].any(axis=1).all()
        assert np.array_equal(rows[st == OK], by_key[st == OK]) and not rows[st != OK].any()
        assert np.array_equal(pool.ticket_sent_by(t, PEERS, n=700), rows), "after the wait, while the slot holds the batch"
        for _ in range(8):                                       # the ring's eight slots taken by later batches
            pool.check_batch(_batch(T, _votes(rnd, 5, hist))[0])
        bits = np.zeros((700, 1), np.uint32)
        assert T.lib().txv_pool_ticket_sent_by(pool._h, ctx._h, t, PEERS.ctypes.data, len(PEERS), bits.ctypes.data) == ESTATE
        # a ticket decided on the host holds no slot
        host = T.TxVotePool(ctx, senders=True)
        t = host.check_submit(_batch(T, votes)[0], senders=snd)
        assert T.lib().txv_pool_ticket_sent_by(host._h, ctx._h, t, PEERS.ctypes.data, len(PEERS), bits.ctypes.data) == ESTATE
        host.check_wait(t)
        host.close()
    finally:
        pool.close()


def test_wire_receive_and_ingest(ctx):
    """receive(senders=) and the three-phase ingest with txv_ingest_decode_from, three tickets in
    flight, against the model; undecodable messages record nothing; the ingest without _from
    records sender 0"""
    rnd = random.Random(33)
    seeds = [rnd.randbytes(32) for _ in range(4)]
    ctx.set_validators([O.pubkey(s) for s in seeds], [1, 1, 1, 1], "test_chain_id")
    cfg = dict(size=1 << 20, cache_size=10000)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True, senders=True)
    model = Model(**cfg)
    hist, seen = [], []

    def wire(n):
        votes = _votes(rnd, n, hist)
        msgs = [O.wire_encode(v["height"], v["txhash"], v["ts_sec"], v["ts_nanos"], v["addr"], v["sig"]) for v in votes]
        bad = sorted(rnd.sample(range(n), 5))
        for i in bad:
            msgs[i] = msgs[i][:-3]
        keys, sizes = _ks(votes)
        snd = PEERS[[rnd.randrange(len(PEERS)) for _ in votes]]
        good = np.setdiff1d(np.arange(n), bad)
        return T.WireBatch(msgs), keys, sizes, snd, good

    def expect(ps, keys, sizes, snd, good, where):
        mst = model.check(keys[good], sizes[good], snd[good] if snd is not None else None)
        assert np.array_equal(ps[good], mst) and (np.delete(ps, good) == T.POOL_NOT_CHECKED).all(), where
        seen.append(keys)
        _same_sets(pool, model, np.unique(np.concatenate(seen), axis=0), where)

    try:
        wb, keys, sizes, snd, good = wire(400)
        ws, ps = pool.receive(wb, senders=snd)
        expect(ps, keys, sizes, snd, good, "receive")
        batches = [wire(300) for _ in range(3)]
        tks = [pool.ingest_decode(b[0], senders=b[3]) for b in batches]          # three tickets in flight
        for tk, (wb, keys, sizes, snd, good) in zip(tks, batches):
            pool.ingest_admit_submit(tk)
            pool.ingest_admit_finish(tk)
            expect(tk.pool_status, keys, sizes, snd, good, "ingest")
        for tk in tks:
            pool.ingest_wait(tk)
        wb, keys, sizes, snd, good = wire(300)                                   # no _from: UnknownPeerID
        tk = pool.ingest_admit(pool.ingest_decode(wb))
        pool.ingest_wait(tk)
        expect(tk.pool_status, keys, sizes, None, good, "ingest without senders")
    finally:
        pool.close()


def test_routed_batches_record_unknown_peer(ctx):
    import torch
    rnd = random.Random(44)
    votes = [vote(rnd.randbytes(64), txhash=b"AB" * 32, ts=(1_700_000_000, i + 1)) for i in range(300)]
    vs = [T.TxVote(Height=v["height"], TxHash=v["txhash"].decode(), Timestamp=(v["ts_sec"], v["ts_nanos"]),
                   ValidatorAddress=v["addr"], Signature=v["sig"]) for v in votes]
    b = T.VoteBatch.from_votes(vs)
    b.is_nil = None
    b.txkey = None
    bufs, metas = T.route_pack_host(b, None, 1)
    dev = torch.from_numpy(bufs[0][:int(metas[0]["bytes"])].copy()).to("cuda:0")
    torch.cuda.synchronize()
    pool = T.TxVotePool(ctx, size=1 << 20, device_cache=True, senders=True)
    try:
        st = pool.check_wait(pool.check_routed_submit(dev.data_ptr(), metas[0]))
        assert (st == OK).all()
        got = pool.sent_by(_ks(votes)[0], PEERS)
        assert got[:, 0].all() and not got[:, 1:].any(), "every admitted vote's set is {0}"
    finally:
        pool.close()
