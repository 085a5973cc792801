"""TxVotePool.Update's argument built on the device (txv_update_sink_enable / txv_update_list /
txv_pool_update_fired; kernels_update.hip).

Reference: after every fired vote the commit path runs txV.Update(height, set.GetVotes())
(txflow/service.go:216-227 -> txvotepool/txvotepool.go:329-359).  tests/test_update_cadence.py
shows on the oracle that one Update per batch with the "grouped" list -- the sets that fired in the
batch, ordered by the arrival index of their last fired vote, each set's accepted votes so far in
arrival order as one block -- leaves the pool exactly as that cadence does.  Here the expected
list is computed from the oracle TxFlow exactly as test_update_cadence._run("grouped") does, the
expected TxVote.Size() with txv_txvote_size, and the list the device leaves after each batch must
equal it byte for byte and in order."""
import hashlib
import random
import struct

import numpy as np
import pytest

import oracle as O
from test_update_cadence import _stream

CHAIN = b"test_chain_id"
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _keys(n_vals, tag=b"upd-by-set"):
    seeds = [hashlib.sha512(tag + struct.pack("<I", i)).digest()[:32] for i in range(n_vals)]
    pubs = [O.pubkey(s) for s in seeds]
    return seeds, pubs, [O.sha256(p)[:20] for p in pubs]


def _vote(seeds, addrs, v, txhash, nanos, height=1, sec=1_700_000_000):
    msg = O.signbytes(height, txhash, sec, nanos, CHAIN)
    return dict(height=height, txhash=txhash, ts_sec=sec, ts_nanos=nanos, addr=addrs[v], sig=O.sign(seeds[v], msg))


def _batch(votes):
    """oracle-style dicts (None: a nil entry) -> VoteBatch"""
    import txflow_amd as T
    return T.VoteBatch.from_votes([None if v is None else
                                   T.TxVote(Height=v["height"], TxHash=v["txhash"], Timestamp=(v["ts_sec"], v["ts_nanos"]),
                                            ValidatorAddress=v["addr"], Signature=v["sig"]) for v in votes])


class Grouped:
    """the oracle TxFlow and, per batch, the grouped Update list (test_update_cadence._run)"""

    def __init__(self, pubs, powers):
        self.flow = O.Flow(pubs, powers, CHAIN)
        self.added = {}                  # TxHash -> its ADDED votes in arrival order (GetVotes)
        self.ids = {}                    # TxHash -> set id (first-seen order)
        self.fired_before = set()

    def batch(self, votes):
        """votes reaching TxFlow, in arrival order -> (Update list, statuses, fired flags, info)"""
        st, _, fired = self.flow.add_votes(votes)
        last, touched = {}, set()
        for j, v in enumerate(votes):
            self.ids.setdefault(v["txhash"], len(self.ids))
            if st[j] == 0:
                self.added.setdefault(v["txhash"], []).append(v)
                touched.add(v["txhash"])
            if fired[j]:
                last[v["txhash"]] = j
        upd = [u for t in sorted(last, key=last.get) for u in self.added[t]]
        info = dict(refired=len(set(last) & self.fired_before), unfired=len(touched - set(last)), sets=len(last))
        self.fired_before |= set(last)
        return upd, st, fired, info

    def columns(self, upd):
        import txflow_amd as T
        sig = np.frombuffer(b"".join(u["sig"] for u in upd), np.uint8).reshape(len(upd), 64)
        size = np.array([T.txvote_size(u["height"], len(u["txhash"]), u["ts_sec"], u["ts_nanos"], 20, 64) for u in upd],
                        np.uint32)
        sets = np.array([self.ids[u["txhash"]] for u in upd], np.uint32)
        return sig, size, sets


def _assert_list(got, exp, what):
    gsig, gsize, gset = got
    esig, esize, eset = exp
    assert len(gsize) == len(esize), f"{what}: {len(gsize)} entries, expected {len(esize)}"
    assert np.array_equal(gset, eset), f"{what}: set ids / block order differ"
    assert np.array_equal(gsig, esig), f"{what}: signatures differ"
    assert np.array_equal(gsize, esize), f"{what}: TxVote.Size() differs"


def _pool_state(pool):
    keys, sizes = pool.reap(-1)
    return pool.cache_keys().tobytes(), keys.tobytes(), sizes.tobytes()


@pytest.fixture(scope="module")
def ctx():
    import txflow_amd as T
    c = T.Context(max_batch=4096, max_txs=1024, max_validators=256, table_w=4)   # small tables: 130 keys build fast
    yield c
    c.close()


@pytest.fixture(scope="module")
def cadence():
    """test_update_cadence's stream: 6 validators with powers 1-3, 40 txs, replays"""
    return _stream(random.Random(2026))


def _start(ctx, pubs, powers, max_entries):
    ctx.enable_update_sink(0)
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()
    ctx.enable_update_sink(max_entries)


# ------------------------------------------------------------------ 1. cadence stream
def test_cadence_stream_lists(ctx, cadence):
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 512)
    ref = Grouped(pubs, powers)
    empty = refired = unfired = 0
    # a first batch of 3 votes (stake <= 8 of the 9 needed: nothing can fire), then batches of 48
    cuts = [0, 3] + list(range(51, len(votes) + 48, 48))
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        part = votes[lo:hi]
        exp, est, efired, info = ref.batch(part)
        tk = ctx.submit_votes(_batch(part))
        st, _ = ctx.wait_votes(tk)
        assert np.array_equal(st, est.astype(np.uint8) | (efired.astype(np.uint8) << 7))
        _assert_list(ctx.update_list(tk), ref.columns(exp), f"batch {k}")
        empty += not exp
        refired += info["refired"]
        unfired += info["unfired"]
    # a batch with nothing fired (n == 0), sets that re-fire whole in a later batch, sets that got
    # votes but no 2/3 (absent from that batch's list)
    assert empty >= 1 and refired >= 1 and unfired >= 1


# ------------------------------------------------------------------ 2. pool parity
@pytest.mark.parametrize("device_cache", [True, False], ids=["device_cache", "host_cache"])
def test_pool_parity(ctx, cadence, device_cache):
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 512)
    cfg = dict(size=1 << 20, cache_size=30, max_txs_bytes=1 << 40)
    pool = T.TxVotePool(ctx, **cfg, device_cache=device_cache)
    twin = T.TxVotePool(ctx, **cfg, device_cache=device_cache)
    opool = O.Pool(**cfg)
    ref = Grouped(pubs, powers)
    applied = 0
    try:
        for k, s in enumerate(range(0, len(votes), 48)):
            part = votes[s:s + 48]
            b = _batch(part)
            ops = opool.check(part)
            exp, _, _, _ = ref.batch([v for v, x in zip(part, ops) if x == 0])
            if exp:
                opool.update(k + 1, exp)
            # the device path: CheckTx -> TryAddVote behind it -> Update with the batch's device list
            ptk = pool.check_submit(b)
            tk = ctx.submit_checked(b, pool, ptk)
            assert np.array_equal(pool.check_wait(ptk), ops)
            ctx.wait_votes(tk)
            _assert_list(ctx.update_list(tk), ref.columns(exp), f"batch {k}")
            pool.update_fired(ctx, k + 1, tk)
            assert pool.Height() == k + 1
            pool.sync()
            # the twin: the same CheckTx, Update with the host-gathered batch
            assert np.array_equal(twin.check_batch(b), ops)
            if exp:
                twin.update_submit(k + 1, _batch(exp))
            twin.sync()
            want = (opool.cache_keys().tobytes(),) + tuple(x.tobytes() for x in opool.reap(-1))
            assert _pool_state(pool) == want, f"batch {k}: pool differs from the oracle's"
            assert _pool_state(twin) == want, f"batch {k}: twin differs from the oracle's"
            assert pool.Size() == twin.Size() == opool.size()
            assert pool.TxsBytes() == twin.TxsBytes() == opool.txs_bytes()
            applied += len(exp)
        assert applied > 100 and len(opool.cache_keys()) == 30      # evictions happened inside the Updates
    finally:
        pool.close()
        twin.close()


# ------------------------------------------------------------------ 3. 130 validators
def test_130_validators_block_in_sequence_order(ctx):
    seeds, pubs, addrs = _keys(130)
    powers = [1] * 130                                   # quorum 87
    _start(ctx, pubs, powers, 256)
    ref = Grouped(pubs, powers)
    tx = hashlib.sha256(b"wide-tx").hexdigest().upper().encode()
    other = hashlib.sha256(b"narrow-tx").hexdigest().upper().encode()
    order = list(range(130))
    random.Random(7).shuffle(order)                      # arrival order against validator order
    votes = [_vote(seeds, addrs, v, tx, i + 1) for i, v in enumerate(order)]
    parts = [votes[:50] + [_vote(seeds, addrs, 3, other, 900)], votes[50:100], votes[100:]]
    sizes = []
    for k, part in enumerate(parts):
        exp, _, _, _ = ref.batch(part)
        tk = ctx.submit_votes(_batch(part))
        ctx.wait_votes(tk)
        got = ctx.update_list(tk)
        _assert_list(got, ref.columns(exp), f"batch {k}")
        sizes.append(len(exp))
    assert sizes == [0, 100, 130]
    # the block is in sequence order, which is not validator order
    assert [addrs.index(u["addr"]) for u in exp] == order and order != sorted(order)


# ------------------------------------------------------------------ 4. Size() edges
def test_size_edges(ctx):
    seeds, pubs, addrs = _keys(4)
    powers = [1, 1, 1, 1]                                # quorum 3
    _start(ctx, pubs, powers, 512)
    ref = Grouped(pubs, powers)
    votes, nanos = [], 1
    for hl in (5, 64, 127, 128, 200):                    # 200: the overflow key arena
        for height in (127, 128):                        # the height varint's 1 -> 2 byte step
            for sec, ns in ((1_700_000_000, None), (1_700_000_000, 0), (0, None), (0, 0)):
                txhash = (b"%05d" % (len(votes) // 4)).ljust(hl, b"X")   # one tx per (length, height, time) case
                for v in range(4):
                    votes.append(_vote(seeds, addrs, v, txhash, nanos if ns is None else 0, height=height, sec=sec))
                    nanos += 1
    assert len({v["txhash"] for v in votes}) == 40
    random.Random(11).shuffle(votes)
    for k, s in enumerate(range(0, len(votes), 64)):
        part = votes[s:s + 64]
        exp, est, _, _ = ref.batch(part)
        assert (est == 0).all()
        tk = ctx.submit_votes(_batch(part))
        ctx.wait_votes(tk)
        _assert_list(ctx.update_list(tk), ref.columns(exp), f"batch {k}")
    sizes = ref.columns([u for t in ref.added for u in ref.added[t]])[1]
    assert len(set(sizes.tolist())) > 10


# ------------------------------------------------------------------ 5. four in flight
def test_four_in_flight_and_stale_tickets(ctx, cadence):
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 512)
    ref = Grouped(pubs, powers)
    parts = [votes[s:s + 32] for s in range(0, 32 * 7, 32)]
    assert len(parts[-1]) == 32
    exps = [ref.columns(ref.batch(p)[0]) for p in parts]
    assert sum(len(e[1]) > 0 for e in exps[2:6]) >= 2
    for p in parts[:2]:                                  # sets open before the four batches in flight
        ctx.wait_votes(ctx.submit_votes(_batch(p)))
    tks = [ctx.submit_votes(_batch(p)) for p in parts[2:6]]
    with pytest.raises(T.UpdateListError) as e:          # not waited yet
        ctx.update_list(tks[0])
    assert e.value.rc == T.E_STATE
    for tk in tks:
        ctx.wait_votes(tk)
    for j, tk in enumerate(tks):                         # every list is as of its own batch
        _assert_list(ctx.update_list(tk), exps[2 + j], f"in-flight batch {j}")
    t5 = ctx.submit_votes(_batch(parts[6]))              # the ring of four: one of the four slots is reused
    stale = [tk for tk in tks if (tk - 1) % T.SUBMIT_RING == (t5 - 1) % T.SUBMIT_RING]
    assert len(stale) == 1
    with pytest.raises(T.UpdateListError) as e:
        ctx.update_list(stale[0])
    assert e.value.rc == T.E_STATE
    ctx.wait_votes(t5)
    _assert_list(ctx.update_list(t5), exps[6], "the fifth batch")
    ctx.enable_update_sink(0)
    with pytest.raises(T.UpdateListError) as e:          # the sink off
        ctx.update_list(t5)
    assert e.value.rc == T.E_STATE


# ------------------------------------------------------------------ 6. capacity
def test_capacity_overflow_leaves_txflow_and_pool_alone(ctx):
    import txflow_amd as T
    seeds, pubs, addrs = _keys(6)
    powers = [1] * 6                                     # quorum 5
    hashes = [hashlib.sha256(b"cap-tx%d" % t).hexdigest().upper().encode() for t in range(3)]
    big = [_vote(seeds, addrs, v, hashes[t], 1 + 6 * t + v) for t in range(2) for v in range(6)]
    fits = [_vote(seeds, addrs, v, hashes[2], 100 + v) for v in range(6)]
    # the same batches with the sink off: the statuses and events to expect
    ctx.enable_update_sink(0)
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()
    st_off, ev_off = ctx.wait_votes(ctx.submit_votes(_batch(big)))
    _start(ctx, pubs, powers, 8)
    ref = Grouped(pubs, powers)
    exp_big = ref.batch(big)[0]
    assert len(exp_big) == 12
    pool = T.TxVotePool(ctx, size=1 << 20, cache_size=30, max_txs_bytes=1 << 40, device_cache=True)
    try:
        assert (pool.check_batch(_batch(big + fits)) == T.POOL_OK).all()
        before = _pool_state(pool), pool.Size(), pool.TxsBytes(), pool.Height()
        tk = ctx.submit_votes(_batch(big))
        st, ev = ctx.wait_votes(tk)
        assert np.array_equal(st, st_off) and np.array_equal(ev, ev_off) and len(ev) == 2
        with pytest.raises(T.UpdateListError) as e:
            ctx.update_list(tk)
        assert (e.value.rc, e.value.n) == (T.E_CAPACITY, 12)
        with pytest.raises(T.UpdateListError) as e:
            pool.update_fired(ctx, 9, tk)
        assert (e.value.rc, e.value.n) == (T.E_CAPACITY, 12)
        pool.sync()
        assert (_pool_state(pool), pool.Size(), pool.TxsBytes(), pool.Height()) == before
        # the next batch, which fits, works (TxFlow was not poisoned)
        exp = ref.batch(fits)[0]
        tk = ctx.submit_votes(_batch(fits))
        ctx.wait_votes(tk)
        _assert_list(ctx.update_list(tk), ref.columns(exp), "the batch that fits")
        pool.update_fired(ctx, 10, tk)
        pool.sync()
        assert pool.Size() == 12 and pool.Height() == 10
    finally:
        pool.close()


# ------------------------------------------------------------------ 7. multi-tile
def test_multi_tile_offsets(ctx):
    seeds, pubs, addrs = _keys(6)
    powers = [1 + (i % 3) for i in range(6)]
    _start(ctx, pubs, powers, 4096)
    ref = Grouped(pubs, powers)
    rnd = random.Random(5)
    hashes = [hashlib.sha256(b"tile-tx%d" % t).hexdigest().upper().encode() for t in range(400)]
    pairs = [(t, v) for t in range(400) for v in range(6)]
    rnd.shuffle(pairs)
    votes = [_vote(seeds, addrs, v, hashes[t], i + 1) for i, (t, v) in enumerate(pairs)]
    for _ in range(100):                                 # replays: 2,500 votes, 3 scan tiles
        votes.insert(rnd.randrange(1, len(votes)), dict(votes[rnd.randrange(len(votes))]))
    assert len(votes) == 2500
    exp, _, _, info = ref.batch(votes)
    assert info["sets"] > 300 and len(exp) > 1500
    tk = ctx.submit_votes(_batch(votes))
    ctx.wait_votes(tk)
    _assert_list(ctx.update_list(tk), ref.columns(exp), "the 2,500-vote batch")


# ------------------------------------------------------------------ 8. large-batch path
def test_large_batch_compacted_stamps():
    """one batch of 2^18 votes: txv_flow_tally lists its stamped sets by compaction there, and the
    list builder takes the compaction's total as n_stamped"""
    import txflow_amd as T
    from txflow_amd.workload import Workload, SEEDS
    m = 1 << 18
    c = T.Context(max_batch=m, max_txs=4096, max_validators=128)
    try:
        wl = Workload(c, 100, 2622, SEEDS["c2"] + 3)
        c.enable_update_sink(m)
        b = wl.head(m)
        tk = c.submit_votes(b)
        st, ev = c.wait_votes(tk)
        sig, size, sets = c.update_list(tk)
        # the host-gathered list (bench.c5_commit_updates' recipe) from the batch's statuses
        tx_of = wl.tx_of[:m].astype(np.int64)
        added = np.nonzero((st & 0x7F) == T.ADDED)[0]
        fired = np.nonzero(st & T.STATUS_FIRED)[0]
        assert len(added) == m and len(fired) > m // 4
        last = np.full(wl.n_txs, -1, np.int64)
        last[tx_of[fired]] = fired                        # ascending: the last fired vote wins
        order = np.argsort(last, kind="stable")
        order = order[last[order] >= 0]
        by_tx = added[np.argsort(tx_of[added], kind="stable")]
        cut = np.searchsorted(tx_of[by_tx], np.arange(wl.n_txs + 1))
        idx = np.concatenate([by_tx[cut[t]:cut[t + 1]] for t in order])
        first_seen = np.full(wl.n_txs, -1, np.int64)     # set ids: first-seen order
        u, f = np.unique(tx_of, return_index=True)
        first_seen[u[np.argsort(f)]] = np.arange(len(u))
        esig = b.sig.reshape(m, 64)[idx]
        assert len(size) == len(idx)
        assert np.array_equal(sets, first_seen[tx_of[idx]].astype(np.uint32))       # the block boundaries
        key = lambda rows: sorted(hashlib.sha256(r.tobytes()).digest() for r in rows)   # noqa: E731
        assert key(sig) == key(esig)                                                 # the key multiset
        for sl in (slice(0, 1000), slice(-1000, None)):                              # full order at both ends
            assert np.array_equal(sig[sl], esig[sl])
        nanos = b.ts_nanos[idx]                           # 1 .. 2^18: a 1-, 2- or 3-byte varint
        s1, s2, s3 = (T.txvote_size(1, 64, 1_700_000_000, x, 20, 64) for x in (100, 10_000, 100_000))
        assert np.array_equal(size, np.where(nanos < 128, s1, np.where(nanos < 16384, s2, s3)).astype(np.uint32))
    finally:
        c.close()


# ------------------------------------------------------------------ 9. a routed batch
def test_routed_batch_list(ctx, cadence):
    """the list behind plain txv_submit_routed: the batch routed as one shard into a buffer in this
    device's HBM and submitted from there"""
    import torch
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 512)
    ref = Grouped(pubs, powers)
    part = votes[:64]
    exp, est, efired, info = ref.batch(part)
    assert info["sets"] >= 2 and info["unfired"] >= 1
    b = _batch(part)
    stride = T.route_stride(b)
    dev = torch.zeros(stride, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    metas = ctx.route_admitted(b, None, 1, dev.data_ptr(), stride)
    assert int(metas[0]["n"]) == len(part)
    tk = ctx.submit_routed(dev.data_ptr(), metas[0])
    st, _ = ctx.wait_votes(tk)
    assert np.array_equal(st, est.astype(np.uint8) | (efired.astype(np.uint8) << 7))
    _assert_list(ctx.update_list(tk), ref.columns(exp), "routed batch")
