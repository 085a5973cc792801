"""The gossip sink: a batch's TxVoteMessages built on the device (txv_gossip_sink_enable /
txv_gossip_msgs; kernels_gossip.hip).

Reference: broadcastTxRoutine (txvotepool/reactor.go:198-265) walks the pool list in order and sends
cdc.MustMarshalBinaryBare(&TxVoteMessage{Tx}) (:247-248) for every entry.  With the sink on, every
batch of the submit ring leaves one entry per non-nil vote in arrival order -- for
txv_submit_checked exactly the votes the pool admitted -- and the messages' bytes in one buffer.
The expected bytes are always oracle.wire_encode (None => TXV_GOSSIP_UNENCODABLE), the expected
admission oracle.Pool.  Every test asserts on every entry at once: the order, idx, flag, len,
off % 16 == 0, the zero padding between messages, n_out and bytes_out."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import oracle as O
import gossip_cases as GC
from test_update_by_set import Grouped, _keys, _pool_state, _assert_list
from test_update_cadence import _stream
from test_store_sink import Stored, _assert_records, _with_keys

CHAIN = b"test_chain_id"
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _batch(votes, with_key=True):
    """votes: oracle-style dicts with the full address / signature bytes; None = a nil entry"""
    import txflow_amd as T
    b = T.VoteBatch.from_votes([None if v is None else
                                T.TxVote(Height=v["height"], TxHash=v["txhash"], Timestamp=(v["ts_sec"], v["ts_nanos"]),
                                         ValidatorAddress=v["addr"], Signature=v["sig"], TxKey=v["txkey"]) for v in votes])
    if not with_key:
        b.txkey = None
    return b


def _expect(votes, with_key=True):
    """[(idx, flag, message bytes)] of the non-nil votes, in arrival order"""
    return [(i,) + GC.expected(v, with_key) for i, v in enumerate(votes) if v is not None]


def _needed(exp):
    return sum((len(e[2]) + 15) // 16 * 16 for e in exp)


def _assert_entries(wb, idx, flag, exp, what):
    """every entry at once: count, order, idx, flag, len, aligned packed offsets, bytes, zero pads"""
    assert wb.n == len(idx) == len(flag) == len(exp), f"{what}: {wb.n} entries, expected {len(exp)}"
    assert idx.tolist() == [e[0] for e in exp], f"{what}: idx / order differ"
    assert flag.tolist() == [e[1] for e in exp], f"{what}: flags differ"
    assert wb.len.tolist() == [len(e[2]) for e in exp], f"{what}: lengths differ"
    buf = wb.wire[:wb.nbytes]
    end = 0
    for k, e in enumerate(exp):
        o = int(wb.off[k])
        assert o % 16 == 0 and o == (end + 15) // 16 * 16, f"{what}: entry {k} at {o}, previous ends at {end}"
        assert not buf[end:o].any(), f"{what}: padding before entry {k} is not zero"
        assert buf[o:o + len(e[2])].tobytes() == e[2], f"{what}: entry {k} (vote {e[0]}): bytes differ"
        end = o + len(e[2])
    assert wb.nbytes == (end + 15) // 16 * 16 == _needed(exp), f"{what}: bytes_out"
    assert not buf[end:].any(), f"{what}: padding behind the last message is not zero"


def _assert_gossip(ctx, tk, votes, what, with_key=True):
    exp = _expect(votes, with_key)
    _assert_entries(*ctx.gossip_msgs(tk), exp, what)
    return exp


@pytest.fixture(scope="module")
def ctx():
    import txflow_amd as T
    c = T.Context(max_batch=4096, max_txs=1024, max_validators=256, table_w=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vals():
    return _keys(4)


@pytest.fixture(scope="module")
def cadence():
    pubs, powers, votes = _stream(random.Random(2026))
    return pubs, powers, _with_keys(votes, random.Random(77))


def _start(ctx, pubs, powers, max_bytes, max_msgs, store=(0, 0), update=0):
    ctx.enable_update_sink(0)
    ctx.enable_store_sink(0, 0)
    ctx.enable_gossip_sink(0, 0)
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()
    ctx.enable_gossip_sink(max_bytes, max_msgs)
    if store[0]:
        ctx.enable_store_sink(*store)
    if update:
        ctx.enable_update_sink(update)


def _edge_batch(rnd):
    """the edge matrix with nil entries in between"""
    votes = []
    for k, v in enumerate(GC.edge_votes(rnd)):
        votes.append(v)
        if k % 4 == 1:
            votes.append(None)
    return [None] + votes + [None]


# ------------------------------------------------------------------ 3. edge matrix
@pytest.mark.parametrize("with_key", [True, False])
def test_edge_matrix(ctx, vals, with_key):
    _, pubs, _ = vals
    _start(ctx, pubs, [1] * 4, 1 << 20, 4096)
    votes = _edge_batch(random.Random(3))
    tk = ctx.submit_votes(_batch(votes, with_key))
    ctx.wait_votes(tk)
    exp = _assert_gossip(ctx, tk, votes, "edge matrix", with_key)
    flags = [e[1] for e in exp]
    assert flags.count(GC.UNENCODABLE) == 6 and flags.count(GC.HOST) == 3 and votes.count(None) > 10
    if with_key:                                              # every encoded message carries its own vote's TxKey
        live = [v for v in votes if v is not None]
        assert all(b"\x1a\x20" + v["txkey"] in e[2] for v, e in zip(live, exp) if e[1] == GC.OK)


# ------------------------------------------------------------------ 4. shapes
@pytest.fixture(scope="module")
def shape_votes():
    """4096 votes over 48 TxHashes of 50 .. 97 bytes (message lengths of every residue mod 16),
    every third one nil"""
    rnd = random.Random(4)
    hashes = [bytes(rnd.choice(b"0123456789ABCDEF") for _ in range(50 + t)) for t in range(48)]
    votes = [None if i % 3 == 2 else GC.vote(rnd, txhash=hashes[rnd.randrange(48)]) for i in range(4096)]
    return votes, _expect(votes)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4096])
def test_shapes(ctx, vals, shape_votes, n):
    _, pubs, _ = vals
    _start(ctx, pubs, [1] * 4, 1 << 20, 4096)
    votes, exp_all = shape_votes
    exp = [e for e in exp_all if e[0] < n]
    tk = ctx.submit_votes(_batch(votes[:n]))
    ctx.wait_votes(tk)
    _assert_entries(*ctx.gossip_msgs(tk), exp, f"n = {n}")
    assert len(exp) == n - n // 3
    if n >= 63:
        assert {15, 0, 1} <= {len(e[2]) % 16 for e in exp}


def test_all_nil_batch(ctx, vals):
    _, pubs, _ = vals
    _start(ctx, pubs, [1] * 4, 1 << 20, 4096)
    tk = ctx.submit_votes(_batch([None] * 70))
    ctx.wait_votes(tk)
    n, nb = ctypes.c_uint32(9), ctypes.c_uint64(9)
    import txflow_amd as T
    assert T.lib().txv_gossip_msgs(ctx._h, tk, None, 0, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(nb)) == 0
    assert (n.value, nb.value) == (0, 0)
    _assert_entries(*ctx.gossip_msgs(tk), [], "all nil")


# ------------------------------------------------------------------ 5. a message of several tiles
def test_long_txhash_spans_tiles(ctx, vals):
    _, pubs, _ = vals
    _start(ctx, pubs, [1] * 4, 1 << 20, 4096)
    rnd = random.Random(5)
    votes = [GC.vote(rnd) for _ in range(9)]
    votes.insert(4, GC.vote(rnd, txhash=GC.rbytes(rnd, 5003)))
    votes.insert(7, GC.vote(rnd, txhash=GC.rbytes(rnd, 1024 - 140)))
    tk = ctx.submit_votes(_batch(votes))
    ctx.wait_votes(tk)
    exp = _assert_gossip(ctx, tk, votes, "long TxHash")
    assert max(len(e[2]) for e in exp) > 5000


# ------------------------------------------------------------------ 6. the pool path
@pytest.mark.parametrize("mode", ["device", "ahead"])
def test_pool_path_admitted_votes(ctx, cadence, mode):
    """check_submit -> submit_checked -> waits over a stream with replays and a small cache.
    "device": each TxFlow batch submitted right after its CheckTx, which is still in the pool
    engine's flight slot; "ahead": ten CheckTx batches submitted first, so the engine's eight flight
    slots are reused and the first batches take their statuses on the host."""
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 4096)
    cfg = dict(size=1 << 20, cache_size=30, max_txs_bytes=1 << 40)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True)
    opool = O.Pool(**cfg)
    parts = [votes[s:s + 20] for s in range(0, len(votes), 20)]
    assert len(parts) >= 12
    ahead = 10 if mode == "ahead" else 1
    batches = [_batch(p) for p in parts]
    ops = [opool.check(p) for p in parts]
    assert sum(int((o != 0).sum()) for o in ops) > 0             # replays the pool rejects
    try:
        ptk = {}

        def flow(j):
            tk = ctx.submit_checked(batches[j], pool, ptk[j])
            assert np.array_equal(pool.check_wait(ptk[j]), ops[j]), f"batch {j}: pool statuses"
            ctx.wait_votes(tk)
            admitted = [v if x == 0 else None for v, x in zip(parts[j], ops[j])]
            exp = _assert_gossip(ctx, tk, admitted, f"{mode}, batch {j}")
            # the host encoder over the admitted votes: the same bytes, message for message
            adm = [v for v in admitted if v is not None]
            if adm:
                hb = _batch(adm)
                hw = T.encode_msgs(hb, txkey=hb.txkey)
                assert [hw.msg(k) for k in range(hw.n)] == [e[2] for e in exp], f"{mode}, batch {j}: txv_encode_msgs"

        for k in range(len(parts)):
            ptk[k] = pool.check_submit(batches[k])
            if k - ahead + 1 >= 0:
                flow(k - ahead + 1)
        for j in range(max(0, len(parts) - ahead + 1), len(parts)):
            flow(j)
    finally:
        pool.close()


# ------------------------------------------------------------------ 7. four in flight
def test_four_in_flight_and_stale_tickets(ctx, cadence):
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 256)
    parts = [[None if (j + k) % 5 == 0 else v for j, v in enumerate(votes[s:s + 32])] for k, s in enumerate(range(0, 32 * 7, 32))]
    for p in parts[:2]:
        ctx.wait_votes(ctx.submit_votes(_batch(p)))
    tks = [ctx.submit_votes(_batch(p)) for p in parts[2:6]]
    with pytest.raises(T.GossipMsgsError) as e:                 # not waited yet
        ctx.gossip_msgs(tks[0])
    assert e.value.rc == T.E_STATE
    for tk in tks:
        ctx.wait_votes(tk)
    for j, tk in enumerate(tks):
        _assert_gossip(ctx, tk, parts[2 + j], f"in-flight batch {j}")
    t5 = ctx.submit_votes(_batch(parts[6]))                     # the ring of four: one of the four slots is reused
    stale = [tk for tk in tks if (tk - 1) % T.SUBMIT_RING == (t5 - 1) % T.SUBMIT_RING]
    assert len(stale) == 1
    with pytest.raises(T.GossipMsgsError) as e:
        ctx.gossip_msgs(stale[0])
    assert e.value.rc == T.E_STATE
    ctx.wait_votes(t5)
    _assert_gossip(ctx, t5, parts[6], "the fifth batch")
    ctx.enable_gossip_sink(0, 0)
    with pytest.raises(T.GossipMsgsError) as e:                 # the sink off
        ctx.gossip_msgs(t5)
    assert e.value.rc == T.E_STATE


# ------------------------------------------------------------------ 8. capacity
def _oracle_results(pubs, powers, votes):
    """statuses (fired bit included) and commit events (vote index, set id, sum) of one first batch"""
    flow = O.Flow(pubs, powers, CHAIN)
    st, sums, fired = flow.add_votes([dict(nil=True) if v is None else v for v in votes])
    ids, first, after = {}, {}, {}
    for i, v in enumerate(votes):
        if v is None:
            continue
        ids.setdefault(v["txhash"], len(ids))
        if st[i] == 0:
            after[v["txhash"]] = int(sums[i])                # an event carries the set's stake after the batch
        if fired[i]:
            first.setdefault(v["txhash"], i)
    ev = sorted((i, ids[t], after[t]) for t, i in first.items())
    return st.astype(np.uint8) | (fired.astype(np.uint8) << 7), ev


@pytest.mark.parametrize("short", ["bytes", "entries"])
def test_capacity_overflow_leaves_txflow_alone(ctx, cadence, short):
    import txflow_amd as T
    pubs, powers, votes = cadence
    big = [None if j % 7 == 3 else v for j, v in enumerate(votes[:60])]
    nxt = votes[60:90]
    exp_big = _expect(big)
    need, n_big = _needed(exp_big), len(exp_big)
    est, eev = _oracle_results(pubs, powers, big)
    assert len(eev) >= 1
    _start(ctx, pubs, powers, need - 16 if short == "bytes" else need, n_big if short == "bytes" else n_big - 1)
    tk = ctx.submit_votes(_batch(big))
    st, ev = ctx.wait_votes(tk)
    assert np.array_equal(st, est)
    assert sorted((int(e["vote_index"]), int(e["tx_index"]), int(e["sum"])) for e in ev) == eev
    with pytest.raises(T.GossipMsgsError) as e:
        ctx.gossip_msgs(tk)
    assert (e.value.rc, e.value.n, e.value.nbytes) == (T.E_CAPACITY, n_big, need)
    # re-enabled with enough room: the next batch reads correctly (TxFlow was not poisoned)
    ctx.enable_gossip_sink(need, n_big)
    tk = ctx.submit_votes(_batch(nxt))
    ctx.wait_votes(tk)
    exp = _assert_gossip(ctx, tk, nxt, "the batch that fits")
    # output arrays too small: the counts, and nothing written
    total = _needed(exp)
    out = np.full(total, 0xAB, np.uint8)
    off = np.full(len(exp), 77, np.uint64); ln = np.full(len(exp), 77, np.uint32)
    idx = np.full(len(exp), 77, np.uint32); fl = np.full(len(exp), 77, np.uint8)
    n, nb = ctypes.c_uint32(), ctypes.c_uint64()
    for cap, msg_cap in ((total - 1, len(exp)), (total, len(exp) - 1)):
        rc = T.lib().txv_gossip_msgs(ctx._h, tk, out.ctypes.data, cap, off.ctypes.data, ln.ctypes.data, idx.ctypes.data,
                                     fl.ctypes.data, msg_cap, ctypes.byref(n), ctypes.byref(nb))
        assert (rc, n.value, nb.value) == (T.E_CAPACITY, len(exp), total)
        assert (out == 0xAB).all() and (off == 77).all() and (ln == 77).all() and (idx == 77).all() and (fl == 77).all()


# ------------------------------------------------------------------ 9. all three sinks on
def test_all_three_sinks_on(ctx, cadence, vals):
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 4096, store=(1 << 20, 256), update=512)
    ref, upd = Stored(pubs, powers), Grouped(pubs, powers)
    cfg = dict(size=1 << 20, cache_size=30, max_txs_bytes=1 << 40)
    pool = T.TxVotePool(ctx, **cfg, device_cache=True)
    opool = O.Pool(**cfg)
    try:
        for k, s in enumerate(range(0, len(votes), 48)):
            part = votes[s:s + 48]
            b = _batch(part)
            ops = opool.check(part)
            adm = [v for v, x in zip(part, ops) if x == 0]
            exp_recs = ref.batch(adm)[0]
            exp_upd = upd.batch(adm)[0]
            if exp_upd:
                opool.update(k + 1, exp_upd)
            ptk = pool.check_submit(b)
            tk = ctx.submit_checked(b, pool, ptk)
            assert np.array_equal(pool.check_wait(ptk), ops)
            ctx.wait_votes(tk)
            _assert_list(ctx.update_list(tk), upd.columns(exp_upd), f"batch {k}")
            _assert_records(ctx.store_records(tk), exp_recs, f"batch {k}")
            _assert_gossip(ctx, tk, [v if x == 0 else None for v, x in zip(part, ops)], f"batch {k}")
            pool.update_fired(ctx, k + 1, tk)
            pool.sync()
            want = (opool.cache_keys().tobytes(),) + tuple(x.tobytes() for x in opool.reap(-1))
            assert _pool_state(pool) == want, f"batch {k}: pool differs from the oracle's"
        # and the edge matrix as in test 3, the other sinks still on
        edge = _edge_batch(random.Random(3))
        tk = ctx.submit_votes(_batch(edge))
        ctx.wait_votes(tk)
        _assert_gossip(ctx, tk, edge, "edge matrix beside the other sinks")
    finally:
        pool.close()
        ctx.enable_update_sink(0)
        ctx.enable_store_sink(0, 0)


# ------------------------------------------------------------------ 10. forced host validator lookup
def test_forced_host_validator_lookup_keeps_the_address(cadence):
    """TXV_HOST_VAL=1 (read at txv_init) makes stage_add look validators up on the host and upload a
    2-byte code instead of the address; with the sink on it must not: an unknown validator's
    address is only in the address column"""
    import txflow_amd as T
    pubs, powers, votes = cadence
    old = os.environ.get("TXV_HOST_VAL")
    os.environ["TXV_HOST_VAL"] = "1"
    try:
        c = T.Context(max_batch=4096, max_txs=1024, max_validators=256, table_w=4)
    finally:
        if old is None:
            del os.environ["TXV_HOST_VAL"]
        else:
            os.environ["TXV_HOST_VAL"] = old
    try:
        c.set_validators(pubs, powers, CHAIN.decode())
        c.enable_gossip_sink(1 << 20, 4096)
        rnd = random.Random(10)
        part = list(votes[:40])
        stranger = dict(part[5], addr=GC.rbytes(rnd, 20), txkey=GC.rbytes(rnd, 32))
        part.insert(17, stranger)
        part.insert(3, None)
        est, _ = _oracle_results(pubs, powers, part)
        tk = c.submit_votes(_batch(part))
        st, _ = c.wait_votes(tk)
        assert np.array_equal(st, est) and st[18] == T.ERR_UNKNOWN_VALIDATOR
        exp = _assert_gossip(c, tk, part, "host validator lookup forced")
        assert exp[17][0] == 18 and stranger["addr"] in exp[17][2]
    finally:
        c.close()


# ------------------------------------------------------------------ 11. a routed batch
def test_routed_batch(ctx, cadence):
    import torch
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 4096)
    rnd = random.Random(11)
    part = [None if j % 9 == 4 else v for j, v in enumerate(votes[:80])]
    b = _batch(part)
    pst = np.array([T.POOL_OK if rnd.random() < 0.85 else T.POOL_ERR_IN_CACHE for _ in range(b.n)], np.uint8)
    bufs, metas = T.route_pack_host(b, pst, 1)
    routed = [v for v, x in zip(part, pst) if x == T.POOL_OK]   # the votes the pool admitted, in arrival order
    assert int(metas[0]["n"]) == len(routed) < len(part) and routed.count(None) > 3
    dev = torch.from_numpy(bufs[0]).to("cuda:0")
    torch.cuda.synchronize()
    tk = ctx.submit_routed(dev.data_ptr(), metas[0])
    ctx.wait_votes(tk)
    _assert_gossip(ctx, tk, routed, "routed batch")
