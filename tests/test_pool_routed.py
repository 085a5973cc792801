"""CheckTx and TryAddVote from a route buffer in HBM (include/txvote.h txv_pool_check_routed_submit /
txv_pool_check_routed / txv_submit_routed_checked / txv_sign_txs_meta; kernels_routepool.hip).

Reference: signTxRoutine hands each vote it signed to txVotePool.CheckTx (txvotepool/reactor.go:126 ->
txvotepool.go:180-261); checkMaj23Routine hands the pool's votes to TryAddVote.

Every expected value comes from the oracle (O.Pool, O.Flow, O.wire_encode, O.sign) and from the
library's existing host paths (a twin TxVotePool fed the same votes through check_batch); every
comparison is exact.  The buffers are built by T.route_pack_host from oracle-signed votes and
uploaded into a torch uint8 tensor."""
import random

import numpy as np
import pytest

import oracle as O
import txflow_amd as T
from test_pool_batch import _check_equal

pytestmark = pytest.mark.gpu

CHAIN = "test_chain_id"
_rnd = random.Random(1126)
SEEDS = [bytes(_rnd.getrandbits(8) for _ in range(32)) for _ in range(5)]     # four validators and an outsider
POWERS = [1, 1, 1, 2]
N_HASH = 150                       # x 4 validators = 600 signed votes
NIL_ST = T.ERR_NIL
NC = T.POOL_NOT_CHECKED


@pytest.fixture(scope="module")
def signed():
    """600 oracle-signed votes, validator-major within each TxHash: computed once"""
    O.build()
    rnd = random.Random(7)
    pubs = [O.pubkey(s) for s in SEEDS[:4]]
    addrs = [O.sha256(p)[:20] for p in pubs]
    votes = []
    for j in range(N_HASH):
        th = "".join(rnd.choice("0123456789ABCDEF") for _ in range(64)).encode()
        for v in range(4):
            ts = (1_700_000_000 + j, 1 + 4 * j + v)
            sig = O.sign(SEEDS[v], O.signbytes(1, th, ts[0], ts[1], CHAIN.encode()))
            votes.append(dict(height=1, txhash=th, ts_sec=ts[0], ts_nanos=ts[1], addr=addrs[v], sig=sig))
    return pubs, votes


@pytest.fixture(scope="module")
def dev_ctx(signed):
    ctx = T.Context(max_batch=1 << 12, max_txs=1024, max_validators=8)
    ctx.set_validators(signed[0], POWERS, CHAIN)
    yield ctx
    ctx.close()


def _batch(votes):
    """oracle-style dicts (None: a nil entry) -> VoteBatch; no nil column without a nil entry"""
    b = T.VoteBatch.from_votes([None if v is None else
                                T.TxVote(Height=v["height"], TxHash=v["txhash"].decode(), Timestamp=(v["ts_sec"], v["ts_nanos"]),
                                         ValidatorAddress=v["addr"], Signature=v["sig"]) for v in votes])
    if all(v is not None for v in votes):
        b.is_nil = None
    b.txkey = None
    return b


def _upload(votes, spare=0):
    """the votes' route buffer in HBM: (tensor, meta)"""
    import torch
    bufs, metas = T.route_pack_host(_batch(votes), None, 1)
    k = int(metas[0]["bytes"])
    host = np.concatenate([bufs[0][:k], np.full(spare, 0xA5, np.uint8)])
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    return dev, metas[0]


def _checked(v):
    return v is not None and len(v["sig"]) <= 64


def _oracle_status(opool, votes):
    """the oracle pool run on the votes that reach CheckTx; TXV_POOL_NOT_CHECKED for the others"""
    idx = [i for i, v in enumerate(votes) if _checked(v)]
    st = np.full(len(votes), NC, np.uint8)
    st[idx] = opool.check([votes[i] for i in idx])
    return st


def _twin_feed(twin, votes):
    live = [v for v in votes if _checked(v)]
    if live:
        twin.check_batch(_batch(live))


def _same_state(pool, twin, where):
    assert pool.Size() == twin.Size() and pool.TxsBytes() == twin.TxsBytes(), where
    a, b = pool.reap(-1), twin.reap(-1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), where
    assert np.array_equal(pool.cache_keys(), twin.cache_keys()), where


def _mix(rnd, n, fresh, earlier):
    """n votes: fresh ones, exact repeats inside the batch, replays of an earlier batch, a vote with
    an un-encodable time, one over a small max_msg_bytes, signatures of 0, 1, 55, 56 and 63 bytes"""
    votes = []
    cut = [0, 1, 55, 56, 63]
    for i in range(n):
        r = i % 16
        v = dict(fresh.pop())
        if r == 3 and votes:
            v = dict(votes[rnd.randrange(len(votes))])
        elif r == 7 and earlier:
            v = dict(earlier[rnd.randrange(len(earlier))])
        elif r == 9:
            v["ts_nanos"] = 10 ** 9                      # amino rejects the time: Size() == 0
        elif r == 11:
            v["txhash"] = b"C" * 127                     # Size() above max_msg_bytes - 8
        elif r >= 12:
            v["sig"] = v["sig"][:cut[(i // 16 + r) % 5]]
        votes.append(v)
    return votes


POOL_CASES = [(n, 10000, False) for n in (1, 63, 64, 65, 255, 256, 257)] + \
             [(257, 8, False), (257, 64, False), (257, 10000, True), (65, 8, True)]


@pytest.mark.parametrize("n,cache,wal", POOL_CASES, ids=[f"n{n}-c{c}{'-wal' if w else ''}" for n, c, w in POOL_CASES])
def test_status_and_state_parity(dev_ctx, signed, n, cache, wal):
    """two routed batches (the second replays the first) against the oracle pool and a twin pool fed
    the same votes through check_batch: statuses, Size, TxsBytes, pool order and LRU order"""
    rnd = random.Random(n * 31 + cache)
    fresh = list(signed[1])
    rnd.shuffle(fresh)
    cfg = dict(size=1 << 16, cache_size=cache, max_txs_bytes=1 << 30, max_msg_bytes=260, wal=wal)
    pool = T.TxVotePool(dev_ctx, device_cache=True, **cfg)
    twin = T.TxVotePool(dev_ctx, device_cache=True, **cfg)
    opool = O.Pool(**cfg)
    try:
        earlier = []
        for b in range(2):
            votes = _mix(rnd, n, fresh, earlier)
            dev, meta = _upload(votes)
            st = pool.check_routed(dev.data_ptr(), meta) if b else pool.check_wait(pool.check_routed_submit(dev.data_ptr(), meta))
            ost = _oracle_status(opool, votes)
            _check_equal(pool, opool, st, ost, f"n={n} cache={cache} wal={wal} batch {b}")
            _twin_feed(twin, votes)
            _same_state(pool, twin, f"twin, batch {b}")
            earlier = votes
        if n >= 63:       # every class of vote took part
            for code in (T.POOL_OK, T.POOL_ERR_IN_CACHE, T.POOL_ERR_TOO_LARGE, T.POOL_ERR_ENCODING if wal else T.POOL_OK):
                assert (ost == code).any(), code
    finally:
        pool.close()
        twin.close()


def test_nil_and_long_signature_votes_are_not_checked(dev_ctx, signed):
    votes = [dict(v) for v in signed[1][:70]]
    votes[3] = None
    votes[64] = None
    votes[10]["sig"] = votes[10]["sig"] + b"\x07"                 # 65 bytes: the buffer carries the first 64
    votes[11] = dict(votes[10], sig=votes[10]["sig"][:64])         # the same first 64 bytes, a checked vote
    votes[20] = dict(votes[5])                                      # a repeat
    cfg = dict(size=1 << 16, cache_size=10000)
    pool = T.TxVotePool(dev_ctx, device_cache=True, **cfg)
    opool = O.Pool(**cfg)
    try:
        dev, meta = _upload(votes)
        assert int(meta["flags"]) & T.ROUTE_NIL
        st = pool.check_routed(dev.data_ptr(), meta)
        assert st[3] == NC and st[64] == NC and st[10] == NC and st[11] == T.POOL_OK and st[20] == T.POOL_ERR_IN_CACHE
        _check_equal(pool, opool, st, _oracle_status(opool, votes), "nil and long")
    finally:
        pool.close()


@pytest.mark.parametrize("mode", ["full", "host_cache", "no_cache", "no_cache_dev", "bytes_cap"])
def test_host_fallback(dev_ctx, signed, mode):
    """pools the device path cannot serve: the buffer is read back and admitted on the host, with the
    same results"""
    rnd = random.Random(17)
    fresh = list(signed[1])
    cfg = dict(size=16 if mode == "full" else 1 << 16, cache_size=T.POOL_NO_CACHE if mode.startswith("no_cache") else 100,
               max_txs_bytes=3000 if mode == "bytes_cap" else 1 << 30, max_msg_bytes=260)
    pool = T.TxVotePool(dev_ctx, device_cache=mode not in ("host_cache", "no_cache"), **cfg)
    opool = O.Pool(**cfg)
    try:
        earlier = []
        for b in range(2):
            votes = _mix(rnd, 65, fresh, earlier)
            if b:
                votes[2] = None
                votes[5] = dict(votes[5], sig=votes[5]["sig"] + b"\x01")
            dev, meta = _upload(votes)
            st = pool.check_routed(dev.data_ptr(), meta)
            ost = _oracle_status(opool, votes)
            _check_equal(pool, opool, st, ost, f"{mode} batch {b}")
            earlier = votes
        if mode in ("full", "bytes_cap"):
            assert (ost == T.POOL_ERR_FULL).any()
    finally:
        pool.close()


def _flow_expect(flow, ids, votes, pool_st):
    """O.Flow run on the admitted votes: the batch's statuses (nil for the others) and commit events"""
    adm = [i for i in range(len(votes)) if pool_st[i] == T.POOL_OK]
    st, sums, fired = flow.add_votes([votes[i] for i in adm])
    exp = np.full(len(votes), NIL_ST, np.uint8)
    first, after = {}, {}
    for k, i in enumerate(adm):
        th = votes[i]["txhash"]
        ids.setdefault(th, len(ids))
        exp[i] = int(st[k]) | (int(fired[k]) << 7)
        if st[k] == 0:
            after[th] = int(sums[k])
        if fired[k]:
            first.setdefault(th, i)
    return exp, sorted((i, ids[t], after[t]) for t, i in first.items())


def _events(ev):
    return sorted((int(e["vote_index"]), int(e["tx_index"]), int(e["sum"])) for e in ev)


def _flow_votes(signed, n, rnd):
    """n votes over whole TxHashes (so sets commit), some replayed inside the batch, one nil, one
    truncated signature"""
    votes = [dict(v) for v in signed[1][:n]]
    for i in range(9, n, 13):
        votes[i] = dict(votes[rnd.randrange(i)])
    return votes


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("waited", [False, True], ids=["in-flight", "waited"])
def test_txflow_parity(dev_ctx, signed, n, waited):
    """submit_routed_checked against O.Flow run on the admitted votes, with the pool ticket still in
    flight (the nil column built on the device) and with it waited first (the host statuses)"""
    rnd = random.Random(n)
    dev_ctx.reset_flow()
    flow = O.Flow(signed[0], POWERS, CHAIN.encode())
    ids = {}
    cfg = dict(size=1 << 16, cache_size=10000)
    pool = T.TxVotePool(dev_ctx, device_cache=True, **cfg)
    opool = O.Pool(**cfg)
    try:
        first = _flow_votes(signed, n, rnd)
        second = [dict(first[rnd.randrange(n)]) if i % 3 == 0 else dict(signed[1][n + i]) for i in range(n)]   # replays of the first
        second[4] = None
        for votes in (first, second):
            dev, meta = _upload(votes)
            pt = pool.check_routed_submit(dev.data_ptr(), meta)
            if waited:
                pst = pool.check_wait(pt)
                ft = dev_ctx.submit_routed_checked(dev.data_ptr(), meta, pool, pt)
            else:
                ft = dev_ctx.submit_routed_checked(dev.data_ptr(), meta, pool, pt)
                pst = pool.check_wait(pt)
            st, ev = dev_ctx.wait_votes(ft)
            assert np.array_equal(pst, _oracle_status(opool, votes))
            exp, exp_ev = _flow_expect(flow, ids, votes, pst)
            assert np.array_equal(st, exp), np.flatnonzero(st != exp)[:8]
            assert _events(ev) == exp_ev
            assert (exp[pst != T.POOL_OK] == NIL_ST).all() and (pst != T.POOL_OK).any()
            assert dev_ctx.num_tx_sets() == flow.num_sets()
        assert len(exp_ev) > 0 or n < 8
    finally:
        pool.close()


def test_guard_refuses_a_meta_that_is_not_the_headers(dev_ctx, signed):
    """a tensor holding a valid buffer of 65 votes, a self-consistent meta for 64 (every address it
    describes lies inside the tensor): nothing beyond the header is read, every vote is not checked,
    the pool is unchanged, the wait says so, and TxFlow runs a batch of nil entries"""
    votes = [dict(v) for v in signed[1][:65]]
    dev, meta = _upload(votes)
    bad = meta.copy()
    bad["n"] = 64
    bad["arena_bytes"] = 64 * 64
    bad["bytes"] = int(T.lib().txv_route_bytes(64, 64 * 64, int(meta["flags"])))
    assert int(bad["bytes"]) < int(meta["bytes"])
    dev_ctx.reset_flow()
    before = dev_ctx.num_tx_sets()
    for device_cache in (True, False):
        pool = T.TxVotePool(dev_ctx, size=1 << 16, cache_size=1000, device_cache=device_cache)
        try:
            pt = pool.check_routed_submit(dev.data_ptr(), bad)
            ft = dev_ctx.submit_routed_checked(dev.data_ptr(), bad, pool, pt)       # the ticket in flight
            with pytest.raises(T.RouteGuardError, match=r"\(-22\).*header") as ei:
                pool.check_wait(pt)
            assert len(ei.value.statuses) == 64 and (ei.value.statuses == NC).all()
            st, ev = dev_ctx.wait_votes(ft)
            assert len(st) == 64 and (st == NIL_ST).all() and len(ev) == 0
            ft = dev_ctx.submit_routed_checked(dev.data_ptr(), bad, pool, pt)       # the ticket waited
            st, ev = dev_ctx.wait_votes(ft)
            assert len(st) == 64 and (st == NIL_ST).all() and len(ev) == 0
            assert pool.Size() == 0 and pool.TxsBytes() == 0 and len(pool.cache_keys()) == 0 and len(pool.reap(-1)[1]) == 0
            assert dev_ctx.num_tx_sets() == before
            with pytest.raises(T.RouteGuardError):
                pool.check_routed(dev.data_ptr(), bad)
            # the pool still works, and the true meta is accepted
            assert (pool.check_routed(dev.data_ptr(), meta) == T.POOL_OK).all() and pool.Size() == 65
        finally:
            pool.close()


def test_argument_errors_and_the_empty_batch(dev_ctx, signed):
    votes = [dict(v) for v in signed[1][:5]]
    dev, meta = _upload(votes, spare=64)
    pool = T.TxVotePool(dev_ctx, size=1 << 16, cache_size=1000, device_cache=True)
    L = T.lib()
    import ctypes
    t = ctypes.c_uint64()
    m = np.asarray(meta, T.ROUTE_META_DTYPE).reshape(1).copy()
    try:
        ptr = ctypes.c_void_p(dev.data_ptr())
        assert L.txv_pool_check_routed_submit(pool._h, dev_ctx._h, None, m.ctypes.data, ctypes.byref(t)) == -22
        assert L.txv_pool_check_routed_submit(pool._h, dev_ctx._h, ptr, None, ctypes.byref(t)) == -22
        assert L.txv_pool_check_routed_submit(pool._h, dev_ctx._h, ptr, m.ctypes.data, None) == -22
        assert L.txv_pool_check_routed_submit(None, dev_ctx._h, ptr, m.ctypes.data, ctypes.byref(t)) == -22
        assert L.txv_submit_routed_checked(dev_ctx._h, ptr, m.ctypes.data, None, 1, ctypes.byref(t)) == -22
        assert L.txv_submit_routed_checked(dev_ctx._h, ptr, m.ctypes.data, pool._h, 1, None) == -22
        with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
            pool.check_routed_submit(dev.data_ptr() + 8, meta)                     # not 16-byte aligned
        wrong = meta.copy()
        wrong["bytes"] = int(meta["bytes"]) + 16
        with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
            pool.check_routed_submit(dev.data_ptr(), wrong)                        # bytes != txv_route_bytes(...)
        big = meta.copy()
        big["n"] = (1 << 12) + 1
        big["bytes"] = int(L.txv_route_bytes(int(big["n"]), int(big["arena_bytes"]), int(big["flags"])))
        with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
            pool.check_routed_submit(dev.data_ptr(), big)                          # n > max_batch
        assert pool.Size() == 0
        # n == 0: a pool ticket with zero statuses, a flow ticket with zero votes
        e_dev, e_meta = _upload([])
        assert int(e_meta["n"]) == 0
        pt = pool.check_routed_submit(e_dev.data_ptr(), e_meta)
        ft = dev_ctx.submit_routed_checked(e_dev.data_ptr(), e_meta, pool, pt)
        assert len(pool.check_wait(pt)) == 0
        st, ev = dev_ctx.wait_votes(ft)
        assert len(st) == 0 and len(ev) == 0
        assert len(pool.check_routed(e_dev.data_ptr(), e_meta)) == 0
        # an unknown pool ticket, and a batch of another size than the ticket's
        with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):
            dev_ctx.submit_routed_checked(dev.data_ptr(), meta, pool, 12345)
        pt = pool.check_routed_submit(dev.data_ptr(), meta)
        with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
            dev_ctx.submit_routed_checked(e_dev.data_ptr(), e_meta, pool, pt)
        assert (pool.check_wait(pt) == T.POOL_OK).all()
    finally:
        pool.close()


@pytest.mark.parametrize("waited", [False, True], ids=["in-flight", "waited"])
def test_routed_ticket_passed_to_submit_checked(dev_ctx, signed, waited):
    """txv_submit_checked given a routed ticket takes its host-status path (the flight slot holds no
    signatures): the result is submit_routed_checked's"""
    rnd = random.Random(3)
    n = 65
    votes = _flow_votes(signed, n, rnd)
    cfg = dict(size=1 << 16, cache_size=10000)
    got = []
    for routed in (True, False):
        dev_ctx.reset_flow()
        pool = T.TxVotePool(dev_ctx, device_cache=True, **cfg)
        try:
            dev, meta = _upload(votes)
            pt = pool.check_routed_submit(dev.data_ptr(), meta)
            if waited:
                pst = pool.check_wait(pt)
            if routed:
                ft = dev_ctx.submit_routed_checked(dev.data_ptr(), meta, pool, pt)
            else:
                ft = dev_ctx.submit_checked(T.route_view(dev.cpu().numpy()), pool, pt)
            if not waited:
                pst = pool.check_wait(pt)
            st, ev = dev_ctx.wait_votes(ft)
            got.append((pst.copy(), st.copy(), _events(ev), dev_ctx.num_tx_sets()))
        finally:
            pool.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert got[0][2] == got[1][2] and got[0][3] == got[1][3]
    flow = O.Flow(signed[0], POWERS, CHAIN.encode())
    exp, exp_ev = _flow_expect(flow, {}, votes, got[0][0])
    assert np.array_equal(got[1][1], exp) and got[1][2] == exp_ev and len(exp_ev) > 0


def test_ordering_with_an_update_between_two_routed_batches(dev_ctx, signed):
    """routed batch, update_submit, routed batch, back to back: the statuses equal the oracle's in
    that order"""
    rnd = random.Random(23)
    a = [dict(v) for v in signed[1][:257]]
    committed = [dict(v) for v in a[10:60]] + [dict(v) for v in signed[1][300:320]]
    b = [dict(a[rnd.randrange(257)]) if i % 4 == 0 else dict(signed[1][290 + i]) for i in range(65)]
    cfg = dict(size=1 << 16, cache_size=10000)
    pool = T.TxVotePool(dev_ctx, device_cache=True, **cfg)
    opool = O.Pool(**cfg)
    try:
        da, ma = _upload(a)
        db, mb = _upload(b)
        ta = pool.check_routed_submit(da.data_ptr(), ma)
        pool.update_submit(1, _batch(committed))
        tb = pool.check_routed_submit(db.data_ptr(), mb)
        sb = pool.check_wait(tb)
        sa = pool.check_wait(ta)
        assert np.array_equal(sa, opool.check(a))
        opool.update(1, committed)
        osb = opool.check(b)
        _check_equal(pool, opool, sb, osb, "after routed, update, routed")
        assert (osb == T.POOL_ERR_IN_CACHE).any() and (osb == T.POOL_OK).any()
    finally:
        pool.close()


# ------------------------------------------------------------------ end to end on the seven-way context
N_E2E, H_E2E = 65, 4


@pytest.fixture(scope="module")
def own():
    """signer 2's own votes over 65 txs, by the oracle: computed once"""
    O.build()
    rnd = random.Random(99)
    txs = [bytes(rnd.getrandbits(8) for _ in range(1 + (i * 7) % 90)) for i in range(N_E2E)]
    tb = T.TxBatch(txs, [1_700_000_000 + i for i in range(N_E2E)], [1 + 3 * i for i in range(N_E2E)])
    addr = O.sha256(O.pubkey(SEEDS[2]))[:20]
    votes = []
    for i, tx in enumerate(txs):
        key = O.sha256(tx)
        th = key.hex().upper().encode()
        ts = (int(tb.ts_sec[i]), int(tb.ts_nanos[i]))
        sig = O.sign(SEEDS[2], O.signbytes(H_E2E, th, ts[0], ts[1], CHAIN.encode()))
        votes.append(dict(height=H_E2E, txhash=th, ts_sec=ts[0], ts_nanos=ts[1], addr=addr, sig=sig, txkey=key))
    return tb, votes


def test_sign_check_gossip_addvote_with_nothing_waited_in_between(gpu_ctx, own):
    import torch
    tb, votes = own
    pubs = gpu_ctx.keygen(SEEDS)
    gpu_ctx.set_validators(pubs[:4], POWERS, CHAIN)
    gpu_ctx.reset_flow()
    gpu_ctx.enable_gossip_sink(1 << 20, 4096)
    pool = T.TxVotePool(gpu_ctx, size=1 << 16, cache_size=10000, device_cache=True)
    cap = T.sign_txs_bytes(N_E2E)
    try:
        for rep in range(2):
            dev = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            sg = gpu_ctx.sign_txs_submit(tb, 2, H_E2E, dev.data_ptr(), cap)
            meta = gpu_ctx.sign_txs_meta(N_E2E, 2)
            pt = pool.check_routed_submit(dev.data_ptr(), meta)
            ft = gpu_ctx.submit_routed_checked(dev.data_ptr(), meta, pool, pt)
            st, ev = gpu_ctx.wait_votes(ft)
            pst = pool.check_wait(pt)
            assert gpu_ctx.sign_txs_wait(sg) == meta
            wb, idx, flag = gpu_ctx.gossip_msgs(ft)
            if rep == 0:
                assert (pst == T.POOL_OK).all()
                assert (st & 0x7F == T.ADDED).all()
                assert list(idx) == list(range(N_E2E)) and not flag.any()
                for i, v in enumerate(votes):
                    assert wb.msg(i) == O.wire_encode(v["height"], v["txhash"], v["ts_sec"], v["ts_nanos"], v["addr"],
                                                      v["sig"], v["txkey"]), i
            else:             # signing is deterministic: the same votes again
                assert (pst == T.POOL_ERR_IN_CACHE).all()
                assert (st == NIL_ST).all() and len(ev) == 0
                assert wb.n == 0 and len(idx) == 0
        assert pool.Size() == N_E2E
        # a signer outside the registry: n = 0 through all three calls
        dev = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        sg = gpu_ctx.sign_txs_submit(tb, 4, H_E2E, dev.data_ptr(), cap)
        meta = gpu_ctx.sign_txs_meta(N_E2E, 4)
        assert int(meta["n"]) == 0
        pt = pool.check_routed_submit(dev.data_ptr(), meta)
        ft = gpu_ctx.submit_routed_checked(dev.data_ptr(), meta, pool, pt)
        assert gpu_ctx.sign_txs_wait(sg) == meta
        assert len(pool.check_wait(pt)) == 0
        st, ev = gpu_ctx.wait_votes(ft)
        assert len(st) == 0 and len(ev) == 0 and pool.Size() == N_E2E
    finally:
        gpu_ctx.enable_gossip_sink(0, 0)
        pool.close()
