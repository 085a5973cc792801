"""TxStore.LoadTxCommit by batch on the device (txv_load_commits_submit / txv_load_commits_wait;
kernels_load.hip): stored Commit records decoded on the GPU into one route buffer, and that buffer
fed back into TxFlow.

Reference: TxStore.LoadTxCommit (tx/store.go:67-80) reached from TxFlow.LoadCommit
(txflow/service.go:115-120); the records are what SaveTx wrote (tx/store.go:83-107).

Every expected value comes from load_model.py (the envelope rules) with oracle.wire_decode for each
CommitSig, from oracle.Flow / oracle.Pool fed the decoded votes, or from the context's own earlier
state (the flow the records were saved from); every comparison is exact.  The route buffers live in
torch uint8 tensors."""
import os
import random
import re

import numpy as np
import pytest

import oracle as O
import load_model as M
import txflow_amd as T
from test_store_sink import _batch, _with_keys
from test_update_cadence import _stream

pytestmark = pytest.mark.gpu

CHAIN = b"test_chain_id"
FLAGS = T.ROUTE_TXKEY | T.ROUTE_NIL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = int(re.search(r"#define\s+TXV_LOAD_WINDOW\s+(\d+)",
                       open(os.path.join(ROOT, "go-txflow_amd", "csrc", "load_dev.h")).read()).group(1))


# ------------------------------------------------------------------ helpers
def _dev(nbytes, fill=0xA5):
    import torch
    return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device="cuda:0")


def _host(dev, nbytes=None):
    import torch
    torch.cuda.synchronize()
    return dev[:nbytes].cpu().numpy() if nbytes is not None else dev.cpu().numpy()


def _records(recs):
    return recs if isinstance(recs, T.CommitRecords) else T.CommitRecords(list(recs))


def _expect(cr):
    """the model's answer for a batch: statuses, first_vote, column rows, TxHash (offset, length), votes"""
    st, first, rows, th, votes = [], [0], [], [], []
    for k in range(cr.n):
        s, t, v = M.decode(O, cr.record(k))
        st.append(s)
        rows += M.columns(v)
        votes += v
        first.append(len(rows))
        th.append((int(cr.off[k]) + t[0], t[1]) if s == M.OK and t[1] else (0, 0))
    return st, first, rows, th, votes


def _need(rows):
    arena = sum(len(r[4]) for r in rows)
    return T.load_commits_bytes(len(rows), arena), arena


def _check_loaded(res, host, cr, exp):
    """the wait's outputs and the buffer read back, against the model"""
    st, first, rows, th, _ = exp
    need, arena = _need(rows)
    assert res.rec_status.tolist() == st
    assert res.first_vote.tolist() == first
    assert [(int(o), int(l)) for o, l in zip(res.txhash_off, res.txhash_len)] == th
    m = res.meta
    mx = max([len(r[4]) for r in rows if not r[0]] or [0])
    assert (int(m["n"]), int(m["arena_bytes"]), int(m["flags"]), int(m["reserved"]), int(m["bytes"]),
            int(m["max_txhash_len"])) == (len(rows), arena, FLAGS, 0, need, mx)
    batch = T.route_view(host[:need])
    assert batch.n == len(rows) and batch.is_nil is not None and batch.txkey is not None
    got = M.batch_columns(batch)
    for i, (g, e) in enumerate(zip(got, rows)):
        assert g == e, f"vote {i} differs"
    offs = batch.txhash_off.astype(np.int64)
    live = batch.is_nil == 0
    assert np.array_equal(offs[live], (np.cumsum(batch.txhash_len[live], dtype=np.int64) - batch.txhash_len[live]))
    assert not offs[~live].any()
    return batch


def _load(ctx, recs, spare=64):
    """load into a fresh tensor sized by the model's need; -> (result, host copy, tensor, expectation)"""
    cr = _records(recs)
    exp = _expect(cr)
    need, _ = _need(exp[2])
    dev = _dev(need + spare)
    res = ctx.load_commits(cr, dev.data_ptr(), need)
    host = _host(dev)
    assert (host[need:] == 0xA5).all(), "bytes at or past dst + cap were written"
    _check_loaded(res, host, cr, exp)
    return res, host, dev, exp


def rb(rnd, n):
    return bytes(rnd.getrandbits(8) for _ in range(n))


def rvote(rnd, **kw):
    """an unsigned vote with random fields (decode-only tests)"""
    v = dict(height=rnd.choice((0, 1, 77, 1 << 45)), txhash=rb(rnd, 32).hex().upper().encode(),
             ts_sec=1_700_000_000 + rnd.randrange(1000), ts_nanos=rnd.randrange(1_000_000_000), addr=rb(rnd, 20),
             sig=rb(rnd, 64), txkey=rb(rnd, 32))
    v.update(kw)
    return v


def rrecord(rnd, n, th=None):
    th = rb(rnd, 32).hex().upper().encode() if th is None else th
    return M.commit_encode(th, [M.vote_body(O, rvote(rnd, txhash=th)) for _ in range(n)])


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ctx():
    O.build()
    c = T.Context(max_batch=4096, max_txs=1024, max_validators=8, table_w=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def saved(ctx):
    """7 validators with unequal stake, 40 sets, three batches with the store sink on (replays and
    forged votes mixed in): each set's last record, and the flow's state when the last batch ended"""
    rnd = random.Random(515)
    pubs, powers, votes = _stream(rnd, n_vals=7, n_txs=40)
    votes = _with_keys(votes, random.Random(516))
    for i in range(5, len(votes), 17):                 # forged: a signature byte flipped, ahead of the real vote
        s = votes[i]["sig"]
        votes.insert(i, dict(votes[i], sig=s[:9] + bytes([s[9] ^ 0x10]) + s[10:]))
    ctx.enable_store_sink(0, 0)
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()
    ctx.enable_store_sink(1 << 20, 256)
    last, fired_in, raw_last = {}, {}, None
    cuts = [0, len(votes) // 3, 2 * len(votes) // 3, len(votes)]
    statuses = []
    for b, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        tk = ctx.submit_votes(_batch(votes[lo:hi]))
        st, _ = ctx.wait_votes(tk)
        statuses.append(st)
        recs = ctx.store_records(tk)
        for r in recs:
            last[r[3]] = r[4]
            fired_in.setdefault(r[3], []).append(b)
        raw_last = (ctx.store_records_raw(tk), recs)
    hashes = sorted({v["txhash"] for v in votes})
    state = {h: ctx.query_tx(h) for h in hashes}
    ctx.enable_store_sink(0, 0)
    st_all = np.concatenate(statuses) & 0x7F
    assert (st_all == T.ERR_INVALID_SIGNATURE).any() and (st_all == T.DUPLICATE).any()
    assert any(len(b) > 1 for b in fired_in.values()), "no set fired in more than one batch"
    records = [(k[2:], last[k]) for k in sorted(last)]     # (TxHash hex of the C-key, Commit bytes)
    return dict(pubs=pubs, powers=powers, records=records, state=state, raw_last=raw_last)


def _replay(ctx, dev, res, saved_, votes):
    """submit_routed of a loaded buffer on a reset flow, against oracle.Flow fed the same votes"""
    ctx.reset_flow()
    st, ev = ctx.wait_votes(ctx.submit_routed(dev.data_ptr(), res.meta))
    flow = O.Flow(saved_["pubs"], saved_["powers"], CHAIN)
    ost, _, ofired = flow.add_votes(votes)
    assert np.array_equal(st, ost.astype(np.uint8) | (ofired.astype(np.uint8) << 7)), np.flatnonzero(st != ost)[:8]
    return st, ev, flow


# ------------------------------------------------------------------ 1. round trip
def test_round_trip_restores_the_flow(ctx, saved):
    recs = [r for _, r in saved["records"]]
    assert len(recs) >= 30
    res, host, dev, exp = _load(ctx, recs)
    assert all(s == T.COMMIT_OK for s in exp[0])
    st, ev, flow = _replay(ctx, dev, res, saved, exp[4])
    assert ((st & 0x7F) == T.ADDED).all() and len(ev) == len(recs)
    for (hexkey, rec), (tho, thl) in zip(saved["records"], exp[3]):
        th = bytes.fromhex(hexkey.decode())
        assert b"".join(recs)[tho:tho + thl] == th
        assert ctx.query_tx(th) == saved["state"][th] == flow.query(th)
        assert saved["state"][th][1]
        assert ctx.make_commit(th) == rec, f"MakeCommit of the restored set {th!r} differs from its record"
    assert ctx.num_tx_sets() == len(recs)


def test_store_read_out_is_accepted_as_it_is(ctx, saved):
    """what store_records and store_records_raw returned, passed without re-packing: the same buffer"""
    (buf, off, lens, sets), recs = saved["raw_last"]
    assert len(recs) > 0
    bufs = []
    for obj in (recs, (buf, off, lens, sets), T.CommitRecords.from_store_raw(buf, off, lens)):
        cr = ctx._commit_records(obj)
        exp = _expect(cr)
        need, _ = _need(exp[2])
        dev = _dev(need)
        res = ctx.load_commits(obj, dev.data_ptr(), need)
        host = _host(dev)
        _check_loaded(res, host, cr, exp)
        bufs.append(host[:need].tobytes())
    assert bufs[0] == bufs[1] == bufs[2]


# ------------------------------------------------------------------ 2. tamper
def test_tampered_and_cut_records(ctx, saved):
    pubs, powers = saved["pubs"], saved["powers"]
    addrs = [O.sha256(p)[:20] for p in pubs]
    (hex_a, rec_a), (hex_b, rec_b) = saved["records"][3], saved["records"][8]
    th_a, th_b = bytes.fromhex(hex_a.decode()), bytes.fromhex(hex_b.decode())
    # a: one signature byte flipped inside the record
    votes_a = M.decode(O, rec_a)[2]
    at = rec_a.index(votes_a[1]["sig"]) + 20
    bad_a = rec_a[:at] + bytes([rec_a[at] ^ 1]) + rec_a[at + 1:]
    # b: cut to the votes below quorum
    _, _, elems = M.envelope(rec_b)
    votes_b = M.decode(O, rec_b)[2]
    quorum = sum(powers) * 2 // 3 + 1
    keep, stake = 0, 0
    while stake + powers[addrs.index(votes_b[keep]["addr"])] < quorum:
        stake += powers[addrs.index(votes_b[keep]["addr"])]
        keep += 1
    assert 0 < keep < len(votes_b)
    cut_b = M.commit_encode(th_b, [rec_b[o:o + l] for o, l in elems[:keep]])
    res, host, dev, exp = _load(ctx, [bad_a, cut_b])
    assert exp[0] == [M.OK, M.OK] and exp[1] == [0, len(votes_a), len(votes_a) + keep]
    st, ev, flow = _replay(ctx, dev, res, saved, exp[4])
    want = [T.ADDED] * (len(votes_a) + keep)
    want[1] = T.ERR_INVALID_SIGNATURE
    assert (st & 0x7F).tolist() == want
    lost = powers[addrs.index(votes_a[1]["addr"])]
    assert ctx.query_tx(th_a)[0] == saved["state"][th_a][0] - lost == flow.query(th_a)[0]
    assert ctx.query_tx(th_b) == (stake, False)
    assert not (st[len(votes_a):] & 0x80).any() and all(int(e["vote_index"]) < len(votes_a) for e in ev)


# ------------------------------------------------------------------ 3. shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_element_counts_around_the_wave(ctx, n):
    rnd = random.Random(n)
    _load(ctx, [rrecord(rnd, 2), rrecord(rnd, n), rrecord(rnd, 3)])


def _walk_refills(rec, base, w):
    """the refills of the envelope walk over a record at byte `base` of the buffer (load_dev.h
    Window: a read outside [lo, lo + w) moves lo to the read's 16-byte floor): (what each refill was
    reading, the last window's start)"""
    kinds, lo = [], None
    st, _, elems = M.envelope(rec)
    assert st == M.OK

    def touch(p, what):
        nonlocal lo
        a = base + p
        if lo is None or not lo <= a < lo + w:
            lo = a & ~15
            kinds.append(what)
    p = 0
    if rec[:1] == b"\x0a":
        touch(0, "key")
        n = M.uvarint(rec, 1, len(rec))
        for j in range(n[1]):
            touch(1 + j, "count%d" % j)
        p = 1 + n[1] + n[0]
    for body, blen in elems:
        touch(p, "key")
        for j in range(body - p - 1):
            touch(p + 1 + j, "count%d" % j)
        p = body + blen
    return kinds, lo


def test_record_longer_than_the_window(ctx):
    """one record of more than 2.5 windows (the size is read from load_dev.h) whose element lengths
    put a window edge between a key and its count, inside a two-byte count, in front of a key, and
    inside bodies"""
    rnd = random.Random(99)
    th = b"F" * 64
    lead = b"\x0a\x05hello"                              # a record ahead: the long one starts at byte 7
    base = len(lead)
    bodies, want = [], [1, 2, 1, 2]                       # the key's distance from the window's end

    def filler():
        return M.vote_body(O, rvote(rnd, txhash=rb(rnd, rnd.randrange(140, 200)), sig=rb(rnd, rnd.choice((63, 64)))))
    while want or len(M.commit_encode(th, bodies)) < 5 * WINDOW // 2:
        rec = M.commit_encode(th, bodies)
        gap = _walk_refills(rec, base, WINDOW)[1] + WINDOW - (base + len(rec))    # from the record's end to the edge
        if want and 300 <= gap <= 700:
            # an element of exactly the size that leaves the next key `want[0]` bytes before the edge
            for hl in range(60, 760):
                b = M.vote_body(O, rvote(rnd, txhash=rb(rnd, hl)))
                if 1 + M.uvarint_size(len(b)) + len(b) == gap - want[0]:
                    bodies.append(b)
                    want.pop(0)
                    break
        bodies.append(filler())
    rec = M.commit_encode(th, bodies)
    kinds = _walk_refills(rec, base, WINDOW)[0]
    assert len(rec) >= 2 * WINDOW and kinds.count("count0") >= 2 and kinds.count("count1") >= 2, kinds
    res, host, dev, exp = _load(ctx, [lead, rec, rrecord(rnd, 2)])
    assert exp[0] == [M.OK] * 3 and exp[1][1:3] == [0, len(bodies)]


def test_every_offset_residue(ctx):
    rnd = random.Random(5)
    buf, off, ln = bytearray(), [], []
    for k in range(33):
        rec = rrecord(rnd, 1 + k % 4, th=rb(rnd, 1 + k))
        buf += b"\xEE" * ((k % 16 - len(buf)) % 16)
        off.append(len(buf)); ln.append(len(rec))
        buf += rec
    assert {o % 16 for o in off} == set(range(16))
    cr = T.CommitRecords(recs=np.frombuffer(bytes(buf), np.uint8), off=np.array(off, np.uint64), length=np.array(ln, np.uint32))
    _load(ctx, cr)


def test_more_records_than_a_scan_tile(ctx):
    rnd = random.Random(6)
    recs = [rrecord(rnd, 1) for _ in range(257)]
    recs.insert(100, b"")
    recs.insert(200, recs[200][:-1])
    res, _, _, exp = _load(ctx, recs)
    assert exp[0].count(M.OK) == 257 and exp[1][-1] == 257 and len(recs) == 259


def test_only_empty_records_and_no_records(ctx):
    res, host, _, _ = _load(ctx, [b""] * 5)
    assert res.rec_status.tolist() == [T.COMMIT_EMPTY] * 5 and int(res.meta["n"]) == 0
    res, host, _, _ = _load(ctx, [])
    assert len(res.rec_status) == 0 and res.first_vote.tolist() == [0] and int(res.meta["n"]) == 0
    assert int(res.meta["bytes"]) == T.load_commits_bytes(0, 0)


# ------------------------------------------------------------------ 4. corrupt among good
def test_corrupt_records_among_good_ones(ctx):
    rnd = random.Random(7)
    good = [rrecord(rnd, n) for n in (3, 70, 2)]
    mid = rrecord(rnd, 4)
    _, _, elems = M.envelope(mid)
    truncated = mid[:elems[2][0] + 11]                   # cut inside the third element
    v = rvote(rnd)
    body = M.vote_body(O, v)
    i = body.index(b"\x1a\x20" + v["txkey"])
    badkey = M.commit_encode(v["txhash"], [M.vote_body(O, rvote(rnd)), body[:i] + b"\x1a\x21" + v["txkey"] + b"\x00" + body[i + 34:]])
    recs = [good[0], truncated, good[1], badkey, good[2]]
    res, host, _, exp = _load(ctx, recs)
    assert res.rec_status.tolist() == [T.COMMIT_OK, T.COMMIT_CORRUPT, T.COMMIT_OK, T.COMMIT_CORRUPT, T.COMMIT_OK]
    assert res.first_vote.tolist() == [0, 3, 3, 73, 73, 75]


# ------------------------------------------------------------------ 5. capacity
def test_capacity_is_decided_on_the_device(ctx, saved):
    rnd = random.Random(8)
    cr = _records([rrecord(rnd, n) for n in (5, 66, 1)])
    exp = _expect(cr)
    need, arena = _need(exp[2])
    dev = _dev(need + 64)
    with pytest.raises(T.LoadCommitsError, match=r"\(-28\)") as ei:
        ctx.load_commits(cr, dev.data_ptr(), need - 16)
    e = ei.value
    assert (e.rc, e.n, e.arena_bytes, e.nbytes) == (T.E_CAPACITY, 72, arena, need)
    assert int(e.meta["reserved"]) == 1 and int(e.meta["flags"]) == FLAGS
    assert e.rec_status.tolist() == exp[0] and e.first_vote.tolist() == exp[1]
    assert (_host(dev) == 0xA5).all(), "a refused load wrote to the buffer"
    # through the ring's wait as well
    t = ctx.load_commits_submit(cr, dev.data_ptr(), need - 16)
    with pytest.raises(T.LoadCommitsError) as ei:
        ctx.load_commits_wait(t)
    assert ei.value.rc == T.E_CAPACITY and ei.value.nbytes == need
    assert (_host(dev) == 0xA5).all()
    # the next load has room, and TxFlow is not poisoned
    res = ctx.load_commits(cr, dev.data_ptr(), need)
    host = _host(dev)
    assert (host[need:] == 0xA5).all()
    _check_loaded(res, host, cr, exp)
    ctx.reset_flow()
    st, _ = ctx.wait_votes(ctx.submit_routed(dev.data_ptr(), res.meta))
    assert len(st) == 72


# ------------------------------------------------------------------ 6. ring
def test_ring_of_two(ctx):
    rnd = random.Random(9)
    crs = [_records([rrecord(rnd, n) for n in ns]) for ns in ((4, 65), (2, 2, 9), (1,))]
    exps = [_expect(cr) for cr in crs]
    needs = [_need(e[2])[0] for e in exps]
    devs = [_dev(n + 32) for n in needs]
    t0 = ctx.load_commits_submit(crs[0], devs[0].data_ptr(), needs[0])
    t1 = ctx.load_commits_submit(crs[1], devs[1].data_ptr(), needs[1])
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):
        ctx.load_commits_submit(crs[2], devs[2].data_ptr(), needs[2])
    r1 = ctx.load_commits_wait(t1)
    r0 = ctx.load_commits_wait(t0)
    assert (_host(devs[2]) == 0xA5).all(), "a refused submit wrote to its buffer"
    for r, d, cr, e, n in ((r0, devs[0], crs[0], exps[0], needs[0]), (r1, devs[1], crs[1], exps[1], needs[1])):
        h = _host(d)
        assert (h[n:] == 0xA5).all()
        _check_loaded(r, h, cr, e)
    for stale in (t0, t1, t1 + 7):
        with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):
            ctx.load_commits_wait(stale)
    t2 = ctx.load_commits_submit(crs[2], devs[2].data_ptr(), needs[2])     # the ring is free again
    ctx.sync()                                                              # waits for the load in flight
    _check_loaded(ctx.load_commits_wait(t2), _host(devs[2]), crs[2], exps[2])
    assert ctx.load_commits_ms() > 0


# ------------------------------------------------------------------ 7. through the pool
def test_loaded_buffer_through_the_pool(ctx, saved):
    recs = [r for _, r in saved["records"]][:12]
    recs.append(recs[2])                                  # a replayed record
    res, host, dev, exp = _load(ctx, recs)
    votes = exp[4]
    n_replayed = exp[1][-1] - exp[1][-2]
    cfg = dict(size=1 << 16, cache_size=10000)
    pool = T.TxVotePool(ctx, device_cache=True, **cfg)
    opool = O.Pool(**cfg)
    try:
        ctx.reset_flow()
        pt = pool.check_routed_submit(dev.data_ptr(), res.meta)
        ft = ctx.submit_routed_checked(dev.data_ptr(), res.meta, pool, pt)
        pst = pool.check_wait(pt)
        st, ev = ctx.wait_votes(ft)
        ost = opool.check(votes)
        assert np.array_equal(pst, ost)
        assert (pst[-n_replayed:] == T.POOL_ERR_IN_CACHE).all() and (pst[:-n_replayed] == T.POOL_OK).all()
        flow = O.Flow(saved["pubs"], saved["powers"], CHAIN)
        adm = [i for i in range(len(votes)) if pst[i] == T.POOL_OK]
        fst, _, ffired = flow.add_votes([votes[i] for i in adm])
        want = np.full(len(votes), T.ERR_NIL, np.uint8)
        want[adm] = fst.astype(np.uint8) | (ffired.astype(np.uint8) << 7)
        assert np.array_equal(st, want)
        assert (st[-n_replayed:] == T.ERR_NIL).all() and len(ev) == 12
    finally:
        pool.close()
