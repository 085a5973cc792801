"""TxStore.SaveTx's records built on the device (txv_store_sink_enable / txv_store_records;
kernels_store.hip).

Reference: the commit block runs txStore.SaveTx(set) for every fired vote (txflow/service.go:216-218
-> tx/store.go:83-117): db.Set("H:%X", TxVoteSet bytes) and db.Set("C:%X", MakeCommit bytes).  Both
keys depend on the TxHash alone, so the last write wins, and one record per set that fired in a
batch -- built from the set's accepted votes as of the end of the batch, in the order of each set's
last fired vote -- leaves a store as the per-vote cadence does.  Here the expected records come from
the oracle: the batches replayed with oracle.Flow, each fired set's accepted votes via get_votes
(validator order), encoded with oracle.save_tx_bytes; set ids and record order by the Grouped recipe
of test_update_by_set (last fired arrival index).  Every vote carries a random TxKey of its own, so
a CommitSig's TxKey and the set's first-vote TxKey are told apart.  The records the device leaves
after each batch must equal the expected ones byte for byte and in order."""
import hashlib
import random

import numpy as np
import pytest

import oracle as O
from test_update_by_set import Grouped, _keys, _pool_state, _assert_list
from test_update_cadence import _stream

CHAIN = b"test_chain_id"
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _vote(seeds, addrs, v, txhash, nanos, height=1, sec=1_700_000_000, rnd=None, bad=False):
    sig = O.sign(seeds[v], O.signbytes(height, txhash, sec, nanos, CHAIN))
    if bad:
        sig = sig[:7] + bytes([sig[7] ^ 0x40]) + sig[8:]
    return dict(height=height, txhash=txhash, ts_sec=sec, ts_nanos=nanos, addr=addrs[v], sig=sig,
                txkey=bytes(rnd.getrandbits(8) for _ in range(32)))


def _with_keys(votes, rnd):
    """copies of the votes, each with a random TxKey of its own"""
    return [dict(v, txkey=bytes(rnd.getrandbits(8) for _ in range(32))) for v in votes]


def _batch(votes):
    import txflow_amd as T
    return T.VoteBatch.from_votes([T.TxVote(Height=v["height"], TxHash=v["txhash"], Timestamp=(v["ts_sec"], v["ts_nanos"]),
                                            ValidatorAddress=v["addr"], Signature=v["sig"], TxKey=v["txkey"])
                                   for v in votes])


class Stored:
    """the oracle TxFlow and, per batch, the SaveTx records: the Grouped recipe's fired sets in the
    order of their last fired vote, each encoded from the oracle's accepted votes"""

    def __init__(self, pubs, powers):
        self.flow = O.Flow(pubs, powers, CHAIN)
        self.addrs = [O.sha256(p)[:20] for p in pubs]
        self.ids = {}                    # TxHash -> set id (first-seen order)
        self.first_key = {}              # TxHash -> TxKey of the vote that created the set
        self.by_sig = {}                 # (TxHash, signature) -> the ADDED vote
        self.fired_before = set()

    def batch(self, votes):
        """-> ([(set id, H-key, TxVoteSet bytes, C-key, Commit bytes)], statuses, fired flags, info)"""
        st, _, fired = self.flow.add_votes(votes)
        last, touched = {}, set()
        for j, v in enumerate(votes):
            self.ids.setdefault(v["txhash"], len(self.ids))
            self.first_key.setdefault(v["txhash"], v["txkey"])
            if st[j] == 0:
                self.by_sig[(v["txhash"], v["sig"])] = v
                touched.add(v["txhash"])
            if fired[j]:
                last[v["txhash"]] = j
        recs = [(self.ids[t],) + self.record(t) for t in sorted(last, key=last.get)]
        info = dict(refired=len(set(last) & self.fired_before), unfired=len(touched - set(last)))
        self.fired_before |= set(last)
        return recs, st, fired, info

    def accepted(self, t):
        return [dict(self.by_sig[(t, sig)], addr=self.addrs[val]) for val, sig in self.flow.get_votes(t)]

    def record(self, t):
        return O.save_tx_bytes(t, self.first_key[t], self.accepted(t))


def _needed(recs):
    """bytes the records take in the sink: offsets rounded up to 16"""
    return sum((sum(len(p) for p in r[1:]) + 15) // 16 * 16 for r in recs)


def _assert_records(got, exp, what):
    assert [g[0] for g in got] == [e[0] for e in exp], f"{what}: set ids / record order differ"
    for k, (g, e) in enumerate(zip(got, exp)):
        for part, name in enumerate(("H key", "TxVoteSet bytes", "C key", "Commit bytes"), 1):
            assert g[part] == e[part], f"{what}: record {k} (set {e[0]}): {name} differ"


@pytest.fixture(scope="module")
def ctx():
    import txflow_amd as T
    c = T.Context(max_batch=4096, max_txs=1024, max_validators=256, table_w=4)   # small tables: 130 keys build fast
    yield c
    c.close()


@pytest.fixture(scope="module")
def cadence():
    """test_update_cadence's stream (6 validators with powers 1-3, 40 txs, replays), a TxKey per vote"""
    pubs, powers, votes = _stream(random.Random(2026))
    return pubs, powers, _with_keys(votes, random.Random(99))


def _start(ctx, pubs, powers, max_bytes, max_records, max_entries=0):
    ctx.enable_update_sink(0)
    ctx.enable_store_sink(0, 0)
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()
    ctx.enable_store_sink(max_bytes, max_records)
    if max_entries:
        ctx.enable_update_sink(max_entries)


def _run(ctx, ref, part, what):
    exp, est, efired, info = ref.batch(part)
    tk = ctx.submit_votes(_batch(part))
    st, _ = ctx.wait_votes(tk)
    assert np.array_equal(st, est.astype(np.uint8) | (efired.astype(np.uint8) << 7)), what
    got = ctx.store_records(tk)
    _assert_records(got, exp, what)
    return got, exp, info, tk


# ------------------------------------------------------------------ 1. cadence stream
def test_cadence_stream_records(ctx, cadence):
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 256)
    ref = Stored(pubs, powers)
    empty = refired = unfired = 0
    grew = False
    seen = {}
    cuts = [0, 3] + list(range(51, len(votes) + 48, 48))      # a first batch of 3: nothing can fire
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        got, exp, info, _ = _run(ctx, ref, votes[lo:hi], f"batch {k}")
        by_id = {i: t for t, i in ref.ids.items()}
        for g in got:                                         # the existing host path, right after the batch
            assert g[1:] == ctx.save_tx_bytes(by_id[g[0]]), f"batch {k}: set {g[0]} differs from txv_save_tx_bytes"
            grew |= g[0] in seen and len(g[4]) > seen[g[0]]
            seen[g[0]] = len(g[4])
        empty += not exp
        refired += info["refired"]
        unfired += info["unfired"]
    # a batch with no record, sets that re-fire in a later batch (their record grows), sets that got
    # votes but no 2/3 (absent from that batch's records)
    assert empty >= 1 and refired >= 1 and unfired >= 1 and grew


# ------------------------------------------------------------------ 2. encoding edges
def test_encoding_edges(ctx):
    import txflow_amd as T
    seeds, pubs, addrs = _keys(4)
    powers = [1, 1, 1, 1]                                     # quorum 3
    _start(ctx, pubs, powers, 4 << 20, 1024)
    ref = Stored(pubs, powers)
    rnd = random.Random(21)
    heights = (0, 1, 127, 128, -1)
    times = ((1_700_000_000, None), (1_700_000_000, 0), (0, None), (0, 0), (-1, None))
    cases = [(h, t) for h in heights for t in times]
    votes, sizes, nanos = [], set(), 1

    def add(txhash, v, height, sec, ns, **kw):
        nonlocal nanos
        n = nanos if ns is None else ns
        votes.append(_vote(seeds, addrs, v, txhash, n, height=height, sec=sec, rnd=rnd, **kw))
        sizes.add(T.txvote_size(height, len(txhash), sec, n, 20, 64))
        nanos += 1

    # the empty TxHash names one set: its four votes take four of the (height, time) cases,
    # among them neither height nor time (122) and both (138)
    for v, (h, (sec, ns)) in enumerate([(0, (0, 0)), (1, (1_700_000_000, 999_999_999)), (128, (0, None)), (-1, (-1, None))]):
        add(b"", v, h, sec, ns)
    assert {122, 138} <= sizes
    for hl in (1, 5, 63, 64, 65, 127, 128, 200):              # 65 and up: the overflow key arena
        for c, (h, (sec, ns)) in enumerate(cases):            # one transaction per (length, height, time) case
            txhash = (bytes([65 + c]) + b"%03d" % hl).ljust(hl, b"X")[:hl]
            for v in range(4):
                add(txhash, v, h, sec, ns)
    assert len({v["txhash"] for v in votes}) == 1 + 8 * 25
    assert min(sizes) < 128 <= max(sizes) and len(sizes) > 10  # the CommitSig length prefix's 1 -> 2 byte step
    rnd.shuffle(votes)
    # a set whose first vote has a bad signature: the stored TxKey is that vote's
    bad_tx = hashlib.sha256(b"bad-first").hexdigest().upper().encode()
    votes = ([_vote(seeds, addrs, 0, bad_tx, 5000, rnd=rnd, bad=True)] +
             [_vote(seeds, addrs, v, bad_tx, 5001 + v, rnd=rnd) for v in range(4)] + votes)
    n_rec = 0
    for k, s in enumerate(range(0, len(votes), 300)):
        got, exp, _, _ = _run(ctx, ref, votes[s:s + 300], f"batch {k}")
        n_rec += len(exp)
        if k == 0:
            assert got[0][0] == 0 and got[0][2].endswith(b"\x12\x20" + votes[0]["txkey"])
    assert n_rec >= 1 + 8 * 25 + 1


# ------------------------------------------------------------------ 3. validator counts
@pytest.mark.parametrize("n_vals", [1, 64, 65, 128, 130])
def test_validator_counts(ctx, n_vals):
    seeds, pubs, addrs = _keys(n_vals)
    powers = [1] * n_vals
    _start(ctx, pubs, powers, 1 << 20, 64)
    ref = Stored(pubs, powers)
    rnd = random.Random(n_vals)
    tx = hashlib.sha256(b"wide-tx").hexdigest().upper().encode()
    other = hashlib.sha256(b"holes-tx").hexdigest().upper().encode()
    order = list(range(n_vals))
    rnd.shuffle(order)                                        # arrival order against validator order
    votes = [_vote(seeds, addrs, v, tx, i + 1, rnd=rnd) for i, v in enumerate(order)]
    # a second set that fires with some validators missing: holes in the scan over the validators
    present = sorted(rnd.sample(range(n_vals), max(1, n_vals - n_vals // 5)))
    rnd.shuffle(present)
    holes = [_vote(seeds, addrs, v, other, 1000 + i, rnd=rnd) for i, v in enumerate(present)]
    if n_vals == 130:
        parts = [votes[:50] + holes[:60], votes[50:100] + holes[60:], votes[100:]]
    else:
        half = max(1, n_vals // 2)
        parts = [p for p in (votes[:half] + holes, votes[half:]) if p]
    sigs = []
    for k, part in enumerate(parts):
        got, _, _, _ = _run(ctx, ref, part, f"{n_vals} validators, batch {k}")
        sigs.append({g[0]: len(ref.accepted(tx if g[0] == 0 else other)) for g in got})
    if n_vals == 130:                                         # the record at 100, then at 130 CommitSigs
        assert sigs == [{}, {0: 100, 1: len(present)}, {0: 130}]
    else:
        assert sigs[-1][0] == n_vals and sigs[0][1] == len(present)
    if n_vals > 1:
        assert [addrs.index(a["addr"]) for a in ref.accepted(tx)] == sorted(order) != order


# ------------------------------------------------------------------ 4. many records
def test_many_records_layout(ctx):
    seeds, pubs, addrs = _keys(6)
    powers = [1 + (i % 3) for i in range(6)]
    _start(ctx, pubs, powers, 4 << 20, 1024)
    ref = Stored(pubs, powers)
    rnd = random.Random(5)
    hashes = [hashlib.sha256(b"tile-tx%d" % t).hexdigest().upper().encode() for t in range(400)]
    pairs = [(t, v) for t in range(400) for v in range(6)]
    rnd.shuffle(pairs)
    votes = [_vote(seeds, addrs, v, hashes[t], i + 1, rnd=rnd) for i, (t, v) in enumerate(pairs)]
    for _ in range(100):                                      # replays: 2,500 votes, 3 scan tiles
        votes.insert(rnd.randrange(1, len(votes)), dict(votes[rnd.randrange(len(votes))]))
    assert len(votes) == 2500
    got, exp, _, tk = _run(ctx, ref, votes, "the 2,500-vote batch")
    assert len(exp) > 300
    buf, off, lens, sets = ctx.store_records_raw(tk)
    assert len(off) == len(exp) and np.array_equal(sets, np.array([e[0] for e in exp], np.uint32))
    end = 0
    for k in range(len(off)):
        o, total = int(off[k]), int(lens[k].sum())
        assert o % 16 == 0 and o == (end + 15) // 16 * 16      # ascending, packed, non-overlapping
        assert not buf[end:o].any()                           # every pad byte is zero
        assert buf[o:o + total].tobytes() == b"".join(exp[k][1:])
        end = o + total
    assert len(buf) == (end + 15) // 16 * 16 == _needed(exp) and not buf[end:].any()


# ------------------------------------------------------------------ 5. four in flight
def test_four_in_flight_and_stale_tickets(ctx, cadence):
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 256)
    ref = Stored(pubs, powers)
    parts = [votes[s:s + 32] for s in range(0, 32 * 7, 32)]
    assert len(parts[-1]) == 32
    exps = [ref.batch(p)[0] for p in parts]                   # each as of its own batch
    assert sum(len(e) > 0 for e in exps[2:6]) >= 2
    for p in parts[:2]:                                       # sets open before the four batches in flight
        ctx.wait_votes(ctx.submit_votes(_batch(p)))
    tks = [ctx.submit_votes(_batch(p)) for p in parts[2:6]]
    with pytest.raises(T.StoreRecordsError) as e:             # not waited yet
        ctx.store_records(tks[0])
    assert e.value.rc == T.E_STATE
    for tk in tks:
        ctx.wait_votes(tk)
    for j, tk in enumerate(tks):
        _assert_records(ctx.store_records(tk), exps[2 + j], f"in-flight batch {j}")
    t5 = ctx.submit_votes(_batch(parts[6]))                   # the ring of four: one of the four slots is reused
    stale = [tk for tk in tks if (tk - 1) % T.SUBMIT_RING == (t5 - 1) % T.SUBMIT_RING]
    assert len(stale) == 1
    with pytest.raises(T.StoreRecordsError) as e:
        ctx.store_records(stale[0])
    assert e.value.rc == T.E_STATE
    ctx.wait_votes(t5)
    _assert_records(ctx.store_records(t5), exps[6], "the fifth batch")
    ctx.enable_store_sink(0, 0)
    with pytest.raises(T.StoreRecordsError) as e:             # the sink off
        ctx.store_records(t5)
    assert e.value.rc == T.E_STATE


# ------------------------------------------------------------------ 6. capacity
@pytest.mark.parametrize("short", ["bytes", "records"])
def test_capacity_overflow_leaves_txflow_alone(ctx, short):
    import ctypes
    import txflow_amd as T
    seeds, pubs, addrs = _keys(6)
    powers = [1] * 6                                          # quorum 5
    rnd = random.Random(6)
    hashes = [hashlib.sha256(b"cap-tx%d" % t).hexdigest().upper().encode() for t in range(3)]
    big = [_vote(seeds, addrs, v, hashes[t], 1 + 6 * t + v, rnd=rnd) for t in range(2) for v in range(6)]
    fits = [_vote(seeds, addrs, v, hashes[2], 100 + v, rnd=rnd) for v in range(6)]
    # the same batch with the sink off: the statuses and events to expect
    ctx.enable_update_sink(0)
    ctx.enable_store_sink(0, 0)
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()
    st_off, ev_off = ctx.wait_votes(ctx.submit_votes(_batch(big)))
    ref = Stored(pubs, powers)
    exp_big = ref.batch(big)[0]
    need = _needed(exp_big)
    assert len(exp_big) == 2 and need > _needed(exp_big[:1]) + 16
    exp_fits = ref.batch(fits)[0]
    assert _needed(exp_fits) <= need - 16
    _start(ctx, pubs, powers, need - 16 if short == "bytes" else need, 2 if short == "bytes" else 1)
    tk = ctx.submit_votes(_batch(big))
    st, ev = ctx.wait_votes(tk)
    assert np.array_equal(st, st_off) and np.array_equal(ev, ev_off) and len(ev) == 2
    with pytest.raises(T.StoreRecordsError) as e:
        ctx.store_records(tk)
    assert (e.value.rc, e.value.n, e.value.nbytes) == (T.E_CAPACITY, 2, need)
    # the next batch, which fits, yields its record (TxFlow was not poisoned)
    tk = ctx.submit_votes(_batch(fits))
    ctx.wait_votes(tk)
    _assert_records(ctx.store_records(tk), exp_fits, "the batch that fits")
    # output arrays too small: the counts, and nothing written
    total = _needed(exp_fits)
    out = np.full(total, 0xAB, np.uint8)
    off = np.full(1, 77, np.uint64); lens = np.full(4, 77, np.uint32); sets = np.full(1, 77, np.uint32)
    n, nb = ctypes.c_uint32(), ctypes.c_uint64()
    for cap, rec_cap in ((total - 1, 1), (total, 0)):
        rc = T.lib().txv_store_records(ctx._h, tk, out.ctypes.data, cap, off.ctypes.data, lens.ctypes.data,
                                       sets.ctypes.data, rec_cap, ctypes.byref(n), ctypes.byref(nb))
        assert (rc, n.value, nb.value) == (T.E_CAPACITY, 1, total)
        assert (out == 0xAB).all() and off[0] == 77 and (lens == 77).all() and sets[0] == 77


# ------------------------------------------------------------------ 7. both sinks on
def test_both_sinks_on(ctx, cadence):
    import txflow_amd as T
    pubs, powers, votes = cadence
    _start(ctx, pubs, powers, 1 << 20, 256, max_entries=512)
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
            pool.update_fired(ctx, k + 1, tk)
            pool.sync()
            want = (opool.cache_keys().tobytes(),) + tuple(x.tobytes() for x in opool.reap(-1))
            assert _pool_state(pool) == want, f"batch {k}: pool differs from the oracle's"
    finally:
        pool.close()
        ctx.enable_update_sink(0)


# ------------------------------------------------------------------ 8. large-batch path
def test_large_batch_compacted_stamps():
    """one batch of 2^18 votes: txv_flow_tally lists its stamped sets by compaction there, and the
    record builder takes the compaction's total as n_stamped"""
    import txflow_amd as T
    from txflow_amd.workload import Workload, SEEDS
    m = 1 << 18
    c = T.Context(max_batch=m, max_txs=4096, max_validators=128)
    try:
        wl = Workload(c, 100, 2622, SEEDS["c2"] + 3)
        c.enable_store_sink(96 << 20, 4096)
        tk = c.submit_votes(wl.head(m))
        st, _ = c.wait_votes(tk)
        buf, off, lens, sets = c.store_records_raw(tk)
        # set ids and record order from the batch's statuses
        tx_of = wl.tx_of[:m].astype(np.int64)
        fired = np.nonzero(st & T.STATUS_FIRED)[0]
        assert len(fired) > m // 4
        last = np.full(wl.n_txs, -1, np.int64)
        last[tx_of[fired]] = fired                            # ascending: the last fired vote wins
        order = np.argsort(last, kind="stable")
        order = order[last[order] >= 0]
        first_seen = np.full(wl.n_txs, -1, np.int64)         # set ids: first-seen order
        u, f = np.unique(tx_of, return_index=True)
        first_seen[u[np.argsort(f)]] = np.arange(len(u))
        assert len(sets) == len(order) == len(np.unique(tx_of[fired]))
        assert np.array_equal(sets, first_seen[order].astype(np.uint32))
        assert (off % 16 == 0).all() and (np.diff(off.astype(np.int64)) >= lens[:-1].sum(axis=1)).all()
        for k in list(range(16)) + list(range(len(order) - 16, len(order))):
            o, parts = int(off[k]), []
            for L in lens[k].tolist():
                parts.append(buf[o:o + L].tobytes())
                o += L
            assert tuple(parts) == c.save_tx_bytes(wl.hashes[order[k]].tobytes()), f"record {k}"
    finally:
        c.close()
