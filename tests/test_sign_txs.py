"""Sign by batch on the device (include/txvote.h txv_sign_txs_submit / txv_sign_txs_wait /
txv_sign_txs / txv_scalarmult_base; kernels_sign.hip; reference: Reactor.signTxRoutine,
txvotepool/reactor.go:87-138 -> NewTxVote types/tx_vote.go:57-71 -> MockPV.SignTxVote
types/priv_validator.go:83-95).

Every expected value comes from the oracle (SHA-256, key derivation, SignBytes, RFC 8032 signing,
[s]B) and from the host route packer (txv_route_pack_host); every comparison is byte-exact."""
import random

import numpy as np
import pytest

import oracle as O
import txflow_amd as T

pytestmark = pytest.mark.gpu

CHAIN = "test_chain_id"
L = 2 ** 252 + 27742317777372353535851937790883648493
TX_LENS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 1000)      # SHA-256's padding edges and a long tx
_rnd = random.Random(20240)
SEEDS = [bytes(_rnd.getrandbits(8) for _ in range(32)) for _ in range(5)]     # four validators and an outsider
POWERS = [1, 1, 1, 2]
N_REF = 200


def _txs(n, seed=1):
    """n txs whose lengths cycle through TX_LENS; the first timestamps are the zero time, a
    nanos-only time and a negative second"""
    rnd = random.Random(seed)
    txs = [bytes(rnd.getrandbits(8) for _ in range(TX_LENS[i % len(TX_LENS)])) for i in range(n)]
    sec = [1_700_000_000 + i for i in range(n)]
    nanos = [1 + 7 * i for i in range(n)]
    for i, (s, ns) in enumerate([(0, 0), (0, 5), (-5, 3)][:n]):
        sec[i], nanos[i] = s, ns
    return T.TxBatch(txs, sec, nanos)


def _expected_votes(signer, txs, height):
    """NewTxVote + SignTxVote per tx, by the oracle"""
    seed = SEEDS[signer]
    addr = O.sha256(O.pubkey(seed))[:20]
    votes = []
    for i in range(txs.n):
        key = O.sha256(txs.tx(i))
        th = key.hex().upper()
        ts = (int(txs.ts_sec[i]), int(txs.ts_nanos[i]))
        sig = O.sign(seed, O.signbytes(height, th.encode(), ts[0], ts[1], CHAIN.encode()))
        votes.append(T.TxVote(Height=height, TxHash=th, TxKey=key, Timestamp=ts, ValidatorAddress=addr, Signature=sig))
    return votes


def _expected_buffer(votes):
    """the route buffer of the votes (TxKey column, no nil column) and its meta, by the host packer"""
    b = T.VoteBatch.from_votes(votes)
    b.is_nil = None
    bufs, metas = T.route_pack_host(b, None, 1)
    return bufs[0][:int(metas[0]["bytes"])], metas[0]


@pytest.fixture(scope="module")
def ref():
    """the reference txs and, per (signer, height), their expected votes: computed once"""
    O.build()
    txs = _txs(N_REF)
    cache = {}

    def votes(signer, height, n=N_REF):
        if (signer, height) not in cache:
            cache[(signer, height)] = _expected_votes(signer, txs, height)
        return cache[(signer, height)][:n]
    return txs, votes


def _head(txs, n):
    return T.TxBatch(arena=txs.arena, off=txs.off[:n], length=txs.length[:n], ts_sec=txs.ts_sec[:n], ts_nanos=txs.ts_nanos[:n])


def _prepare(ctx):
    pubs = ctx.keygen(SEEDS)
    assert pubs == [O.pubkey(s) for s in SEEDS]
    ctx.set_validators(pubs[:4], POWERS, CHAIN)
    return pubs


def _dev_a5(nbytes):
    import torch
    d = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return d


SPARE = 256   # bytes behind the buffer that must stay as they were


def _assert_buffer(dev, meta, votes):
    want, wmeta = _expected_buffer(votes)
    assert meta == wmeta, (meta, wmeta)
    got = dev.cpu().numpy()
    k = int(wmeta["bytes"])
    assert np.array_equal(got[:k], want)
    assert (got[k:] == 0xA5).all()


# ------------------------------------------------------------------ buffer parity
@pytest.mark.parametrize("n,height", [(1, 7), (63, 7), (64, 0), (65, 7), (200, 7)])
def test_buffer_equals_the_host_packer(gpu_ctx, ref, n, height):
    txs, votes = ref
    _prepare(gpu_ctx)
    cap = T.sign_txs_bytes(n)
    dev = _dev_a5(cap + SPARE)
    meta = gpu_ctx.sign_txs(_head(txs, n), 2, height, dev.data_ptr(), cap)
    assert int(meta["n"]) == n and int(meta["bytes"]) == cap and int(meta["arena_bytes"]) == 64 * n
    assert int(meta["max_txhash_len"]) == 64 and int(meta["flags"]) == T.ROUTE_TXKEY
    _assert_buffer(dev, meta, votes(2, height, n))
    v = T.route_view(dev.cpu().numpy()[:cap])
    assert v.n == n and v.txhash(n - 1) == votes(2, height, n)[-1].TxHash.encode()


# ------------------------------------------------------------------ walk edges
def _edge_scalars(w):
    half, top = 1 << (w - 1), 252 // w
    low = sum(half << (w * i) for i in range(top))
    return [0, 1, 2, L - 1, L, 2 ** 252, 2 ** 253 - 1,
            low % 2 ** 253,                          # every window 2^(w-1): digit -2^(w-1), the carry rippling to the top
            (1 << (w * top)) - low,                  # signed digits all -2^(w-1) below a top digit of 1
            sum((half - 1) << (w * i) for i in range(top)),   # every digit the largest positive one
            1 << (w * top)]                          # all zero but the top one


def test_scalarmult_base_walk_edges(gpu_ctx):
    O.build()
    _prepare(gpu_ctx)
    w = gpu_ctx.base_w
    rnd = random.Random(300 + w)
    sc = _edge_scalars(w) + [rnd.randrange(L) for _ in range(64)]
    assert all(0 <= s < 2 ** 253 for s in sc)
    for n in (65, 129):                              # 64 k + 1: the last wave carries one live lane and 63 idle ones
        s = (sc + [rnd.randrange(2 ** 253) for _ in range(n)])[:n - 1]
        s.append(sc[7])                              # the lone lane of the last wave walks a rippling carry
        raw = [x.to_bytes(32, "little") for x in s]
        got = gpu_ctx.scalarmult_base(raw)
        for i, r in enumerate(raw):
            assert got[i].tobytes() == O.scalarmult_base(r), (w, n, i, hex(s[i]))
    with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
        gpu_ctx.scalarmult_base([(2 ** 253).to_bytes(32, "little")])


# ------------------------------------------------------------------ signer parity
def test_signatures_equal_sign_votes(gpu_ctx, ref):
    txs, votes = ref
    _prepare(gpu_ctx)
    cap = T.sign_txs_bytes(N_REF)
    dev = _dev_a5(cap)
    meta = gpu_ctx.sign_txs(txs, 3, 9, dev.data_ptr(), cap)
    got = T.route_view(dev.cpu().numpy()[:int(meta["bytes"])])
    exp = T.VoteBatch.from_votes(votes(3, 9))
    old = gpu_ctx.sign_votes(exp, np.full(N_REF, 3, np.uint32), CHAIN)
    assert np.array_equal(got.sig.reshape(N_REF, 64), np.asarray(old).reshape(N_REF, 64))
    assert np.array_equal(got.sig, exp.sig)


# ------------------------------------------------------------------ round trip through TxFlow
def _oracle_batches(batches):
    """the oracle TxFlow fed the batches in turn: per batch the statuses (fired bit included) and
    the commit events (vote index, set id, stake after the batch); and the flow"""
    flow = O.Flow([O.pubkey(s) for s in SEEDS[:4]], POWERS, CHAIN.encode())
    ids, out = {}, []
    for votes in batches:
        dv = [dict(height=v.Height, txhash=v.TxHash.encode(), ts_sec=v.Timestamp[0], ts_nanos=v.Timestamp[1],
                   addr=v.ValidatorAddress, sig=v.Signature) for v in votes]
        st, sums, fired = flow.add_votes(dv)
        first, after = {}, {}
        for i, v in enumerate(dv):
            ids.setdefault(v["txhash"], len(ids))
            if st[i] == 0:
                after[v["txhash"]] = int(sums[i])
            if fired[i]:
                first.setdefault(v["txhash"], i)
        out.append((st.astype(np.uint8) | (fired.astype(np.uint8) << 7), sorted((i, ids[t], after[t]) for t, i in first.items())))
    return out, flow


N_TRIP, H_TRIP = 70, 5


@pytest.fixture(scope="module")
def trip(ref):
    """the round trip's expected votes (validator s signs the first 70 reference txs) and the oracle
    TxFlow's verdicts over them, validator by validator: computed once"""
    _, votes = ref
    batches = [votes(s, H_TRIP, N_TRIP) for s in range(4)]
    want, flow = _oracle_batches(batches)
    return batches, want, flow


def _round_trip(ctx, ref, trip, gossip):
    """four validators (weights 1, 1, 1, 2) each sign their own buffer of 70 txs on ctx; the buffers
    go through submit_routed in turn: statuses, fired bits, commit events and the sets' state equal
    the oracle TxFlow's; with gossip, the sink's messages equal the oracle's TxVoteMessage bytes"""
    txs, _ = ref
    batches, want, flow = trip
    n = N_TRIP
    cap = T.sign_txs_bytes(n)
    fired_total = 0
    for s in range(4):
        dev = _dev_a5(cap)
        meta = ctx.sign_txs(_head(txs, n), s, H_TRIP, dev.data_ptr(), cap)
        tk = ctx.submit_routed(dev.data_ptr(), meta)
        st, ev = ctx.wait_votes(tk)
        assert np.array_equal(st, want[s][0]), s
        assert [(int(e["vote_index"]), int(e["tx_index"]), int(e["sum"])) for e in ev] == want[s][1], s
        fired_total += len(ev)
        if gossip:
            wb, idx, flag = ctx.gossip_msgs(tk)
            assert list(idx) == list(range(n)) and not flag.any()
            for i, v in enumerate(batches[s]):
                assert wb.msg(i) == O.wire_encode(v.Height, v.TxHash.encode(), v.Timestamp[0], v.Timestamp[1],
                                                  v.ValidatorAddress, v.Signature, v.TxKey), (s, i)
    assert fired_total == len({v.TxHash for v in batches[0]}) > 0
    hashes = [v.TxHash.encode() for v in batches[0]]
    ex, sm, mj, tk32 = ctx.query_txs(hashes)
    for i, h in enumerate(hashes):
        assert ex[i] and (int(sm[i]), bool(mj[i])) == flow.query(h)
        assert tk32[i].tobytes() == batches[0][i].TxKey


def test_round_trip_through_txflow(gpu_ctx, ref, trip):
    """over every window: what the signer's walk kernels signed, the context's own verify and tally
    kernels accept, vote for vote as the oracle TxFlow does"""
    _prepare(gpu_ctx)
    gpu_ctx.reset_flow()
    _round_trip(gpu_ctx, ref, trip, gossip=False)


def test_a_signer_outside_the_registry_signs_nothing(gpu_ctx, ref):
    txs, _ = ref
    _prepare(gpu_ctx)
    gpu_ctx.reset_flow()
    n = 70
    cap = T.sign_txs_bytes(n)
    dev = _dev_a5(cap)
    meta = gpu_ctx.sign_txs(_head(txs, n), 4, 5, dev.data_ptr(), cap)
    assert int(meta["n"]) == 0 and int(meta["bytes"]) == T.sign_txs_bytes(0) == 80
    _assert_buffer(dev, meta, [])
    assert T.route_view(dev.cpu().numpy()[:80]).n == 0
    before = gpu_ctx.num_tx_sets()
    st, ev = gpu_ctx.wait_votes(gpu_ctx.submit_routed(dev.data_ptr(), meta))
    assert len(st) == 0 and len(ev) == 0 and gpu_ctx.num_tx_sets() == before


# ------------------------------------------------------------------ one context: gossip sink, ring, refusals
@pytest.fixture(scope="module")
def sctx():
    ctx = T.Context(max_batch=4096, max_txs=1024, max_validators=8)
    _prepare(ctx)
    yield ctx
    ctx.close()


def test_round_trip_with_the_gossip_sink(sctx, ref, trip):
    sctx.reset_flow()
    sctx.enable_gossip_sink(1 << 20, 4096)
    try:
        _round_trip(sctx, ref, trip, gossip=True)
    finally:
        sctx.enable_gossip_sink(0, 0)


def test_ring_and_refusals(sctx, ref):
    txs, votes = ref
    na, nb = 100, 37
    da, db, dc = (_dev_a5(T.sign_txs_bytes(k) + SPARE) for k in (na, nb, na))
    ta = sctx.sign_txs_submit(_head(txs, na), 0, 3, da.data_ptr(), T.sign_txs_bytes(na))
    tb = sctx.sign_txs_submit(_head(txs, nb), 1, 3, db.data_ptr(), T.sign_txs_bytes(nb))
    assert (ta - 1) % T.SIGN_RING != (tb - 1) % T.SIGN_RING
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):                 # TXV_ESTATE: the entry holds ticket ta
        sctx.sign_txs_submit(_head(txs, na), 0, 3, dc.data_ptr(), T.sign_txs_bytes(na))
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):                 # the synchronous call shares the ring
        sctx.sign_txs(_head(txs, na), 0, 3, dc.data_ptr(), T.sign_txs_bytes(na))
    mb = sctx.sign_txs_wait(tb)                                            # waits in reverse order
    ma = sctx.sign_txs_wait(ta)
    assert int(ma["n"]) == na and int(mb["n"]) == nb
    _assert_buffer(da, ma, votes(0, 3, na))
    _assert_buffer(db, mb, votes(1, 3, nb))
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):                 # a ticket is waited once
        sctx.sign_txs_wait(ta)
    assert bool((dc == 0xA5).all())
    # refusals: TXV_EINVAL, nothing written
    small = _head(txs, nb)
    with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
        sctx.sign_txs(small, 0, 3, dc.data_ptr(), T.sign_txs_bytes(nb) - 1)
    bad = _head(txs, nb)
    bad.ts_nanos = bad.ts_nanos.copy()
    bad.ts_nanos[nb - 1] = 10 ** 9
    with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
        sctx.sign_txs(bad, 0, 3, dc.data_ptr(), T.sign_txs_bytes(nb))
    with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
        sctx.sign_txs(small, len(SEEDS), 3, dc.data_ptr(), T.sign_txs_bytes(nb))
    with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
        sctx.sign_txs(small, 0, 3, dc.data_ptr() + 8, T.sign_txs_bytes(nb))
    assert bool((dc == 0xA5).all())
    # n = 0 succeeds: a header and the arena's zero bytes
    m0 = sctx.sign_txs(T.TxBatch([]), 0, 3, dc.data_ptr(), 80)
    assert int(m0["n"]) == 0 and int(m0["bytes"]) == 80
    _assert_buffer(dc, m0, [])


def test_no_validator_set_is_estate():
    ctx = T.Context(max_batch=1024, max_txs=64, max_validators=8)
    try:
        ctx.keygen(SEEDS[:1])
        dev = _dev_a5(T.sign_txs_bytes(1))
        with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):
            ctx.sign_txs(T.TxBatch([b"tx"]), 0, 1, dev.data_ptr(), T.sign_txs_bytes(1))
        assert bool((dev == 0xA5).all())
    finally:
        ctx.close()
