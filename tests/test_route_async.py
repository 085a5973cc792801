"""The owner route as a submit / wait ring with a stride guard (include/txvote.h
txv_route_submit_admitted / txv_route_submit_checked / txv_route_wait; reference hop
txvotepool/reactor.go:170-190 -> txvotepool/txvotepool.go:187-261 -> txflow/service.go:123-166).

Up to TXV_ROUTE_RING routes are in flight per context, each on its own ring entry; every waited
ticket's buffers and metas are byte-identical to the host packer's (txv_route_pack_host) fed the
same statuses.  The stride guard: a rank's buffer holds the sum of its votes' TxHash lengths, which
exceeds the arena extent when votes share TxHash offsets; a rank over its stride is refused (its
region untouched, its meta carrying the size it needs, TXV_ECAPACITY), on the host before a byte
is written and on the device in txv_k_route_scan / txv_k_route_scatter.

The guard tests hand the packers a destination allocated at the size the rank needs and prefilled
with 0xA5: a wrong guard writes inside the allocation and fails the assertion.

Route tests need no valid signatures (the route never verifies); only the pool-fed test builds a
signed StreamWorkload."""
import ctypes
import random

import numpy as np
import pytest

import txflow_amd as T
from txflow_amd import sharding

E_INVAL = -22
RING = 4


def _batch(seed, n, n_hashes=None, cols=True, shared=False):
    """n votes over n_hashes TxHashes (most 64 bytes, some shorter or empty), random addresses and
    signature bytes; cols: the TxKey and nil columns.  shared: votes of one TxHash share its arena
    offset (the workloads' layout), else every vote has its own arena bytes."""
    rng = np.random.default_rng(seed)
    nh = n_hashes or max(1, n // 7)
    hexd = np.frombuffer(b"0123456789ABCDEF", np.uint8)
    hashes = hexd[rng.integers(0, 16, (nh, 64))]
    pick = rng.integers(0, nh, n)
    ln = rng.choice(np.array([64, 64, 64, 64, 64, 33, 7, 0], np.uint32), n)
    if shared:
        arena, off = hashes.reshape(-1), pick * 64
    else:
        arena, off = hashes[pick].reshape(-1), np.arange(n) * 64
    return T.VoteBatch(n, height=1 + rng.integers(0, 3, n), txhash_arena=arena if n else np.zeros(1, np.uint8),
                       txhash_off=off.astype(np.uint32), txhash_len=ln, ts_sec=1_700_000_000 + rng.integers(0, 5, n),
                       ts_nanos=1 + np.arange(n), addr=rng.integers(0, 256, (n, 20)).astype(np.uint8),
                       addr_len=rng.choice(np.array([20, 20, 20, 0, 11], np.uint32), n),
                       sig=rng.integers(0, 256, (n, 64)).astype(np.uint8),
                       sig_len=rng.choice(np.array([64, 64, 64, 0, 40], np.uint32), n),
                       is_nil=(rng.random(n) < 0.03).astype(np.uint8) if cols else None,
                       txkey=rng.integers(0, 256, (n, 32)).astype(np.uint8) if cols else None)


def _statuses(seed, n):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([T.POOL_OK] * 5 + [T.POOL_ERR_IN_CACHE, T.POOL_ERR_TOO_LARGE], np.uint8), n)


def _shared_batch():
    """256 votes sharing 4 TxHashes of 64 bytes (txhash_off = (i % 4) * 64): the arena extent is
    256 B, the sum of the lengths 16,384 B"""
    rng = np.random.default_rng(5)
    n = 256
    hexd = np.frombuffer(b"0123456789ABCDEF", np.uint8)
    return T.VoteBatch(n, height=np.ones(n, np.int64), txhash_arena=hexd[rng.integers(0, 16, 256)],
                       txhash_off=((np.arange(n) % 4) * 64).astype(np.uint32), txhash_len=np.full(n, 64, np.uint32),
                       ts_sec=np.full(n, 1_700_000_000, np.int64), ts_nanos=1 + np.arange(n),
                       addr=rng.integers(0, 256, (n, 20)).astype(np.uint8), addr_len=np.full(n, 20, np.uint32),
                       sig=rng.integers(0, 256, (n, 64)).astype(np.uint8), sig_len=np.full(n, 64, np.uint32),
                       txkey=rng.integers(0, 256, (n, 32)).astype(np.uint8))


def _pack_host_raw(b, st, G, out, stride):
    """txv_route_pack_host into `out` with the given stride: (return code, metas)"""
    meta = np.zeros(G, T.ROUTE_META_DTYPE)
    vs = b.c_struct()
    rc = T.lib().txv_route_pack_host(ctypes.byref(vs), None if st is None else st.ctypes.data, G, out.ctypes.data,
                                     stride, meta.ctypes.data)
    return rc, meta


def _same_votes(a, b):
    assert a.n == b.n
    for name in ("height", "ts_sec", "ts_nanos", "txhash_len", "addr", "addr_len", "sig", "sig_len", "txkey", "is_nil"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert np.array_equal(x, y), name
    for i in range(a.n):
        assert a.txhash(i) == b.txhash(i)


def _refused_meta_ok(m, b, flags):
    assert int(m["n"]) == 256 and int(m["arena_bytes"]) == 16384 and int(m["reserved"]) == 1
    assert int(m["bytes"]) == int(T.lib().txv_route_bytes(256, 16384, flags))
    assert int(m["max_txhash_len"]) == 64 and int(m["flags"]) == flags


# ---------------------------------------------------------------------------------------- CPU
def test_host_packer_refuses_an_over_long_shard():
    """G = 1 with the extent-based stride: TXV_ECAPACITY, the meta tells the size needed, not a
    byte of the destination written (it overran the caller's buffer before the guard)"""
    b = _shared_batch()
    flags = T.route_flags(b)
    need = int(T.lib().txv_route_bytes(256, 16384, flags))
    out = np.full(need, 0xA5, np.uint8)
    rc, meta = _pack_host_raw(b, None, 1, out, int(T.lib().txv_route_bytes(256, 256, flags)))
    assert rc == T.E_CAPACITY
    _refused_meta_ok(meta[0], b, flags)
    assert (out == 0xA5).all()


def test_host_packer_fits_with_route_stride():
    b = _shared_batch()
    stride = T.route_stride(b)
    assert stride == int(T.lib().txv_route_bytes(256, 16384, T.route_flags(b)))
    out = np.full(stride, 0xA5, np.uint8)
    rc, meta = _pack_host_raw(b, None, 1, out, stride)
    assert rc == 0 and int(meta[0]["reserved"]) == 0 and int(meta[0]["bytes"]) == stride
    _same_votes(T.route_view(out[:int(meta[0]["bytes"])]), b)
    bufs, metas = T.route_pack_host(b, None, 1)
    assert np.array_equal(metas, meta) and np.array_equal(bufs[0], out)


def test_route_stride_covers_the_sum_of_lengths():
    b = _batch(11, 500)                      # own arena bytes per vote: sum <= extent
    live = b.is_nil == 0
    ext = int((b.txhash_off[live].astype(np.int64) + b.txhash_len[live]).max())
    assert T.route_stride(b) >= int(T.lib().txv_route_bytes(b.n, ext, T.route_flags(b)))
    s = _shared_batch()                      # shared offsets: the sum decides
    assert T.route_stride(s) == int(T.lib().txv_route_bytes(256, 16384, T.route_flags(s)))
    assert T.route_stride(s) > int(T.lib().txv_route_bytes(256, 256, T.route_flags(s)))
    assert T.route_stride(b) % 16 == 0 and T.route_stride(s) % 16 == 0


def test_host_packer_wants_a_16_byte_stride():
    b = _batch(12, 100)
    stride = T.route_stride(b)
    out = np.zeros(2 * (stride + 8), np.uint8)
    assert _pack_host_raw(b, None, 2, out, stride + 8)[0] == E_INVAL
    assert _pack_host_raw(b, None, 2, out, stride)[0] == 0


# ---------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def rctx():
    """one context for the route-only tests (no validator set: the route never verifies)"""
    ctx = T.Context(max_batch=1 << 17, max_txs=64, max_validators=8)
    yield ctx
    ctx.close()


def _dev_zeros(nbytes):
    import torch
    d = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return d


def _expect_host(dev_region, G, stride, dm, b, st):
    """the G buffers at dev_region (torch uint8 [G * stride]) and the metas dm equal the host packer's"""
    hb, hm = T.route_pack_host(b, st, G)
    assert np.array_equal(dm, hm)
    db = dev_region.view(G, stride).cpu().numpy()
    for r in range(G):
        k = int(hm[r]["bytes"])
        assert np.array_equal(db[r, :k], hb[r, :k]), r


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["device", "ahead", "waited"])
def test_four_in_flight_equal_the_host_packer(mode):
    """a C5-like stream with 5 % replays through a device-cache pool, four route tickets in flight
    (CheckTx k submitted, then its route; the oldest waited once four are out), G = 3, destination
    [4][G][stride]: every waited ticket byte-identical to the host packer fed that pool ticket's
    statuses.  "device": routed right behind each CheckTx; "ahead": ten CheckTx batches first (the
    engine's flight slots reused: the first take the host statuses); "waited": each pool ticket
    waited before its route."""
    import torch
    from txflow_amd.workload import StreamWorkload, SEEDS
    G = 3
    ctx = T.Context(max_batch=4096, max_txs=1536, max_validators=32)
    try:
        wl = StreamWorkload(ctx, 24, 640, SEEDS["c5"] + 21, 1024, replay=0.05)
        pool = T.TxVotePool(ctx, size=1 << 20, cache_size=600, max_txs_bytes=1 << 40, device_cache=True)
        stride = max(T.route_stride(b) for b in wl.batches)
        dev = _dev_zeros(RING * G * stride).view(RING, G * stride)
        ahead = 10 if mode == "ahead" else 1
        tks, flight, seen = {}, [], {"checked": 0, "in_cache": 0}

        def finish():
            j, rt, ps = flight.pop(0)
            dm = ctx.route_wait(rt, G)
            if ps is None:
                ps = pool.check_wait(tks[j])
            _expect_host(dev[j % RING], G, stride, dm, wl.batches[j], ps)
            assert int(dm["n"].sum()) == int((ps == T.POOL_OK).sum())
            dev[j % RING].zero_()            # the columns' alignment pads are left as they were (host: zero)
            torch.cuda.synchronize()
            seen["checked"] += 1
            seen["in_cache"] += int((ps == T.POOL_ERR_IN_CACHE).sum())

        def start(j):
            if len(flight) == RING:
                finish()
            ps = pool.check_wait(tks[j]) if mode == "waited" else None
            rt = ctx.route_submit_checked(wl.batches[j], pool, tks[j], G, dev[j % RING].data_ptr(), stride)
            flight.append((j, rt, ps))

        nb = len(wl.batches)
        for k in range(nb):
            tks[k] = pool.check_submit(wl.batches[k])
            if k - ahead + 1 >= 0:
                start(k - ahead + 1)
        for j in range(max(0, nb - ahead + 1), nb):
            start(j)
        while flight:
            finish()
        assert seen["checked"] == nb >= 14 and seen["in_cache"] > 0
        pool.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_out_of_order_waits(rctx):
    """four tickets waited as 3, 1, 4, 2 give the bytes in-order waits give (and the host packer's)"""
    G = 3
    bs = [_batch(100 + k, 700 + 300 * k) for k in range(RING)]
    sts = [_statuses(200 + k, b.n) for k, b in enumerate(bs)]
    stride = max(T.route_stride(b) for b in bs)
    got = {}
    for order in ((2, 0, 3, 1), (0, 1, 2, 3)):
        dev = _dev_zeros(RING * G * stride).view(RING, G * stride)
        tk = [rctx.route_submit_admitted(bs[k], sts[k], G, dev[k].data_ptr(), stride) for k in range(RING)]
        assert tk == sorted(tk) and len(set(tk)) == RING
        metas = {k: rctx.route_wait(tk[k], G) for k in order}
        for k in range(RING):
            _expect_host(dev[k], G, stride, metas[k], bs[k], sts[k])
        got[order] = (dev.cpu().numpy(), [metas[k] for k in range(RING)])
    a, b = got[(2, 0, 3, 1)], got[(0, 1, 2, 3)]
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.gpu
def test_fifth_submit_waits_for_a_free_entry(rctx):
    G = 2
    bs = [_batch(300 + k, 400 + 50 * k) for k in range(RING + 1)]
    sts = [_statuses(310 + k, b.n) for k, b in enumerate(bs)]
    stride = max(T.route_stride(b) for b in bs)
    dev = _dev_zeros((RING + 1) * G * stride).view(RING + 1, G * stride)
    tk = [rctx.route_submit_admitted(bs[k], sts[k], G, dev[k].data_ptr(), stride) for k in range(RING)]
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):            # TXV_ESTATE, nothing changed
        rctx.route_submit_admitted(bs[RING], sts[RING], G, dev[RING].data_ptr(), stride)
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):            # the synchronous call shares the ring
        rctx.route_admitted(bs[RING], sts[RING], G, dev[RING].data_ptr(), stride)
    metas = [rctx.route_wait(tk[0], G)]
    tk.append(rctx.route_submit_admitted(bs[RING], sts[RING], G, dev[RING].data_ptr(), stride))
    metas += [rctx.route_wait(t, G) for t in tk[1:]]
    for k in range(RING + 1):
        _expect_host(dev[k], G, stride, metas[k], bs[k], sts[k])
    with pytest.raises(T.TxvInfraError, match=r"\(-1\)"):            # a ticket is waited once
        rctx.route_wait(tk[0], G)


@pytest.mark.gpu
def test_sync_equals_async(rctx):
    G = 3
    b, st = _batch(400, 5000), _statuses(401, 5000)
    stride = T.route_stride(b)
    d1, d2 = _dev_zeros(G * stride), _dev_zeros(G * stride)
    m1 = rctx.route_admitted(b, st, G, d1.data_ptr(), stride)
    m2 = rctx.route_wait(rctx.route_submit_admitted(b, st, G, d2.data_ptr(), stride), G)
    assert np.array_equal(m1, m2) and np.array_equal(d1.cpu().numpy(), d2.cpu().numpy())
    _expect_host(d2, G, stride, m2, b, st)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [True, False], ids=["txkey_nil", "bare"])
@pytest.mark.parametrize("G", [1, 3, 255])
@pytest.mark.parametrize("n", [1, 65, 65600])
def test_shapes_equal_the_host_packer(rctx, n, G, cols):
    """one vote; a second wave with one lane; more than 1024 waves (the scan's second round and
    its carry); one shard, a few, the most the ABI takes; with and without the optional columns"""
    b, st = _batch(500 + n + G, n, cols=cols), _statuses(501 + n + G, n)
    stride = T.route_stride(b)
    dev = _dev_zeros(G * stride)
    dm = rctx.route_wait(rctx.route_submit_admitted(b, st, G, dev.data_ptr(), stride), G)
    _expect_host(dev, G, stride, dm, b, st)
    assert int(dm["n"].sum()) == int((st == T.POOL_OK).sum())


@pytest.mark.gpu
def test_an_empty_batch_among_tickets_in_flight(rctx):
    G = 3
    bs = [_batch(600, 3000), _batch(601, 0), _batch(602, 65)]
    sts = [_statuses(610, 3000), None, _statuses(612, 65)]
    stride = max(T.route_stride(b) for b in bs)
    dev = _dev_zeros(3 * G * stride).view(3, G * stride)
    tk = [rctx.route_submit_admitted(bs[k], sts[k], G, dev[k].data_ptr(), stride) for k in range(3)]
    for k in range(3):
        dm = rctx.route_wait(tk[k], G)
        _expect_host(dev[k], G, stride, dm, bs[k], sts[k])
        assert int(dm["n"].sum()) == (0 if k == 1 else int((sts[k] == T.POOL_OK).sum()))


@pytest.mark.gpu
def test_route_calls_want_16_byte_alignment(rctx):
    b = _batch(700, 200)
    stride = T.route_stride(b)
    dev = _dev_zeros(2 * stride + 64)
    for ptr, s in ((dev.data_ptr(), stride + 8), (dev.data_ptr() + 8, stride)):
        with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
            rctx.route_submit_admitted(b, None, 2, ptr, s)
        with pytest.raises(T.TxvInfraError, match=r"\(-22\)"):
            rctx.route_admitted(b, None, 2, ptr, s)
    rctx.route_wait(rctx.route_submit_admitted(b, None, 2, dev.data_ptr() + 16, stride), 2)   # the ring is untouched


def _dev_a5(nbytes):
    import torch
    d = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return d


@pytest.mark.gpu
def test_device_guard_refuses_an_over_long_shard(rctx):
    """the shared-offset batch, G = 1, the extent-based stride: TXV_ECAPACITY at the wait, the
    meta as the host packer's, the destination (allocated at the needed size) still all 0xA5"""
    b = _shared_batch()
    flags = T.route_flags(b)
    dev = _dev_a5(int(T.lib().txv_route_bytes(256, 16384, flags)))
    t = rctx.route_submit_admitted(b, None, 1, dev.data_ptr(), int(T.lib().txv_route_bytes(256, 256, flags)))
    with pytest.raises(T.TxvCapacityError) as ei:
        rctx.route_wait(t, 1)
    _refused_meta_ok(ei.value.metas[0], b, flags)
    assert bool((dev == 0xA5).all())
    with pytest.raises(T.TxvCapacityError):       # the synchronous call: the same code
        rctx.route_admitted(b, None, 1, dev.data_ptr(), int(T.lib().txv_route_bytes(256, 256, flags)))
    assert bool((dev == 0xA5).all())


SKEW_LEN = 1024


def _one_hash_batch(n):
    """every vote carries the same SKEW_LEN-byte TxHash (one shared arena offset).  A long TxHash:
    the route calls require a stride of at least txv_route_bytes(n, extent), which an even-split
    stride only reaches when the arena outweighs the n-sized columns"""
    b = _batch(800, n, n_hashes=1, shared=True)
    b.txhash_arena = np.random.default_rng(801).integers(0, 256, SKEW_LEN).astype(np.uint8)
    b.txhash_off[:] = 0
    b.txhash_len[:] = SKEW_LEN
    b.is_nil[:] = 0
    return b


@pytest.mark.gpu
def test_skew_refuses_only_the_owning_shard(rctx):
    """G = 3, every vote carrying the same TxHash, the stride sized for an even split: the owning
    shard is refused and its region untouched, the two empty shards get valid headers with n = 0;
    with route_stride the same batch succeeds and equals the host packer"""
    n, G = 1500, 3
    b = _one_hash_batch(n)
    flags = T.route_flags(b)
    per = (n + G - 1) // G + 64
    stride = int(T.lib().txv_route_bytes(per, per * SKEW_LEN, flags))
    full = T.route_stride(b)
    assert stride % 16 == 0 and int(T.lib().txv_route_bytes(n, SKEW_LEN, flags)) <= stride < full
    dev = _dev_zeros(G * full).view(G, full)
    t = rctx.route_submit_admitted(b, None, G, dev.data_ptr(), full)
    ok = rctx.route_wait(t, G)
    owner = int(np.argmax(ok["n"]))
    assert int(ok[owner]["n"]) == n and int(ok["n"].sum()) == n
    _expect_host(dev.view(-1), G, full, ok, b, None)
    # the even-split stride; `full` spare bytes behind the last region, so a wrong guard writes
    # inside the allocation
    dev2 = _dev_a5(G * stride + full)
    t = rctx.route_submit_admitted(b, None, G, dev2.data_ptr(), stride)
    with pytest.raises(T.TxvCapacityError) as ei:
        rctx.route_wait(t, G)
    m = ei.value.metas
    d = dev2.cpu().numpy()
    empty = int(T.lib().txv_route_bytes(0, 0, flags))
    for r in range(G):
        if r == owner:
            assert int(m[r]["reserved"]) == 1 and int(m[r]["n"]) == n and int(m[r]["bytes"]) == int(ok[owner]["bytes"])
            continue
        assert int(m[r]["reserved"]) == 0 and int(m[r]["n"]) == 0 and int(m[r]["bytes"]) == empty
        v = T.route_view(d[r * stride:r * stride + empty])
        assert v.n == 0
    # untouched: everything but the empty shards' own buffers
    keep = np.ones(d.size, bool)
    for r in range(G):
        if r != owner:
            keep[r * stride:r * stride + empty] = False
    assert (d[keep] == 0xA5).all()


@pytest.mark.gpu
def test_a_refused_ticket_between_two_good_ones(rctx):
    G = 1
    good1, good2, bad = _batch(900, 2000), _batch(901, 1500), _shared_batch()
    s1, s2 = _statuses(910, 2000), _statuses(911, 1500)
    flags = T.route_flags(bad)
    need, small = int(T.lib().txv_route_bytes(256, 16384, flags)), int(T.lib().txv_route_bytes(256, 256, flags))
    st1, st2 = T.route_stride(good1), T.route_stride(good2)
    d1, d2, db = _dev_zeros(st1), _dev_zeros(st2), _dev_a5(need)
    t1 = rctx.route_submit_admitted(good1, s1, G, d1.data_ptr(), st1)
    tb = rctx.route_submit_admitted(bad, None, G, db.data_ptr(), small)
    t2 = rctx.route_submit_admitted(good2, s2, G, d2.data_ptr(), st2)
    m1 = rctx.route_wait(t1, G)
    with pytest.raises(T.TxvCapacityError):
        rctx.route_wait(tb, G)
    m2 = rctx.route_wait(t2, G)
    _expect_host(d1, G, st1, m1, good1, s1)
    _expect_host(d2, G, st2, m2, good2, s2)
    assert bool((db == 0xA5).all())


@pytest.mark.gpu
def test_async_routed_buffers_tally_like_submit_votes():
    """one ticket's three buffers from the async route through submit_routed on receiving contexts:
    the statuses and commit events the same votes give through submit_votes"""
    G = 3
    owner = T.Context(max_batch=4096, max_txs=256, max_validators=8)
    ranks = []
    try:
        rnd = random.Random(77)
        seeds = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(4)]
        pubs = owner.keygen(seeds)
        powers = [1, 2, 3, 1]
        owner.set_validators(pubs, powers, "test_chain_id")
        addrs, _ = owner.validator_info()
        hashes = ["".join(rnd.choice("0123456789ABCDEF") for _ in range(64)) for _ in range(60)]
        votes, signer = [], []
        for i in range(900):
            vi = rnd.randrange(4)
            votes.append(T.TxVote(Height=1, TxHash=rnd.choice(hashes), Timestamp=(1_700_000_000, i + 1),
                                  ValidatorAddress=addrs[vi]))
            signer.append(vi)
        sigs = owner.sign_votes(T.VoteBatch.from_votes(votes), np.array(signer, np.uint32), "test_chain_id")
        for v, s in zip(votes, sigs):
            v.Signature = s.tobytes()
        for i in range(0, 900, 9):
            s = bytearray(votes[i].Signature); s[7] ^= 2; votes[i].Signature = bytes(s)
        votes += [votes[rnd.randrange(900)] for _ in range(90)] + [None] * 5
        rnd.shuffle(votes)
        b = T.VoteBatch.from_votes(votes)
        st = np.array([T.POOL_OK if rnd.random() < 0.9 else T.POOL_ERR_IN_CACHE for _ in range(b.n)], np.uint8)
        stride = T.route_stride(b)
        dev = _dev_zeros(G * stride)
        metas = owner.route_wait(owner.route_submit_admitted(b, st, G, dev.data_ptr(), stride), G)
        idx = sharding.route_admitted(b, st, G, T.POOL_OK)
        # the ranks' TxHash sets are disjoint, so one receiving context per path takes all three
        for _ in range(2):
            ctx = T.Context(max_batch=4096, max_txs=256, max_validators=8)
            ranks.append(ctx)
            ctx.set_validators(pubs, powers, "test_chain_id")
        fired = 0
        for r in range(G):
            mine = sharding.subset(b, idx[r])
            assert int(metas[r]["n"]) == mine.n > 100
            got = ranks[0].wait_votes(ranks[0].submit_routed(dev.data_ptr() + r * stride, metas[r]))
            want = ranks[1].wait_votes(ranks[1].submit_votes(mine))
            assert np.array_equal(got[0], want[0]), r
            assert np.array_equal(got[1], want[1]), r
            fired += len(got[1])
        assert fired > 0
    finally:
        owner.close()
        for c in ranks:
            c.close()
