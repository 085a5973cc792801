"""K1a without a message buffer (go-txflow_amd/csrc/signbytes_dev.h): the AddVote chain hashes
R || A || SignBytes assembled in registers from the vote's field columns.  Every vote here is signed
by sign_votes, whose SignBytes come from txv_k_signbytes (the buffer path), and every status is
checked against the sequential oracle; verify_batch (buffer path) must agree vote for vote."""
import copy
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN = "test_chain_id"
POWERS = [1, 2, 3, 1]
HEIGHTS = (0, 1, 2 ** 63 - 1, -1)
HASH_LENS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100)
SECS = (0, 1, 127, 128, 2 ** 31, 2 ** 35 - 1)
NANOS = (0, 1, 127, 128, 16383, 16384, 2 ** 28 - 1, 2 ** 28, 999999999)
SIZES = (1, 64, 65, 200)

_cache = {}


def _edge_vote(T, rnd):
    return T.TxVote(Height=rnd.choice(HEIGHTS), TxHash=bytes(rnd.getrandbits(8) for _ in range(rnd.choice(HASH_LENS))),
                    Timestamp=(rnd.choice(SECS), rnd.choice(NANOS)))


def _common_vote(T, rnd, hl):
    """the shapes the compile-time layout takes: every nanos length, heights of every width"""
    return T.TxVote(Height=rnd.choice((1, 77, -1, 2 ** 40 + 3)), TxHash=bytes(rnd.getrandbits(8) for _ in range(hl)),
                    Timestamp=(rnd.choice((2 ** 28, 1_700_000_000, 2 ** 35 - 1)), rnd.choice(NANOS)))


def _votes(T, kind, n, rnd):
    """n votes with distinct (TxHash, validator): a properly signed one is ADDED"""
    votes, signer, seen = [], [], set()
    while len(votes) < n:
        i = len(votes)
        if kind == "u32":
            v = _common_vote(T, rnd, 32)
        elif kind == "u64":
            v = _common_vote(T, rnd, 64)
        elif (i // 64) % 3 == 1:      # "mixed": waves 1 and 2 uniform, the others every shape side by side
            v = _common_vote(T, rnd, 64)
        elif (i // 64) % 3 == 2:
            v = _common_vote(T, rnd, 32)
        else:
            v = _common_vote(T, rnd, rnd.choice((32, 64))) if i % 4 == 3 else _edge_vote(T, rnd)
        k = rnd.randrange(4)
        if (v.TxHash, k) in seen:
            continue
        seen.add((v.TxHash, k))
        votes.append(v)
        signer.append(k)
    return votes, signer


def _signed(ctx, kind, n):
    """(seeds, pubs, votes): signed once per (kind, n) -- ed25519 signatures do not depend on the context"""
    import txflow_amd as T
    if "keys" not in _cache:
        rnd = random.Random(99)
        seeds = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(4)]
        _cache["keys"] = (seeds, ctx.keygen(seeds))
    seeds, pubs = _cache["keys"]
    ctx.set_validators(pubs, POWERS, CHAIN)
    ctx.reset_flow()
    if (kind, n) not in _cache:
        rnd = random.Random(1000 * n + len(kind) + ord(kind[1]))
        addrs, ok = ctx.validator_info()
        assert ok.all()
        votes, signer = _votes(T, kind, n, rnd)
        for v, k in zip(votes, signer):
            v.ValidatorAddress = addrs[k]
        sigs = ctx.sign_votes(T.VoteBatch.from_votes(votes), np.array(signer, np.uint32), CHAIN)
        for v, s in zip(votes, sigs):
            v.Signature = s.tobytes()
        _cache[(kind, n)] = votes
    return seeds, pubs, copy.deepcopy(_cache[(kind, n)])


def _oracle(oracle_lib, pubs, batches):
    flow = oracle_lib.Flow(pubs, POWERS, CHAIN.encode())
    out = []
    for b in batches:
        st, _, fired = flow.add_batch(b)
        out.append(st.astype(np.uint8) | (fired.astype(np.uint8) << 7))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["mixed", "u32", "u64"])
def test_signed_votes_are_added(gpu_ctx, oracle_lib, kind, n):
    import txflow_amd as T
    _, pubs, votes = _signed(gpu_ctx, kind, n)
    b = T.VoteBatch.from_votes(votes)
    st, _ = gpu_ctx.add_votes(b)
    assert np.all((st & 0x7F) == T.ADDED), np.nonzero((st & 0x7F) != T.ADDED)[0][:10]
    assert np.array_equal(st, _oracle(oracle_lib, pubs, [b])[0])
    assert np.all(gpu_ctx.verify_batch(b) == T.ADDED)


def _tamper(votes, rnd):
    """every fourth vote changed after signing: height, a TxHash byte, sec, nanos in turn; every
    eleventh signature cut to 63 bytes"""
    for i, v in enumerate(votes):
        if i % 4 == 1:
            k = i // 4 % 4
            if k == 0:
                v.Height ^= 1
            elif k == 1 and v.TxHash:
                t = bytearray(v.TxHash); t[rnd.randrange(len(t))] ^= 1 << rnd.randrange(8); v.TxHash = bytes(t)
            elif k == 2:
                v.Timestamp = (v.Timestamp[0] ^ 1, v.Timestamp[1])
            else:
                v.Timestamp = (v.Timestamp[0], v.Timestamp[1] ^ 1)
        if i % 11 == 5:
            v.Signature = v.Signature[:63]


@pytest.mark.parametrize("n", SIZES)
def test_changed_votes_nil_entries_and_short_signatures(gpu_ctx, oracle_lib, n):
    import txflow_amd as T
    _, pubs, votes = _signed(gpu_ctx, "mixed", n)
    rnd = random.Random(n)
    _tamper(votes, rnd)
    b = T.VoteBatch.from_votes(votes)
    vb = gpu_ctx.verify_batch(b)                       # the buffer path's verdicts
    with_nil = []
    for i, v in enumerate(votes):
        if i % 13 == 7:
            with_nil.append(None)
        with_nil.append(v)
    bn = T.VoteBatch.from_votes(with_nil)
    st, _ = gpu_ctx.add_votes(bn)
    exp = _oracle(oracle_lib, pubs, [bn])[0]
    assert np.array_equal(st, exp), [(int(i), int(st[i]), int(exp[i])) for i in np.nonzero(st != exp)[0][:10]]
    live = np.array([v is not None for v in with_nil])
    assert np.all(st[~live] == T.ERR_NIL)
    # distinct (TxHash, validator) pairs: a vote is ADDED exactly when its signature verifies
    assert np.array_equal((st[live] & 0x7F) == T.ADDED, vb == T.ADDED)
    if n >= 64:
        assert 0 < np.count_nonzero(vb == T.ADDED) < n


def test_two_staged_slots_back_to_back(gpu_ctx, oracle_lib):
    """two runs queued without a wait between them give what each gives alone: K1b's claim counters
    start from zero in both"""
    import txflow_amd as T
    _, pubs, va = _signed(gpu_ctx, "mixed", 200)
    _, _, vb = _signed(gpu_ctx, "u64", 65)
    _tamper(va, random.Random(5))
    ba, bb = T.VoteBatch.from_votes(va), T.VoteBatch.from_votes(vb)
    alone = []
    for b in (ba, bb):
        gpu_ctx.reset_flow()
        gpu_ctx.stage(0, b)
        gpu_ctx.run_staged(0)
        alone.append(gpu_ctx.fetch_staged(0, b.n)[0].copy())
    gpu_ctx.reset_flow()
    gpu_ctx.stage(0, ba)
    gpu_ctx.stage(1, bb)
    gpu_ctx.run_staged(0)
    gpu_ctx.run_staged(1)
    got = [gpu_ctx.fetch_staged(0, ba.n)[0].copy(), gpu_ctx.fetch_staged(1, bb.n)[0].copy()]
    exp = _oracle(oracle_lib, pubs, [ba, bb])          # no TxHash in both: the second sees nothing of the first
    for g, a, e in zip(got, alone, exp):
        assert np.array_equal(g, a)
        assert np.array_equal(g, e)
