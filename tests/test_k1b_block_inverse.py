"""K1b's one inversion per block (txv_k_scalarmult_dyn's hand-off, kernels_verify.hip): verdicts
against the oracle at the batch sizes and idle patterns at which the hand-off takes another path.

The context has lane_votes = 8 and the default wide base table, so batches of every size run the
work-stealing kernel.  A chunk is 64 consecutive items (one per lane) and goes to whichever wave
claims it; a block of 8 waves starting together over 8 chunks or fewer normally takes one each, and
a wave that gets none joins the hand-off with P = 1.  An item K1a rejects (ok != 2) leaves its lane
idle in the walk (the identity entries); a chunk of nothing but rejects is still a group of its wave.

Every (key, message, signature) item comes from one pool whose oracle verdicts are computed once."""
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHAIN = "test_chain_id"
# kinds of tests/golden/verify_vectors.json: small-order and mixed-order keys, R' on a small-order
# point; and the ones K1a rejects before K1b (s >= L, the top bits of s, an undecodable key, a
# signature that is not 64 bytes)
GOLDEN_K1B = ("torsion_", "mixed_order_", "smallorder_rprime_")
GOLDEN_K1A = ("s_plus_L", "s_top_bit", "undecodable_pub", "len63")


@pytest.fixture(scope="module")
def pool(oracle_lib):
    """{category: [(pub, msg, sig, oracle verdict)]} and the validators' keys"""
    O = oracle_lib
    rnd = random.Random(814)
    seeds = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(4)]
    pubs = [O.pubkey(s) for s in seeds]
    cat = {k: [] for k in ("valid", "flip_r", "flip_s", "flip_msg", "golden", "k1a_reject")}

    def add(kind, pub, msg, sig):
        cat[kind].append((pub, msg, sig, O.verify(pub, msg, sig)))

    def flipped(b, lo, hi):
        b = bytearray(b)
        b[rnd.randrange(lo, hi)] ^= 1 << rnd.randrange(8)
        return bytes(b)

    for i in range(48):
        v = i % 4
        msg = O.signbytes(1, ("%064X" % rnd.getrandbits(256)).encode(), 1_700_000_000, i + 1, CHAIN.encode())
        sig = O.sign(seeds[v], msg)
        add("valid", pubs[v], msg, sig)
        if i < 16:
            add("flip_r", pubs[v], msg, flipped(sig, 0, 32))
            # a low bit of s (bytes 0..30): s stays below L, so K1a passes the vote on to K1b
            add("flip_s", pubs[v], msg, flipped(sig, 32, 63))
            add("flip_msg", pubs[v], flipped(msg, 0, len(msg)), sig)
    with open(os.path.join(HERE, "golden", "verify_vectors.json")) as f:
        vec = json.load(f)
    for g in vec:
        kind = "golden" if g["kind"].startswith(GOLDEN_K1B) else "k1a_reject" if g["kind"].startswith(GOLDEN_K1A) else None
        if kind:
            add(kind, bytes.fromhex(g["pub"]), bytes.fromhex(g["msg"]), bytes.fromhex(g["sig"]))
            assert cat[kind][-1][3] == g["expect"], g["kind"]
    assert all(c[3] for c in cat["valid"]) and not any(c[3] for k in ("flip_r", "flip_s", "flip_msg", "k1a_reject")
                                                       for c in cat[k])
    assert sum(c[3] for c in cat["golden"]) > 40 and sum(not c[3] for c in cat["golden"]) > 60
    assert len(cat["k1a_reject"]) == 56
    return cat, pubs


@pytest.fixture(scope="module")
def v8_ctx(pool):
    import txflow_amd as T
    # max_validators as in conftest's gpu_ctx: the same automatic window, which the items' ~55
    # distinct keys (throw-away tables at the registry's window) fit beside
    ctx = T.Context(max_batch=1 << 13, max_txs=1 << 10, max_validators=256, lane_votes=8)
    ctx.set_validators(pool[1], [1, 1, 1, 1], CHAIN)
    assert ctx.base_w in (24, 26)              # the wide base table: V = 8 runs txv_k_scalarmult_dyn
    yield ctx
    ctx.close()


def check(ctx, items):
    got = ctx.verify_bytes([c[0] for c in items], [c[1] for c in items], [c[2] for c in items])
    exp = np.array([c[3] for c in items])
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (len(items), bad[:20].tolist())


def mixed(cat, rnd):
    kind = rnd.choices(("valid", "flip_r", "flip_s", "flip_msg", "golden", "k1a_reject"), (40, 6, 6, 6, 27, 15))[0]
    return rnd.choice(cat[kind])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 4097])
def test_sizes_with_the_full_input_mix(v8_ctx, pool, n):
    """one lane, one wave, one block and their neighbours; 513 and 4097 leave the last block one
    nearly idle wave; every size mixes all six categories (from 63 on, each is present)"""
    cat, _ = pool
    rnd = random.Random(n)
    items = [mixed(cat, rnd) for _ in range(n)]
    if n >= 63:
        for j, kind in enumerate(cat):
            items[(7 * j + 3) % n] = cat[kind][j % len(cat[kind])]
    else:
        items = [cat["valid"][0]]
    check(v8_ctx, items)
    if n == 1:
        for kind in cat:                         # one lane of one wave, seven waves without a chunk
            check(v8_ctx, [cat[kind][-1]])


IDLE = {
    # name: (items, chunks made of K1a rejects only)
    "one_chunk_idle": (512, {3}),
    "only_chunk_7_has_work": (512, set(range(7))),
    "only_chunk_0_idle": (512, {0}),
    "a_whole_block_idle": (1024, set(range(8, 16))),
    "first_block_idle": (1024, set(range(8))),
    "everything_rejected": (512, set(range(8))),
}


@pytest.mark.parametrize("name", list(IDLE))
def test_idle_patterns(v8_ctx, pool, name):
    """whole chunks of K1a rejects: every lane of such a group is idle, and a block made of them
    (or a batch: no vote reaches an encoding) still goes through the hand-off"""
    cat, _ = pool
    n, idle = IDLE[name]
    rnd = random.Random(len(name) * 1000 + n)
    items = [rnd.choice(cat["k1a_reject"]) if i // 64 in idle else mixed(cat, rnd) for i in range(n)]
    check(v8_ctx, items)


def test_one_invalid_vote_in_every_wave_of_a_block(v8_ctx, pool):
    """512 votes, valid but for one per chunk (a different lane and a different kind of defect in
    each) that K1b itself must reject: a wrong 1/P_w out of the block's product chain would flip
    the verdicts of that wave's valid votes, and a 1/P_w handed to the wrong wave all of them"""
    cat, _ = pool
    rnd = random.Random(77)
    bad_golden = [c for c in cat["golden"] if not c[3]]
    items = [rnd.choice(cat["valid"]) for _ in range(512)]
    for c in range(8):
        defect = (cat["flip_r"], cat["flip_s"], cat["flip_msg"], bad_golden)[c % 4]
        items[64 * c + (9 * c + 5) % 64] = rnd.choice(defect)
    assert sum(not c[3] for c in items) == 8
    check(v8_ctx, items)
    # and with the valid votes only in the lanes around the bad ones, the rest idle
    sparse = [it if (i % 64 - (9 * (i // 64) + 5) % 64) in (-1, 0, 1) else cat["k1a_reject"][i % 56]
              for i, it in enumerate(items)]
    check(v8_ctx, sparse)


def test_more_than_V_chunks_per_wave(oracle_lib):
    """The smallest batch above verify_grid x 8 waves x 8 chunks x 64 votes (the grid is two blocks
    per CU): some wave must take a ninth chunk, so it inverts a full group by itself and hands a
    further, last group to its block.  4 validators, automatic table window, device-signed votes;
    one vote in 997 gets a signature bit flipped.  Expected verdicts: the flipped votes are invalid
    and the others valid by construction, and the oracle confirms every flipped vote and a sample
    of 400 others (it would need minutes for all 2.1M)."""
    import torch
    import txflow_amd as T
    from txflow_amd.workload import CHAIN_ID, Workload
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_min = 2 * cus * 8 * 8 * 64 + 1
    n_txs = (n_min + 3) // 4
    ctx = T.Context(max_batch=4 * n_txs, max_txs=n_txs, max_validators=16, lane_votes=8)
    try:
        wl = Workload(ctx, 4, n_txs, seed=2097)
        assert ctx.base_w in (24, 26) and wl.n >= n_min
        rnd = random.Random(5)
        flips = np.arange(rnd.randrange(997), wl.n, 997)
        for i in flips:
            wl.batch.sig[64 * int(i) + rnd.randrange(63)] ^= 1 << rnd.randrange(8)
        st = ctx.verify_batch(wl.batch)
        exp = np.ones(wl.n, bool)
        exp[flips] = False
        bad = np.flatnonzero((st == T.ADDED) != exp)
        assert bad.size == 0, bad[:20].tolist()
        sample = np.concatenate([flips, np.random.default_rng(3).integers(0, wl.n, 400)])
        for i in sample:
            v = wl.vote(int(i))
            msg = oracle_lib.signbytes(1, v["txhash"], v["ts_sec"], v["ts_nanos"], CHAIN_ID.encode())
            assert oracle_lib.verify(wl.pubs[wl.val_of[i]], msg, v["sig"]) == bool(exp[i]), int(i)
    finally:
        ctx.close()
