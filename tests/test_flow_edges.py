"""TxFlow's set table and stake tally at their edges (csrc/kernels_flow.hip).

A. The set table is keyed by the raw TxHash bytes: two key paths switched at kKeyRegBytes = 64,
   load_key's 16-way realignment with per-word tail masks, hash_regs (bit-identical to
   txv_hash::hash_chunks), ld64u / key_eq for longer keys, NewSetAct's masked copy into the key slots
   or the overflow arena, txv_k_lookup for the readers.  Here: keys equal up to their last byte, keys
   ending in zero bytes, keys that are prefixes of one another, keys that first differ at byte 64, a
   key at every off % 16 with 0xFF in the gaps, a key ending at the arena's last byte, keys sharing
   one offset, kept keys met again at another alignment, a full table and a full overflow arena.
B. The stake tally (txv_k_tally_cross and what reads set_sum) is 64-bit throughout.  Here: powers up
   to tendermint's MaxTotalVotingPower = MaxInt64 / 8, sets that stop at quorum - 1 or land on quorum,
   sets with exactly Cap (128, 1024) and Cap + 1 ADDED votes, crossing votes on the digit
   boundaries of the 6-bit search (63 | 64, 4095 | 4096), and one batch of 2^18 votes (the stamped-set
   compaction at kStampCompactMin).

The expectation is tests/flow_model.py, a sequential model in plain Python (stake as unbounded ints)
that tests/test_flow_model.py pins to the C oracle on these same inputs.  Every comparison is exact
equality.  Votes are signed once per module with the oracle's signer; each VoteBatch is laid out by
hand (txhash_arena, txhash_off, txhash_len) so the test controls where every key lies."""
import random
import time

import numpy as np
import pytest

import flow_model as M
import oracle as O
from test_configs import _cores, _expected, _first_fired

CHAIN = b"test_chain_id"
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _layout(keys, align=None, fill=0xFF):
    """one copy of each vote's key in an arena: back to back (align None), or every copy at an offset
    with off % 16 == align and `fill` bytes in the gaps; nothing follows the last key"""
    arena, offs = bytearray(), []
    for k in keys:
        if align is not None:
            arena += bytes([fill]) * ((align - len(arena)) % 16)
        offs.append(len(arena))
        arena += k
    return bytes(arena), offs


def _batch(votes, align=None, placed=None):
    """oracle-style dicts (nil=True: a nil entry) -> VoteBatch; placed = (arena, offsets) overrides the layout"""
    import txflow_amd as T
    n = len(votes)
    live = [v for v in votes if not v.get("nil")]
    arena, offs = placed if placed is not None else _layout([v["txhash"] for v in live], align)
    off = np.zeros(n, np.uint32); ln = np.zeros(n, np.uint32)
    h = np.zeros(n, np.int64); ts = np.zeros(n, np.int64); tn = np.zeros(n, np.int32)
    addr = np.zeros((n, 20), np.uint8); al = np.zeros(n, np.uint32)
    sig = np.zeros((n, 64), np.uint8); sl = np.zeros(n, np.uint32)
    nil = np.zeros(n, np.uint8); tk = np.zeros((n, 32), np.uint8)
    j = 0
    for i, v in enumerate(votes):
        if v.get("nil"):
            nil[i] = 1
            continue
        off[i], ln[i] = offs[j], len(v["txhash"])
        j += 1
        h[i], ts[i], tn[i] = v["height"], v["ts_sec"], v["ts_nanos"]
        al[i] = len(v["addr"]); addr[i, :len(v["addr"])] = np.frombuffer(v["addr"], np.uint8)
        sl[i] = len(v["sig"]); sig[i] = np.frombuffer(v["sig"], np.uint8)
        tk[i] = np.frombuffer(v["txkey"], np.uint8)
    b = T.VoteBatch(n, height=h, txhash_arena=arena, txhash_off=off, txhash_len=ln, ts_sec=ts, ts_nanos=tn,
                    addr=addr, addr_len=al, sig=sig, sig_len=sl, is_nil=nil, txkey=tk)
    for i, v in enumerate(votes):                             # the layout holds what it was asked to hold
        assert v.get("nil") or b.txhash(i) == v["txhash"]
    return b


def _events(ev):
    return [(int(e["vote_index"]), int(e["tx_index"]), int(e["sum"])) for e in ev]


def _check(st, ev, exp, what):
    est, efired, eev = exp
    want = np.array(M.expected(est, efired), np.uint8)
    bad = np.nonzero(st != want)[0]
    assert len(bad) == 0, (what, [(int(i), int(st[i]), int(want[i])) for i in bad[:10]])
    assert _events(ev) == [(e["vote_index"], e["tx_index"], e["sum"]) for e in eev], what


def _run(ctx, model, votes, ok, what, **layout):
    """one batch through txv_add_votes and through the model: statuses, fired bits, events"""
    b = _batch(votes, **layout)
    st, ev = ctx.add_votes(b, ev_cap=max(b.n, 1))
    _check(st, ev, model.add_votes(votes, ok), what)
    return b


def _start(ctx, pubs, powers):
    ctx.set_validators(pubs, powers, CHAIN.decode())
    ctx.reset_flow()


def _readers(ctx, model, signer, keys, what):
    """txv_query_tx, txv_get_votes and txv_make_commit of every key (the txv_k_lookup path)"""
    for k in keys:
        assert ctx.query_tx(k) == model.query(k), (what, k)
        acc = model.get_votes(k)
        assert [(v, s) for v, _, s in ctx.get_votes(k)] == acc, (what, k)
        if model.query(k)[1]:
            assert ctx.make_commit(k) == O.commit_bytes(k, [signer.by_sig[(k, s)] for _, s in acc]), (what, k)


class _Signer(M.Signer):
    """M.Signer that remembers every vote it made by (TxHash, signature), for MakeCommit's expectation"""

    def __init__(self, *a):
        super().__init__(*a)
        self.by_sig = {}

    def vote(self, txhash, v, kind="ok"):
        vote, ok = super().vote(txhash, v, kind)
        if not vote.get("nil"):
            self.by_sig[(txhash, vote["sig"])] = vote
        return vote, ok


def _raises_rc(rc, fn, *a):
    import txflow_amd as T
    with pytest.raises(T.TxvInfraError) as e:
        fn(*a)
    assert f"({rc})" in str(e.value), str(e.value)
    return str(e.value)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ctx():
    import txflow_amd as T
    c = T.Context(max_batch=8192, max_txs=1024, max_validators=1056, table_w=4)   # radix-16 tables build fast
    yield c
    c.close()


@pytest.fixture(scope="module")
def vals(oracle_lib):
    """1025 validators (B3's largest registry); the other tests use the first few"""
    seeds, pubs, addrs = M.validator_keys(O, 1025)
    return seeds, pubs, addrs, _Signer(O, seeds, addrs, CHAIN)


@pytest.fixture(scope="module")
def fam(vals):
    """A1's key family and its votes in arrival order, signed once"""
    seeds, pubs, addrs, signer = vals
    keys = M.key_family()
    assert len(set(keys)) == len(keys) >= 320
    votes, ok = signer.votes([(keys[k], v, "ok") for k, v in M.family_order(len(keys))])
    return keys, votes, ok


# ------------------------------------------------------------------ A1
def test_a1_key_family(ctx, vals, fam):
    seeds, pubs, addrs, signer = vals
    keys, votes, ok = fam
    _start(ctx, pubs[:4], [1] * 4)
    model = M.FlowModel(addrs[:4], [1] * 4)
    assert model.quorum == 3
    for k, s in enumerate(range(0, len(votes), 300)):
        _run(ctx, model, votes[s:s + 300], ok[s:s + 300], f"batch {k}")
    assert ctx.num_tx_sets() == model.num_sets() == len(keys)
    assert all(model.query(k) == (3, True) for k in keys)
    _readers(ctx, model, signer, keys, "key family")
    assert ctx.query_tx(keys[5] + b"\0") is None and ctx.query_tx(b"\0" * 81) is None   # a longer run of zeros is no set


# ------------------------------------------------------------------ A2
def _first_batch(fam):
    keys, votes, ok = fam
    votes, ok = list(votes[:300]), list(ok[:300])
    last = max(i for i, v in enumerate(votes) if len(v["txhash"]) > 0)
    votes[last], votes[-1] = votes[-1], votes[last]           # the batch ends with a key that has bytes
    ok[last], ok[-1] = ok[-1], ok[last]
    return votes, ok


@pytest.mark.parametrize("a", range(16))
def test_a2_every_alignment(ctx, vals, fam, a):
    seeds, pubs, addrs, signer = vals
    votes, ok = _first_batch(fam)
    _start(ctx, pubs[:4], [1] * 4)
    model = M.FlowModel(addrs[:4], [1] * 4)
    b = _run(ctx, model, votes, ok, f"alignment {a}", align=a)
    assert (b.txhash_off % 16 == a).all()
    end = int(b.txhash_off[-1]) + int(b.txhash_len[-1])
    assert b.txhash_len[-1] > 0 and end == b.txhash_arena.size    # the last key ends at the arena's last byte
    used = np.zeros(b.txhash_arena.size, bool)
    for o, l in zip(b.txhash_off.tolist(), b.txhash_len.tolist()):
        used[o:o + l] = True
    assert (b.txhash_arena[~used] == 0xFF).all() and (~used).sum() > 0
    assert ctx.num_tx_sets() == model.num_sets()
    _readers(ctx, model, signer, sorted({v["txhash"] for v in votes}), f"alignment {a}")


@pytest.mark.parametrize("at", [0, 5, 15])
def test_a2_prefixes_at_one_offset(ctx, vals, at):
    """base[:n] for every n in 0..80 at the same offset of one shared buffer: the votes differ in
    txhash_len only, and the longest key ends at the arena's last byte"""
    seeds, pubs, addrs, signer = vals
    base = bytes(range(1, 81))
    pairs = [(n, v) for n in range(81) for v in range(3)]
    random.Random(7).shuffle(pairs)
    votes, ok = signer.votes([(base[:n], v, "ok") for n, v in pairs])
    _start(ctx, pubs[:4], [1] * 4)
    model = M.FlowModel(addrs[:4], [1] * 4)
    _run(ctx, model, votes, ok, f"shared offset {at}", placed=(b"\xFF" * at + base, [at] * len(votes)))
    assert ctx.num_tx_sets() == model.num_sets() == 81
    _readers(ctx, model, signer, [base[:n] for n in range(81)], f"shared offset {at}")


# ------------------------------------------------------------------ A3
def test_a3_kept_keys_across_batches(ctx, vals, fam, oracle_lib):
    seeds, pubs, addrs, signer = vals
    keys, _, _ = fam
    rnd = random.Random(33)
    first = [(k, 0, "ok") for k in keys]
    rnd.shuffle(first)
    alt_keys = keys[::5]
    second = first + [(k, v, "ok") for k in keys for v in (1, 2)] + [(k, 0, "alt") for k in alt_keys]
    rnd.shuffle(second)
    # the oracle's verdict for a second valid signature of a validator that already has a vote in the set
    probe, _ = signer.vote(keys[7], 0, "alt")
    assert oracle_lib.verify(pubs[0], oracle_lib.signbytes(1, keys[7], M.SEC, probe["ts_nanos"], CHAIN), probe["sig"])
    flow = oracle_lib.Flow(pubs[:4], [1] * 4, CHAIN)
    _start(ctx, pubs[:4], [1] * 4)
    model = M.FlowModel(addrs[:4], [1] * 4)
    for part, a in ((first, 3), (second, 11)):                # batch 2 meets every kept key at another alignment
        votes, ok = signer.votes(part)
        exp = model.add_votes(votes, ok)
        ost, _, ofired = flow.add_votes(votes)
        assert exp[0] == [int(x) for x in ost] and exp[1] == [bool(x) for x in ofired]
        b = _batch(votes, align=a)
        st, ev = ctx.add_votes(b, ev_cap=b.n)
        _check(st, ev, exp, f"batch at alignment {a}")
        if a == 3:
            assert ctx.num_tx_sets() == len(keys) and set(exp[0]) == {M.ADDED}
    by_kind = {}
    for (k, v, kind), st in zip(second, exp[0]):
        by_kind.setdefault((v, kind), set()).add(st)
    assert by_kind[(0, "ok")] == {M.DUPLICATE} and by_kind[(0, "alt")] == {M.ERR_NONDETERMINISTIC}
    assert by_kind[(1, "ok")] == by_kind[(2, "ok")] == {M.ADDED}
    assert ctx.num_tx_sets() == model.num_sets() == len(keys)   # no new set
    _readers(ctx, model, signer, keys, "after batch 2")


# ------------------------------------------------------------------ A4
def _fill(c, model, signer, keys, cuts, what):
    """first and second votes of `keys` in the batches `cuts` names, then every third vote: the
    events of the last batch carry every set's id"""
    for lo, hi in zip(cuts, cuts[1:]):
        items = [(k, v, "ok") for k in keys[lo:hi] for v in (0, 1)]
        random.Random(hi).shuffle(items)
        votes, ok = signer.votes(items)
        _run(c, model, votes, ok, f"{what}: keys {lo}..{hi}")
    votes, ok = signer.votes([(k, 2, "ok") for k in reversed(keys)])
    b = _batch(votes)
    st, ev = c.add_votes(b, ev_cap=b.n)
    exp = model.add_votes(votes, ok)
    _check(st, ev, exp, f"{what}: third votes")
    assert sorted(int(e["tx_index"]) for e in ev) == list(range(len(keys)))
    return {votes[int(e["vote_index"])]["txhash"]: int(e["tx_index"]) for e in ev}


def test_a4_full_table_and_refusal(vals, fam):
    """max_txs sets exactly, in one batch and split 100 / 156; one key more is refused with
    TXV_ECAPACITY (include/txvote.h: txv_config, txv_reset_flow) and txv_reset_flow recovers"""
    import txflow_amd as T
    seeds, pubs, addrs, signer = vals
    fkeys, _, _ = fam
    keys = fkeys[-32:] + fkeys[:224]                           # 32 keys of 127..256 bytes, 224 of 0..56
    assert len(keys) == 256 and len({len(k) for k in keys}) > 40
    c = T.Context(max_txs=256, max_batch=512, max_validators=8, table_w=4)
    try:
        _start(c, pubs[:4], [1] * 4)
        for cuts in ((0, 256), (0, 100, 256)):
            c.reset_flow()
            model = M.FlowModel(addrs[:4], [1] * 4)
            ids = _fill(c, model, signer, keys, cuts, f"cuts {cuts}")
            assert ids == {k: model.set_id(k) for k in keys}   # every key its first-seen id
            assert c.num_tx_sets() == 256
            _readers(c, model, signer, keys, f"cuts {cuts}")
        more = b"one key more"
        extra, ok = signer.votes([(more, 0, "ok")])
        msg = _raises_rc(T.E_CAPACITY, c.add_votes, _batch(extra))
        assert "max_txs" in msg
        _raises_rc(T.E_CAPACITY, c.add_votes, _batch(extra))   # refused until the reset
        c.reset_flow()
        model = M.FlowModel(addrs[:4], [1] * 4)
        _run(c, model, extra, ok, "the refused vote again, after the reset")
        ids = _fill(c, model, signer, [more] + keys[:40], (0, 41), "after the reset")
        assert ids[more] == 0 and c.num_tx_sets() == 41
    finally:
        c.close()


def test_a4_full_key_arena_and_refusal(vals):
    """keys longer than the 64-byte key slot live in the overflow arena (key_arena_bytes, each rounded
    up to 8): eight 128-byte keys fit 1040 bytes, a ninth is refused, txv_reset_flow recovers"""
    import txflow_amd as T
    seeds, pubs, addrs, signer = vals
    keys = [bytes((j + 1) % 256 for j in range(127)) + bytes([i]) for i in range(9)]   # equal up to the last byte
    c = T.Context(max_txs=256, max_batch=512, max_validators=8, table_w=4, key_arena_bytes=1040)
    try:
        _start(c, pubs[:4], [1] * 4)
        model = M.FlowModel(addrs[:4], [1] * 4)
        _fill(c, model, signer, keys[:8], (0, 8), "eight long keys")
        _readers(c, model, signer, keys[:8], "eight long keys")
        short, ok = signer.votes([(b"short keys take no arena", v, "ok") for v in range(3)])
        _run(c, model, short, ok, "a short key beside the full arena")
        ninth, ok = signer.votes([(keys[8], 0, "ok")])
        msg = _raises_rc(T.E_CAPACITY, c.add_votes, _batch(ninth))
        assert "key_arena_bytes" in msg
        c.reset_flow()
        model = M.FlowModel(addrs[:4], [1] * 4)
        _fill(c, model, signer, keys[1:9], (0, 3, 8), "after the reset")
        _readers(c, model, signer, keys[1:9], "after the reset")
    finally:
        c.close()


# ------------------------------------------------------------------ B1
@pytest.mark.parametrize("which", range(len(M.B1_POWERS)))
def test_b1_stake_width(ctx, vals, which):
    import torch
    import txflow_amd as T
    seeds, pubs, addrs, signer = vals
    powers = M.B1_POWERS[which]
    hashes = M.b1_hashes()
    votes, ok = signer.votes([(hashes[t], v, kind) for t, v, kind in M.b1_stream()])
    n_v, cap = M.B1_VALS, 64
    _start(ctx, pubs[:n_v], powers)
    assert ctx.total_power() == sum(powers)
    model = M.FlowModel(addrs[:n_v], powers)
    words = T.commit_state_bytes(cap) // 4
    sinks = [torch.zeros(words, dtype=torch.int32, device="cuda:0") for _ in range(T.SUBMIT_RING)]
    try:
        for sl in range(T.SUBMIT_RING):
            ctx.set_commit_sink(sl, sinks[sl].data_ptr(), cap)
        n_ev = 0
        for s in range(0, len(votes), M.B1_CUT):
            part, pok = votes[s:s + M.B1_CUT], ok[s:s + M.B1_CUT]
            tk = ctx.submit_votes(_batch(part))
            st, ev = ctx.wait_votes(tk, ev_cap=len(part))
            exp = model.add_votes(part, pok)
            _check(st, ev, exp, f"powers {which}, batch at {s}")
            n_ev += len(ev)
            # the packed commit state the device wrote behind this batch: 8-byte sums and commit bits by set id
            packed = sinks[(tk - 1) % T.SUBMIT_RING].cpu().numpy().view(np.uint8)
            committed, sums, _ = T.commit_state_unpack(packed, cap)
            by_id = sorted(model.sets.values(), key=lambda x: x["id"])
            assert [int(x) for x in sums] == [x["sum"] for x in by_id], f"powers {which}, batch at {s}"
            assert [bool(x) for x in committed] == [x["maj23"] for x in by_id]
        assert n_ev == M.B1_TXS
        for h in hashes:
            assert ctx.query_tx(h) == model.query(h) == (sum(powers), True)
    finally:
        for sl in range(T.SUBMIT_RING):
            ctx.set_commit_sink(sl, None)


# ------------------------------------------------------------------ B2
def test_b2_exact_threshold(ctx, vals):
    seeds, pubs, addrs, signer = vals
    powers = [2**40] * 3 + [1] * 3
    _start(ctx, pubs[:6], powers)
    model = M.FlowModel(addrs[:6], powers)
    q = model.quorum
    below = [0, 1, 3, 4]                                      # two large and two small: quorum - 1
    assert sum(powers[v] for v in below) == q - 1 and sum(powers[v] for v in below + [5]) == q
    x, y, z = b"stops one short", b"lands on quorum in one batch", b"lands on quorum with prior stake"
    # one batch: x stops at quorum - 1; y's fifth vote lands on quorum
    votes, ok = signer.votes([(x, v, "ok") for v in below] + [(y, v, "ok") for v in below + [5]])
    _run(ctx, model, votes, ok, "batch 1")
    assert model.query(x) == (q - 1, False) and model.query(y) == (q, True)
    assert ctx.query_tx(x) == (q - 1, False) and ctx.query_tx(y) == (q, True)
    _raises_rc(-1, ctx.make_commit, x)                        # TXV_ESTATE: MakeCommit without +2/3
    # z: quorum - 1 in an earlier batch, then the cross step searches for need = 1
    votes, ok = signer.votes([(z, v, "ok") for v in below] + [(x, 0, "ok")])
    _run(ctx, model, votes, ok, "batch 2")
    assert model.query(z) == (q - 1, False) and ctx.query_tx(z) == (q - 1, False)
    votes, ok = signer.votes([(x, 1, "ok"), (z, 5, "ok"), (z, 2, "ok")])
    exp = model.add_votes(votes, ok)
    assert [(e["vote_index"], e["sum"]) for e in exp[2]] == [(1, q + 2**40)] and exp[1] == [False, True, True]
    b = _batch(votes)
    st, ev = ctx.add_votes(b, ev_cap=b.n)
    _check(st, ev, exp, "batch 3")
    assert ctx.query_tx(x) == model.query(x) == (q - 1, False)  # replays moved nothing
    _raises_rc(-1, ctx.make_commit, x)
    _readers(ctx, model, signer, [x, y, z], "threshold sets")


# ------------------------------------------------------------------ B3
@pytest.mark.parametrize("n_vals", [128, 129, 1024, 1025])
def test_b3_list_capacity(ctx, vals, n_vals):
    """k == Cap and k == Cap + 1 ADDED votes of one set in one batch, for txv_k_tally_cross<128>
    (registries of <= 128 validators) and <1024>: set `full` gets a valid vote of every validator
    (k = n_vals), set `flip` the same with about 3 % of the signatures flipped, set `part` only some
    of the validators"""
    seeds, pubs, addrs, signer = vals
    rnd = random.Random(n_vals)
    powers = [M.MAXT // n_vals - i for i in range(n_vals)]
    assert min(powers) > 0 and sum(powers) <= M.MAXT
    full, flip, part = b"B3 full %d" % n_vals, b"B3 flip %d" % n_vals, b"B3 part %d" % n_vals
    items = [(full, v, "ok") for v in range(n_vals)]
    items += [(flip, v, "bad" if rnd.random() < 0.03 else "ok") for v in range(n_vals)]
    items += [(part, v, "ok") for v in rnd.sample(range(n_vals), n_vals * 3 // 5)]
    rnd.shuffle(items)
    votes, ok = signer.votes(items)
    assert 0 < ok.count(False) < n_vals // 10
    _start(ctx, pubs[:n_vals], powers)
    model = M.FlowModel(addrs[:n_vals], powers)
    exp = model.add_votes(votes, ok)
    assert len(model.get_votes(full)) == n_vals and model.query(full) == (sum(powers), True)
    assert model.query(flip)[1] and not model.query(part)[1] and len(exp[2]) == 2
    b = _batch(votes)
    st, ev = ctx.add_votes(b, ev_cap=b.n)
    _check(st, ev, exp, f"{n_vals} validators")
    for k in (full, flip, part):
        assert ctx.query_tx(k) == model.query(k)
        assert [(v, s) for v, _, s in ctx.get_votes(k)] == model.get_votes(k)


# ------------------------------------------------------------------ B4
def _b4_cases():
    out = []
    for n in (1, 2, 64, 65, 4096, 4097):
        for pos in sorted({n - 1, 0} | {p for p in (63, 64, 4095, 4096) if p < n}):
            out.append((n, pos))
    return out


@pytest.mark.parametrize("n,pos", _b4_cases())
def test_b4_digit_boundaries(ctx, vals, n, pos):
    """a batch of n votes, nil votes as filler, whose crossing vote sits at index pos: validators 0
    and 1 vote earlier in the batch where it has room, in an earlier batch where it has none"""
    seeds, pubs, addrs, signer = vals
    tx = b"B4 " + b"%061d" % 4
    v0, v1, v2, v3 = [signer.vote(tx, v)[0] for v in range(4)]
    _start(ctx, pubs[:4], [1] * 4)
    model = M.FlowModel(addrs[:4], [1] * 4)
    votes = [dict(nil=True) for _ in range(n)]
    votes[pos] = v2
    prior = []
    if pos >= 2:
        votes[0], votes[pos // 2 if pos // 2 > 0 else 1] = v0, v1
    elif pos == 1:
        prior, votes[0] = [v0], v1
    else:
        prior = [v0, v1]
    if pos < n - 1:
        votes[n - 1] = v3                                     # re-fires after the crossing
    if prior:
        _run(ctx, model, prior, None, "prior stake")
    exp = model.add_votes(votes, None)
    assert [(e["vote_index"], e["tx_index"], e["sum"]) for e in exp[2]] == [(pos, 0, 3 + (pos < n - 1))]
    assert exp[1] == [i >= pos and not votes[i].get("nil") for i in range(n)]
    b = _batch(votes)
    st, ev = ctx.add_votes(b, ev_cap=b.n)
    _check(st, ev, exp, f"n {n}, crossing at {pos}")
    assert ctx.query_tx(tx) == model.query(tx)


# ------------------------------------------------------------------ B5
def test_b5_large_batch_near_max_total(oracle_lib):
    """one batch of 2^18 votes (128 validators x 2048 txs): txv_flow_tally lists its stamped sets by
    compaction (kStampCompactMin); five validators hold nearly all of a total just under
    MaxTotalVotingPower.  Against the oracle's add_batch, as tests/test_tally_cross.py's _run"""
    import txflow_amd as T
    from txflow_amd.workload import Workload
    t0 = time.perf_counter()
    n_vals, n_txs = 128, 2048
    powers = np.ones(n_vals, np.int64)
    powers[[3, 77, 100, 120, 127]] = (M.MAXT - (n_vals - 5)) // 5
    assert M.MAXT - 5 < int(powers.sum()) <= M.MAXT
    c = T.Context(max_batch=1 << 18, max_txs=n_txs + 64, max_validators=n_vals, table_w=8)
    try:
        wl = Workload(c, n_vals, n_txs, 0x7478763105, powers=powers)
        assert wl.n == 1 << 18
        sig = wl.batch.sig.reshape(wl.n, 64)
        sig[np.random.default_rng(5).random(wl.n) < 0.03, 5] ^= 0x10
        st, ev = c.add_votes(wl.batch, ev_cap=n_txs)
        flow = oracle_lib.Flow(wl.pubs, wl.powers, CHAIN)
        ost, _, ofired = flow.add_batch(wl.batch, _cores())
        exp = _expected(ost, ofired)
        bad = np.nonzero(st != exp)[0]
        assert len(bad) == 0, [(int(i), int(st[i]), int(exp[i])) for i in bad[:10]]
        crossing = _first_fired(wl.batch, ofired, set())
        assert [int(e["vote_index"]) for e in ev] == crossing and len(crossing) > n_txs // 2
        u, f = np.unique(wl.tx_of, return_index=True)          # set ids: first-seen order
        first_seen = np.empty(n_txs, np.int64)
        first_seen[u[np.argsort(f)]] = np.arange(n_txs)
        for e in ev:
            t = int(wl.tx_of[e["vote_index"]])
            assert int(e["tx_index"]) == first_seen[t]
            assert (int(e["sum"]), True) == flow.query(wl.hashes[t].tobytes())
        for h in wl.hashes:
            assert c.query_tx(h.tobytes()) == flow.query(h.tobytes())
        assert c.num_tx_sets() == flow.num_sets() == n_txs
    finally:
        c.close()
    print(f"test_b5 wall time: {time.perf_counter() - t0:.1f} s")


# ------------------------------------------------------------------ txv_set_validators' range check
def test_set_validators_power_range(ctx, vals):
    """a negative power or a total above INT64_MAX / 8 (tendermint's MaxTotalVotingPower: the reference
    panics) is TXV_EINVAL with an error string and leaves the previous registry usable; a total of
    exactly INT64_MAX / 8 and a power of 0 are accepted"""
    seeds, pubs, addrs, signer = vals
    assert M.MAXT == (2**63 - 1) // 8
    _start(ctx, pubs[:4], [1] * 4)
    for powers, word in (([1, -1, 1, 1], "negative"), ([M.MAXT, 1, 0, 0], "total"), ([2**62, 0, 0, 0], "total"),
                         ([M.MAXT // 2 + 1] * 2 + [0, 0], "total"), ([-2**63, 2**62, 2**62, 0], "negative")):
        msg = _raises_rc(-22, ctx.set_validators, pubs[:4], powers, CHAIN.decode())
        assert word in msg, msg
    assert ctx.total_power() == 4 and ctx.n_vals == 4          # the registry of before, and it still tallies
    tx = b"after the refusals"
    votes, ok = signer.votes([(tx, v, "ok") for v in (2, 0, 3)])
    model = M.FlowModel(addrs[:4], [1] * 4)
    _run(ctx, model, votes, ok, "the previous registry")
    assert ctx.query_tx(tx) == (3, True)
    powers = [M.MAXT - 1, 1, 0, 0]
    _start(ctx, pubs[:4], powers)
    assert ctx.total_power() == M.MAXT
    model = M.FlowModel(addrs[:4], powers)
    votes, ok = signer.votes([(tx, v, "ok") for v in (2, 1, 3, 0)])   # 0, 1, 1, then MaxTotalVotingPower
    exp = model.add_votes(votes, ok)
    assert exp[1] == [False, False, False, True] and exp[2][0]["sum"] == M.MAXT
    b = _batch(votes)
    st, ev = ctx.add_votes(b, ev_cap=b.n)
    _check(st, ev, exp, "total of exactly INT64_MAX / 8")
    assert ctx.query_tx(tx) == (M.MAXT, True)
