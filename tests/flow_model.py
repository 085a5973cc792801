"""A sequential model of TxFlow.addVote / TxVoteSet.AddVote / addVerifiedVote in plain Python
(txflow/service.go:192-234, types/vote_set.go:81-166), and the inputs the set-table and stake-tally
edge tests share (tests/test_flow_model.py pins it to the C oracle on the CPU, tests/test_flow_edges.py
runs the same inputs through the kernels).

The model keeps a dict keyed by the TxHash bytes (set ids in first-seen order), per set
{validator: signature} and the stake as a Python int -- no width, so a sum that left int64 would show
as a difference, not wrap the same way twice -- and quorum = total * 2 // 3 + 1.  Signatures are not
verified here: the caller passes a verdict per vote, read only where the reference reaches Verify.

It imports neither the library under test nor the oracle."""
import hashlib
import random
import struct

ADDED, DUPLICATE, ERR_NIL, ERR_EMPTY_ADDR, ERR_UNKNOWN_VALIDATOR, ERR_NONDETERMINISTIC, ERR_INVALID_SIGNATURE = range(7)
FIRED = 0x80

MAXT = (2**63 - 1) // 8                      # tendermint MaxTotalVotingPower = MaxInt64 / 8


class FlowModel:
    def __init__(self, addrs, powers):
        self.val_of = {bytes(a): i for i, a in enumerate(addrs)}
        self.powers = [int(p) for p in powers]
        self.total = sum(self.powers)
        self.quorum = self.total * 2 // 3 + 1
        self.sets = {}                        # TxHash bytes -> dict(id, votes {validator: signature}, sum, maj23)

    def add_votes(self, votes, verdicts=None):
        """votes: oracle-style dicts (nil, txhash, addr, sig) in arrival order; verdicts[i]: whether
        vote i's signature verifies (None: all do).  -> (status [n], fired [n], events): one event per
        set whose +2/3 crossing happened in this batch, in arrival order of the crossing vote, as
        dict(vote_index = the crossing vote, tx_index = the set id, sum = the set's sum at the end
        of the batch)."""
        status, fired, crossed = [], [], []
        for i, v in enumerate(votes):
            st, f = self._add_one(v, True if verdicts is None else bool(verdicts[i]), i, crossed)
            status.append(st)
            fired.append(f)
        events = [dict(vote_index=i, tx_index=s["id"], sum=s["sum"]) for i, s in crossed]
        return status, fired, events

    def _add_one(self, v, verdict, i, crossed):
        if v is None or v.get("nil"):
            return ERR_NIL, False             # no TxHash to route by: no set is created
        s = self.sets.setdefault(bytes(v["txhash"]), dict(id=len(self.sets), votes={}, sum=0, maj23=False))
        if len(v["addr"]) == 0:
            return ERR_EMPTY_ADDR, False
        val = self.val_of.get(bytes(v["addr"]))
        if val is None:
            return ERR_UNKNOWN_VALIDATOR, False
        have = s["votes"].get(val)
        if have is not None:                  # decided before Verify
            return (DUPLICATE if have == bytes(v["sig"]) else ERR_NONDETERMINISTIC), False
        if not verdict:
            return ERR_INVALID_SIGNATURE, False
        s["votes"][val] = bytes(v["sig"])
        s["sum"] += self.powers[val]
        if not s["maj23"] and s["sum"] >= self.quorum:
            s["maj23"] = True
            crossed.append((i, s))
        return ADDED, s["maj23"]

    def query(self, txhash):
        s = self.sets.get(bytes(txhash))
        return None if s is None else (s["sum"], s["maj23"])

    def get_votes(self, txhash):
        """the accepted votes in validator order: [(validator, signature)]"""
        s = self.sets.get(bytes(txhash))
        return [] if s is None else sorted(s["votes"].items())

    def set_id(self, txhash):
        return self.sets[bytes(txhash)]["id"]

    def num_sets(self):
        return len(self.sets)


def expected(status, fired):
    """the status bytes txv_add_votes reports: code | FIRED"""
    return [st | (FIRED if f else 0) for st, f in zip(status, fired)]


# ------------------------------------------------------------------ A1: the key family
def key_family():
    """TxHash keys that differ where a set table can go wrong: every length 0..80 of one run of
    bytes (each a prefix of the next), the same with the last byte's top bit flipped, with a zero
    last byte, all zeros; and at 127, 128, 200 and 256 bytes (the overflow arena) pairs that differ
    in one byte only: the last, byte 64, byte 0, byte 63."""
    base = bytes(range(1, 81))
    keys = [b""]
    for n in range(1, 81):
        keys += [base[:n], base[:n - 1] + bytes([base[n - 1] ^ 0x80]), base[:n - 1] + b"\0", b"\0" * n]
    for n in (127, 128, 200, 256):
        for k, at in enumerate((n - 1, 64, 0, 63)):
            a = bytes((37 * n + 11 * k + 3 * j) % 251 + 1 for j in range(n))
            keys += [a, a[:at] + bytes([a[at] ^ 0x01]) + a[at + 1:]]
    keys = list(dict.fromkeys(keys))          # at length 1 the zero-last-byte key is the all-zero key
    assert len(set(keys)) == len(keys) >= 320
    return keys


def family_order(n_keys, seed=20260101):
    """(key index, validator) of A1's votes: validators 0..2 of 4 vote every key (quorum 3: each set
    fires on its third vote), arrival order shuffled"""
    pairs = [(k, v) for k in range(n_keys) for v in range(3)]
    random.Random(seed).shuffle(pairs)
    return pairs


# ------------------------------------------------------------------ B1: stake width
B1_POWERS = [
    [MAXT // 7] * 7,
    [MAXT - 6, 1, 1, 1, 1, 1, 1],
    [2**59, 2**58, 2**57, 3, 2, 1, 1],
    [2**32, 2**32 - 1, 2**32 + 1, 1, 2**31, 2**33, 5],
    [2, 2, 2, 1, 1, 1, 1],
]
B1_VALS, B1_TXS, B1_CUT = 7, 20, 37


def b1_order(seed=20260102):
    """(tx, validator) of B1's 140 votes in arrival order"""
    pairs = [(t, v) for t in range(B1_TXS) for v in range(B1_VALS)]
    random.Random(seed).shuffle(pairs)
    return pairs


def b1_hashes():
    return [b"%064X" % (0xB1 << 200 | t * 0x9E3779B97F4A7C15) for t in range(B1_TXS)]


def b1_stream(seed=20260102):
    """B1's arrival order as (tx, validator, kind): the 140 signed votes, and among them exact
    replays ("ok" again), flipped signatures ("bad"), second valid signatures of a validator
    ("alt": another timestamp), nil votes, empty and unknown addresses"""
    rnd = random.Random(seed)
    items = [(t, v, "ok") for t, v in b1_order(seed)]
    for kind, count in (("ok", 10), ("bad", 10), ("alt", 6), ("nil", 3), ("empty", 3), ("unknown", 3)):
        for _ in range(count):
            t, v, _k = items[rnd.randrange(len(items))]
            items.insert(rnd.randrange(len(items) + 1), (t, v, kind))
    return items


# ------------------------------------------------------------------ signed votes
SEC = 1_700_000_000


def validator_keys(O, n, tag=b"flow-edges"):
    """(seeds, public keys, addresses) of n validators, derived by the oracle"""
    seeds = [hashlib.sha512(tag + struct.pack("<I", i)).digest()[:32] for i in range(n)]
    pubs = [O.pubkey(s) for s in seeds]
    return seeds, pubs, [O.sha256(p)[:20] for p in pubs]


class Signer:
    """oracle-style vote dicts for (TxHash, validator, kind), each signature made once with the
    oracle's RFC 8032 signer (O: the oracle module, passed in by the test)"""

    def __init__(self, O, seeds, addrs, chain):
        self.O, self.seeds, self.addrs, self.chain = O, seeds, addrs, chain
        self.cache = {}

    def sig(self, txhash, v, nanos):
        key = (txhash, v, nanos)
        if key not in self.cache:
            self.cache[key] = self.O.sign(self.seeds[v], self.O.signbytes(1, txhash, SEC, nanos, self.chain))
        return self.cache[key]

    def vote(self, txhash, v, kind="ok"):
        """-> (vote dict, verdict)"""
        if kind == "nil":
            return dict(nil=True), True
        nanos = 1 + v + (1000 if kind == "alt" else 0)
        sig = self.sig(txhash, v, nanos)
        if kind == "bad":
            sig = sig[:9] + bytes([sig[9] ^ 0x20]) + sig[10:]
        addr = {"empty": b"", "unknown": b"\xEE" * 20}.get(kind, self.addrs[v])
        return (dict(height=1, txhash=txhash, ts_sec=SEC, ts_nanos=nanos, addr=addr, sig=sig,
                     txkey=hashlib.sha256(txhash).digest()), kind != "bad")

    def votes(self, items):
        """items: (txhash, validator, kind) -> (vote dicts, verdicts)"""
        out = [self.vote(*it) for it in items]
        return [v for v, _ in out], [ok for _, ok in out]
