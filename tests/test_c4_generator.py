"""CPU check of the C4 adversarial stream generator (tests/adversarial.py) before it is used as the
GPU gate: a stand-in context built from the oracle (keygen / sign / a second sequential Flow)
runs a small stream; it must agree with the checker trivially (0 mismatches) and -- the real
point -- the stream must exercise every outcome the gate is meant to cover."""
import numpy as np
import pytest


class OracleCtx:
    """Implements the Context methods adversarial.C4Stream calls, on the CPU oracle."""

    def __init__(self):
        import oracle as O
        self.O = O
        self.flow = None

    def keygen(self, seeds):
        self.seeds = list(seeds)              # the signer keys, as txv_keygen sets them
        return [self.O.pubkey(s) for s in seeds]

    def set_validators(self, pubs, powers, chain):
        self.pubs, self.powers, self.chain = list(pubs), np.asarray(powers), chain.encode()

    def validator_info(self):
        return [self.O.sha256(p)[:20] for p in self.pubs], np.array([self.O.decode_ok(p) for p in self.pubs])

    def sign_votes(self, b, signer, chain):
        out = np.zeros((b.n, 64), np.uint8)
        for i in range(b.n):
            m = self.O.signbytes(int(b.height[i]), b.txhash(i), int(b.ts_sec[i]), int(b.ts_nanos[i]), chain.encode())
            out[i] = np.frombuffer(self.O.sign(self.seeds[int(signer[i])], m), np.uint8)
        return out

    def reset_flow(self):
        self.flow = None

    def add_votes(self, b, ev_cap=0):
        if self.flow is None:
            self.flow = self.O.Flow(self.pubs, self.powers, self.chain)
            self.done = set()
        st, _, fired = self.flow.add_batch(b, 4)
        ev = []
        for i in np.nonzero(fired)[0]:
            h = b.txhash(int(i))
            if h not in self.done:
                self.done.add(h)
                ev.append({"vote_index": int(i)})
        return st.astype(np.uint8) | (fired.astype(np.uint8) << 7), ev

    def verify_batch(self, b, pubs):
        return self.O.txvote_verify_batch(b, pubs, self.chain, 4)

    def query_tx(self, h):
        q = self.flow.query(h)
        return q


def test_c4_stream_covers_every_outcome(oracle_lib):
    import adversarial as A
    import txflow_amd as T
    ctx = OracleCtx()
    s = A.C4Stream(ctx, batch=6000, batches_per_epoch=2, oracle_threads=4, verify_slice=512)
    for _ in range(3):
        r = s.run_batch()
        assert r["status_mismatches"] == 0 and r["events_ok"] and r["verify_mismatches"] == 0
    s.stats["mismatches"] += s.check_sets()
    assert s.stats["mismatches"] == 0
    seen = s.stats["by_status"]
    for code in (T.ADDED, T.DUPLICATE, T.ERR_NIL, T.ERR_EMPTY_ADDR, T.ERR_UNKNOWN_VALIDATOR,
                 T.ERR_NONDETERMINISTIC, T.ERR_INVALID_SIGNATURE):
        assert seen.get(T.STATUS_NAMES[code], 0) > 0, (T.STATUS_NAMES[code], seen)
    assert s.stats["events"] > 0
    for name, share in A.CLASSES:               # every Appendix C class is generated at about its share
        if share:
            got = s.stats["class_generated"].get(name, 0) / s.stats["generated"]
            assert 0.7 * share <= got <= 1.4 * share, (name, got, share)
    # crafted keys: identity forgeries verify, order-2/4/8 and mixed-order forgeries verify only
    # when [k]T = 0, the undecodable key never -- so both verdicts occur among crafted votes
    names = [k[0] for k in s.crafted]
    for must in ("identity", "identity_y+p", "identity_negzero", "order2", "order4", "order8", "mixed8",
                 "undecodable"):
        assert must in names


def _checktx(oracle_lib, b, f):
    """the batch's gossiped votes through the oracle's CheckTx: (indices into f, pool statuses)"""
    import txflow_amd as T
    gossip = np.nonzero(f["is_nil"] == 0)[0]
    m = len(gossip)
    sub = T.VoteBatch(m, height=f["height"][gossip], txhash_arena=b.txhash_arena, txhash_off=f["txoff"][gossip],
                      txhash_len=np.full(m, 64, np.uint32), ts_sec=np.full(m, 1_700_000_000, np.int64),
                      ts_nanos=f["ts_nanos"][gossip], addr=f["addr"][gossip], addr_len=f["addr_len"][gossip],
                      sig=f["sig"][gossip], sig_len=f["sig_len"][gossip])
    long_sigs = {int(q): sub.sig[64 * q:64 * q + 64].tobytes() + bytes(int(sub.sig_len[q]) - 64)
                 for q in np.nonzero(sub.sig_len > 64)[0]}
    pool = oracle_lib.Pool(size=(1 << 31) - 1, cache_size=1 << 16, max_txs_bytes=1 << 40)
    return gossip, pool.check_batch(sub, long_sigs)


def test_c4_noncanonical_r_class_survives_checktx_and_separates(oracle_lib):
    """The non-canonical-R class (adversarial.C4Stream._small_order_vote): every vote has signature
    bytes of its own, so CheckTx admits at least 0.8 of the class's share (it kept 78 of 529,442
    when the class was three fixed signatures).  Both verdicts occur; every vote whose R is a
    non-canonical encoding is rejected by the oracle and by the Python model of the rule, yet
    accepted by the model's point-comparing variant, with R' the small-order point R names and
    s != 0 (generic digits): the class tells a verifier that canonicalises R' from one that
    does not.  Checked on the primaries, their conflict copies and their replays."""
    import adversarial as A
    import ed_math as E
    import txflow_amd as T
    import verify_model as V
    n, share = 16000, 0.005
    s = A.C4Stream(OracleCtx(), batch=n, batches_per_epoch=2, oracle_threads=4, verify_slice=0)
    canon = {e[1] for e in E.torsion_encodings() if e[3]}
    noncanon = {e[1] for e in E.torsion_encodings() if not e[3]}
    seen_enc, verdicts = set(), {True: 0, False: 0}
    for _ in range(2):                         # the second batch has conflicts sourced from the first
        b, f = s.next_batch()
        gossip, ops = _checktx(oracle_lib, b, f)
        cls = f["cls"][gossip]
        prim = cls == A.CLS["noncanonical_r"]
        assert int(prim.sum()) >= 0.95 * share * n
        assert int(np.count_nonzero(prim & (ops == T.POOL_OK))) >= 0.8 * share * n
        idx = np.nonzero(f["kind"] == 2)[0]    # primaries, their conflicts and replays
        assert len(idx) > int(prim.sum())
        sigs = {f["sig"][i].tobytes() for i in np.nonzero((f["kind"] == 2) & (f["cls"] != A.CLS["exact_replay"]))[0]}
        assert len(sigs) == int(np.count_nonzero((f["kind"] == 2) & (f["cls"] != A.CLS["exact_replay"])))
        for i in idx:
            name, pub, _ = s.crafted[int(f["val"][i]) - s.n_honest]
            assert name in ("mixed4", "mixed8")
            sig = f["sig"][i].tobytes()
            msg = T.sign_bytes(int(f["height"][i]), s.hashes[f["tx"][i]].tobytes(), 1_700_000_000,
                               int(f["ts_nanos"][i]), A.CHAIN)
            exp = sig[:32] in canon
            assert exp or sig[:32] in noncanon
            assert oracle_lib.verify(pub, msg, sig) == exp == V.verify(pub, msg, sig)
            assert V.verify_point_compare(pub, msg, sig) and int.from_bytes(sig[32:], "little") != 0
            seen_enc.add(sig[:32])
            verdicts[exp] += 1
    assert verdicts[True] > 0 and verdicts[False] > verdicts[True]
    assert noncanon <= seen_enc and len(seen_enc & canon) >= 4


def test_c4_keyless_classes_survive_checktx(oracle_lib):
    """Unknown-validator, empty-address and nil votes carry distinct signatures, so CheckTx's LRU
    (keyed by SHA-256(Signature), txvotepool.go:467-469) admits them and Appendix C's shares of
    those classes reach TxFlow (with shared / all-zero signatures only a few
    dozen empty-address votes survived 10^8)."""
    import adversarial as A
    import txflow_amd as T
    n = 40000
    s = A.C4Stream(OracleCtx(), batch=n, batches_per_epoch=2, oracle_threads=4, verify_slice=0)
    b, f = s.next_batch()
    gossip = np.nonzero(f["is_nil"] == 0)[0]
    m = len(gossip)
    sub = T.VoteBatch(m, height=f["height"][gossip], txhash_arena=b.txhash_arena, txhash_off=f["txoff"][gossip],
                      txhash_len=np.full(m, 64, np.uint32), ts_sec=np.full(m, 1_700_000_000, np.int64),
                      ts_nanos=f["ts_nanos"][gossip], addr=f["addr"][gossip], addr_len=f["addr_len"][gossip],
                      sig=f["sig"][gossip], sig_len=f["sig_len"][gossip])
    long_sigs = {int(q): sub.sig[64 * q:64 * q + 64].tobytes() + bytes(int(sub.sig_len[q]) - 64)
                 for q in np.nonzero(sub.sig_len > 64)[0]}
    pool = oracle_lib.Pool(size=(1 << 31) - 1, cache_size=1 << 16, max_txs_bytes=1 << 40)
    ops = pool.check_batch(sub, long_sigs)
    kind = f["kind"][gossip]
    for k, share in ((3, 0.005), (4, 0.0025)):
        admitted = int(np.count_nonzero((kind == k) & (ops == T.POOL_OK)))
        assert admitted >= 0.8 * share * n, (k, admitted)
    assert int(np.count_nonzero(f["is_nil"])) >= 0.8 * 0.001 * n
