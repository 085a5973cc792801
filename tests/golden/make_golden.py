"""Generates the committed golden fixtures under tests/golden/ (run from the repo root:
`python tests/golden/make_golden.py`).  Test infrastructure only.

Provenance of each expected value:
  ed25519_openssl.json  seed -> pub, (seed, msg) -> sig from OpenSSL 3 (libcrypto EVP Ed25519,
                        RFC 8032 deterministic = byte-identical to Go's ed25519.Sign); the
                        oracle must reproduce them and accept the signatures.
  verify_vectors.json   adversarial (pub, msg, sig) with the x/crypto@c2843e01d9a2 verdict as
                        restated by the oracle; the OpenSSL verdict is
                        recorded beside it.  Cases where the two differ are decided by Appendix A
                        and are "parity unpinned" beyond that restatement.  The edge kinds
                        (edge_vectors below: small-order R', edge scalars, cancellation) are
                        appended last from an RNG of their own, and their verdicts are also
                        checked against the Python model of the rule (verify_model.py).
  signbytes.json        amino SignBytes / Size cases; two are pinned by the reference's own tests
                        (types/vote_test.go:62 zero-time bytes, txvotepool/txvotepool_test.go:102
                        Size()==114); the rest come from the oracle's restatement (Appendix B).
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ed_math as E  # noqa: E402
import openssl_ed25519 as S  # noqa: E402
import oracle as O  # noqa: E402

H = lambda b: b.hex()  # noqa: E731


def sc(b):
    return int.from_bytes(hashlib.sha512(b).digest(), "little") % E.L


def forge(a_pub: bytes, msg: bytes, rnd, secret=None):
    """R = [r]B, S = r + k*secret (secret None -> S = r): valid iff [k]A == [k*secret]B"""
    r = rnd.randrange(1, E.L)
    R = E.encode(E.mul(r, E.B))
    k = sc(R + a_pub + msg)
    s = (r + k * (secret or 0)) % E.L
    return R + s.to_bytes(32, "little")


# s values of the s_edge vectors: the ends of [0, L), the values around 2^252 where the long top
# digit of the radix-2^21 tables (Tab<21>, unsigned, up to 2^21 + 1) is at or near its maximum, and
# the all-half-digit patterns of tests/test_cpu_emu.py::test_table_digits_cover_every_scalar_below_L
S_EDGE = [0, 1, 2, E.L - 1, E.L - 2, 2 ** 252, 2 ** 252 - 1, 2 ** 252 + 2 ** 124, 2 ** 252 - 2 ** 231,
          2 ** 252 - 2 ** 230, (2 ** 231 - 1) * (2 ** 21 + 1) % E.L, sum(1 << (21 * i + 20) for i in range(12)) % E.L,
          sum(1 << (21 * i + 20) for i in range(11)), sum(1 << (21 * i + 19) for i in range(12)) % E.L]
S_EDGE_ORD8 = [0, 1, E.L - 1, 2 ** 252 - 2 ** 231, 2 ** 252 + 2 ** 124, sum(1 << (21 * i + 20) for i in range(11))]
K_TOP, K_LOW = 2 ** 252 - 2 ** 231, 2 ** 231
GRIND_CAP = 1 << 25


def edge_vectors(add, vec, base, mixed_keys, tors):
    """Vectors at the edges of the verify path, appended after everything above and drawn from an
    RNG of their own (so every earlier entry of every fixture stays byte-identical):

      smallorder_rprime_*   R' = [s]B - [k]A lands EXACTLY on a point of E[8] after a full walk with
                            generic digits (ed_math.rprime_sig over the mixed-order keys above, and
                            over pure torsion keys with s = 0); R is one of the 14 encodings of
                            that point.  x/crypto accepts the 8 canonical ones only.
      s_edge*               s at the ends of its range and at the table digits' extremes, under the
                            identity key (R = [s]B) and an order-8 key (R = [s]B - [j]T, k = j mod 8)
      cancel_*              key B or -B: the B walk and the A walk cancel to the identity
      k_top / k_low         an honest key, the message ground until k >= 2^252 - 2^231 / k < 2^231

    Each verdict is the oracle's (add) and must equal the Python model's (verify_model.verify);
    every *_noncanon_* vector must be accepted by the point-comparing variant, i.e. it separates
    a right implementation from a wrong one."""
    import verify_model as V
    rnd = random.Random(20261020)
    n0 = len(vec)

    def rmsg():
        return bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(1, 160)))

    def le(x):
        return x.to_bytes(32, "little")

    # ---- small-order R'
    encs = E.torsion_encodings()
    mixed = [(pub, a, E.neg_multiples(T)) for pub, a, T in mixed_keys]
    pure = [(E.encode(T), 0, E.neg_multiples(T)) for T in tors if E.order(T) == 8]
    for ei, (tag, rb, q, canon) in enumerate(encs):
        elig = [k for k in mixed if q in k[2]]
        assert len(elig) >= 2
        # two different mixed-order keys (rotating through the eligible ones) and one pure torsion key
        for pub, a, neg_t in [elig[ei % len(elig)], elig[(ei + 1) % len(elig)], pure[ei % len(pure)]]:
            for _ in range(4096):
                m = rmsg()
                sig = E.rprime_sig(pub, a, neg_t, rb, q, m)
                if sig is not None:
                    break
            else:
                raise AssertionError("no message found for " + tag)
            add("smallorder_rprime_" + tag, pub, m, sig)
            assert vec[-1]["expect"] == canon, tag

    # ---- s at its edges
    ident = E.encode((0, 1))
    for s in S_EDGE:
        assert 0 <= s < E.L
        add("s_edge", ident, rmsg(), E.encode(E.mul(s, E.B)) + le(s))
        assert vec[-1]["expect"]
    for s in (E.L - 1, 2 ** 252 - 1):                       # R taken from s + 1
        add("s_edge_twin", ident, rmsg(), E.encode(E.mul(s + 1, E.B)) + le(s))
        assert not vec[-1]["expect"]
    t8 = next(T for T in tors if E.order(T) == 8)
    pub8, neg8 = E.encode(t8), E.neg_multiples(t8)

    def ord8_sig(s_point, s):
        """R = [s_point]B - [j]T for the j that this message's k turns out to be (mod 8)"""
        sb = E.mul(s_point, E.B)
        cand = [E.encode(E.add(sb, neg8[j])) for j in range(8)]
        while True:
            m = rmsg()
            for j, rb in enumerate(cand):
                if sc(rb + pub8 + m) % 8 == j:
                    return m, rb + le(s)

    for s in S_EDGE_ORD8:
        add("s_edge_ord8", pub8, *ord8_sig(s, s))
        assert vec[-1]["expect"]
    add("s_edge_ord8_twin", pub8, *ord8_sig(2 ** 252 - 2 ** 231 + 1, 2 ** 252 - 2 ** 231))
    assert not vec[-1]["expect"]

    # ---- B and A cancel
    pub_b, pub_nb = E.encode(E.B), E.encode(E.neg(E.B))
    for _ in range(2):
        m = rmsg()
        for tag, rb, q, canon in encs:
            if q == (0, 1):      # s = k: [k]B - [k]B = identity, named canonically or not
                add("cancel_ident_canon" if canon else "cancel_" + tag, pub_b, m, rb + le(sc(rb + pub_b + m)))
                assert vec[-1]["expect"] == canon
        add("cancel_R_eq_B", pub_b, m, pub_b + le((sc(pub_b + pub_b + m) + 1) % E.L))
        assert vec[-1]["expect"]
        add("cancel_negB", pub_nb, m, ident + le((E.L - sc(ident + pub_nb + m)) % E.L))
        assert vec[-1]["expect"]

    # ---- k at the top / bottom of its range, an honest key
    seed, pub = bytes.fromhex(base[0]["seed"]), bytes.fromhex(base[0]["pub"])
    h = hashlib.sha512(seed).digest()
    a = (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254)
    assert E.encode(E.mul(a, E.B)) == pub

    def grind(kind, n, pred):
        for i in range(n):
            r = rnd.randrange(1, E.L)
            rb = E.encode(E.mul(r, E.B))
            prefix = b"%s/%d/" % (kind.encode(), i)
            h0 = hashlib.sha512(rb + pub + prefix)
            for ctr in range(GRIND_CAP):
                hh = h0.copy()
                hh.update(ctr.to_bytes(8, "little"))
                k = int.from_bytes(hh.digest(), "little") % E.L
                if pred(k):
                    break
            else:
                raise AssertionError("grind cap reached for " + kind)
            sig = rb + le((r + k * a) % E.L)
            m = prefix + ctr.to_bytes(8, "little")
            add(kind, pub, m, sig)
            assert vec[-1]["expect"]
            s = bytearray(sig)
            s[32 + rnd.randrange(31)] ^= 1 << rnd.randrange(8)
            add(kind + "_s_bitflip", pub, m, bytes(s))
            assert not vec[-1]["expect"]

    grind("k_top", 3, lambda k: k >= K_TOP)
    grind("k_low", 2, lambda k: k < K_LOW)

    # ---- the second implementation: the Python model on every new vector
    for v in vec[n0:]:
        p, m, s = bytes.fromhex(v["pub"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])
        assert V.verify(p, m, s) == v["expect"], v["kind"]
        if "_noncanon_" in v["kind"]:
            assert not v["expect"] and V.verify_point_compare(p, m, s), v["kind"]


def main():
    rnd = random.Random(20260501)
    out = {}
    # ---------------------------------------------------------------- OpenSSL vectors
    cases = []
    for i in range(48):
        seed = bytes(rnd.getrandbits(8) for _ in range(32))
        if i < 16:
            msg = bytes(rnd.getrandbits(8) for _ in range(rnd.choice([0, 1, 63, 64, 111, 112, 127, 128, 255, 300])))
        else:
            th = "".join(rnd.choice("0123456789ABCDEF") for _ in range(64)).encode()
            msg = O.signbytes(rnd.choice([0, 1, 12345]), th, 1_700_000_000 + i, rnd.randrange(1, 10 ** 9),
                              b"test_chain_id")
        cases.append(dict(seed=H(seed), pub=H(S.pubkey(seed)), msg=H(msg), sig=H(S.sign(seed, msg))))
    out["ed25519_openssl"] = cases

    # ---------------------------------------------------------------- adversarial verify vectors
    vec = []

    def add(kind, pub, msg, sig):
        exp = O.verify(pub, msg, sig)
        try:
            ossl = S.verify(pub, msg, sig)
        except Exception:  # pragma: no cover
            ossl = None
        vec.append(dict(kind=kind, pub=H(pub), msg=H(msg), sig=H(sig), expect=bool(exp), openssl=ossl))

    base = cases[16:32]
    for c in base:
        pub, msg, sig = bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"])
        add("valid", pub, msg, sig)
        s = bytearray(sig); s[rnd.randrange(32)] ^= 1 << rnd.randrange(8); add("r_bitflip", pub, msg, bytes(s))
        s = bytearray(sig); s[32 + rnd.randrange(31)] ^= 1 << rnd.randrange(8); add("s_bitflip", pub, msg, bytes(s))
        sv = int.from_bytes(sig[32:], "little") + E.L
        if sv < 2 ** 256:
            add("s_plus_L", pub, msg, sig[:32] + sv.to_bytes(32, "little"))
        s = bytearray(sig); s[63] |= 0x20; add("s_top_bit", pub, msg, bytes(s))
        add("msg_changed", pub, msg + b"\x00", sig)
        add("len63", pub, msg, sig[:63])
        add("len65", pub, msg, sig + b"\x00")
        add("len0", pub, msg, b"")
        # R non-canonical: flip the sign bit of R (a different point or undecodable) is just a bit flip;
        # non-canonical y: only possible when y < 19 (R = small-y point), covered with the torsion keys below
    # torsion / small-order public keys, canonical and non-canonical encodings
    tors = E.torsion_points()
    msgs = [bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(0, 200))) for _ in range(6)]
    for T in tors:
        encs = [("torsion_canon_ord%d" % E.order(T), E.encode(T))]
        x, y = T
        if y < 19:
            encs.append(("torsion_noncanon_y_ord%d" % E.order(T), E.encode_raw(y + E.P, x & 1)))
        if x == 0:
            encs.append(("torsion_negzero_ord%d" % E.order(T), E.encode_raw(y, 1)))
            if y < 19:
                encs.append(("torsion_negzero_noncanon_ord%d" % E.order(T), E.encode_raw(y + E.P, 1)))
        for kind, pub in encs:
            for m in msgs:
                add(kind, pub, m, forge(pub, m, rnd))
    # non-canonical R with the identity key: R = identity encoded non-canonically / as -0
    ident = E.encode((0, 1))
    for m in msgs[:3]:
        add("ident_R_canon", ident, m, E.encode_raw(1, 0) + (0).to_bytes(32, "little"))
        add("ident_R_noncanon_y", ident, m, E.encode_raw(1 + E.P, 0) + (0).to_bytes(32, "little"))
        add("ident_R_negzero", ident, m, E.encode_raw(1, 1) + (0).to_bytes(32, "little"))
    # mixed-order keys: A' = [a]B + T (cofactorless check: valid iff [k]T = 0)
    mixed_keys = []    # (pub, a, T): kept for the small-order R' vectors below
    for i, T in enumerate(tors):
        if T == (0, 1):
            continue
        a = rnd.randrange(1, E.L)
        Ap = E.encode(E.add(E.mul(a, E.B), T))
        mixed_keys.append((Ap, a, T))
        for m in msgs:
            add("mixed_order_ord%d" % E.order(T), Ap, m, forge(Ap, m, rnd, secret=a))
    # undecodable public keys
    n_und = 0
    while n_und < 8:
        yb = rnd.getrandbits(255)
        if E.recover_x(yb, 0) is None:
            pub = E.encode_raw(yb, rnd.randrange(2))
            add("undecodable_pub", pub, msgs[0], forge(pub, msgs[0], rnd))
            n_und += 1
    # y >= p encodings of valid non-torsion points are impossible (y+p >= 2^255 for y >= 19);
    # high bit set on a canonical key flips x only:
    for c in base[:4]:
        pub = bytearray(bytes.fromhex(c["pub"])); pub[31] ^= 0x80
        add("pub_signflip", bytes(pub), bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]))
    edge_vectors(add, vec, base, mixed_keys, tors)
    out["verify_vectors"] = vec

    # ---------------------------------------------------------------- SignBytes / Size
    sb = []
    # pinned by types/vote_test.go:62: the Go zero time encodes as 0x08 0x80 0x92 0xb8 0xc3 0x98 0xfe 0xff 0xff 0xff 0x01
    sb.append(dict(note="vote_test.go:62 zero time", height=0, txhash="", ts_sec=-62135596800, ts_nanos=0, chain="",
                   hex=O.signbytes(0, b"", -62135596800, 0, b"").hex()))
    for i in range(24):
        th = "".join(rnd.choice("0123456789ABCDEF") for _ in range(rnd.choice([0, 1, 64, 64, 200])))
        h = rnd.choice([0, 1, 12345, -1, 2 ** 62])
        ts = rnd.choice([0, 1_700_000_000, 1514170801, -62135596800, 253402300799])
        tn = rnd.choice([0, 234000000, 1, 999999999, 2 ** 28])
        ch = rnd.choice(["", "test_chain_id"])
        enc = O.signbytes(h, th.encode(), ts, tn, ch.encode())
        sb.append(dict(height=h, txhash=th, ts_sec=ts, ts_nanos=tn, chain=ch, hex=None if enc is None else enc.hex()))
    for ts in (-62135596801, 253402300800):
        sb.append(dict(note="amino time range error (SignBytes panics)", height=1, txhash="AB", ts_sec=ts, ts_nanos=0,
                       chain="test_chain_id", hex=None))
    out["signbytes"] = sb
    out["size"] = [
        dict(note="txvotepool_test.go:102 Size()==114 (20-byte tx, Height 0, nanos >= 2^28)", height=0,
             txhash_len=64, ts_sec=1560000000, ts_nanos=300000000, addr_len=0, sig_len=0, size=114),
        dict(note="nanos < 2^28 gives 113 (the reference test's flaky case)", height=0, txhash_len=64,
             ts_sec=1560000000, ts_nanos=200000000, addr_len=0, sig_len=0, size=113),
    ]

    for name, data in out.items():
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(data, f, indent=1)
    agree = sum(1 for v in vec if v["openssl"] == v["expect"])
    print(f"wrote {len(out)} fixtures; verify vectors {len(vec)}, OpenSSL agrees on {agree}")
    for v in vec:
        if v["openssl"] != v["expect"]:
            print("  differs:", v["kind"], "oracle", v["expect"], "openssl", v["openssl"])


if __name__ == "__main__":
    main()
