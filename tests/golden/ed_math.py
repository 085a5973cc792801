"""Tiny pure-Python edwards25519 arithmetic used only to CRAFT adversarial inputs
(torsion points, non-canonical encodings, forged signatures) for the golden fixtures.
Verdicts are never computed here: they come from the oracle and are cross-checked with
OpenSSL.  Test infrastructure only."""
P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
I = pow(2, (P - 1) // 4, P)


def inv(x):
    return pow(x, P - 2, P)


def add(p, q):
    x1, y1 = p
    x2, y2 = q
    t = D * x1 * x2 * y1 * y2 % P
    x3 = (x1 * y2 + x2 * y1) * inv(1 + t) % P
    y3 = (y1 * y2 + x1 * x2) * inv(1 - t) % P
    return (x3, y3)


def mul(k, p):
    r = (0, 1)
    while k:
        if k & 1:
            r = add(r, p)
        p = add(p, p)
        k >>= 1
    return r


def recover_x(y, sign):
    """x for y (mod p) with parity sign, or None"""
    y %= P
    x2 = (y * y - 1) * inv(D * y * y + 1) % P
    if x2 == 0:
        return 0
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * I % P
    if (x * x - x2) % P:
        return None
    if (x & 1) != sign:
        x = P - x
    return x


def encode(p):
    x, y = p
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def encode_raw(y_int, sign):
    return (y_int | (sign << 255)).to_bytes(32, "little")


B = (recover_x(4 * inv(5) % P, 0), 4 * inv(5) % P)


def order(p):
    for k in (1, 2, 4, 8):
        if mul(k, p) == (0, 1):
            return k
    return None


def neg(p):
    return ((P - p[0]) % P, p[1])


def torsion_encodings():
    """The 14 byte strings x/crypto's point decoding maps to a point of E[8]:
    [(tag, bytes, point, canonical)].  8 canonical ones, and the 6 non-canonical ones there are:
    the identity as (y = 1, sign 1), (y = p + 1, sign 0 / 1); (0, -1) with the sign bit; and
    y = p (= 0) with either sign, the two order-4 points.  (Every other torsion y is >= 19, so
    y + p does not fit 255 bits.)"""
    out = [("canon_ord%d" % order(t), encode(t), t, True) for t in torsion_points()]
    out += [("noncanon_ident_negzero", encode_raw(1, 1), (0, 1), False),
            ("noncanon_ident_yp", encode_raw(1 + P, 0), (0, 1), False),
            ("noncanon_ident_yp_negzero", encode_raw(1 + P, 1), (0, 1), False),
            ("noncanon_ord2_negzero", encode_raw(P - 1, 1), (0, P - 1), False),
            ("noncanon_ord4_yp_s0", encode_raw(P, 0), (recover_x(0, 0), 0), False),
            ("noncanon_ord4_yp_s1", encode_raw(P, 1), (recover_x(0, 1), 0), False)]
    return out


def neg_multiples(t):
    """[-[j]T for j in 0..7] of a torsion point T"""
    return [mul(j, neg(t)) for j in range(8)]


def rprime_sig(pub, a, neg_t, rb, q, msg):
    """(rb || s) under the key A = [a]B + T (pub its encoding, neg_t = neg_multiples(T)) whose
    R' = [s]B - [k]A is EXACTLY the torsion point q that rb names, after a walk with generic
    digits: k = SHA-512(rb || A || msg) mod L, and s = k a gives [s]B - [k]A = -[k mod 8]T.
    None when this message's k does not land on q (the caller draws another message).
    A verifier that encodes R' canonically and compares bytes accepts exactly the canonical rb;
    one that compares points accepts every rb."""
    import hashlib
    k = int.from_bytes(hashlib.sha512(rb + pub + msg).digest(), "little") % L
    if neg_t[k % 8] != q:
        return None
    return rb + (k * a % L).to_bytes(32, "little")


def torsion_points():
    """all 8 points of E[8]"""
    pts = set()
    import random
    rnd = random.Random(8)
    while len(pts) < 8:
        y = rnd.randrange(P)
        x = recover_x(y, rnd.randrange(2))
        if x is None:
            continue
        t = mul(L, (x, y))
        pts.add(t)
        for k in range(8):
            pts.add(mul(k, t))
    return sorted(pts)
