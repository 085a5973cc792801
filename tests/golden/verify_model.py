"""Python model of the acceptance rule of x/crypto@c2843e01d9a2 ed25519.Verify (SURVEY.md
Appendix A.1), written from the rule and independent of the oracle's C: the second
implementation the small-order-R' / edge-scalar golden vectors rest on.  Test infrastructure only.

  verify(pub, msg, sig)           the rule: len(sig) == 64, sig[63] & 0xE0 == 0, A decodes (y >= p
                                  and x = 0 with the sign bit both accepted), s < L, and
                                  encode([s]B - [k]A) == sig[:32] BYTE FOR BYTE (canonical encode)
  verify_point_compare(...)       the WRONG rule an implementation may slip into: decode R with the
                                  same lenient rules and compare points.  It accepts a
                                  non-canonical encoding of the point R' lands on; x/crypto does not.

Points are extended homogeneous (X, Y, Z, T) with Python integers."""
import hashlib

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
IDENT = (0, 1, 1, 0)


def padd(p, q):
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = t1 * D2 % P * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def pneg(p):
    x, y, z, t = p
    return ((P - x) % P, y, z, (P - t) % P)


def pmul(k, p):
    r = IDENT
    while k:
        if k & 1:
            r = padd(r, p)
        p = padd(p, p)
        k >>= 1
    return r


def affine(p):
    x, y, z, _ = p
    zi = pow(z, P - 2, P)
    return (x * zi % P, y * zi % P)


def from_affine(xy):
    x, y = xy
    return (x % P, y % P, 1, x * y % P)


def decode(b: bytes):
    """x/crypto FromBytes: y is taken mod p (y >= p accepted), x = 0 keeps whatever sign bit"""
    n = int.from_bytes(b, "little")
    sign, y = n >> 255, (n & ((1 << 255) - 1)) % P
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = pow(u * pow(v, P - 2, P) % P, (P + 3) // 8, P)
    if (v * x * x - u) % P:
        x = x * SQRT_M1 % P
    if (v * x * x - u) % P:
        return None
    if (x & 1) != sign:
        x = (P - x) % P
    return from_affine((x, y))


def encode(p) -> bytes:
    x, y = affine(p)
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


_by = 4 * pow(5, P - 2, P) % P
B = decode(_by.to_bytes(32, "little"))


def challenge(r32: bytes, pub: bytes, msg: bytes) -> int:
    return int.from_bytes(hashlib.sha512(r32 + pub + msg).digest(), "little") % L


def r_prime(pub: bytes, msg: bytes, sig: bytes):
    """[s]B - [k]A, or None where the rule rejects before the multiplication"""
    if len(sig) != 64 or len(pub) != 32 or sig[63] & 0xE0:
        return None
    a = decode(pub)
    s = int.from_bytes(sig[32:], "little")
    if a is None or s >= L:
        return None
    k = challenge(sig[:32], pub, msg)
    return padd(pmul(s, B), pmul(k, pneg(a)))


def verify(pub: bytes, msg: bytes, sig: bytes) -> bool:
    r = r_prime(pub, msg, sig)
    return r is not None and encode(r) == sig[:32]


def verify_point_compare(pub: bytes, msg: bytes, sig: bytes) -> bool:
    r = r_prime(pub, msg, sig)
    if r is None:
        return False
    named = decode(sig[:32])
    return named is not None and affine(named) == affine(r)
