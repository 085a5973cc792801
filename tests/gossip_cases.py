"""Votes for the gossip sink's tests (test_gossip_encode_emu.py, test_gossip_sink.py): the edge
matrix of the TxVoteMessage encoding, and what the sink must leave for a vote.  A vote is an
oracle-style dict with the FULL address and signature bytes; the expected bytes are always
oracle.wire_encode."""
import oracle as O

OK, HOST, UNENCODABLE = 0, 1, 2          # TXV_GOSSIP_*
SEC = 1_700_000_000
MIN_SEC, MAX_SEC = -62135596800, 253402300800   # amino's time range [0001-01-01, 10000-01-01)


def rbytes(rnd, n):
    return bytes(rnd.getrandbits(8) for _ in range(n))


def vote(rnd, height=1, txhash=None, ts_sec=SEC, ts_nanos=None, al=20, sl=64):
    if txhash is None:
        txhash = bytes(rnd.choice(b"0123456789ABCDEF") for _ in range(64))
    return dict(height=height, txhash=txhash, ts_sec=ts_sec, ts_nanos=rnd.randrange(1, 10**9) if ts_nanos is None else ts_nanos,
                addr=rbytes(rnd, al), sig=rbytes(rnd, sl), txkey=rbytes(rnd, 32))


def expected(v, with_key=True):
    """(flag, message bytes) the sink leaves for a non-nil vote; no bytes when flagged"""
    enc = O.wire_encode(v["height"], v["txhash"], v["ts_sec"], v["ts_nanos"], v["addr"], v["sig"],
                        v["txkey"] if with_key else bytes(32))
    if enc is None:
        return UNENCODABLE, b""
    if len(v["sig"]) > 64 or len(v["addr"]) > 20:
        return HOST, b""
    return OK, enc


def body_len(v):
    """TxVote.Size() of an encodable vote, from the message's own length prefix"""
    enc = O.wire_encode(v["height"], v["txhash"], v["ts_sec"], v["ts_nanos"], v["addr"], v["sig"], v["txkey"])
    n, shift, p = 0, 0, 5
    while True:
        n |= (enc[p] & 0x7F) << shift
        shift += 7
        p += 1
        if not enc[p - 1] & 0x80:
            return n


def edge_votes(rnd):
    """the edge matrix: every case of the issue's list at least once (no nil entries: the caller
    puts them in between)"""
    th = lambda n: bytes(rnd.choice(b"0123456789ABCDEF") for _ in range(n))
    vs = []
    for h in (0, -1, (1 << 63) - 1, 1, 127, 128, -(1 << 63)):
        vs.append(vote(rnd, height=h))
    for hl in (0, 1, 127, 128, 63, 64, 65, 300):
        vs.append(vote(rnd, txhash=th(hl)))
    # TxHash lengths that put the body at 127 and 128 (the message's own length prefix steps to 2 bytes)
    at = {}
    for hl in range(0, 130):
        v = vote(rnd, txhash=th(hl), ts_nanos=1, sl=0)
        at.setdefault(body_len(v), v)
    assert 127 in at and 128 in at
    vs += [at[127], at[128]]
    for sec, ns in ((0, 5), (SEC, 0), (0, 0), (-1, 1), (MIN_SEC, 0), (MAX_SEC - 1, 999_999_999), (-1, 0)):
        vs.append(vote(rnd, ts_sec=sec, ts_nanos=ns))
    vs.append(vote(rnd, height=0, txhash=b"", ts_sec=0, ts_nanos=0, al=0, sl=0))   # only the TxKey field
    for sec, ns in ((MIN_SEC - 1, 1), (MAX_SEC, 1), (SEC, -1), (SEC, 1_000_000_000), (1 << 62, 0)):
        vs.append(vote(rnd, ts_sec=sec, ts_nanos=ns))                              # amino rejects: flag 2
    vs.append(vote(rnd, ts_sec=MAX_SEC, ts_nanos=1, al=21, sl=65))                # rejected and too long: still flag 2
    for al in (0, 1, 2, 3, 4, 5, 19, 20, 21):
        vs.append(vote(rnd, al=al))
    for sl in (0, 1, 3, 4, 63, 64, 65, 100):
        vs.append(vote(rnd, sl=sl))
    flags = [expected(v)[0] for v in vs]
    assert flags.count(UNENCODABLE) == 6 and flags.count(HOST) == 3
    return vs
