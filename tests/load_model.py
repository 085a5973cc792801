"""A small Python model of TxStore.LoadTxCommit's decode of one stored Commit record
(tx/store.go:67-80): the envelope rules of go-txflow_amd/csrc/load_dev.h's header restated
independently, with every element's TxVote body handed to the oracle's TxVoteMessage decoder
(oracle.wire_decode of wire_prefix() + 0x0a + uvarint(len) + body), which makes oracle/wire.c the
reference for every field of every vote.  Test infrastructure only."""
OK, CORRUPT, EMPTY = range(3)          # TXV_COMMIT_*
VARINT, B8, BYTES, B4 = 0, 1, 2, 5     # typ3


def uvarint_enc(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def uvarint_size(v: int) -> int:
    return len(uvarint_enc(v))


def uvarint(b: bytes, p: int, end: int):
    """Go binary.Uvarint over b[p:end]: (value, bytes read) or None (ran out of bytes, overflow)"""
    x = 0
    for i in range(10):
        if p + i >= end:
            return None
        c = b[p + i]
        if c < 0x80:
            if i == 9 and c > 1:
                return None
            return x | (c << (7 * i)), i + 1
        x |= (c & 0x7F) << (7 * i)
    return None


def field_key(b, p, end):
    r = uvarint(b, p, end)
    if r is None or (r[0] >> 3) > (1 << 29) - 1:
        return None
    return r[0] >> 3, r[0] & 7, r[1]


def byte_slice(b, p, end):
    """(body offset, body length, bytes read) or None"""
    r = uvarint(b, p, end)
    if r is None or r[0] > end - p - r[1]:
        return None
    return p + r[1], r[0], r[1] + r[0]


def skip_rest(b, p, end, last) -> bool:
    while p < end:
        k = field_key(b, p, end)
        if k is None or k[0] <= last:
            return False
        last = k[0]
        p += k[2]
        if k[1] == VARINT:
            r = uvarint(b, p, end)
            if r is None:
                return False
            p += r[1]
        elif k[1] == B8:
            if end - p < 8:
                return False
            p += 8
        elif k[1] == B4:
            if end - p < 4:
                return False
            p += 4
        elif k[1] == BYTES:
            r = byte_slice(b, p, end)
            if r is None:
                return False
            p += r[2]
        else:
            return False
    return True


def envelope(rec: bytes):
    """(status, (TxHash offset, length), [(element body offset, length)]) by the envelope rules alone"""
    end = len(rec)
    if end == 0:
        return EMPTY, (0, 0), []
    p, last, th, elems = 0, 0, (0, 0), []
    k = field_key(rec, 0, end)
    if k is None:
        return CORRUPT, (0, 0), []
    if k[0] == 1:
        if k[1] != BYTES:
            return CORRUPT, (0, 0), []
        r = byte_slice(rec, k[2], end)
        if r is None:
            return CORRUPT, (0, 0), []
        th = (r[0], r[1])
        last = 1
        p = k[2] + r[2]
    while p < end:
        k = field_key(rec, p, end)
        if k is None:
            return CORRUPT, (0, 0), []
        if k[0] != 2 or last > 2:
            break
        if k[1] != BYTES:
            return CORRUPT, (0, 0), []
        last = 2
        r = byte_slice(rec, p + k[2], end)
        if r is None:
            return CORRUPT, (0, 0), []
        elems.append((r[0], r[1]))
        p += k[2] + uvarint_size(r[1]) + r[1]      # the minimal prefix size, not the bytes read
    if not skip_rest(rec, p, end, last):
        return CORRUPT, (0, 0), []
    return OK, th, elems


def decode(O, rec: bytes):
    """(status, (TxHash offset, length), votes): votes are dicts nil / height / txhash / ts_sec /
    ts_nanos / addr / sig / txkey with the FULL addr and sig bytes; [] unless status is OK"""
    st, th, elems = envelope(rec)
    if st != OK:
        return st, (0, 0), []
    prefix = O.wire_prefix()[1]
    votes = []
    for body, blen in elems:
        if blen == 0:
            votes.append(dict(nil=True))
            continue
        msg = prefix + b"\x0a" + uvarint_enc(blen) + rec[body:body + blen]
        wst, f = O.wire_decode(msg, max_msg_bytes=1 << 30)
        if wst != O.WIRE_OK:
            return CORRUPT, (0, 0), []
        votes.append(dict(nil=False, height=f["height"], txhash=f["txhash"], ts_sec=f["ts_sec"], ts_nanos=f["ts_nanos"],
                          addr=f["addr"], sig=f["sig"], txkey=f["txkey"]))
    return OK, th, votes


def commit_encode(txhash: bytes, bodies) -> bytes:
    """a Commit record from its TxHash and its elements' bytes (b"" = a nil *CommitSig)"""
    out = bytearray()
    if txhash:
        out += b"\x0a" + uvarint_enc(len(txhash)) + txhash
    for body in bodies:
        out += b"\x12" + uvarint_enc(len(body)) + body
    return bytes(out)


def vote_body(O, v) -> bytes:
    """cdc.MarshalBinaryBare(TxVote) of a vote dict (a CommitSig's bytes)"""
    body = O.txvote_bytes(v["height"], v["txhash"], v["ts_sec"], v["ts_nanos"], v["addr"], v["sig"], v["txkey"])
    assert body is not None, v
    return body


def columns(votes):
    """the route buffer's columns for decoded votes: a list of tuples (is_nil, height, ts_sec,
    ts_nanos, txhash, addr_len, sig_len, addr[:20] zero padded, sig[:64] zero padded, txkey)"""
    rows = []
    for v in votes:
        if v["nil"]:
            rows.append((1, 0, 0, 0, b"", 0, 0, bytes(20), bytes(64), bytes(32)))
        else:
            rows.append((0, v["height"], v["ts_sec"], v["ts_nanos"], v["txhash"], len(v["addr"]), len(v["sig"]),
                         v["addr"][:20].ljust(20, b"\0"), v["sig"][:64].ljust(64, b"\0"), v["txkey"]))
    return rows


def batch_columns(batch, first=0, count=None):
    """the same tuples out of a txflow_amd.VoteBatch (route_view of a loaded buffer)"""
    count = batch.n - first if count is None else count
    rows = []
    for i in range(first, first + count):
        nil = int(batch.is_nil[i]) if batch.is_nil is not None else 0
        rows.append((nil, int(batch.height[i]), int(batch.ts_sec[i]), int(batch.ts_nanos[i]), batch.txhash(i),
                     int(batch.addr_len[i]), int(batch.sig_len[i]), batch.addr[20 * i:20 * i + 20].tobytes(),
                     batch.sig[64 * i:64 * i + 64].tobytes(), batch.txkey[32 * i:32 * i + 32].tobytes()))
    return rows
