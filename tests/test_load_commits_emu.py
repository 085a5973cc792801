"""The Commit loader's decode SOURCE (go-txflow_amd/csrc/load_dev.h: the envelope walk through a
refilled window, the element parse, the row copies), compiled for the host by
tests/cpu_emu/emu_load.hip and driven as kernels_load.hip drives it, against two references: the
Python model of the envelope rules in load_model.py, and oracle.wire_decode for every element body
(wrapped as a TxVoteMessage).  Windows of 32 and 48 bytes put every key and count across a window
edge; byte residues 0..15 move the row copies through every alignment."""
import ctypes
import os
import random
import subprocess

import pytest

import oracle as O
import load_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_load.so")
MIN_SEC, MAX_SEC = -62135596800, 253402300800


class EmuVote(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int64), ("sec", ctypes.c_int64), ("nanos", ctypes.c_int32),
                ("is_nil", ctypes.c_uint32), ("th_off", ctypes.c_uint32), ("th_len", ctypes.c_uint32),
                ("addr_len", ctypes.c_uint32), ("sig_len", ctypes.c_uint32), ("has_key", ctypes.c_uint32),
                ("addr", ctypes.c_uint8 * 20), ("sig", ctypes.c_uint8 * 64), ("key", ctypes.c_uint8 * 32)]


@pytest.fixture(scope="module")
def emu():
    O.build()
    src = os.path.join(EMU_DIR, "emu_load.hip")
    deps = [src] + [os.path.join(HERE, "..", "go-txflow_amd", "csrc", f) for f in ("load_dev.h", "wire_dev.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    E.emu_load_record.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                  u32p, u32p, u32p, ctypes.POINTER(EmuVote), u32p]
    return E


def run(emu, rec: bytes, window: int, shift: int):
    """-> (status, (TxHash offset, length), column tuples as load_model.columns, refills)"""
    cap = len(rec) // 2 + 1
    votes = (EmuVote * cap)()
    tho, thl, n, fills = (ctypes.c_uint32() for _ in range(4))
    st = emu.emu_load_record(rec, len(rec), window, shift, cap, ctypes.byref(tho), ctypes.byref(thl), ctypes.byref(n),
                             votes, ctypes.byref(fills))
    assert st >= 0, st
    rows = []
    for v in votes[:n.value]:
        rows.append((v.is_nil, v.height, v.sec, v.nanos, rec[v.th_off:v.th_off + v.th_len], v.addr_len, v.sig_len,
                     bytes(v.addr), bytes(v.sig), bytes(v.key)))
    return st, (tho.value, thl.value), rows, fills.value


def check(emu, rec: bytes, windows=(32, 48, 256, 640, 4096), shifts=(0, 5)):
    """the emulated decode equals the model's at every window and residue; returns the model's answer"""
    st, th, votes = M.decode(O, rec)
    want = (st, th if st == M.OK and th[1] else (0, 0), M.columns(votes))
    for w in windows:
        for s in shifts:
            got = run(emu, rec, w, s)
            th_got = got[1] if got[1][1] else (0, 0)
            assert (got[0], th_got, got[2]) == want, (rec.hex(), w, s)
    return st, th, votes


def rb(rnd, n):
    return bytes(rnd.getrandbits(8) for _ in range(n))


def vote(rnd, **kw):
    v = dict(height=rnd.randrange(1, 1 << 40), txhash=rb(rnd, 64).hex()[:64].upper().encode(),
             ts_sec=1_700_000_000 + rnd.randrange(1000), ts_nanos=rnd.randrange(1_000_000_000), addr=rb(rnd, 20),
             sig=rb(rnd, 64), txkey=rb(rnd, 32))
    v.update(kw)
    return v


def same(votes, want):
    """model votes == the vote dicts a record was written from"""
    assert len(votes) == len(want)
    for g, w in zip(votes, want):
        assert not g["nil"]
        assert {k: g[k] for k in w} == w


def test_commit_bytes_round_trip(emu):
    """every record oracle.commit_bytes writes decodes to the votes it was written from"""
    rnd = random.Random(11)
    for height in (0, 1, (1 << 63) - 1):
        for hl in (0, 1, 64, 127, 128, 200):
            th = rb(rnd, hl)
            votes = [vote(rnd, height=height, txhash=th) for _ in range(3)]
            rec = O.commit_bytes(th, votes)
            st, tho, got = check(emu, rec, shifts=range(16) if hl == 64 else (0, 5))
            assert st == M.OK and rec[tho[0]:tho[0] + tho[1]] == th
            same(got, votes)


def test_field_edges(emu):
    rnd = random.Random(12)
    th = b"A" * 64
    cases = [dict(ts_sec=MIN_SEC, ts_nanos=0), dict(ts_sec=MAX_SEC - 1, ts_nanos=999999999), dict(ts_sec=0, ts_nanos=0)]
    cases += [dict(sig=rb(rnd, n)) for n in (0, 63, 64, 65)]
    cases += [dict(addr=rb(rnd, n)) for n in (0, 19, 20, 21)]
    votes = [vote(rnd, txhash=th, **c) for c in cases]
    st, _, got = check(emu, O.commit_bytes(th, votes), shifts=range(16))
    assert st == M.OK
    same(got, votes)
    for c in cases:     # ... and each alone, so that it is also the record's last element
        v = vote(rnd, txhash=th, **c)
        st, _, got = check(emu, O.commit_bytes(th, [v]))
        assert st == M.OK
        same(got, [v])


def test_nil_empty_and_absent_parts(emu):
    rnd = random.Random(13)
    th = b"B" * 64
    a, b = vote(rnd, txhash=th), vote(rnd, txhash=th)
    st, _, got = check(emu, M.commit_encode(th, [M.vote_body(O, a), b"", M.vote_body(O, b)]))
    assert st == M.OK and [g["nil"] for g in got] == [False, True, False]
    st, tho, got = check(emu, M.commit_encode(th, []))                 # no elements
    assert st == M.OK and got == [] and tho[1] == 64
    st, tho, got = check(emu, M.commit_encode(b"", [M.vote_body(O, a)]))   # no TxHash
    assert st == M.OK and tho[1] == 0 and len(got) == 1
    assert check(emu, b"")[0] == M.EMPTY
    # a CommitSig carries its own TxHash, whatever the envelope says
    c = vote(rnd, txhash=b"another hash")
    st, _, got = check(emu, M.commit_encode(th, [M.vote_body(O, c)]))
    assert st == M.OK and got[0]["txhash"] == b"another hash"


def test_malformed_envelopes(emu):
    rnd = random.Random(14)
    th = b"C" * 64
    bodies = [M.vote_body(O, vote(rnd, txhash=th)) for _ in range(2)]
    good = M.commit_encode(th, bodies)
    assert check(emu, good)[0] == M.OK
    # an unknown field 3 at the end is skipped, whatever its typ3
    for tail in (b"\x18\x07", b"\x1a\x03abc", b"\x19" + bytes(8), b"\x1d" + bytes(4)):
        st, _, got = check(emu, good + tail)
        assert st == M.OK and len(got) == 2
    assert check(emu, good + b"\x1b")[0] == M.CORRUPT                   # typ3 3 cannot be skipped
    assert check(emu, good + b"\x1a\x05ab")[0] == M.CORRUPT             # count past the record
    # field 1 after field 2, field 2 after field 3, field 2 as a varint, field 1 as a varint, key 0
    one = b"\x12" + M.uvarint_enc(len(bodies[0])) + bodies[0]
    assert check(emu, one + b"\x0a\x01x")[0] == M.CORRUPT
    assert check(emu, good + b"\x18\x07" + one)[0] == M.CORRUPT
    assert check(emu, b"\x0a\x01x\x10\x05")[0] == M.CORRUPT
    assert check(emu, b"\x08\x05" + one)[0] == M.CORRUPT
    assert check(emu, b"\x00\x00")[0] == M.CORRUPT
    assert check(emu, b"\x0a\x01x\x0a\x01y")[0] == M.CORRUPT            # TxHash twice
    # overlong uvarints in a length: Go accepts them; the parent then advances by the MINIMAL size
    body = bodies[0]
    over = b"\x12" + bytes([0x80 | (len(body) & 0x7F), 0x80 | (len(body) >> 7), 0x00]) + body
    check(emu, M.commit_encode(th, []) + over)                           # the model decides
    check(emu, M.commit_encode(th, []) + over + one)
    assert check(emu, b"\x0a\xc0\x80\x00" + th + one)[0] == M.OK         # overlong TxHash count: a bytes field
    assert check(emu, b"\x12" + b"\xff" * 10 + b"\x01")[0] == M.CORRUPT  # uvarint overflow
    assert check(emu, b"\x12\x80")[0] == M.CORRUPT                       # count runs out of bytes
    # a bad inner TxKey length makes the whole record CORRUPT
    v = vote(rnd, txhash=th)
    b0 = M.vote_body(O, v)
    i = b0.index(b"\x1a\x20" + v["txkey"])
    bad = b0[:i] + b"\x1a\x1f" + v["txkey"][:31] + b0[i + 34:]
    assert check(emu, M.commit_encode(th, [bodies[0], bad, bodies[1]]))[0] == M.CORRUPT


def test_every_truncation(emu):
    """a cut at an element boundary is a valid shorter Commit, so the model decides, not this test"""
    rnd = random.Random(15)
    th = b"D" * 64
    rec = O.commit_bytes(th, [vote(rnd, txhash=th) for _ in range(3)])
    seen = {}
    for cut in range(len(rec) + 1):
        st, _, got = check(emu, rec[:cut], windows=(32, 256, 4096), shifts=(cut % 16,))
        seen.setdefault((st, len(got)), cut)
    assert {(M.EMPTY, 0), (M.CORRUPT, 0), (M.OK, 0), (M.OK, 1), (M.OK, 2), (M.OK, 3)} <= set(seen)


def test_window_refills_on_a_long_record(emu):
    """200 elements of varied length through a 32-byte window: a refill per hop at least, the same votes"""
    rnd = random.Random(16)
    votes = [vote(rnd, txhash=rb(rnd, rnd.randrange(0, 90)), sig=rb(rnd, rnd.choice((0, 1, 63, 64))),
                  height=rnd.choice((0, 1, 300, 1 << 50))) for _ in range(200)]
    rec = M.commit_encode(b"E" * 64, [M.vote_body(O, v) for v in votes])
    st, _, got = check(emu, rec, windows=(32, 64, 256, 400, 1024, 12288), shifts=(3, 7))
    assert st == M.OK
    same(got, votes)
    assert run(emu, rec, 32, 3)[3] >= 200 and run(emu, rec, 1 << 20, 3)[3] == 1


def test_mutated_records_agree_with_the_model(emu):
    """random byte edits of valid records: whatever the rules make of them, both sides agree"""
    rnd = random.Random(17)
    seen = set()
    for _ in range(1500):
        th = rb(rnd, rnd.choice((0, 3, 64)))
        bodies = [b"" if rnd.random() < 0.1 else M.vote_body(O, vote(rnd, txhash=th, height=rnd.choice((0, 7))))
                  for _ in range(rnd.randrange(0, 4))]
        rec = bytearray(M.commit_encode(th, bodies))
        for _ in range(rnd.randrange(0, 3)):
            if rec:
                rec[rnd.randrange(len(rec))] = rnd.choice((0, 1, 0x0A, 0x12, 0x1A, 0x7F, 0x80, 0xFF, rnd.getrandbits(8)))
        if rnd.random() < 0.2 and rec:
            del rec[rnd.randrange(len(rec)):]
        seen.add(check(emu, bytes(rec), windows=(32, 256, 512, 4096), shifts=(rnd.randrange(16),))[0])
    assert seen == {M.OK, M.CORRUPT, M.EMPTY}
