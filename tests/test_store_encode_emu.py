"""The store sink's encoder SOURCE (go-txflow_amd/csrc/store_dev.h: the record front, the CommitSig
lookup and the per-lane CommitSig writer txv_k_st_emit runs, over txvote_lanes.h), compiled for the
host by tests/cpu_emu/emu_store.hip and driven as the kernel drives it -- the record tile by tile,
16 lanes per CommitSig, each tile starting as garbage -- against oracle.save_tx_bytes: TxHash
lengths, vote counts with absent validators, the height and time edges, at several tile sizes."""
import ctypes
import os
import random
import subprocess

import pytest

import oracle as O
import gossip_cases as GC

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_store.so")

TILES = (16, 64, 3840, 4096)             # 3840 and 4096: txv_k_st_emit's own
HASH_LENS = (0, 1, 63, 64, 65, 127, 128, 300, 5000)
HEIGHTS = (0, 1, 127, 128, -1, (1 << 63) - 1, -(1 << 63))
COUNTS = ((3, 1), (4, 2), (24, 17))      # (validators, accepted votes): the rest are holes in the offset list


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(EMU_DIR, "emu_store.hip")
    deps = [src] + [os.path.join(HERE, "..", "go-txflow_amd", "csrc", f) for f in ("store_dev.h", "txvote_lanes.h", "amino.hpp")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    p = ctypes.c_char_p
    E.emu_store_record.argtypes = [p, ctypes.c_uint32, p, ctypes.c_uint32, p, ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), p, p, p, ctypes.c_uint32,
                                   p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    E.emu_store_record.restype = ctypes.c_int64
    return E


@pytest.fixture(scope="module")
def time_edges():
    """the (sec, nanos) of gossip_cases.edge_votes that amino encodes"""
    ts = sorted({(v["ts_sec"], v["ts_nanos"]) for v in GC.edge_votes(random.Random(41)) if GC.expected(v)[0] != GC.UNENCODABLE})
    assert {(0, 0), (0, 5), (GC.SEC, 0), (-1, 1), (-1, 0), (GC.MIN_SEC, 0), (GC.MAX_SEC - 1, 999_999_999)} <= set(ts)
    return ts


def _set(rnd, hl, n_vals, stamps):
    """a set over n_vals validators: one accepted vote per (height, sec, nanos) of stamps, at random
    validators; every vote with a TxKey of its own, none the set's"""
    txhash = GC.rbytes(rnd, hl)
    who = sorted(rnd.sample(range(n_vals), len(stamps)))
    votes = {v: dict(height=h, ts_sec=s, ts_nanos=ns, addr=GC.rbytes(rnd, 20), sig=GC.rbytes(rnd, 64), txkey=GC.rbytes(rnd, 32))
             for v, (h, s, ns) in zip(who, stamps)}
    return txhash, GC.rbytes(rnd, 32), n_vals, votes


def _check(emu, case, tile):
    txhash, set_txkey, n_vals, votes = case
    parts = O.save_tx_bytes(txhash, set_txkey, [votes[v] for v in sorted(votes)])   # CommitSigs in validator order
    assert all(v["txkey"] != set_txkey for v in votes.values())
    want = b"".join(parts)
    col = lambda key, n: b"".join(votes[v][key] if v in votes else b"\xAA" * n for v in range(n_vals))
    num = lambda key, ct: (ct * n_vals)(*[votes[v][key] if v in votes else 77 for v in range(n_vals)])
    cap = (len(want) + 15) // 16 * 16 + 16
    out = ctypes.create_string_buffer(b"\xEE" * cap, cap)
    lens = (ctypes.c_uint32 * 4)()
    len16 = emu.emu_store_record(txhash, len(txhash), set_txkey, n_vals, bytes(int(v in votes) for v in range(n_vals)),
                                 num("height", ctypes.c_int64), num("ts_sec", ctypes.c_int64), num("ts_nanos", ctypes.c_int32),
                                 col("sig", 64), col("txkey", 32), col("addr", 20), tile, out, cap, lens)
    what = (len(txhash), n_vals, len(votes), tile)
    assert len16 == (len(want) + 15) // 16 * 16, what
    assert list(lens) == [len(p) for p in parts], what
    o = 0
    for k, part in enumerate(parts):
        assert out.raw[o:o + len(part)] == part, (what, k)
        o += len(part)
    assert not any(out.raw[o:len16]), what
    assert out.raw[len16:] == b"\xEE" * (cap - len16), what


def test_hash_lengths_counts_tiles(emu, time_edges):
    rnd = random.Random(53)
    for hl in HASH_LENS:
        for n_vals, n_votes in COUNTS:
            stamps = [(rnd.choice(HEIGHTS), *rnd.choice(time_edges)) for _ in range(n_votes)]
            case = _set(rnd, hl, n_vals, stamps)
            for tile in TILES:
                _check(emu, case, tile)


def test_height_and_time_edges(emu, time_edges):
    """every height with every encodable time once, as the votes of one set with holes"""
    rnd = random.Random(59)
    stamps = [(h, s, ns) for h in HEIGHTS for (s, ns) in time_edges]
    assert (0, 0, 0) in stamps                    # neither a Height nor a Timestamp field
    for hl in (0, 64, 300):
        for lo in range(0, len(stamps), 100):
            part = stamps[lo:lo + 100]
            case = _set(rnd, hl, 128, part)
            for tile in TILES:
                _check(emu, case, tile)
