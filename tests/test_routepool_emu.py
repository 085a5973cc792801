"""The per-vote SOURCE of CheckTx from a route buffer (go-txflow_amd/csrc/routepool_dev.h), compiled
for the host by tests/cpu_emu/emu_routepool.hip: the signature key against hashlib for every length
0..64, TxVote.Size() against the oracle over the encoder's edges, the valid flag, and the header
compare that guards every read beyond the buffer's first 64 bytes."""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_routepool.so")
MAGIC = int.from_bytes(b"TVXTVR01", "little")


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(EMU_DIR, "emu_routepool.hip")
    csrc = os.path.join(HERE, "..", "go-txflow_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("routepool_dev.h", "route.h", "amino.hpp", "sha2.h", "fe.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    E.emu_route_key.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    E.emu_route_key.restype = None
    E.emu_route_size.argtypes = [ctypes.c_int64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32,
                                 ctypes.c_uint32]
    E.emu_route_size.restype = ctypes.c_uint32
    E.emu_route_valid.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    E.emu_route_valid.restype = ctypes.c_uint32
    E.emu_route_header_ok.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint64]
    E.emu_route_header_ok.restype = ctypes.c_int
    return E


def test_key_is_sha256_of_the_first_len_bytes(emu):
    """every sig_len 0..64 (one block up to 55, two from 56; the 0x80 in the second block only at
    64), the row's bytes beyond len being garbage the key must not see"""
    rnd = random.Random(11)
    for ln in range(65):
        for _ in range(4):
            row = bytes(rnd.getrandbits(8) for _ in range(64))
            out = ctypes.create_string_buffer(32)
            emu.emu_route_key(row, ln, out)
            assert out.raw == hashlib.sha256(row[:ln]).digest(), ln
    for ln in (0, 1, 55, 56, 63, 64):           # all-ones rows: no stray bit survives the masks
        out = ctypes.create_string_buffer(32)
        emu.emu_route_key(b"\xff" * 64, ln, out)
        assert out.raw == hashlib.sha256(b"\xff" * ln).digest(), ln


HEIGHTS = (0, 1, 2 ** 63 - 1)
TH_LENS = (0, 64, 127, 128)
TIMES = ((0, 0), (0, 5), (-5, 3), (1_700_000_000, 999_999_999), (-62135596800, 0), (253402300799, 1))
BAD_TIMES = ((-62135596801, 0), (253402300800, 0), (5, -1), (5, 10 ** 9))
ADDR_LENS = (0, 20, 21)
SIG_LENS = (0, 1, 64, 65)


def test_size_equals_the_oracle_over_the_edges(emu):
    O.build()
    for h in HEIGHTS:
        for tl in TH_LENS:
            for sec, ns in TIMES:
                for al in ADDR_LENS:
                    for sl in SIG_LENS:
                        want = O.txvote_size(h, tl, sec, ns, al, sl)
                        assert want > 0
                        assert emu.emu_route_size(h, tl, sec, ns, al, sl) == want, (h, tl, sec, ns, al, sl)


def test_size_is_zero_when_amino_rejects_the_time(emu):
    O.build()
    for sec, ns in BAD_TIMES:
        assert O.txvote_size(1, 64, sec, ns, 20, 64) == 0
        assert emu.emu_route_size(1, 64, sec, ns, 20, 64) == 0, (sec, ns)


def test_valid_flag(emu):
    for sl in (0, 1, 63, 64):
        assert emu.emu_route_valid(0, sl) == 1
        assert emu.emu_route_valid(1, sl) == 0
    assert emu.emu_route_valid(0, 65) == 0
    assert emu.emu_route_valid(0, 2 ** 32 - 1) == 0
    assert emu.emu_route_valid(1, 65) == 0


def test_header_compare_accepts_the_true_header_and_rejects_each_field(emu):
    import txflow_amd as T
    n, arena, flags, mx = 65, 4160, T.ROUTE_TXKEY | T.ROUTE_NIL, 64
    total = int(T.lib().txv_route_bytes(n, arena, flags))
    hdr = np.array([MAGIC, n, arena, flags, mx, total, 0, 0], np.uint64)
    args = (n, arena, flags, mx, total)
    assert emu.emu_route_header_ok(hdr.ctypes.data, *args) == 1
    for k in range(6):                           # each header word changed in turn
        for delta in (1, 2 ** 32):
            bad = hdr.copy()
            bad[k] = (int(bad[k]) + delta) % 2 ** 64
            assert emu.emu_route_header_ok(bad.ctypes.data, *args) == 0, (k, delta)
    for k in range(5):                           # each meta field changed in turn
        a = list(args)
        a[k] += 1
        assert emu.emu_route_header_ok(hdr.ctypes.data, *a) == 0, k
    assert emu.emu_route_header_ok(np.zeros(8, np.uint64).ctypes.data, 0, 0, 0, 0, 0) == 0   # no magic
    # the header txv_route_pack_host writes is the one the compare expects
    b = T.VoteBatch.from_votes([T.TxVote(Height=1, TxHash="AB" * 32, Timestamp=(5, 6), ValidatorAddress=b"\1" * 20,
                                         Signature=b"\2" * 64) for _ in range(3)])
    bufs, metas = T.route_pack_host(b, None, 1)
    m = metas[0]
    h8 = np.frombuffer(bufs[0][:64].tobytes(), np.uint64).copy()
    assert emu.emu_route_header_ok(h8.ctypes.data, int(m["n"]), int(m["arena_bytes"]), int(m["flags"]),
                                   int(m["max_txhash_len"]), int(m["bytes"])) == 1
