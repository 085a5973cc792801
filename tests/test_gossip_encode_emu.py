"""The gossip sink's encoder SOURCE (go-txflow_amd/csrc/gossip_dev.h: the length / flag rule of a
batch entry and the per-lane field encoder txv_k_gs_emit runs), compiled for the host by
tests/cpu_emu/emu_gossip.hip and driven as the kernel drives it -- 16 lanes per message, tile by
tile, each tile starting as garbage -- against oracle.wire_encode: the edge matrix of
gossip_cases.py and a few thousand random votes of wire_gen.rand_vote, at several tile sizes."""
import ctypes
import os
import random
import subprocess

import pytest

import oracle as O
import gossip_cases as GC

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_gossip.so")


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(EMU_DIR, "emu_gossip.hip")
    deps = [src] + [os.path.join(HERE, "..", "go-txflow_amd", "csrc", f) for f in ("gossip_dev.h", "txvote_lanes.h", "amino.hpp")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    E.emu_gossip_encode.argtypes = [ctypes.c_int64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int32,
                                    ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p,
                                    ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                    ctypes.POINTER(ctypes.c_uint32)]
    return E


def _encode(emu, v, prefix, tile, with_key=True):
    """-> (flag, message bytes, the padding behind them)"""
    cap = (len(v["txhash"]) + 400) // 16 * 16
    out = ctypes.create_string_buffer(b"\xEE" * cap, cap)
    n = ctypes.c_uint32()
    flag = emu.emu_gossip_encode(v["height"], v["txhash"], len(v["txhash"]), v["ts_sec"], v["ts_nanos"],
                                 v["addr"][:20].ljust(20, b"\0"), len(v["addr"]), v["sig"][:64].ljust(64, b"\0"),
                                 len(v["sig"]), v["txkey"] if with_key else None, prefix, tile, out, cap,
                                 ctypes.byref(n))
    assert flag >= 0
    return flag, out.raw[:n.value], out.raw[n.value:(n.value + 15) // 16 * 16]


def _check(emu, v, prefix, tile, with_key=True):
    eflag, ebytes = GC.expected(v, with_key)
    flag, got, pad = _encode(emu, v, prefix, tile, with_key)
    assert flag == eflag, v
    assert got == ebytes, (v, tile)
    assert not any(pad), (v, tile)


def test_edge_matrix(emu):
    prefix = int.from_bytes(O.wire_prefix()[1], "little")
    for v in GC.edge_votes(random.Random(41)):
        for tile in (16, 64, 512):
            _check(emu, v, prefix, tile)
        _check(emu, v, prefix, 512, with_key=False)


def test_random_votes(emu):
    import wire_gen as G
    prefix = int.from_bytes(O.wire_prefix()[1], "little")
    rng = random.Random(43)
    flags = set()
    for k in range(4000):
        r = G.rand_vote(rng)
        v = dict(height=r["height"], txhash=r["txhash"], ts_sec=r["ts"][0], ts_nanos=r["ts"][1], addr=r["addr"],
                 sig=r["sig"], txkey=r["txkey"])
        flags.add(GC.expected(v)[0])
        _check(emu, v, prefix, (16, 48, 512, 4096)[k % 4])
    assert flags == {GC.OK, GC.HOST}


def test_long_txhash_spans_tiles(emu):
    prefix = int.from_bytes(O.wire_prefix()[1], "little")
    rnd = random.Random(47)
    for hl in (5000, 16383, 16384, 70000):
        v = GC.vote(rnd, txhash=GC.rbytes(rnd, hl))
        _check(emu, v, prefix, 512)
