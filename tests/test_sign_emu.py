"""The batch signer's integer SOURCE (go-txflow_amd/csrc/sign_dev.h and ed25519_dev.h's next_digit),
compiled for the host by tests/cpu_emu/emu_sign.hip: the tx hash (SHA-256 with its padding, read by
aligned words at every alignment) and its upper-case hex against hashlib, S = (r + k a) mod L against
Python integers, and the base-point walk's signed digits reassembled against the scalar."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_sign.so")
L = 2 ** 252 + 27742317777372353535851937790883648493
BASE_WINDOWS = (4, 8, 10, 12, 14, 16, 20, 22, 24, 26)


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(EMU_DIR, "emu_sign.hip")
    csrc = os.path.join(HERE, "..", "go-txflow_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("sign_dev.h", "ed25519_dev.h", "sha2.h", "sc.h", "fe.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    E.emu_tx_hash.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
    E.emu_tx_hash.restype = None
    E.emu_sc_muladd.argtypes = [ctypes.c_char_p] * 4
    E.emu_sc_muladd.restype = None
    E.emu_base_digits.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)]
    return E


def test_tx_hash_and_hex_at_every_length_and_alignment(emu):
    rnd = random.Random(5)
    for n in range(0, 131):
        tx = bytes(rnd.getrandbits(8) for _ in range(n))
        want = hashlib.sha256(tx).digest()
        for shift in range(4):
            key, hx = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
            emu.emu_tx_hash(tx, n, shift, key, hx)
            assert key.raw == want, (n, shift)
            assert hx.raw == want.hex().upper().encode(), (n, shift)


def _muladd(emu, k, a, r):
    out = ctypes.create_string_buffer(32)
    emu.emu_sc_muladd(k.to_bytes(32, "little"), a.to_bytes(32, "little"), r.to_bytes(32, "little"), out)
    return int.from_bytes(out.raw, "little")


def test_sc_muladd_edges_and_random(emu):
    for a in (2 ** 254, 2 ** 255 - 8):
        for k in (0, 1, L - 1):
            for r in (0, 1, L - 1):
                assert _muladd(emu, k, a, r) == (r + k * a) % L, (k, a, r)
    rnd = random.Random(7)
    for _ in range(1000):
        k, r = rnd.randrange(L), rnd.randrange(L)
        a = (rnd.getrandbits(256) & ~7 & (2 ** 255 - 1)) | 2 ** 254     # a clamped scalar
        assert _muladd(emu, k, a, r) == (r + k * a) % L


@pytest.mark.parametrize("w", BASE_WINDOWS)
def test_base_digits_reassemble_the_scalar(emu, w):
    rnd = random.Random(100 + w)
    half = 1 << (w - 1)
    pos = (256 + w - 1) // w
    top = (252 // w)
    scalars = [0, 1, 2, L - 1, L, 2 ** 252, 2 ** 253 - 1,
               sum(half << (w * i) for i in range(top)) % 2 ** 253,          # every digit rolls over to -2^(w-1)
               sum((half - 1) << (w * i) for i in range(top)),               # every digit +2^(w-1) - 1
               1 << (w * top)]                                               # all zero but the top one
    scalars += [rnd.randrange(L) for _ in range(300)]
    out = (ctypes.c_int32 * 64)()
    for s in scalars:
        assert emu.emu_base_digits(w, s.to_bytes(32, "little"), out) == pos
        d = list(out[:pos])
        assert sum(x << (w * i) for i, x in enumerate(d)) == s, (w, s)
        assert all(-half <= x < half for x in d[:-1]) and 0 <= d[-1] <= half, (w, s, d)   # table entries 0 .. 2^(w-1)
    assert emu.emu_base_digits(7, bytes(32), out) == -1
