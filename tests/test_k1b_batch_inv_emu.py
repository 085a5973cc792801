"""K1b's block hand-off arithmetic SOURCE (go-txflow_amd/csrc/fe_batch_inv.h: fe_invert_each, the
product over a block's waves and its back-substitution), compiled for the host by
tests/cpu_emu/emu_batch_inv.hip: every 1/x_i against fe_invert of that element alone and against
Python integers, for chains of 1..8 elements, with ONE call of the inverter per chain.

No element is 0 mod p: the function has no zero fallback on purpose (its header says why), and
K1b's elements -- products of Z coordinates of complete additions, 1 for idle lanes -- never are."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "cpu_emu")
EMU = os.path.join(EMU_DIR, "build", "libemu_batch_inv.so")
P = 2 ** 255 - 19

# fe (fe.h) is 8 x 32-bit limbs, "weakly reduced": fe_mul takes and returns any value in
# [0, 2^256).  Its bounds are therefore the ends of that range and of the canonical one, limbs all
# ones, and the values around the 2^256 = 38 fold; 0, p and 2p = 2^256 - 38 (0 mod p) are left out.
BOUNDS = [1, 2, 18, 19, 20, 37, 38, 39, P - 1, P + 1, P + 18, P + 19, 2 ** 255 - 1, 2 ** 255, 2 ** 255 + 18,
          2 * P - 1, 2 * P + 1, 2 ** 256 - 36, 2 ** 256 - 2, 2 ** 256 - 1, 2 ** 32 - 1, 2 ** 32,
          2 ** 224, 2 ** 256 - 2 ** 224, (2 ** 256 - 1) // 3, int("10" * 128, 2)]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(EMU_DIR, "emu_batch_inv.hip")
    csrc = os.path.join(HERE, "..", "go-txflow_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("fe_batch_inv.h", "fe_inv_var.h", "fe.h")]
    if not os.path.exists(EMU) or any(os.path.getmtime(d) > os.path.getmtime(EMU) for d in deps):
        os.makedirs(os.path.dirname(EMU), exist_ok=True)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", EMU], check=True)
    E = ctypes.CDLL(EMU)
    E.emu_invert_each.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    E.emu_invert_each.restype = ctypes.c_int
    E.emu_fe_invert_canon.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return E


def words(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def value(ws):
    return sum(int(v) << (32 * i) for i, v in enumerate(ws))


def check_chain(emu, xs):
    """fe_invert_each over xs with both inverters: one inverter call, every result in [0, 2^256)
    and equal mod p to fe_invert of the element alone and to pow(x, p - 2, p)"""
    n = len(xs)
    one = (ctypes.c_uint32 * 8)()
    alone = []
    for x in xs:
        emu.emu_fe_invert_canon((ctypes.c_uint32 * 8)(*words(x)), one)
        alone.append(value(one))
        assert alone[-1] == pow(x, P - 2, P)
    for which in (0, 1):
        buf = (ctypes.c_uint32 * (8 * n))(*[w for x in xs for w in words(x)])
        assert emu.emu_invert_each(buf, n, which) == 1
        for i, x in enumerate(xs):
            got = value(buf[8 * i:8 * i + 8])
            assert got < 2 ** 256 and got % P == alone[i], (which, n, i, [hex(v) for v in xs])


@pytest.mark.parametrize("n", range(1, 9))
def test_random_chains(emu, n):
    rnd = random.Random(100 + n)
    for _ in range(40):
        check_chain(emu, [rnd.randrange(1, 2 ** 256) for _ in range(n)])
    for _ in range(10):                      # canonical values, as verify_invert returns them
        check_chain(emu, [rnd.randrange(1, P) for _ in range(n)])


@pytest.mark.parametrize("n", range(1, 9))
def test_ones_in_every_position(emu, n):
    """idle waves and idle lanes hand in P = 1: alone, everywhere, and every subset of positions"""
    rnd = random.Random(200 + n)
    for mask in range(1 << n):
        check_chain(emu, [1 if mask >> i & 1 else rnd.randrange(2, 2 ** 256) for i in range(n)])


@pytest.mark.parametrize("n", range(1, 9))
def test_values_at_the_limb_bounds(emu, n):
    rnd = random.Random(300 + n)
    for k in range(len(BOUNDS)):             # every bound in every position, bounds as neighbours
        check_chain(emu, [BOUNDS[(k + i) % len(BOUNDS)] for i in range(n)])
    for b in BOUNDS:
        for pos in range(n):
            xs = [rnd.randrange(1, 2 ** 256) for _ in range(n)]
            xs[pos] = b
            check_chain(emu, xs)
    check_chain(emu, [2 ** 256 - 1] * n)
    check_chain(emu, [P - 1] * n)


def test_chain_length_is_checked(emu):
    buf = (ctypes.c_uint32 * 72)(*([1] + [0] * 7) * 9)
    assert emu.emu_invert_each(buf, 0, 0) == -1 and emu.emu_invert_each(buf, 9, 0) == -1
