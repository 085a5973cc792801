"""TXV_POOL_SENDERS at the drop-in boundary (no GPU, no compute beyond a host pool of two votes): the
header declares the flag and the functions, the library exports them, the argument checks answer
as include/txvote.h says, and the Python mirror exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import txflow_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -22, -1

FUNCS = ["txv_pool_check_submit_from", "txv_pool_check_from", "txv_pool_check_keys_from", "txv_pool_receive_from",
         "txv_ingest_decode_from", "txv_pool_sent_by", "txv_pool_ticket_sent_by"]


def header():
    return open(os.path.join(ROOT, "include", "txvote.h")).read()


def test_header_declares_flag_and_functions():
    h = header()
    assert re.search(r"#define\s+TXV_POOL_SENDERS\s+0x4u", h)
    assert re.search(r"#define\s+TXV_ABI_VERSION\s+2\b", h), "additions only: the ABI version stays 2"
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
    assert T.POOL_SENDERS == 0x4


def test_library_exports_them():
    lib = ctypes.CDLL(T.LIB_PATH)
    for f in FUNCS:
        assert hasattr(lib, f), f
        assert f in T.EXPORTED_SYMBOLS, f


def _args():
    keys = np.zeros((2, 32), np.uint8)
    keys[1, 0] = 1
    return keys, np.full(2, 120, np.uint32), np.array([1, 2], np.uint16), np.zeros(2, np.uint8), np.zeros(2, np.uint32)


def test_null_pool_is_einval():
    L = T.lib()
    keys, sizes, snd, st, bits = _args()
    t = ctypes.c_uint64()
    assert L.txv_pool_check_keys_from(None, None, keys.ctypes.data, sizes.ctypes.data, 2, snd.ctypes.data,
                                      st.ctypes.data) == EINVAL
    assert L.txv_pool_sent_by(None, None, keys.ctypes.data, 2, snd.ctypes.data, 2, bits.ctypes.data) == EINVAL
    assert L.txv_pool_ticket_sent_by(None, None, 1, snd.ctypes.data, 2, bits.ctypes.data) == EINVAL
    assert L.txv_pool_check_submit_from(None, None, None, None, None, snd.ctypes.data, ctypes.byref(t)) == EINVAL
    assert L.txv_pool_check_from(None, None, None, None, None, snd.ctypes.data, st.ctypes.data) == EINVAL
    assert L.txv_pool_receive_from(None, None, None, 0, None, None, 0, snd.ctypes.data, None, None) == EINVAL
    assert L.txv_ingest_decode_from(None, None, None, 0, None, None, 0, snd.ctypes.data, ctypes.byref(t)) == EINVAL


def test_sent_by_argument_checks():
    L = T.lib()
    keys, sizes, snd, st, bits = _args()
    p = T.TxVotePool(None, senders=True)
    assert L.txv_pool_sent_by(p._h, None, keys.ctypes.data, 2, None, 2, bits.ctypes.data) == EINVAL
    assert L.txv_pool_sent_by(p._h, None, keys.ctypes.data, 2, snd.ctypes.data, 0, bits.ctypes.data) == EINVAL
    assert L.txv_pool_sent_by(p._h, None, None, 2, snd.ctypes.data, 2, bits.ctypes.data) == EINVAL
    assert L.txv_pool_sent_by(p._h, None, keys.ctypes.data, 2, snd.ctypes.data, 2, None) == EINVAL
    assert L.txv_pool_sent_by(p._h, None, keys.ctypes.data, 2, snd.ctypes.data, 2, bits.ctypes.data) == 0
    p.close()


def test_pool_without_the_flag_is_estate_and_untouched():
    L = T.lib()
    keys, sizes, snd, st, bits = _args()
    p = T.TxVotePool(None)
    assert L.txv_pool_sent_by(p._h, None, keys.ctypes.data, 2, snd.ctypes.data, 2, bits.ctypes.data) == ESTATE
    assert L.txv_pool_check_keys_from(p._h, None, keys.ctypes.data, sizes.ctypes.data, 2, snd.ctypes.data,
                                      st.ctypes.data) == ESTATE
    assert p.Size() == 0 and len(p.cache_keys()) == 0, "a refused _from call touches nothing"
    with pytest.raises(T.TxvInfraError):
        p.check_keys(keys, sizes, senders=snd)
    with pytest.raises(T.TxvInfraError):
        p.sent_by(keys, snd)
    # a NULL column is the plain call
    assert L.txv_pool_check_keys_from(p._h, None, keys.ctypes.data, sizes.ctypes.data, 2, None, st.ctypes.data) == 0
    assert p.Size() == 2
    p.close()


def test_python_mirror():
    import inspect
    for m in ("check", "check_batch", "check_submit", "check_keys", "receive", "ingest_decode"):
        assert "senders" in inspect.signature(getattr(T.TxVotePool, m)).parameters, m
    assert "senders" in inspect.signature(T.TxVotePool.__init__).parameters
    assert callable(T.TxVotePool.sent_by) and callable(T.TxVotePool.ticket_sent_by)
    keys, sizes, snd, _, _ = _args()
    p = T.TxVotePool(None, senders=True)
    assert list(p.check_keys(keys, sizes, senders=snd)) == [0, 0]
    got = p.sent_by(keys, [1, 2, 3])
    assert got.dtype == bool and got.tolist() == [[True, False, False], [False, True, False]]
    with pytest.raises(ValueError):
        p.check_keys(keys, sizes, senders=snd[:1])
    p.close()
