"""CheckTx and TryAddVote from a route buffer in HBM, the surface without a GPU: include/txvote.h
declares txv_pool_check_routed_submit / txv_pool_check_routed / txv_submit_routed_checked /
txv_sign_txs_meta, libtxvote.so exports them, the Python mirror has the methods, and a NULL pool,
context, buffer, meta or ticket is TXV_EINVAL before anything is touched."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXV_EINVAL = -22
NAMES = ("txv_pool_check_routed_submit", "txv_pool_check_routed", "txv_submit_routed_checked", "txv_sign_txs_meta")


def test_header_declares_the_calls():
    src = open(os.path.join(ROOT, "include", "txvote.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+txv_pool_check_routed_submit\s*\(\s*txv_pool\s*\*\s*\w+,\s*txv_ctx\s*\*\s*\w+,\s*const\s+void\s*\*"
                     r"\s*\w+,\s*const\s+txv_route_meta\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\)", src)
    assert re.search(r"\bint\s+txv_pool_check_routed\s*\(\s*txv_pool\s*\*\s*\w+,\s*txv_ctx\s*\*\s*\w+,\s*const\s+void\s*\*\s*\w+,"
                     r"\s*const\s+txv_route_meta\s*\*\s*\w+,\s*uint8_t\s*\*\s*\w+\)", src)
    assert re.search(r"\bint\s+txv_submit_routed_checked\s*\(\s*txv_ctx\s*\*\s*\w+,\s*const\s+void\s*\*\s*\w+,\s*const\s+"
                     r"txv_route_meta\s*\*\s*\w+,\s*txv_pool\s*\*\s*\w+,\s*uint64_t\s+\w+,\s*uint64_t\s*\*\s*\w+\)", src)
    assert re.search(r"\bint\s+txv_sign_txs_meta\s*\(\s*txv_ctx\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*"
                     r"txv_route_meta\s*\*\s*\w+\)", src)
    assert "#define TXV_ABI_VERSION 2" in src


def test_header_cites_the_reference_lines():
    src = open(os.path.join(ROOT, "include", "txvote.h")).read()
    assert "txvotepool/reactor.go:126" in src and "txvotepool.go:180-261" in src


def test_library_exports_the_calls_and_python_mirrors_them():
    import txflow_amd as T
    lib = ctypes.CDLL(T.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in T.EXPORTED_SYMBOLS
    for m in ("check_routed_submit", "check_routed"):
        assert callable(getattr(T.TxVotePool, m)), m
    for m in ("submit_routed_checked", "sign_txs_meta"):
        assert callable(getattr(T.Context, m)), m
    assert issubclass(T.RouteGuardError, T.TxvInfraError)


def test_null_arguments_are_einval():
    """every pointer in turn; the others are non-null dummies the calls must not touch"""
    import txflow_amd as T
    L = T.lib()
    pool = T.TxVotePool(None, size=16, cache_size=16)
    meta = np.zeros(1, T.ROUTE_META_DTYPE)
    meta[0]["bytes"] = int(L.txv_route_bytes(0, 0, 0))
    mp = meta.ctypes.data
    t = ctypes.c_uint64()
    tp = ctypes.byref(t)
    st = np.zeros(4, np.uint8)
    dummy = ctypes.c_void_p(0x1000)          # aligned, never dereferenced: the context is NULL or another argument fails first
    try:
        assert L.txv_pool_check_routed_submit(None, None, dummy, mp, tp) == TXV_EINVAL
        assert L.txv_pool_check_routed_submit(pool._h, None, dummy, mp, tp) == TXV_EINVAL
        assert L.txv_pool_check_routed_submit(pool._h, None, None, mp, tp) == TXV_EINVAL
        assert L.txv_pool_check_routed_submit(pool._h, None, dummy, None, tp) == TXV_EINVAL
        assert L.txv_pool_check_routed_submit(pool._h, None, dummy, mp, None) == TXV_EINVAL
        assert L.txv_pool_check_routed(None, None, dummy, mp, st.ctypes.data) == TXV_EINVAL
        assert L.txv_pool_check_routed(pool._h, None, dummy, mp, st.ctypes.data) == TXV_EINVAL
        assert L.txv_pool_check_routed(pool._h, None, None, mp, st.ctypes.data) == TXV_EINVAL
        assert L.txv_pool_check_routed(pool._h, None, dummy, None, st.ctypes.data) == TXV_EINVAL
        assert L.txv_submit_routed_checked(None, dummy, mp, pool._h, 1, tp) == TXV_EINVAL
        assert L.txv_submit_routed_checked(None, None, mp, pool._h, 1, tp) == TXV_EINVAL
        assert L.txv_submit_routed_checked(None, dummy, None, pool._h, 1, tp) == TXV_EINVAL
        assert L.txv_submit_routed_checked(None, dummy, mp, None, 1, tp) == TXV_EINVAL
        assert L.txv_submit_routed_checked(None, dummy, mp, pool._h, 0, tp) == TXV_EINVAL
        assert L.txv_submit_routed_checked(None, dummy, mp, pool._h, 1, None) == TXV_EINVAL
        assert L.txv_sign_txs_meta(None, 1, 0, mp) == TXV_EINVAL
        assert pool.Size() == 0
    finally:
        pool.close()
