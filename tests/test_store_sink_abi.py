"""The store sink's surface without a GPU: libtxvote.so exports txv_store_sink_enable and
txv_store_records, include/txvote.h declares them, a NULL context is TXV_EINVAL, and the Python
mirror is there."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXV_EINVAL = -22
NAMES = ("txv_store_sink_enable", "txv_store_records")


def test_header_declares_the_store_sink():
    src = open(os.path.join(ROOT, "include", "txvote.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*txv_ctx\s*\*" % name, src), name
    assert "#define TXV_ABI_VERSION 2" in src or re.search(r"TXV_ABI_VERSION\s*=?\s*2\b", src)


def test_library_exports_the_store_sink():
    import txflow_amd as T
    lib = ctypes.CDLL(T.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in T.EXPORTED_SYMBOLS


def test_null_context_is_einval():
    import txflow_amd as T
    n, nb = ctypes.c_uint32(7), ctypes.c_uint64(7)
    assert T.lib().txv_store_sink_enable(None, 1 << 20, 16) == TXV_EINVAL
    assert T.lib().txv_store_records(None, 1, None, 0, None, None, None, 0, ctypes.byref(n), ctypes.byref(nb)) == TXV_EINVAL
    assert T.lib().txv_store_records(None, 1, None, 0, None, None, None, 0, None, None) == TXV_EINVAL


def test_python_mirror_exists():
    import txflow_amd as T
    assert callable(T.Context.enable_store_sink) and callable(T.Context.store_records)
    assert issubclass(T.StoreRecordsError, T.TxvInfraError)
    e = T.StoreRecordsError("txv_store_records", T.E_CAPACITY, 3, 4096, "overflow")
    assert (e.rc, e.n, e.nbytes) == (T.E_CAPACITY, 3, 4096)
