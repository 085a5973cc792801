"""The Commit loader's surface without a GPU: libtxvote.so exports the txv_load_commits_* entry
points, include/txvote.h declares them (citing the Go lines) with the TXV_COMMIT_* statuses, a NULL
context is TXV_EINVAL, txv_load_commits_bytes is the route size it says it is, and the Python
mirror is there."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXV_EINVAL = -22
INT_NAMES = ("txv_load_commits_submit", "txv_load_commits_wait", "txv_load_commits", "txv_load_commits_ms")
NAMES = INT_NAMES + ("txv_load_commits_bytes",)


def test_header_declares_the_loader():
    raw = open(os.path.join(ROOT, "include", "txvote.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in INT_NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*txv_ctx\s*\*" % name, src), name
    assert re.search(r"\buint64_t\s+txv_load_commits_bytes\s*\(\s*uint32_t", src)
    for name, val in (("TXV_COMMIT_OK", 0), ("TXV_COMMIT_CORRUPT", 1), ("TXV_COMMIT_EMPTY", 2), ("TXV_LOAD_RING", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    assert "#define TXV_ABI_VERSION 2" in src or re.search(r"TXV_ABI_VERSION\s*=?\s*2\b", src)
    assert "tx/store.go:67-80" in raw and "txflow/service.go:115-120" in raw


def test_library_exports_the_loader():
    import txflow_amd as T
    lib = ctypes.CDLL(T.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in T.EXPORTED_SYMBOLS


def test_null_context_is_einval():
    import txflow_amd as T
    L = T.lib()
    t, ms = ctypes.c_uint64(7), ctypes.c_float()
    rec = np.frombuffer(b"\x0a\x01x", np.uint8)
    off, ln = np.zeros(1, np.uint64), np.array([3], np.uint32)
    meta = np.zeros(1, T.ROUTE_META_DTYPE)
    assert L.txv_load_commits_submit(None, rec.ctypes.data, 3, off.ctypes.data, ln.ctypes.data, 1, ctypes.c_void_p(4096),
                                     4096, ctypes.byref(t)) == TXV_EINVAL
    assert L.txv_load_commits_wait(None, 1, meta.ctypes.data, None, None, None, None) == TXV_EINVAL
    assert L.txv_load_commits(None, rec.ctypes.data, 3, off.ctypes.data, ln.ctypes.data, 1, ctypes.c_void_p(4096), 4096,
                              meta.ctypes.data, None, None, None, None) == TXV_EINVAL
    assert L.txv_load_commits_ms(None, ctypes.byref(ms)) == TXV_EINVAL
    assert t.value == 7


def test_bytes_is_the_route_size():
    import txflow_amd as T
    for n, b in ((0, 0), (1, 64), (7, 448), (1000, 123457)):
        want = T.lib().txv_route_bytes(n, b, T.ROUTE_TXKEY | T.ROUTE_NIL)
        assert T.load_commits_bytes(n, b) == want and want % 16 == 0


def test_python_mirror_exists():
    import txflow_amd as T
    for m in ("load_commits", "load_commits_submit", "load_commits_wait", "load_commits_ms"):
        assert callable(getattr(T.Context, m)), m
    assert issubclass(T.LoadCommitsError, T.TxvInfraError)
    meta = np.zeros(1, T.ROUTE_META_DTYPE)[0]
    meta["n"], meta["arena_bytes"], meta["bytes"], meta["reserved"] = 3, 192, 4096, 1
    e = T.LoadCommitsError("txv_load_commits_wait", T.E_CAPACITY, "does not fit", meta)
    assert (e.rc, e.n, e.arena_bytes, e.nbytes) == (T.E_CAPACITY, 3, 192, 4096)
    assert (T.COMMIT_OK, T.COMMIT_CORRUPT, T.COMMIT_EMPTY, T.LOAD_RING) == (0, 1, 2, 2)


def test_commit_records_addresses_a_store_read_out():
    """record k's Commit part of a txv_store_records read-out: off[k] + lens[k, 0] + lens[k, 1] + lens[k, 2]"""
    import txflow_amd as T
    parts = [(b"H:AA", b"set-a", b"C:AA", b"commit-a"), (b"H:BBBB", b"set-bb", b"C:BBBB", b"")]
    buf, off, lens = bytearray(), [], []
    for p in parts:
        buf += b"\xEE" * ((-len(buf)) % 16)
        off.append(len(buf))
        lens.append([len(x) for x in p])
        buf += b"".join(p)
    cr = T.CommitRecords.from_store_raw(np.frombuffer(bytes(buf), np.uint8), np.array(off, np.uint64),
                                        np.array(lens, np.uint32))
    assert [cr.record(k) for k in range(cr.n)] == [b"commit-a", b""]
    cr = T.CommitRecords([(0, *parts[0]), (1, *parts[1])])        # Context.store_records' tuples
    assert [cr.record(k) for k in range(cr.n)] == [b"commit-a", b""]
    cr = T.CommitRecords([b"abc", b"", b"de"])
    assert cr.off.tolist() == [0, 3, 3] and cr.length.tolist() == [3, 0, 2] and cr.nbytes == 5
