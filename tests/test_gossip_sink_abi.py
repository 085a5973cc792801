"""The gossip sink's surface without a GPU: libtxvote.so exports txv_gossip_sink_enable and
txv_gossip_msgs, include/txvote.h declares them and the entry flags, a NULL context is TXV_EINVAL,
and the Python mirror is there."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXV_EINVAL = -22
NAMES = ("txv_gossip_sink_enable", "txv_gossip_msgs")


def test_header_declares_the_gossip_sink():
    src = open(os.path.join(ROOT, "include", "txvote.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*txv_ctx\s*\*" % name, src), name
    for flag, value in (("TXV_GOSSIP_OK", 0), ("TXV_GOSSIP_HOST", 1), ("TXV_GOSSIP_UNENCODABLE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, value), src), flag
    assert "#define TXV_ABI_VERSION 2" in src


def test_library_exports_the_gossip_sink():
    import txflow_amd as T
    lib = ctypes.CDLL(T.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in T.EXPORTED_SYMBOLS


def test_null_context_is_einval():
    import txflow_amd as T
    n, nb = ctypes.c_uint32(7), ctypes.c_uint64(7)
    assert T.lib().txv_gossip_sink_enable(None, 1 << 20, 16) == TXV_EINVAL
    assert T.lib().txv_gossip_msgs(None, 1, None, 0, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(nb)) == TXV_EINVAL
    assert T.lib().txv_gossip_msgs(None, 1, None, 0, None, None, None, None, 0, None, None) == TXV_EINVAL


def test_python_mirror_exists():
    import txflow_amd as T
    assert callable(T.Context.enable_gossip_sink) and callable(T.Context.gossip_msgs)
    assert issubclass(T.GossipMsgsError, T.TxvInfraError)
    e = T.GossipMsgsError("txv_gossip_msgs", T.E_CAPACITY, 3, 4096, "overflow")
    assert (e.rc, e.n, e.nbytes) == (T.E_CAPACITY, 3, 4096)
    assert (T.GOSSIP_OK, T.GOSSIP_HOST, T.GOSSIP_UNENCODABLE) == (0, 1, 2)
