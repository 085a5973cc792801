"""The batch signer's surface without a GPU: include/txvote.h declares txv_txs, TXV_SIGN_RING and the
sign calls, libtxvote.so exports them, txv_sign_txs_bytes is the route buffer's size, the C struct's
layout (compiled from the header) is the ctypes mirror's, and a NULL context is TXV_EINVAL."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXV_EINVAL = -22
NAMES = ("txv_sign_txs_bytes", "txv_sign_txs_submit", "txv_sign_txs_wait", "txv_sign_txs", "txv_sign_txs_ms",
         "txv_scalarmult_base")
FIELDS = ("n", "tx", "tx_off", "tx_len", "ts_sec", "ts_nanos")


def test_header_declares_the_signer():
    src = open(os.path.join(ROOT, "include", "txvote.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+%s\s*\(\s*txv_ctx\s*\*" % name, src), name
    assert re.search(r"\buint64_t\s+txv_sign_txs_bytes\s*\(\s*uint32_t", src)
    assert re.search(r"#define\s+TXV_SIGN_RING\s+2\b", src)
    assert "#define TXV_ABI_VERSION 2" in src


def test_library_exports_the_signer():
    import txflow_amd as T
    lib = ctypes.CDLL(T.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in T.EXPORTED_SYMBOLS
    assert T.SIGN_RING == 2
    for m in ("sign_txs_submit", "sign_txs_wait", "sign_txs", "sign_txs_ms", "scalarmult_base"):
        assert callable(getattr(T.Context, m)), m


def test_sign_txs_bytes_is_the_route_buffer_size():
    import txflow_amd as T
    for n in (0, 1, 64, 65537):
        assert int(T.lib().txv_sign_txs_bytes(n)) == int(T.lib().txv_route_bytes(n, 64 * n, T.ROUTE_TXKEY)) == T.sign_txs_bytes(n)
    assert T.sign_txs_bytes(0) == 80


def test_txv_txs_layout_is_the_ctypes_mirror(tmp_path):
    import txflow_amd as T
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "txvote.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(txv_txs));\n' +
                   "".join('  printf(" %%zu", offsetof(txv_txs, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or "/opt/rocm/llvm/bin/clang"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(T._Txs)] + [getattr(T._Txs, f).offset for f in FIELDS]
    assert [n for n, _ in T._Txs._fields_] == list(FIELDS)
    assert got == want == [48, 0, 8, 16, 24, 32, 40]


def test_tx_batch_packs_an_arena():
    import numpy as np
    import txflow_amd as T
    b = T.TxBatch([b"", b"abc", b"x" * 70], ts_sec=[0, 5, -3], ts_nanos=[0, 7, 9])
    assert b.n == 3 and list(b.off) == [0, 0, 3] and list(b.length) == [0, 3, 70]
    assert b.tx(0) == b"" and b.tx(1) == b"abc" and b.tx(2) == b"x" * 70
    assert b.ts_sec.dtype == np.int64 and b.ts_nanos.dtype == np.int32
    s = b.c_struct()
    assert s.n == 3 and s.tx == b.arena.ctypes.data and s.tx_off == b.off.ctypes.data
    assert T.TxBatch([]).n == 0


def test_null_context_is_einval():
    import txflow_amd as T
    t = ctypes.c_uint64()
    assert T.lib().txv_sign_txs_submit(None, None, 0, 0, None, 0, ctypes.byref(t)) == TXV_EINVAL
    assert T.lib().txv_sign_txs_wait(None, 1, None) == TXV_EINVAL
    assert T.lib().txv_sign_txs(None, None, 0, 0, None, 0, None) == TXV_EINVAL
    assert T.lib().txv_scalarmult_base(None, None, 0, None) == TXV_EINVAL
    assert T.lib().txv_sign_txs_ms(None, None) == TXV_EINVAL
