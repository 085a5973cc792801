"""Sign by batch on the device, measured (include/txvote.h txv_sign_txs_submit;
reference: Reactor.signTxRoutine, txvotepool/reactor.go:87-138).

One signer over batches of 64k and 1M txs of 256 bytes, on a context with the library's default
windows (the bench's C2 windows: radix-2^24 base-point table).  Per batch size, after WARMUP untimed
calls, REPEATS calls of each form in one process:

  new   txv_sign_txs: wall time from submit to wait, and the chain's device time by HIP events on
        the stream it runs on (txv_sign_txs_ms)
  old   the way to the same bytes before this entry point: SHA-256 + hex of every tx on the host
        (hashlib; timed apart), the votes' columns, then txv_sign_votes (wall time of the call: its
        host loops, its upload, txv_k_sign, its read-back)

and the two forms' signatures compared.  --trace runs one call of each form per size and nothing
else, for a `rocprofv3 --kernel-trace --stats -- python tools/bench/sign_txs.py --trace` run (the
per-kernel split).  Writes profiles/r10/sign/sign_txs.json.
Usage: python tools/bench/sign_txs.py [--sizes 65536,1048576] [--trace] [--commit ID]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "go-txflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import txflow_amd as T  # noqa: E402

WARMUP, REPEATS = 2, 7
TX_BYTES, CHAIN, HEIGHT = 256, "bench_chain", 12345


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True,
                               check=True).stdout.strip()
        return head + ("+worktree" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def make_txs(n):
    rng = np.random.default_rng(n)
    arena = rng.integers(0, 256, n * TX_BYTES, dtype=np.uint8)
    return T.TxBatch(arena=arena, off=np.arange(n, dtype=np.uint64) * TX_BYTES, length=np.full(n, TX_BYTES, np.uint32),
                     ts_sec=np.full(n, 1_700_000_000, np.int64), ts_nanos=1 + np.arange(n, dtype=np.int32))


def old_batch(txs, addr):
    """the votes' columns from the host: (VoteBatch, seconds spent hashing)"""
    n = txs.n
    t0 = time.perf_counter()
    mv = memoryview(txs.arena)
    dig = np.frombuffer(b"".join(hashlib.sha256(mv[i * TX_BYTES:(i + 1) * TX_BYTES]).digest() for i in range(n)), np.uint8)
    hexd = np.frombuffer(b"0123456789ABCDEF", np.uint8)
    arena = np.stack([hexd[dig >> 4], hexd[dig & 15]], axis=1).reshape(-1)
    t_hash = time.perf_counter() - t0
    b = T.VoteBatch(n, height=np.full(n, HEIGHT, np.int64), txhash_arena=arena,
                    txhash_off=(np.arange(n, dtype=np.uint32) * 64), txhash_len=np.full(n, 64, np.uint32),
                    ts_sec=txs.ts_sec, ts_nanos=txs.ts_nanos, addr=np.tile(np.frombuffer(addr, np.uint8), n),
                    addr_len=np.full(n, 20, np.uint32), sig=np.zeros((n, 64), np.uint8), sig_len=np.full(n, 64, np.uint32),
                    txkey=dig.reshape(n, 32))
    return b, t_hash


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--trace", action="store_true", help="one call of each form per size (for a kernel trace)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "sign", "sign_txs.json"))
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    torch.cuda.init()
    ctx = T.Context(device=0, max_batch=max(sizes), max_txs=64, max_validators=4)
    seeds = [bytes([k + 1]) * 32 for k in range(4)]
    pubs = ctx.keygen(seeds)
    ctx.set_validators(pubs, [1, 1, 1, 1], CHAIN)
    addr = ctx.validator_info()[0][0]
    results = []
    for n in sizes:
        txs = make_txs(n)
        cap = T.sign_txs_bytes(n)
        dev = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        wall, devms = [], []
        for k in range(1 if args.trace else WARMUP + REPEATS):
            t0 = time.perf_counter()
            meta = ctx.sign_txs_wait(ctx.sign_txs_submit(txs, 0, HEIGHT, dev.data_ptr(), cap))
            t1 = time.perf_counter()
            if args.trace or k >= WARMUP:
                wall.append((t1 - t0) * 1e3)
                devms.append(ctx.sign_txs_ms())
        new_sig = T.route_view(dev.cpu().numpy()[:int(meta["bytes"])]).sig.reshape(n, 64)
        b, t_hash = old_batch(txs, addr)
        signer = np.zeros(n, np.uint32)
        old_wall = []
        for k in range(1 if args.trace else 1 + 3):
            t0 = time.perf_counter()
            old_sig = ctx.sign_votes(b, signer, CHAIN)
            if args.trace or k >= 1:
                old_wall.append((time.perf_counter() - t0) * 1e3)
        r = {"n": n, "tx_bytes": TX_BYTES, "new_device_ms": stats(devms), "new_wall_ms": stats(wall),
             "new_device_ns_per_vote": round(statistics.median(devms) * 1e6 / n, 2),
             "old_host_hash_hex_ms": round(t_hash * 1e3, 2), "old_sign_votes_wall_ms": stats(old_wall),
             "signatures_equal": bool(np.array_equal(new_sig, np.asarray(old_sig).reshape(n, 64)))}
        results.append(r)
        print(json.dumps(r), flush=True)
    out = {"commit": args.commit or commit_id(), "device": ctx.device_name(), "base_window": ctx.base_w,
           "table_window": ctx.table_w, "warmup": WARMUP, "repeats": REPEATS, "trace_mode": args.trace, "results": results}
    ctx.close()
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
