"""A validator's own-vote path, measured (include/txvote.h txv_pool_check_routed_submit /
txv_submit_routed_checked; reference: signTxRoutine -> CheckTx -> checkMaj23Routine -> TryAddVote,
txvotepool/reactor.go:108-126).

One signer of 100 validators over batches of 64k and 1M txs of 256 bytes, in one process on one GPU.
Per batch size, after WARMUP untimed passes, REPEATS passes of each form, timed from the sign submit
to the last wait (the pool flushed and TxFlow reset between passes, untimed):

  a  the read-out path, from entry points that predate the routed calls: txv_sign_txs, the buffer
     copied to the host, txv_route_view, txv_pool_check_submit, txv_submit_checked, the waits
  b  the routed chain issued back to back: txv_sign_txs_submit, txv_sign_txs_meta,
     txv_pool_check_routed_submit, txv_submit_routed_checked, then the three waits

with each form's bytes over the link beside it, and the two forms' pool and TxFlow statuses compared.
--trace runs one pass of form b per size and txv_sig_keys over the same signatures and nothing else,
for a `rocprofv3 --kernel-trace --stats -- python tools/bench/sign_admit.py --trace` run
(txv_k_route_keys beside txv_k_sig_keys).  Writes profiles/r11/sign_admit/sign_admit.json.
Usage: python tools/bench/sign_admit.py [--sizes 65536,1048576] [--trace] [--commit ID]"""
import argparse
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

WARMUP, REPEATS = 2, 5
TX_BYTES, CHAIN, HEIGHT, N_VALS = 256, "bench_chain", 12345, 100


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


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def form_a(ctx, pool, txs, dev, cap):
    """-> (phase times ms, pool statuses, flow statuses, bytes read out, bytes staged by submit_checked)"""
    t0 = time.perf_counter()
    meta = ctx.sign_txs(txs, 0, HEIGHT, dev.data_ptr(), cap)
    t1 = time.perf_counter()
    host = dev.cpu().numpy()[:int(meta["bytes"])]
    t2 = time.perf_counter()
    batch = T.route_view(host)
    t3 = time.perf_counter()
    pt = pool.check_submit(batch)
    ft = ctx.submit_checked(batch, pool, pt)
    staged = ctx.staged_bytes()
    t4 = time.perf_counter()
    fst, _ = ctx.wait_votes(ft)
    pst = pool.check_wait(pt)
    t5 = time.perf_counter()
    ph = {"sign": t1 - t0, "read_out": t2 - t1, "route_view": t3 - t2, "submits": t4 - t3, "waits": t5 - t4, "total": t5 - t0}
    return {k: v * 1e3 for k, v in ph.items()}, pst, fst, int(meta["bytes"]), int(staged)


def form_b(ctx, pool, txs, dev, cap):
    t0 = time.perf_counter()
    sg = ctx.sign_txs_submit(txs, 0, HEIGHT, dev.data_ptr(), cap)
    meta = ctx.sign_txs_meta(txs.n, 0)
    pt = pool.check_routed_submit(dev.data_ptr(), meta)
    ft = ctx.submit_routed_checked(dev.data_ptr(), meta, pool, pt)
    staged = ctx.staged_bytes()
    t1 = time.perf_counter()
    fst, _ = ctx.wait_votes(ft)
    pst = pool.check_wait(pt)
    ctx.sign_txs_wait(sg)
    t2 = time.perf_counter()
    ph = {"submits": t1 - t0, "waits": t2 - t1, "total": t2 - t0}
    return {k: v * 1e3 for k, v in ph.items()}, pst, fst, 0, int(staged)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--trace", action="store_true", help="one pass of form b and one txv_sig_keys per size (for a kernel trace)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "sign_admit", "sign_admit.json"))
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    torch.cuda.init()
    ctx = T.Context(device=0, max_batch=max(sizes), max_txs=max(sizes) + 1024, max_validators=128)
    seeds = [bytes([k + 1]) * 32 for k in range(N_VALS)]
    pubs = ctx.keygen(seeds)
    ctx.set_validators(pubs, [1] * N_VALS, CHAIN)
    pool = T.TxVotePool(ctx, size=1 << 22, cache_size=10000, max_txs_bytes=1 << 40, device_cache=True)
    results = []
    for n in sizes:
        txs = make_txs(n)
        cap = T.sign_txs_bytes(n)
        dev = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        upload = int(txs.arena.nbytes + 16 + n * (8 + 4 + 8 + 4))          # the txs and their columns: both forms

        def fresh():
            pool.flush()
            ctx.reset_flow()
        if args.trace:
            fresh()
            form_b(ctx, pool, txs, dev, cap)
            ctx.sig_keys(T.route_view(dev.cpu().numpy()))
            continue
        runs = {"a": [], "b": []}
        last = {}
        for k in range(WARMUP + REPEATS):
            for name, form in (("a", form_a), ("b", form_b)):
                fresh()
                ph, pst, fst, read_out, staged = form(ctx, pool, txs, dev, cap)
                last[name] = (pst, fst, read_out, staged)
                if k >= WARMUP:
                    runs[name].append(ph)
        r = {"n": n, "tx_bytes": TX_BYTES, "validators": N_VALS}
        for name in ("a", "b"):
            r[name + "_ms"] = {key: stats([p[key] for p in runs[name]]) for key in runs[name][0]}
            pst, fst, read_out, staged = last[name]
            # form a uploads the signatures and their lengths and sizes for the pool engine, then the
            # columns txv_submit_checked stages (txv_staged_bytes); form b neither
            pool_up = n * (64 + 4 + 4) if name == "a" else 0
            r[name + "_link_bytes"] = {"tx_upload": upload, "read_out": read_out, "pool_upload": pool_up,
                                       "txv_staged_bytes": staged, "beyond_the_txs": read_out + pool_up + staged}
        r["statuses_equal"] = bool(np.array_equal(last["a"][0], last["b"][0]) and np.array_equal(last["a"][1], last["b"][1]))
        r["admitted"] = int((last["b"][0] == T.POOL_OK).sum())
        r["b_over_a"] = round(r["b_ms"]["total"]["median"] / r["a_ms"]["total"]["median"], 4)
        results.append(r)
        print(json.dumps(r), flush=True)
    out = {"commit": args.commit or commit_id(), "device": ctx.device_name(), "warmup": WARMUP, "repeats": REPEATS,
           "results": results}
    pool.close()
    ctx.close()
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
