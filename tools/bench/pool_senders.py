"""What TXV_POOL_SENDERS costs the device CheckTx engine (txvotepool/txvotepool.go:187-261
with and without the Senders bookkeeping of :213-227 / :250).

Workload: C5's CheckTx stream shape -- 64k-vote batches of (txVoteKey, Size(), sender) triples, 5 %
replays of earlier votes, CacheSize 10000, eight sender ids -- through txv_pool_check_keys(_from)
with a context, i.e. uploaded and decided by the engine chain in HBM; the pool is flushed every 16
batches so the list stays about a million entries.  Three builds, alternated pass by pass in one
run, each pass a fresh process:

  parent     --parent-lib: libtxvote.so built from the parent commit (TXV_LIB_PATH)
  off        this tree, the flag off
  on         this tree, the flag on, a sender column with every batch

Per pass: votes/s over --batches batches after --warmup, and the mean wall time of one
check_keys call (upload + engine chain + statuses back).  What this does NOT measure: the engine
chain's own time (the engine records no device events) and bench.py's C5 leg itself (keys are fed,
not votes; no signature is hashed and no TxFlow runs beside it).  The `on` passes also time
txv_pool_ticket_sent_by for a 64k-vote ticket x 50 peers.  Prints one JSON line with every pass, the medians and the spread (max - min) / median of
each build.  Usage: python tools/bench/pool_senders.py --parent-lib PATH [--passes 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "go-txflow_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH, CACHE, REPLAY, N_PEERS_IDS = 65536, 10000, 0.05, 8


def stream(n_batches):
    rng = np.random.default_rng(5)
    out, prev = [], None
    for _ in range(n_batches):
        keys = rng.integers(0, 256, size=(BATCH, 32), dtype=np.uint8)
        sizes = rng.integers(150, 190, size=BATCH).astype(np.uint32)
        if prev is not None:                      # replays of the previous batch's votes
            pick = rng.random(BATCH) < REPLAY
            src = rng.integers(0, BATCH, size=int(pick.sum()))
            keys[pick], sizes[pick] = prev[0][src], prev[1][src]
        senders = rng.integers(1, N_PEERS_IDS + 1, size=BATCH).astype(np.uint16)
        out.append((keys, sizes, senders))
        prev = (keys, sizes)
    return out


def child(flag, batches, warmup):
    import txflow_amd as T
    ctx = T.Context(max_batch=1 << 17, max_txs=1024, max_validators=8)
    pool = T.TxVotePool(ctx, size=1 << 22, cache_size=CACHE, device_cache=True, **({"senders": True} if flag else {}))
    data = stream(16)
    t0, per = None, []
    for b in range(warmup + batches):
        if b == warmup:
            t0 = time.perf_counter()
        if b % 16 == 0:
            pool.flush()
        keys, sizes, snd = data[b % 16]
        t1 = time.perf_counter()
        st = pool.check_keys(keys, sizes, senders=snd) if flag else pool.check_keys(keys, sizes)
        if b >= warmup:
            per.append(time.perf_counter() - t1)
    dt = time.perf_counter() - t0
    res = {"votes_per_s": batches * BATCH / dt, "call_ms_mean": 1e3 * statistics.mean(per), "admitted_last": int((st == 0).sum())}
    if flag:
        rng = np.random.default_rng(9)
        n = BATCH
        vb = T.VoteBatch(n, height=np.ones(n, np.int64), txhash_arena=np.frombuffer(b"AB" * 32, np.uint8),
                         txhash_off=np.zeros(n, np.uint32), txhash_len=np.full(n, 64, np.uint32),
                         ts_sec=np.full(n, 1_700_000_000, np.int64), ts_nanos=np.arange(1, n + 1, dtype=np.int32),
                         addr=np.ones((n, 20), np.uint8), addr_len=np.full(n, 20, np.uint32),
                         sig=rng.integers(0, 256, size=(n, 64), dtype=np.uint8), sig_len=np.full(n, 64, np.uint32))
        pool.flush()
        t = pool.check_submit(vb, senders=rng.integers(1, 9, size=n).astype(np.uint16))
        peers = np.arange(1, 51, dtype=np.uint16)
        pool.ticket_sent_by(t, peers)             # finishes the ticket; allocations warm
        ts = []
        for _ in range(5):
            t1 = time.perf_counter()
            rows = pool.ticket_sent_by(t, peers)
            ts.append(1e3 * (time.perf_counter() - t1))
        pool.check_wait(t)
        res["ticket_sent_by_ms"] = statistics.median(ts)
        res["ticket_rows_set"] = int(rows.any(axis=1).sum())
    pool.close()
    ctx.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", choices=["parent", "off", "on"])
    a = ap.parse_args()
    if a.child:
        child(a.child == "on", a.batches, a.warmup)
        return
    builds = (["parent"] if a.parent_lib else []) + ["off", "on"]
    runs = {b: [] for b in builds}
    for _ in range(a.passes):
        for b in builds:                          # alternated: parent, off, on, parent, ...
            env = dict(os.environ)
            if b == "parent":
                env["TXV_LIB_PATH"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", b, "--batches", str(a.batches),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode or not line:
                raise SystemExit(f"pass of build {b} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            runs[b].append(json.loads(line[0][7:]))
    out = {"workload": dict(batch=BATCH, cache=CACHE, replay=REPLAY, sender_ids=N_PEERS_IDS, batches=a.batches), "runs": runs}
    for b in builds:
        v = [r["votes_per_s"] for r in runs[b]]
        out[b] = {"votes_per_s_median": statistics.median(v), "spread": (max(v) - min(v)) / statistics.median(v),
                  "call_ms_median": statistics.median(r["call_ms_mean"] for r in runs[b])}
    if runs["on"]:
        out["on"]["ticket_sent_by_ms"] = statistics.median(r["ticket_sent_by_ms"] for r in runs["on"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
