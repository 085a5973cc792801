"""The owner rank's CheckTx + ingest route, synchronous against pipelined, over the same stream in
one process (the reference hop txvotepool/reactor.go:170-190 ->
txvotepool/txvotepool.go:187-261 -> txflow/service.go:123-166).

The stream and pool are bench.py's owner_route leg's: 1000 validators, --c5-txs 2048, 64k-vote
batches, 8 ranks, C5's replay rate and cache size, the cache in HBM, the batches' columns
registered.  One untimed warm-up pass of each form (a ring entry allocates its slot at its first
ticket), then PASSES passes of each form, interleaved (sync, pipelined, sync, ...):

  sync       bench.owner_route_leg's loop: a submit thread enqueues batch k+1's CheckTx while the
             main thread runs txv_route_checked (one route on the GPU at a time) and waits the pool
             ticket
  pipelined  the submit thread: CheckTx submit -> txv_route_submit_checked, up to TXV_ROUTE_RING
             routes in flight, each into its own [ranks][stride] region; the main thread:
             txv_route_wait + txv_pool_check_wait of the oldest

Per pass: votes/s, the p50 of the submit call (sync: the whole txv_route_checked call) and of the
wait call, routed == admitted; once per form, one batch's device buffers against
txv_route_pack_host.  Writes profiles/r07/owner_route_async.json (commit, device, all passes, the
medians and the synchronous form's spread (max - min) / median, the margin the pipelined median
has to clear).  Usage: python tools/bench/owner_route_async.py [--c5-txs 2048] [--commit ID]"""
import argparse
import json
import os
import queue
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "go-txflow_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402
import txflow_amd as T  # noqa: E402
from txflow_amd.workload import StreamWorkload, SEEDS  # noqa: E402

PASSES = 5
N_VALS, BATCH, N_RANKS = 1000, 65536, 8


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True,
                               check=True).stdout.strip()
        return head + ("+worktree" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def equals_host(dev_region, stride, metas, batch, statuses):
    hb, hm = T.route_pack_host(batch, statuses, N_RANKS)
    db = dev_region.view(N_RANKS, stride).cpu().numpy()
    return bool(np.array_equal(metas, hm)) and all(
        np.array_equal(db[r, :int(hm[r]["bytes"])], hb[r, :int(hm[r]["bytes"])]) for r in range(N_RANKS))


def sync_pass(ctx, pool, wl, buf, stride):
    tickets = queue.Queue(maxsize=2)
    routed = admitted = 0
    call_ms, wait_ms = [], []

    def submit():
        for b in wl.batches:
            tickets.put((b, pool.check_submit(b)))
        tickets.put(None)

    t0 = time.perf_counter()
    th = threading.Thread(target=submit, daemon=True)
    th.start()
    while True:
        item = tickets.get()
        if item is None:
            break
        b, tk = item
        ta = time.perf_counter()
        m = ctx.route_checked(b, pool, tk, N_RANKS, buf.data_ptr(), stride)
        tb = time.perf_counter()
        ps = pool.check_wait(tk)
        call_ms.append((tb - ta) * 1e3)
        wait_ms.append((time.perf_counter() - tb) * 1e3)
        routed += int(m["n"].sum())
        admitted += int((ps == T.POOL_OK).sum())
    th.join()
    total = time.perf_counter() - t0
    return {"form": "sync", "votes_per_s": round(wl.n / total, 1), "p50_submit_ms": round(float(np.median(call_ms)), 3),
            "p50_wait_ms": round(float(np.median(wait_ms)), 3), "routed": routed, "admitted": admitted}


def pipelined_pass(ctx, pool, wl, buf, stride):
    ring = T.ROUTE_RING
    region = N_RANKS * stride
    flight = queue.Queue()
    free = threading.Semaphore(ring)        # a ring entry (and its destination region) per route in flight
    submit_ms, wait_ms = [], []
    routed = admitted = 0
    failed = []

    def submit():
        try:
            for k, b in enumerate(wl.batches):
                free.acquire()
                tk = pool.check_submit(b)
                ta = time.perf_counter()
                rt = ctx.route_submit_checked(b, pool, tk, N_RANKS, buf.data_ptr() + (k % ring) * region, stride)
                submit_ms.append((time.perf_counter() - ta) * 1e3)
                flight.put((tk, rt))
        except Exception as e:              # the main thread must not wait for a ticket that never comes
            failed.append(e)
        flight.put(None)

    t0 = time.perf_counter()
    th = threading.Thread(target=submit, daemon=True)
    th.start()
    while True:
        item = flight.get()
        if item is None:
            break
        tk, rt = item
        ta = time.perf_counter()
        m = ctx.route_wait(rt, N_RANKS)
        wait_ms.append((time.perf_counter() - ta) * 1e3)
        ps = pool.check_wait(tk)
        free.release()
        routed += int(m["n"].sum())
        admitted += int((ps == T.POOL_OK).sum())
    th.join()
    total = time.perf_counter() - t0
    if failed:
        raise failed[0]
    return {"form": "pipelined", "votes_per_s": round(wl.n / total, 1),
            "p50_submit_ms": round(float(np.median(submit_ms)), 3), "p50_wait_ms": round(float(np.median(wait_ms)), 3),
            "routed": routed, "admitted": admitted}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--c5-txs", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=PASSES)
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git HEAD of this tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "owner_route_async.json"))
    args = ap.parse_args()
    ctx = T.Context(device=0, max_batch=BATCH, max_txs=64, max_validators=N_VALS)
    ctx.bind_host_numa()
    wl = StreamWorkload(ctx, N_VALS, args.c5_txs, SEEDS["c5"], BATCH, replay=bench.C5_REPLAY)
    seen = set()
    for b in wl.batches:
        b.is_nil = None
        for col in (b.height, b.ts_sec, b.ts_nanos, b.txhash_off, b.txhash_len, b.addr, b.addr_len, b.sig,
                    b.sig_len, b.txhash_arena, b.txkey):
            if col is not None and col.nbytes and col.ctypes.data not in seen:
                seen.add(col.ctypes.data)
                ctx.host_register(col)
    stride = max(T.route_stride(b) for b in wl.batches)
    buf = torch.zeros(T.ROUTE_RING * N_RANKS * stride, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    pool = T.TxVotePool(ctx, size=bench.C5_LONG_POOL_SIZE, cache_size=bench.C5_CACHE, max_txs_bytes=1 << 40,
                        device_cache=True)
    # parity of one batch per form (untimed)
    st0 = pool.check_batch(wl.batches[0])
    m0 = ctx.route_admitted(wl.batches[0], st0, N_RANKS, buf.data_ptr(), stride)
    same_sync = equals_host(buf[:N_RANKS * stride], stride, m0, wl.batches[0], st0)
    buf.zero_()
    torch.cuda.synchronize()
    m1 = ctx.route_wait(ctx.route_submit_admitted(wl.batches[0], st0, N_RANKS, buf.data_ptr(), stride), N_RANKS)
    same_async = equals_host(buf[:N_RANKS * stride], stride, m1, wl.batches[0], st0)
    pool.flush()
    # one untimed pass of each form first: every ring entry allocates its slot at its first ticket
    warmup = []
    for fn in (sync_pass, pipelined_pass):
        warmup.append(fn(ctx, pool, wl, buf, stride))
        pool.flush()
    passes = []
    for _ in range(args.passes):
        for fn, same in ((sync_pass, same_sync), (pipelined_pass, same_async)):
            r = fn(ctx, pool, wl, buf, stride)
            r["device_route_equals_host"] = same
            passes.append(r)
            pool.flush()
            print(json.dumps(r), flush=True)
    device = ctx.device_name()
    pool.close()
    ctx.close()
    rates = {f: [p["votes_per_s"] for p in passes if p["form"] == f] for f in ("sync", "pipelined")}
    med = {f: statistics.median(v) for f, v in rates.items()}
    spread = (max(rates["sync"]) - min(rates["sync"])) / med["sync"]
    out = {"commit": args.commit or commit_id(), "device": device,
           "workload": f"owner rank: the C5 stream ({wl.n} votes, {BATCH}-vote batches, {N_VALS} validators, "
                       f"{args.c5_txs} txs) through TxVotePool.CheckTx (cache in HBM) + the route to {N_RANKS} ranks",
           "route_ring": T.ROUTE_RING, "stride": stride, "warmup_passes": warmup, "passes": passes,
           "median_votes_per_s": med, "sync_spread": round(spread, 4),
           "pipelined_over_sync": round(med["pipelined"] / med["sync"], 4),
           "pipelined_clears_sync_spread": bool(med["pipelined"] - med["sync"] > spread * med["sync"]),
           "correct": all(p["routed"] == p["admitted"] and p["device_route_equals_host"] for p in passes)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("passes", "warmup_passes")}), flush=True)


if __name__ == "__main__":
    main()
