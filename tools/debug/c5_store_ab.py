"""A/B of the C5 commit path's TxStore.SaveTx records, over the same stream in one process:

  fired        the Update list built in HBM and applied (txv_pool_update_fired), no store records
  store        fired + the store sink on (txv_store_sink_enable): every batch's SaveTx records
               encoded in HBM behind its tally, never read
  store_read   store + txv_store_records of every waited batch into pinned host memory, on the
               drain thread right after its txv_wait_votes

and, outside the pipeline, for the one batch that fires the most votes: the wall time of the
per-transaction txv_save_tx_bytes loop over that batch's fired sets against one txv_store_records,
and whether the two give the same records.

The workload, the Update lists and the pipelined pass are bench.py's C5 helpers, imported
(c5_prepare_updates, c5_pass); three batches in flight (TXV_C5_INFLIGHT=3), as c5_update_ab.py: the
fourth ring slot keeps the waited batch's list and records.  Each leg: one warm-up pass, then PASSES
timed passes (the median is reported).

Writes profiles/r08/c5_store_sink.json.  Usage: python tools/debug/c5_store_ab.py [--txs 2048]
(--legs store --passes 1 under `rocprofv3 --kernel-trace --stats` gives the store chain's kernel times)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ.setdefault("TXV_C5_INFLIGHT", "3")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "go-txflow_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools", "debug")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import txflow_amd as T  # noqa: E402
from txflow_amd.workload import StreamWorkload, SEEDS  # noqa: E402
from c5_update_ab import _CtxTap, _FiredPool  # noqa: E402

PASSES = 5
N_VALS, BATCH = 1000, 65536
SINK_BYTES, SINK_RECORDS = 48 << 20, 4096      # per ring slot; a C5 batch needs ~20 MB in ~100 records


class _StoreTap(_CtxTap):
    """_CtxTap whose wait also reads the waited batch's store records into pinned memory"""

    def __init__(self, ctx, read):
        super().__init__(ctx)
        self.read = read
        self.records = self.bytes = 0
        self.read_s = 0.0
        self.error = None
        self.out = np.zeros(SINK_BYTES, np.uint8)
        ctx.host_register(self.out)
        self.off = np.zeros(SINK_RECORDS, np.uint64)
        self.lens = np.zeros((SINK_RECORDS, 4), np.uint32)
        self.sets = np.zeros(SINK_RECORDS, np.uint32)

    def wait_votes(self, ticket, ev_cap=0):
        r = super().wait_votes(ticket, ev_cap=ev_cap)
        n, nb = ctypes.c_uint32(), ctypes.c_uint64()
        t0 = time.perf_counter()
        if self.read:
            rc = T.lib().txv_store_records(self._obj._h, ticket, self.out.ctypes.data, self.out.nbytes, self.off.ctypes.data,
                                           self.lens.ctypes.data, self.sets.ctypes.data, SINK_RECORDS,
                                           ctypes.byref(n), ctypes.byref(nb))
        else:                                    # the counts only: nothing is copied
            rc = T.lib().txv_store_records(self._obj._h, ticket, None, 0, None, None, None, 0, ctypes.byref(n), ctypes.byref(nb))
        self.read_s += time.perf_counter() - t0
        if rc < 0:                               # kept for the report: a raise would end the drain thread mid-pass
            self.error = self.error or f"txv_store_records {rc}: needs {n.value} records, {nb.value} bytes"
        self.records += n.value
        self.bytes += nb.value
        return r

    def close(self):
        self._obj.host_unregister(self.out)


def _single_batch(ctx, wl, upd):
    """(d): the batch with the longest Update list, reached one batch at a time"""
    k_star = max((k for k in range(len(upd)) if upd[k] is not None), key=lambda k: upd[k].n)
    pool = T.TxVotePool(ctx, size=bench.C5_POOL_SIZE, cache_size=bench.C5_CACHE, max_txs_bytes=1 << 40, device_cache=True)
    out = np.zeros(SINK_BYTES, np.uint8)
    ctx.host_register(out)
    try:
        for k in range(k_star + 1):
            b = wl.batches[k]
            b.is_nil = None
            ptk = pool.check_submit(b)
            tk = ctx.submit_checked(b, pool, ptk)
            pool.check_wait(ptk)
            ctx.wait_votes(tk, ev_cap=b.n)
            pool.update_fired(ctx, 1, tk)
        t0 = time.perf_counter()
        buf, off, lens, sets = ctx.store_records_raw(tk, out)
        t1 = time.perf_counter()
        recs = []
        for o, ln in zip(off.tolist(), lens.tolist()):
            parts = []
            for L in ln:
                parts.append(buf[o:o + L].tobytes())
                o += L
            recs.append(tuple(parts))
        hashes = [bytes.fromhex(r[0][2:].decode()) for r in recs]      # "H:%X" spells the TxHash
        t2 = time.perf_counter()
        host = [ctx.save_tx_bytes(h) for h in hashes]
        t3 = time.perf_counter()
        pool.sync()
    finally:
        ctx.host_unregister(out)
        pool.close()
        ctx.reset_flow()
    return {"batch": k_star, "records": len(recs), "bytes": int(len(buf)),
            "store_records_ms": round((t1 - t0) * 1e3, 3), "save_tx_bytes_loop_ms": round((t3 - t2) * 1e3, 3),
            "records_equal_host_path": bool(recs) and recs == host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "c5_store_sink.json"))
    ap.add_argument("--passes", type=int, default=PASSES, help="timed passes per leg (fewer: under a kernel trace)")
    ap.add_argument("--legs", default="fired,store,store_read", help="a subset skips the report (kernel traces)")
    args = ap.parse_args()
    ctx = T.Context(device=0, max_batch=BATCH, max_txs=args.txs + 64, max_validators=N_VALS)
    ctx.bind_host_numa()
    wl = StreamWorkload(ctx, N_VALS, args.txs, SEEDS["c5"], BATCH, replay=bench.C5_REPLAY)
    upd, n_upd = bench.c5_prepare_updates(ctx, wl)
    max_list = max(u.n for u in upd if u is not None)
    bench.log(f"[store] stream ready: {wl.n} votes in {len(wl.batches)} batches, {n_upd} Update entries per pass, "
              f"{bench.C5_INFLIGHT} batches in flight")
    seen = set()
    for b in wl.batches:                               # pinned once, as bench.c5_streaming does
        for col in (b.height, b.ts_sec, b.ts_nanos, b.txhash_off, b.txhash_len, b.addr, b.addr_len, b.sig, b.sig_len,
                    b.txhash_arena, b.txkey):
            if col is not None and col.nbytes and col.ctypes.data not in seen:
                seen.add(col.ctypes.data)
                ctx.host_register(col)
    ctx.enable_update_sink(max_list + max_list // 4)
    legs = {}
    for leg in args.legs.split(","):
        if leg == "fired":
            ctx.enable_store_sink(0, 0)
        else:
            ctx.enable_store_sink(SINK_BYTES, SINK_RECORDS)
        pool = T.TxVotePool(ctx, size=bench.C5_POOL_SIZE, cache_size=bench.C5_CACHE, max_txs_bytes=1 << 40, device_cache=True)
        tap = _StoreTap(ctx, leg == "store_read") if leg != "fired" else _CtxTap(ctx)
        ppool = _FiredPool(pool, tap)
        runs, per_pass = [], []
        for rep in range(-1, args.passes):
            if leg != "fired":
                tap.records = tap.bytes = 0
                tap.read_s = 0.0
            out, _, _, _ = bench.c5_pass(tap, wl, ppool, upd, True, BATCH, N_VALS,
                                         label=f"{leg} " + (("pass %d" % rep) if rep >= 0 else "warm-up"))
            if rep >= 0:
                runs.append(out)
                if leg != "fired":
                    per_pass.append((tap.records, tap.bytes, tap.read_s))
            ctx.reset_flow()
            pool.flush()
        err = ppool.error or getattr(tap, "error", None)
        if err:
            raise SystemExit(f"{leg}: failed inside a pass: {err}")
        pool.close()
        if leg != "fired":
            tap.close()
        rates = [r["votes_per_s"] for r in runs]
        legs[leg] = {"votes_per_s": statistics.median(rates), "votes_per_s_passes": rates,
                     "passes_correct": all(r["correct"] for r in runs)}
        if leg != "fired":
            legs[leg].update(records_per_pass=[p[0] for p in per_pass], bytes_per_pass=[p[1] for p in per_pass])
        if leg == "store_read":
            legs[leg].update(read_s_per_pass=[round(p[2], 4) for p in per_pass],
                             copy_gb_per_s_in_call=[round(p[1] / p[2] / 1e9, 2) for p in per_pass],
                             gb_per_s_over_pass=[round(p[1] * r / wl.n / 1e9, 2) for p, r in zip(per_pass, rates)])
        bench.log(f"[store] {leg}: {legs[leg]['votes_per_s'] / 1e6:.1f}M votes/s {rates}")
    if len(legs) < 3:
        print(json.dumps(legs), flush=True)
        return 0
    single = _single_batch(ctx, wl, upd)
    ctx.enable_store_sink(0, 0)
    ctx.enable_update_sink(0)
    base = legs["fired"]
    res = {"workload": f"C5: {N_VALS} validators, {wl.n} votes ({wl.n - wl.n_unique} exact replays) in {BATCH}-vote "
                       f"batches, CacheSize {bench.C5_CACHE}, TXV_POOL_DEVICE_CACHE, txv_submit_checked, "
                       f"txv_pool_update_fired, {bench.C5_INFLIGHT} batches in flight; median of {args.passes} passes "
                       f"per leg, one process; store sink {SINK_BYTES} bytes / {SINK_RECORDS} records per slot",
           "device": ctx.device_name(), "votes_per_pass": int(wl.n), "batches_per_pass": len(wl.batches), "legs": legs,
           "store_vs_fired": round(legs["store"]["votes_per_s"] / base["votes_per_s"], 4),
           "store_read_vs_fired": round(legs["store_read"]["votes_per_s"] / base["votes_per_s"], 4),
           "store_below_fired_slowest_pass": legs["store"]["votes_per_s"] < min(base["votes_per_s_passes"]),
           "single_batch": single, "records_equal_host_path": single["records_equal_host_path"]}
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return 0 if res["records_equal_host_path"] and all(v["passes_correct"] for v in legs.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
