"""A/B of the C5 commit path's TxVotePool.Update, three ways over the same stream in one process:

  none    no Update at all (the pool's Size cap raised so nothing fills)
  submit  the parent path: txv_pool_update_submit of the host-gathered lists (bench.c5_commit_updates),
          their signatures uploaded again
  fired   txv_pool_update_fired: the list each batch's TxFlow chain left in HBM
          (txv_update_sink_enable), staged device to device

The workload, the Update lists and the pipelined pass are bench.py's C5 helpers, imported
(c5_prepare_updates, c5_pass: CheckTx -> txv_submit_checked -> txv_wait_votes -> Update on the
node's threads).  bench.c5_pass frees a batch's ring slot before it issues the batch's Update, so
with four batches in flight the slot could take its next batch -- and lose its list -- before the
Update reads it: every leg here runs with three in flight (TXV_C5_INFLIGHT=3), the fourth ring slot
keeping the waited batch's list.

Each leg: one pipelined warm-up pass, then PASSES timed passes (the median is reported); every
pass checks the pool's statuses against the oracle pool replaying the CheckTx batches and Updates
in the order the pool took them.  Then one sequential pass per leg (CheckTx, TryAddVote, Update one
batch at a time) whose final pool -- LRU cache, pool list, Size, TxsBytes -- must equal the oracle
pool's after the same sequence.

Writes profiles/r07/c5_update_by_set.json.  Usage: python tools/debug/c5_update_ab.py [--txs 2048]
(--legs fired --passes 1 under `rocprofv3 --kernel-trace --stats` gives the list builder's kernel times)"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("TXV_C5_INFLIGHT", "3")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "go-txflow_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402
import txflow_amd as T  # noqa: E402
from txflow_amd.workload import StreamWorkload, SEEDS  # noqa: E402

PASSES = 5
N_VALS, BATCH = 1000, 65536
NO_UPDATE_POOL_SIZE = 1 << 23      # bench.py's TXV_C5_NO_UPDATE cap: above the stream


class _Fwd:
    def __init__(self, obj):
        self._obj = obj

    def __getattr__(self, name):
        return getattr(self._obj, name)


class _CtxTap(_Fwd):
    """the context, remembering the ticket the drain thread waited last"""
    last_waited = 0

    def wait_votes(self, ticket, ev_cap=0):
        r = self._obj.wait_votes(ticket, ev_cap=ev_cap)
        self.last_waited = ticket
        return r


class _FiredPool(_Fwd):
    """the pool, its update_submit(height, host list) replaced by update_fired of the batch just
    waited (c5_pass calls it on the drain thread right after that wait)"""

    def __init__(self, pool, tap):
        super().__init__(pool)
        self._tap = tap

    error = None

    def update_submit(self, height, batch, long_sigs=None):
        try:
            self._obj.update_fired(self._tap._obj, height, self._tap.last_waited)
        except Exception as e:       # kept for the report: a raise would end the drain thread mid-pass
            self.error = self.error or repr(e)


def _state(pool):
    keys, sizes = pool.reap(-1)
    return pool.cache_keys().tobytes(), keys.tobytes(), sizes.tobytes(), int(pool.Size()), int(pool.TxsBytes())


def _oracle_final(wl, upd, pool_size):
    import oracle as O
    O.build()
    op = O.Pool(size=pool_size, cache_size=bench.C5_CACHE, max_txs_bytes=1 << 40)
    for k, b in enumerate(wl.batches):
        op.check_batch(b)
        if upd[k] is not None:
            op.update_batch(1, upd[k])
    keys, sizes = op.reap(-1)
    return op.cache_keys().tobytes(), keys.tobytes(), sizes.tobytes(), int(op.size()), int(op.txs_bytes())


def _sequential_final(ctx, wl, pool, upd, leg):
    """one batch at a time; the final pool state"""
    for k, b in enumerate(wl.batches):
        b.is_nil = None
        ptk = pool.check_submit(b)
        tk = ctx.submit_checked(b, pool, ptk)
        pool.check_wait(ptk)
        ctx.wait_votes(tk, ev_cap=b.n)
        if leg == "fired":
            pool.update_fired(ctx, 1, tk)
        elif leg == "submit" and upd[k] is not None:
            pool.update_submit(1, upd[k])
    pool.sync()
    return _state(pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "c5_update_by_set.json"))
    ap.add_argument("--passes", type=int, default=PASSES, help="timed passes per leg (fewer: under a kernel trace)")
    ap.add_argument("--legs", default="none,submit,fired", help="a subset skips the comparison (kernel traces)")
    args = ap.parse_args()
    ctx = T.Context(device=0, max_batch=BATCH, max_txs=args.txs + 64, max_validators=N_VALS)
    ctx.bind_host_numa()
    wl = StreamWorkload(ctx, N_VALS, args.txs, SEEDS["c5"], BATCH, replay=bench.C5_REPLAY)
    upd, n_upd = bench.c5_prepare_updates(ctx, wl)
    none = [None] * len(upd)
    max_list = max(u.n for u in upd if u is not None)
    bench.log(f"[ab] stream ready: {wl.n} votes in {len(wl.batches)} batches, {n_upd} Update entries per pass "
              f"(largest list {max_list}), {bench.C5_INFLIGHT} batches in flight")
    seen = set()
    for b in wl.batches:                               # pinned once, as bench.c5_streaming does
        for col in (b.height, b.ts_sec, b.ts_nanos, b.txhash_off, b.txhash_len, b.addr, b.addr_len, b.sig, b.sig_len,
                    b.txhash_arena, b.txkey):
            if col is not None and col.nbytes and col.ctypes.data not in seen:
                seen.add(col.ctypes.data)
                ctx.host_register(col)
    oracle_final = {"none": _oracle_final(wl, none, NO_UPDATE_POOL_SIZE)}
    oracle_final["submit"] = oracle_final["fired"] = _oracle_final(wl, upd, bench.C5_POOL_SIZE)
    legs = {}
    for leg in args.legs.split(","):
        size = NO_UPDATE_POOL_SIZE if leg == "none" else bench.C5_POOL_SIZE
        ctx.enable_update_sink(max_list + max_list // 4 if leg == "fired" else 0)
        pool = T.TxVotePool(ctx, size=size, cache_size=bench.C5_CACHE, max_txs_bytes=1 << 40, device_cache=True)
        tap = _CtxTap(ctx)
        pctx, ppool = (tap, _FiredPool(pool, tap)) if leg == "fired" else (ctx, pool)
        lists = none if leg == "none" else upd         # fired: which batches fire, and the oracle's replay
        runs = []
        for rep in range(-1, args.passes):
            out, _, _, _ = bench.c5_pass(pctx, wl, ppool, lists, True, BATCH, N_VALS,
                                         label=f"{leg} " + (("pass %d" % rep) if rep >= 0 else "warm-up"), pool_size=size)
            if rep >= 0:
                runs.append(out)
            ctx.reset_flow()
            pool.flush()
        if leg == "fired" and ppool.error:
            raise SystemExit(f"update_fired failed inside a pass: {ppool.error}")
        final = _sequential_final(ctx, wl, pool, upd, leg)
        ctx.reset_flow()
        pool.close()
        rates = [r["votes_per_s"] for r in runs]
        legs[leg] = {
            "votes_per_s": statistics.median(rates), "votes_per_s_passes": rates,
            "p50_pool_update_ms": statistics.median(r["p50_pool_update_ms"] for r in runs) if leg != "none" else None,
            "update_entries_per_pass": 0 if leg == "none" else n_upd,
            "bytes_uploaded_for_update_per_pass": n_upd * (64 + 4 + 4) if leg == "submit" else 0,
            "passes_correct": all(r["correct"] for r in runs),
            "pool_statuses_match_oracle": all(r["pool_matches_oracle"] for r in runs),
            "final_pool_equals_oracle": final == oracle_final[leg]}
        bench.log(f"[ab] {leg}: {legs[leg]['votes_per_s'] / 1e6:.1f}M votes/s {rates}, "
                  f"final pool == oracle {legs[leg]['final_pool_equals_oracle']}")
    ctx.enable_update_sink(0)
    if len(legs) < 3:
        print(json.dumps(legs), flush=True)
        return 0
    base = legs["none"]["votes_per_s"]
    res = {"workload": f"C5: {N_VALS} validators, {wl.n} votes ({wl.n - wl.n_unique} exact replays) in {BATCH}-vote "
                       f"batches, CacheSize {bench.C5_CACHE}, TXV_POOL_DEVICE_CACHE, txv_submit_checked, "
                       f"{bench.C5_INFLIGHT} batches in flight; median of {args.passes} passes per leg, one process",
           "device": ctx.device_name(), "votes_per_pass": int(wl.n), "update_entries_per_pass": int(n_upd),
           "largest_update_list": int(max_list), "legs": legs,
           "update_cost_vs_none": {k: round(1 - legs[k]["votes_per_s"] / base, 4) for k in ("submit", "fired")},
           "fired_vs_submit": round(legs["fired"]["votes_per_s"] / legs["submit"]["votes_per_s"], 4),
           "all_pools_equal_oracle": all(v["final_pool_equals_oracle"] and v["pool_statuses_match_oracle"]
                                         for v in legs.values())}
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return 0 if res["all_pools_equal_oracle"] else 1


if __name__ == "__main__":
    sys.exit(main())
