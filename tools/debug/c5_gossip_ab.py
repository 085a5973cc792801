"""A/B of the C5 path's gossip side effect -- the TxVoteMessage bytes of every admitted vote
(broadcastTxRoutine, txvotepool/reactor.go:198-265) -- over the same stream in one process:

  fired        the parent's C5 path: the Update list built in HBM and applied (txv_pool_update_fired)
  gossip       fired + the gossip sink on (txv_gossip_sink_enable): every batch's messages encoded
               in HBM before its tally, never read
  gossip_read  gossip + txv_gossip_msgs of every waited batch into pinned host memory, on a reader
               thread of its own: the drain thread hands it the ticket and releases the slot at once;
               it waits for the reader only when the read-out of the PREVIOUS ticket is still running
               (the next submit would take that ticket's ring slot)
  host_encode  fired + the status quo: an encoder thread takes each pool ticket's statuses
               (txv_pool_check_wait), gathers the admitted votes and runs txv_encode_msgs

A leg's votes/s is that of bench.py's pass; votes_per_s_with_tail also counts the time its reader /
encoder thread needed after the pass's last wait.  With --copy the tool then times, with events, a
plain device-to-device copy of as many bytes as one batch's sink holds (the yardstick of the emit
kernel; run the tool under `rocprofv3 --kernel-trace --memory-copy-trace --stats` with
--legs gossip --passes 1 --copy to get both in one process).

The workload, the Update lists and the pipelined pass are bench.py's C5 helpers, imported; three
batches in flight (TXV_C5_INFLIGHT=3), as c5_store_ab.py.  Each leg: one warm-up pass, then PASSES
timed passes (the median is reported).

Writes profiles/r09/c5_gossip_sink.json.  Usage: python tools/debug/c5_gossip_ab.py [--txs 2048]"""
import argparse
import ctypes
import json
import os
import queue
import statistics
import sys
import threading
import time

os.environ.setdefault("TXV_C5_INFLIGHT", "3")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "go-txflow_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools", "debug")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import bench  # noqa: E402
import txflow_amd as T  # noqa: E402
from txflow_amd import sharding  # noqa: E402
from txflow_amd.workload import StreamWorkload, SEEDS  # noqa: E402
from c5_update_ab import _CtxTap, _FiredPool  # noqa: E402

PASSES = 5
N_VALS, BATCH = 1000, 65536
SINK_BYTES, SINK_MSGS = 24 << 20, BATCH        # per ring slot; a C5 batch needs ~14 MB for ~62k messages


class _Worker:
    """a thread of its own taking items in order; when its last item ended"""

    def __init__(self, fn):
        self.q = queue.Queue()
        self.t_last = 0.0
        self.error = None
        self.th = threading.Thread(target=self._run, args=(fn,), daemon=True)
        self.th.start()

    def _run(self, fn):
        while True:
            item = self.q.get()
            if item is None:
                return
            try:
                fn(*item)
            except Exception as e:       # kept for the report: a raise would end the thread mid-pass
                self.error = self.error or repr(e)
            self.t_last = time.perf_counter()
            self.q.task_done()

    def close(self):
        self.q.put(None)
        self.th.join()


class _GossipTap(_CtxTap):
    """_CtxTap whose wait hands the waited ticket to the reader thread (read) or only takes the
    batch's counts (not read)"""

    def __init__(self, ctx, read):
        super().__init__(ctx)
        self.read = read
        self.msgs = self.bytes = 0
        self.read_s = 0.0
        self.error = None
        self.out = np.zeros(SINK_BYTES, np.uint8)
        ctx.host_register(self.out)
        self.off = np.zeros(SINK_MSGS, np.uint64)
        self.len = np.zeros(SINK_MSGS, np.uint32)
        self.idx = np.zeros(SINK_MSGS, np.uint32)
        self.flag = np.zeros(SINK_MSGS, np.uint8)
        self.prev = None                         # the previous ticket's read-out
        self.worker = _Worker(self._read)

    def _read(self, ticket, ended):
        n, nb = ctypes.c_uint32(), ctypes.c_uint64()
        t0 = time.perf_counter()
        rc = T.lib().txv_gossip_msgs(self._obj._h, ticket, self.out.ctypes.data, self.out.nbytes, self.off.ctypes.data,
                                     self.len.ctypes.data, self.idx.ctypes.data, self.flag.ctypes.data, SINK_MSGS,
                                     ctypes.byref(n), ctypes.byref(nb))
        self.read_s += time.perf_counter() - t0
        ended.set()
        self._count(rc, n, nb)

    def _count(self, rc, n, nb):
        if rc < 0:
            self.error = self.error or f"txv_gossip_msgs {rc}: needs {n.value} entries, {nb.value} bytes"
        self.msgs += n.value
        self.bytes += nb.value

    def wait_votes(self, ticket, ev_cap=0):
        r = super().wait_votes(ticket, ev_cap=ev_cap)
        if self.read:
            if self.prev is not None:            # its ring slot is the next submit's
                self.prev.wait()
            self.prev = threading.Event()
            self.worker.q.put((ticket, self.prev))
        else:                                    # the counts only: nothing is copied
            n, nb = ctypes.c_uint32(), ctypes.c_uint64()
            self._count(T.lib().txv_gossip_msgs(self._obj._h, ticket, None, 0, None, None, None, None, 0, ctypes.byref(n),
                                                ctypes.byref(nb)), n, nb)
        return r

    def close(self):
        self.worker.close()
        self._obj.host_unregister(self.out)


class _EncodePool(_FiredPool):
    """_FiredPool whose check_wait also hands the ticket's statuses to the encoder thread: the
    admitted votes gathered (numpy) and encoded with txv_encode_msgs"""

    def __init__(self, pool, tap, encode):
        super().__init__(pool, tap)
        self.encode = encode
        self.batch_of = {}
        self.t_first = None
        self.msgs = self.bytes = 0
        self.out = np.zeros(SINK_BYTES, np.uint8)
        self.off = np.zeros(BATCH, np.uint64)
        self.len = np.zeros(BATCH, np.uint32)
        self.worker = _Worker(self._encode) if encode else None

    def check_submit(self, b, *a, **kw):
        if self.t_first is None:
            self.t_first = time.perf_counter()
        tk = self._obj.check_submit(b, *a, **kw)
        self.batch_of[tk] = b
        return tk

    def check_wait(self, tk):
        ps = self._obj.check_wait(tk)
        b = self.batch_of.pop(tk, None)
        if self.encode and b is not None:
            self.worker.q.put((b, ps))
        return ps

    def _encode(self, b, ps):
        sub = sharding.subset(b, np.nonzero(ps == T.POOL_OK)[0])
        sub.is_nil = None
        vs = sub.c_struct()
        total = ctypes.c_uint64()
        rc = T.lib().txv_encode_msgs(ctypes.byref(vs), None if sub.txkey is None else sub.txkey.ctypes.data, None, None,
                                     self.out.ctypes.data, self.out.nbytes, self.off.ctypes.data, self.len.ctypes.data,
                                     ctypes.byref(total))
        if rc:
            raise RuntimeError(f"txv_encode_msgs {rc}")
        self.msgs += sub.n
        self.bytes += total.value

    def close(self):
        if self.worker:
            self.worker.close()


def _copy_yardstick(nbytes):
    """a plain device-to-device copy of nbytes, timed with events: median of 20 after 3 warm-ups"""
    hip = ctypes.CDLL("libamdhip64.so")          # the runtime libtxvote.so already loaded

    def chk(rc):
        if rc:
            raise RuntimeError(f"HIP error {rc}")

    vp = ctypes.c_void_p
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipFree.argtypes = [vp]
    hip.hipEventDestroy.argtypes = [vp]
    src, dst, a, b = vp(), vp(), vp(), vp()
    chk(hip.hipSetDevice(0))
    chk(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)))
    chk(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)))
    chk(hip.hipEventCreate(ctypes.byref(a)))
    chk(hip.hipEventCreate(ctypes.byref(b)))
    ms = []
    for rep in range(23):
        el = ctypes.c_float()
        chk(hip.hipEventRecord(a, None))
        chk(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))   # hipMemcpyDeviceToDevice
        chk(hip.hipEventRecord(b, None))
        chk(hip.hipEventSynchronize(b))
        chk(hip.hipEventElapsedTime(ctypes.byref(el), a, b))
        if rep >= 3:
            ms.append(el.value)
    for p in (src, dst):
        chk(hip.hipFree(p))
    for e in (a, b):
        chk(hip.hipEventDestroy(e))
    return {"bytes": int(nbytes), "copy_us_median": round(statistics.median(ms) * 1e3, 2),
            "copy_us_min": round(min(ms) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "c5_gossip_sink.json"))
    ap.add_argument("--passes", type=int, default=PASSES, help="timed passes per leg (fewer: under a kernel trace)")
    ap.add_argument("--legs", default="fired,gossip,gossip_read,host_encode", help="a subset skips the report (kernel traces)")
    ap.add_argument("--copy", action="store_true", help="time a device-to-device copy of one batch's sink bytes")
    args = ap.parse_args()
    ctx = T.Context(device=0, max_batch=BATCH, max_txs=args.txs + 64, max_validators=N_VALS)
    ctx.bind_host_numa()
    wl = StreamWorkload(ctx, N_VALS, args.txs, SEEDS["c5"], BATCH, replay=bench.C5_REPLAY)
    upd, n_upd = bench.c5_prepare_updates(ctx, wl)
    max_list = max(u.n for u in upd if u is not None)
    bench.log(f"[gossip] stream ready: {wl.n} votes in {len(wl.batches)} batches, {n_upd} Update entries per pass, "
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
        sink = leg in ("gossip", "gossip_read")
        ctx.enable_gossip_sink(SINK_BYTES if sink else 0, SINK_MSGS if sink else 0)
        pool = T.TxVotePool(ctx, size=bench.C5_POOL_SIZE, cache_size=bench.C5_CACHE, max_txs_bytes=1 << 40, device_cache=True)
        tap = _GossipTap(ctx, leg == "gossip_read") if sink else _CtxTap(ctx)
        ppool = _EncodePool(pool, tap, leg == "host_encode")
        side = tap if sink else ppool
        runs, per_pass = [], []
        for rep in range(-1, args.passes):
            side.msgs = side.bytes = 0
            ppool.t_first = None
            out, _, _, _ = bench.c5_pass(tap, wl, ppool, upd, True, BATCH, N_VALS,
                                         label=f"{leg} " + (("pass %d" % rep) if rep >= 0 else "warm-up"))
            worker = getattr(side, "worker", None)
            tail = 0.0
            if worker is not None:                     # the reader / encoder thread's last item
                worker.q.join()
                tail = max(0.0, (worker.t_last - ppool.t_first) - wl.n / out["votes_per_s"])
            if rep >= 0:
                runs.append(out)
                per_pass.append((side.msgs, side.bytes, wl.n / (wl.n / out["votes_per_s"] + tail)))
            ctx.reset_flow()
            pool.flush()
        err = ppool.error or getattr(tap, "error", None) or getattr(getattr(side, "worker", None), "error", None)
        if err:
            raise SystemExit(f"{leg}: failed inside a pass: {err}")
        ppool.close()
        pool.close()
        if sink:
            tap.close()
        rates = [r["votes_per_s"] for r in runs]
        legs[leg] = {"votes_per_s": statistics.median(rates), "votes_per_s_passes": rates,
                     "votes_per_s_with_tail": round(statistics.median(p[2] for p in per_pass), 1),
                     "votes_per_s_with_tail_passes": [round(p[2], 1) for p in per_pass],
                     "passes_correct": all(r["correct"] for r in runs)}
        if leg != "fired":
            legs[leg].update(msgs_per_pass=[p[0] for p in per_pass], bytes_per_pass=[p[1] for p in per_pass],
                             bytes_per_batch=round(per_pass[0][1] / len(wl.batches)))
        if leg == "gossip_read":
            # (the calls of the warm-up pass included: the mean over passes + 1 passes)
            legs[leg]["read_s_per_pass_mean_incl_warmup"] = round(tap.read_s / (args.passes + 1), 4)
        bench.log(f"[gossip] {leg}: {legs[leg]['votes_per_s'] / 1e6:.1f}M votes/s {rates}; with the side thread's tail "
                  f"{legs[leg]['votes_per_s_with_tail'] / 1e6:.1f}M")
    ctx.enable_gossip_sink(0, 0)
    ctx.enable_update_sink(0)
    copy = None
    if args.copy:
        per_batch = max((v.get("bytes_per_batch", 0) for v in legs.values()), default=0)
        copy = _copy_yardstick(per_batch or 14 << 20)
        bench.log(f"[gossip] device-to-device copy of {copy['bytes']} bytes: {copy['copy_us_median']} us")
    if len(legs) < 4:
        print(json.dumps({"legs": legs, "copy": copy}), flush=True)
        return 0
    base = legs["fired"]
    res = {"workload": f"C5: {N_VALS} validators, {wl.n} votes ({wl.n - wl.n_unique} exact replays) in {BATCH}-vote "
                       f"batches, CacheSize {bench.C5_CACHE}, TXV_POOL_DEVICE_CACHE, txv_submit_checked, "
                       f"txv_pool_update_fired, {bench.C5_INFLIGHT} batches in flight; median of {args.passes} passes "
                       f"per leg, one process; gossip sink {SINK_BYTES} bytes / {SINK_MSGS} entries per slot",
           "device": ctx.device_name(), "votes_per_pass": int(wl.n), "batches_per_pass": len(wl.batches), "legs": legs,
           "gossip_vs_fired": round(legs["gossip"]["votes_per_s"] / base["votes_per_s"], 4),
           "gossip_below_fired_slowest_pass": legs["gossip"]["votes_per_s"] < min(base["votes_per_s_passes"]),
           "gossip_read_vs_fired": round(legs["gossip_read"]["votes_per_s_with_tail"] / base["votes_per_s"], 4),
           "host_encode_vs_fired": round(legs["host_encode"]["votes_per_s_with_tail"] / base["votes_per_s"], 4),
           "gossip_read_faster_than_host_encode":
               legs["gossip_read"]["votes_per_s_with_tail"] > legs["host_encode"]["votes_per_s_with_tail"],
           "copy_yardstick": copy}
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return 0 if all(v["passes_correct"] for v in legs.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
