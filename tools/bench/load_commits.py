"""LoadTxCommit by batch on the device, measured (include/txvote.h
txv_load_commits_submit; reference: TxStore.LoadTxCommit, tx/store.go:67-80).

Two shapes: C5's (1000 validators: 64 records of 667 to 1000 CommitSigs) and C2's (100 validators:
10,000 records of 67 to 100 CommitSigs).  Every CommitSig is a full vote (Height, 64-byte TxHash,
TxKey, Timestamp, 20-byte address, 64-byte signature; the bytes are random: nothing is verified
here).  Per shape, after WARMUP untimed calls, the median of REPEATS runs of

  load   txv_load_commits: the chain's device time by HIP events on the stream it runs on
         (txv_load_commits_ms), and the wall time from submit to wait (staging copy and upload
         included)
  (a)    txv_k_decode_msgs on the same votes as TxVoteMessages (txv_decode_stage + txv_decode_run):
         the existing decoder doing the same inner parse without the two-level structure
  (b)    the host path: oracle.wire_decode_many over the same messages on one thread

with votes/s and record bytes/s for each, and the loaded signature column compared with the bytes
the records were built from.  --trace runs one load per shape and nothing else, for a
`rocprofv3 --kernel-trace --stats -- python tools/bench/load_commits.py --trace` run (the per-kernel
split).  Writes profiles/r15/load_commits/load_commits.json (or --out).
Usage: python tools/bench/load_commits.py [--shapes c5,c2] [--trace] [--out FILE] [--commit ID]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "go-txflow_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import txflow_amd as T  # noqa: E402
import oracle as O  # noqa: E402

WARMUP, REPEATS = 2, 5
SHAPES = {"c5": dict(validators=1000, records=64), "c2": dict(validators=100, records=10000)}


def commit_id():
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "-uno"], capture_output=True, text=True,
                               check=True).stdout.strip()
        return head + ("+worktree" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def build(validators, records, seed):
    """-> (CommitRecords, WireBatch of the same votes as TxVoteMessages, signatures [n, 64])"""
    rng = np.random.default_rng(seed)
    marks = dict(th=b"H" * 64, key=b"K" * 32, addr=b"A" * 20, sig=b"S" * 64)
    body = O.txvote_bytes(12345, marks["th"], 1_700_000_000, 123456789, marks["addr"], marks["sig"], marks["key"])
    pos = {k: body.index(v) for k, v in marks.items()}
    cnt = rng.integers(validators * 2 // 3 + 1, validators + 1, records)      # above 2/3 of equal stakes
    n = int(cnt.sum())
    B = np.tile(np.frombuffer(body, np.uint8), (n, 1))
    hexd = np.frombuffer(b"0123456789ABCDEF", np.uint8)
    th = hexd[rng.integers(0, 16, (records, 64))]
    B[:, pos["th"]:pos["th"] + 64] = np.repeat(th, cnt, axis=0)
    for k, w in (("key", 32), ("addr", 20), ("sig", 64)):
        B[:, pos[k]:pos[k] + w] = rng.integers(0, 256, (n, w), dtype=np.uint8)
    sigs = B[:, pos["sig"]:pos["sig"] + 64].copy()
    ehdr = np.frombuffer(b"\x12" + uvarint(len(body)), np.uint8)
    E = np.concatenate([np.tile(ehdr, (n, 1)), B], axis=1)                     # the records' elements
    esz = E.shape[1]
    rhdr = np.frombuffer(b"\x0a\x40", np.uint8)
    first = np.cumsum(cnt) - cnt
    off = first * esz + np.arange(records) * 66
    length = cnt * esz + 66
    recs = np.zeros(int(off[-1] + length[-1]), np.uint8)
    flat = E.reshape(-1)
    for k in range(records):
        o = int(off[k])
        recs[o:o + 2] = rhdr
        recs[o + 2:o + 66] = th[k]
        recs[o + 66:o + int(length[k])] = flat[int(first[k]) * esz:int(first[k] + cnt[k]) * esz]
    cr = T.CommitRecords(recs=recs, off=off.astype(np.uint64), length=length.astype(np.uint32))
    mhdr = np.frombuffer(O.wire_prefix()[1] + b"\x0a" + uvarint(len(body)), np.uint8)
    W = np.concatenate([np.tile(mhdr, (n, 1)), B], axis=1)
    wb = T.WireBatch(wire=W.reshape(-1), off=(np.arange(n, dtype=np.uint64) * W.shape[1]),
                     length=np.full(n, W.shape[1], np.uint32))
    return cr, wb, sigs


def rates(ms, n, nbytes):
    return {"ms": round(ms, 4), "votes_per_s": round(n / (ms * 1e-3)), "bytes_per_s": round(nbytes / (ms * 1e-3)),
            "ns_per_vote": round(ms * 1e6 / n, 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c5,c2")
    ap.add_argument("--trace", action="store_true", help="one load per shape (for a kernel trace)")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "load_commits", "load_commits.json"))
    args = ap.parse_args()
    O.build()
    torch.cuda.init()
    results = []
    device = None
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        cr, wb, sigs = build(shape["validators"], shape["records"], seed=len(name) + shape["records"])
        n = len(sigs)
        ctx = T.Context(device=0, max_batch=n, max_txs=64, max_validators=4)
        device = ctx.device_name()
        cap = T.load_commits_bytes(n, 64 * n)
        dev = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        devms, wall = [], []
        for k in range(1 if args.trace else WARMUP + REPEATS):
            t0 = time.perf_counter()
            res = ctx.load_commits_wait(ctx.load_commits_submit(cr, dev.data_ptr(), cap))
            t1 = time.perf_counter()
            if args.trace or k >= WARMUP:
                devms.append(ctx.load_commits_ms())
                wall.append((t1 - t0) * 1e3)
        ok = int(res.meta["n"]) == n and not res.rec_status.any()
        got = T.route_view(dev.cpu().numpy()[:int(res.meta["bytes"])]).sig.reshape(-1, 64)
        r = {"shape": name, "validators": shape["validators"], "records": cr.n, "votes": n, "record_bytes": cr.nbytes,
             "load_device": rates(statistics.median(devms), n, cr.nbytes),
             "load_device_ms_runs": [round(x, 4) for x in devms],
             "load_wall_ms": round(statistics.median(wall), 3),
             "all_records_ok": bool(ok), "signatures_equal": bool(ok and np.array_equal(got, sigs))}
        if not args.trace:
            ctx.decode_stage(wb)
            dec = [ctx.decode_run(1 << 20, 1) for _ in range(WARMUP + REPEATS)][WARMUP:]
            host = [O.wire_decode_many(wb.wire, wb.off, wb.len)[0] * 1e3 for _ in range(REPEATS)]
            r["decode_msgs_device"] = rates(statistics.median(dec), n, wb.nbytes)
            r["host_one_thread"] = rates(statistics.median(host), n, wb.nbytes)
            r["load_over_decode_msgs_per_vote"] = round(statistics.median(devms) / statistics.median(dec), 2)
        results.append(r)
        print(json.dumps(r), flush=True)
        ctx.close()
        del dev
    out = {"commit": args.commit or commit_id(), "device": device, "warmup": WARMUP, "repeats": REPEATS,
           "trace_mode": args.trace, "results": results}
    if not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
