"""A small sequential model of the reference TxVotePool WITH MempoolTxVote.Senders, for the
TXV_POOL_SENDERS tests (the oracle pool keeps no Senders, so the expected sets come from here; the
model's statuses are asserted equal to the oracle's wherever it is used, so it cannot drift).

txvotepool/txvotepool.go: CheckTxWithInfo :187-261, addTx :265-270, removeTx :275-284,
Update :329-359, Flush :146-159, mapTxCache.Push :416-438, MempoolTxVote :364-371."""
from collections import OrderedDict

import numpy as np

OK, FULL, TOO_LARGE, IN_CACHE, ENCODING = 0, 1, 2, 3, 4
NO_CACHE = 0xFFFFFFFF
PEERS = np.array([0, 1, 2, 3, 7, 65535], np.uint16)   # UnknownPeerID, five peers (the last id a u16 can hold)


class _Entry:
    __slots__ = ("key", "size", "senders", "alive")

    def __init__(self, key, size, sender):
        self.key, self.size, self.senders, self.alive = key, size, {sender}, True


class Model:
    def __init__(self, size=5000, cache_size=10000, max_txs_bytes=1 << 30, max_msg_bytes=1 << 20, wal=False):
        self.size, self.cache_size, self.max_txs_bytes = size, cache_size, max_txs_bytes
        self.max_tx, self.wal = max_msg_bytes - 8, wal
        self.cache = OrderedDict()      # mapTxCache: front = oldest
        self.txs = []                   # the clist, in order (dead elements dropped lazily)
        self.txs_map = {}               # txsMap: key -> element
        self.n_live = 0
        self.txs_bytes = 0

    def _push(self, key):               # mapTxCache.Push (nopTxCache: always true)
        if self.cache_size == NO_CACHE:
            return True
        if key in self.cache:
            self.cache.move_to_end(key)
            return False
        if len(self.cache) >= self.cache_size:
            self.cache.popitem(last=False)
        self.cache[key] = True
        return True

    def check_one(self, key, size, sender):
        if self.n_live >= self.size or size + self.txs_bytes > self.max_txs_bytes:
            return FULL
        if size > self.max_tx:
            return TOO_LARGE
        if not self._push(key):
            e = self.txs_map.get(key)                    # :213-227
            if e is not None:
                e.senders.add(sender)                    # LoadOrStore
            return IN_CACHE
        if self.wal and size == 0:
            return ENCODING                              # the WAL write panics before addTx
        e = _Entry(key, size, sender)                    # :250
        self.txs.append(e)
        self.txs_map[key] = e                            # Store overwrites
        self.n_live += 1
        self.txs_bytes += size
        return OK

    def check(self, keys, sizes, senders=None):
        out = np.zeros(len(sizes), np.uint8)
        for i in range(len(sizes)):
            out[i] = self.check_one(keys[i].tobytes(), int(sizes[i]), int(senders[i]) if senders is not None else 0)
        return out

    def update(self, keys, sizes):
        for i in range(len(sizes)):
            k = keys[i].tobytes()
            self._push(k)
            e = self.txs_map.pop(k, None)
            if e is not None:                            # removeTx(tx, e, false): the committed vote's Size()
                e.alive = False
                self.n_live -= 1
                self.txs_bytes -= int(sizes[i])
        if len(self.txs) > 2 * self.n_live + 64:
            self.txs = [e for e in self.txs if e.alive]

    def flush(self):
        self.cache.clear()
        self.txs, self.txs_map, self.n_live, self.txs_bytes = [], {}, 0, 0

    def sent_by(self, keys, peers=PEERS):
        out = np.zeros((len(keys), len(peers)), bool)
        for i in range(len(keys)):
            e = self.txs_map.get(keys[i].tobytes())
            if e is not None:
                out[i] = [int(p) in e.senders for p in peers]
        return out

    def reap_keys(self):
        return [e.key for e in self.txs if e.alive]


def stream(rng, batch_sizes, replay=0.30, zero_frac=0.0, big_frac=0.0, max_msg=1 << 20):
    """batches of (keys [n, 32] u8, sizes [n] u32, senders [n] u16): fresh keys and replays of any
    earlier key of the stream (half of them from the last 8 votes, so tiny caches still hit)"""
    hist, hsz, out = [], [], []
    for n in batch_sizes:
        keys = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sizes = rng.integers(100, 200, size=n).astype(np.uint32)
        senders = PEERS[rng.integers(0, len(PEERS), size=n)]
        for i in range(n):
            total = len(hist) + i
            if total and rng.random() < replay:
                j = int(rng.integers(0, total)) if rng.random() < 0.5 else max(0, total - 1 - int(rng.integers(0, 8)))
                keys[i] = hist[j] if j < len(hist) else keys[j - len(hist)]
                sizes[i] = hsz[j] if j < len(hist) else sizes[j - len(hist)]
                continue
            if rng.random() < big_frac:
                sizes[i] = max_msg
            elif rng.random() < zero_frac:
                sizes[i] = 0
        hist.extend(list(keys))
        hsz.extend(int(x) for x in sizes)
        out.append((keys, sizes, senders))
    return out
