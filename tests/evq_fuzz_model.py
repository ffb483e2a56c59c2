"""Plain references for the event-queue fuzz (tests/evq_fuzz_cases.py), Python and numpy only.

* `hold_model`: utils/bench-simulator.cc's Bench::Cb (:109-127) over a heapq in MapScheduler's (ts, uid) order:
  the full pop log, the counters of nsgpu_hold_stats and the order-sensitive digest
  (nsgpu_dispatch_digest_term, include/nsgpu_types.h, which oracle/nsref_engine.hpp sums).
* `hold_rounds`: the round structure both hold kernels share (csrc/nsgpu_hold.hip, steps 1-3), recomputed from the
  same order: (K, P, p, m) of every round.  Used for claims about the cases, never for expected results.
* `sched_expected`: a heapq model of the ns3::Scheduler interface with lazy deletion: what every pop and peek of an
  `ops` script returns and the size after every op.
* `SchedPlacement`: where HipBatchScheduler keeps each event for a fixed front size (front, host heap, stage,
  device array: csrc/nsgpu_sched_host.h), so that a script can aim at a placement and a test can prove it did.
"""
import bisect
import heapq

import numpy as np

M64 = (1 << 64) - 1
HOLD_BATCH = 1024          # candidates a round examines (HOLD_BATCH in csrc/nsgpu_hold.hip)
HOLD_MAX_PENDING = 11264   # the largest n the hold kernels take
TILE = 2048                # events per block-local sort tile (csrc/nsgpu_sched.hip)


# ---------------- digest ----------------
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def digest_term(rank, ts, uid):
    return mix64(((rank * 0x9e3779b97f4a7c15) & M64) ^ mix64(ts ^ ((uid << 40) & M64) ^ uid))


def _mix64_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def digest_of_log(ts, uid):
    """sum_k digest_term(k, ts_k, uid_k) mod 2^64 (uint64 arithmetic wraps, as in C)."""
    ts = np.asarray(ts, dtype=np.uint64)
    uid = np.asarray(uid, dtype=np.uint64)
    rank = np.arange(ts.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        inner = _mix64_np(ts ^ (uid << np.uint64(40)) ^ uid)
        terms = _mix64_np(rank * np.uint64(0x9e3779b97f4a7c15) ^ inner)
        return int(np.sum(terms, dtype=np.uint64))


# ---------------- bench-simulator hold model ----------------
class HoldResult:
    __slots__ = ("log_ts", "log_uid", "dispatched", "holds", "final_ts", "next_uid", "digest")


def hold_model(dist, total):
    d = [int(x) for x in dist]
    n = len(d)
    heap = [(d[i], 4 + i) for i in range(n)]       # RunBench :84-88: Schedule (NanoSeconds (d[i]))
    heapq.heapify(heap)
    uid, cur, m_n = 4 + n, 0, 0
    lts, luid = [], []
    while heap:
        ts, u = heapq.heappop(heap)
        lts.append(ts)
        luid.append(u)
        if m_n > total:                            # Cb :109-127
            continue
        if cur == n:
            cur = 0
        heapq.heappush(heap, (ts + d[cur], uid))
        uid += 1
        cur += 1
        m_n += 1
    r = HoldResult()
    r.log_ts = np.array(lts, dtype=np.uint64)
    r.log_uid = np.array(luid, dtype=np.uint32)
    r.dispatched, r.holds, r.final_ts, r.next_uid = len(lts), m_n, lts[-1], uid
    r.digest = digest_of_log(r.log_ts, r.log_uid)
    return r


def hold_rounds(dist, total):
    """[(K, P, p, m)] of every device round, and the pop log the rounds imply."""
    d = [int(x) for x in dist]
    n = len(d)
    pend = sorted((d[i], 4 + i) for i in range(n))
    K, hl = 0, total + 1
    rounds, log = [], []
    while pend:
        P = len(pend)
        B = min(P, HOLD_BATCH)
        inf = 1 << 80
        pref = inf                                  # min child time of the candidates before r
        kids = []
        p = B
        for r in range(B):
            ts = pend[r][0]
            if r > 0 and pref < ts:                 # an earlier child precedes candidate r
                p = r
                break
            k = K + r
            c = ts + d[k % n] if k < hl else inf
            kids.append(c)
            pref = min(pref, c)
        m = min(p, max(hl - K, 0))
        log.extend(pend[:p])
        del pend[:p]
        for r in range(m):
            bisect.insort(pend, (kids[r], 4 + n + K + r))
        rounds.append((K, P, p, m))
        K += p
    return rounds, log


# ---------------- Scheduler interface model ----------------
def sched_expected(ops):
    """For every op of the script: ("insert" | "remove", size), ("pop" | "drain", [events], size) or
    ("peek", event, size); an event is (ts, uid, context, handle)."""
    heap, alive, out = [], {}, []
    for op in ops:
        kind = op[0]
        if kind == "insert":
            for ev in op[1]:
                assert ev[1] not in alive
                alive[ev[1]] = ev
                heapq.heappush(heap, (ev[0], ev[1]))
            out.append((kind, len(alive)))
        elif kind == "remove":
            del alive[op[1]]                        # lazy: the heap entry is dropped when it surfaces
            out.append((kind, len(alive)))
        elif kind == "peek":
            while heap[0][1] not in alive:
                heapq.heappop(heap)
            out.append((kind, alive[heap[0][1]], len(alive)))
        else:
            k = op[1] if kind == "pop" else len(alive)
            got = []
            for _ in range(k):
                while heap[0][1] not in alive:
                    heapq.heappop(heap)
                got.append(alive.pop(heapq.heappop(heap)[1]))
            out.append((kind, got, len(alive)))
    return out


def script_calls(ops):
    """Library calls the script makes (one per insert op, one per pop, peek and remove)."""
    calls, live = 0, 0
    for op in ops:
        if op[0] == "insert":
            live += len(op[1])
            calls += 1
        elif op[0] == "pop":
            live -= op[1]
            calls += op[1]
        elif op[0] == "drain":
            calls += live
            live = 0
        else:
            calls += 1
            live -= op[0] == "remove"
    return calls


class SchedPlacement:
    """HipBatchScheduler's host paths for a fixed front size `batch` >= 1 (sched_insert1, sched_next, sched_refill)."""

    def __init__(self, batch):
        assert batch >= 1
        self.batch = batch
        self.front, self.fi = [], 0
        self.heap, self.stage = [], []
        self.dev, self.dh = [], 0
        self.bound = (0, 0)
        self.removed = set()
        self.size = 0
        self.refills = 0
        self.refill_log = []        # (stage events, live device events, front size) of every refill

    @staticmethod
    def key(ev):
        return (ev[0], ev[1])

    def active(self):
        return self.fi < len(self.front) or bool(self.heap)

    def insert(self, ev):
        if self.active() and self.key(ev) < self.bound:
            heapq.heappush(self.heap, ev)           # uids are unique: tuple order is (ts, uid) order
            where = "heap"
        else:
            self.stage.append(ev)
            where = "stage"
        self.size += 1
        return where

    def _refill(self):
        ns, live = len(self.stage), len(self.dev) - self.dh
        take = min(self.batch, ns + live)
        if ns:
            merged = sorted(self.dev[self.dh:] + self.stage)
            self.front, self.dev, self.dh, self.stage = merged[:take], merged[take:], 0, []
        else:
            self.front = self.dev[self.dh:self.dh + take]
            self.dh += take
        self.fi = 0
        if take:
            self.bound = self.key(self.front[-1])
        self.refills += 1
        self.refill_log.append((ns, live, take))

    def next(self, pop):
        while True:
            hf, hh = self.fi < len(self.front), bool(self.heap)
            if not hf and not hh:
                if not self.stage and self.dh == len(self.dev):
                    return None
                self._refill()
                continue
            from_front = hf and (not hh or self.front[self.fi] < self.heap[0])
            e = self.front[self.fi] if from_front else self.heap[0]
            dead = e[1] in self.removed
            if dead:
                self.removed.discard(e[1])
            if dead or pop:
                if from_front:
                    self.fi += 1
                else:
                    heapq.heappop(self.heap)
            if dead:
                continue
            if pop:
                self.size -= 1
            return e

    def where(self, uid):
        """The place of a pending event: "front", "heap", "stage" or "device"."""
        for name, seq in (("front", self.front[self.fi:]), ("heap", self.heap), ("stage", self.stage),
                          ("device", self.dev[self.dh:])):
            if any(e[1] == uid for e in seq):
                return name
        return None

    def remove(self, uid):
        self.removed.add(uid)
        self.size -= 1

    def replay(self, ops):
        """Runs a script; returns per op: insert -> [(place, event, bound at the insert)], remove -> place,
        everything else -> None."""
        notes = []
        for op in ops:
            kind = op[0]
            if kind == "insert":
                row = []
                for ev in op[1]:
                    bound, act = self.bound, self.active()
                    row.append((self.insert(ev), ev, bound if act else None))
                notes.append(row)
            elif kind == "remove":
                notes.append(self.where(op[1]))
                self.remove(op[1])
            elif kind == "peek":
                self.next(False)
                notes.append(None)
            else:
                k = op[1] if kind == "pop" else self.size
                for _ in range(k):
                    self.next(True)
                notes.append(None)
        return notes
