"""Seeded cases for the event queue: the hold kernels (csrc/nsgpu_hold.hip) and the batch scheduler
(csrc/nsgpu_sched.hip, nsgpu_sched_host.h) at their structural edges.  Pure Python / numpy, no GPU import.

hold_cases()  -> [(name, dist: np.uint64[n], total, log_cap)]       families wide_big, wide_mixed, packed_edges,
                                                                    zeros, ties, short_log
sched_cases() -> [(name, batch, ops)]                               families tiles, keys, front, refill
sim_scripts() -> [(name, seed, batch)]                              runs of sim_scripts.burst_script

`ops` is a flat script: ("insert", [(ts, uid, ctx, handle), ...]), ("pop", k), ("peek",), ("remove", uid),
("drain",).  uids are unique within a case; handle = uid * 8.  tests/test_evq_fuzz_cpu.py proves on the models of
tests/evq_fuzz_model.py that the cases reach what their names claim.
"""
import functools
import random

import numpy as np

from evq_fuzz_model import HOLD_MAX_PENDING, TILE, SchedPlacement

W = 1 << 31   # the first delay the packed hold kernel does not take


# ---------------- hold ----------------
def _full(n, total):
    return n + total + 1          # the dispatch count: every event pops, dispatches 0 .. total schedule a child


def _wide_big(n, total, seed):
    # utils/generate-distributions.pl: U[0, 1e7) seconds
    secs = np.random.default_rng(seed).random(n) * 1e7
    return (secs * 1000000000).astype(np.uint64)


def _wide_mixed(n, seed):
    rng = np.random.default_rng(seed)
    small = np.array([0, 1, 2, 5], dtype=np.uint64)
    pick = rng.integers(0, 5, n)
    dist = np.where(pick < 4, small[np.minimum(pick, 3)], rng.integers(0, 1000, n).astype(np.uint64))
    wide = rng.random(n) < 0.01
    wide[rng.integers(0, n, 3)] = True
    vals = np.array([W, W + 1, 1 << 40], dtype=np.uint64)
    dist = np.where(wide, vals[rng.integers(0, 3, n)], dist).astype(np.uint64)
    # each of the three wide values at least once
    at = rng.choice(n, 3, replace=False)
    dist[at] = vals
    return dist


def _packed(n, seed):
    rng = np.random.default_rng(seed)
    dist = rng.integers(0, W, n).astype(np.uint64)
    r = rng.random(n)
    dist[r < 0.02] = W - 1
    dist[r > 0.98] = 0
    return dist


def _ties(n, pool, seed):
    rng = np.random.default_rng(seed)
    return np.array(pool, dtype=np.uint64)[rng.integers(0, len(pool), n)]


@functools.lru_cache(maxsize=None)
def hold_cases():
    cases = []
    seed = 1000
    for n in (1025, 2049, 10000, HOLD_MAX_PENDING):
        for total in (n // 3, 3000, 20000):
            seed += 1
            cases.append((f"wide_big/n{n}/t{total}", _wide_big(n, total, seed), total, _full(n, total)))
    for n in (1500, HOLD_MAX_PENDING):
        seed += 1
        total = min(2 * n, 20000)
        cases.append((f"wide_mixed/n{n}/t{total}", _wide_mixed(n, seed), total, _full(n, total)))
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, HOLD_MAX_PENDING - 1, HOLD_MAX_PENDING):
        seed += 1
        dist = _packed(n, seed)
        for total in sorted({min(t, 30000) for t in (0, 1, n - 1, n, n + 1, 4 * n)}):
            cases.append((f"packed_edges/n{n}/t{total}", dist, total, _full(n, total)))
    for n in (1, 1024, 1025, 5000):
        cases.append((f"zeros/all/n{n}", np.zeros(n, dtype=np.uint64), 3 * n, _full(n, 3 * n)))
        one = np.zeros(n, dtype=np.uint64)
        one[(7 * n) // 11] = 1
        cases.append((f"zeros/one/n{n}", one, 3 * n, _full(n, 3 * n)))
    for n in (2048, HOLD_MAX_PENDING):
        for kind, pool in (("packed", (0, 3, 1000)), ("wide", (0, W, 1 << 32))):
            seed += 1
            total = min(2 * n, 20000)
            cases.append((f"ties/{kind}/n{n}", _ties(n, pool, seed), total, _full(n, total)))
    by_name = {c[0]: c for c in cases}
    for base in ("wide_big/n1025/t3000", "packed_edges/n1025/t4100", "zeros/all/n1025"):
        _, dist, total, _ = by_name[base]
        n = dist.size
        for cap in (1, n // 2, n + total):
            cases.append((f"short_log/{base}/cap{cap}", dist, total, cap))
    for _, dist, _, _ in cases:
        dist.setflags(write=False)
        assert int(dist.max()) < 1 << 62
    return cases


# ---------------- sched ----------------
def _ev(ts, uid, ctx=0):
    return (int(ts), int(uid), int(ctx), int(uid) * 8)


TILE_INSERTS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE, 5 * TILE + 1, 20000)
TILE_LIVE = (0, 1, 7, TILE, 9001)
TILE_BATCHES = (1, 256, 4096)


def _tiles_case(batch, live, size, seed):
    rng = random.Random(seed)
    uids = rng.sample(range(4, 200000), live + 1 + size)
    first = [_ev(rng.randrange(10000, 20000), uids[i], i % 5) for i in range(live + 1)]
    # the bulk insert reaches below, into and above the live keys; many ts tie
    bulk = [_ev(rng.randrange(5000, 25000), uids[live + 1 + i], i % 5) for i in range(size)]
    return [("insert", first), ("pop", 1), ("insert", bulk), ("pop", min(300, live + size)), ("drain",)]


KEY_TS = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 5, (1 << 63) - 1)


def _keys_case(batch, seed):
    rng = random.Random(seed)
    uid_pool = rng.sample(range(4, 60000), 6500) + rng.sample(range((1 << 32) - 300, (1 << 32) - 1), 250)
    rng.shuffle(uid_pool)
    take = iter(uid_pool)
    first, second = [], []

    def put(ev, where=None):
        (where if where is not None else (first if rng.random() < 0.5 else second)).append(ev)

    for ts in KEY_TS:
        for i in range(6):
            put(_ev(ts, next(take), rng.randrange(9)), (first, second)[i % 2])
    # blocks of 300 and more events at one ts: only the uid orders them
    for ts in (1, 1 << 32, (1 << 40) + 5, (1 << 63) - 1, rng.randrange(1 << 63)):
        for _ in range(rng.randrange(300, 400)):
            put(_ev(ts, next(take), rng.randrange(9)))
    for _ in range(2500):
        put(_ev(rng.randrange(1 << 63), next(take), rng.randrange(9)))
    # pairs that differ only in the high word of ts and carry their uids in the opposite order; a third of them
    # meet in one tile sort or merge pass, the others in the merge of the stage with the device array
    for i in range(300):
        lo = rng.randrange(1 << 32)
        hi_a, hi_b = sorted(rng.sample(range(1 << 31), 2))
        ua, ub = sorted((next(take), next(take)), reverse=True)
        ctx = rng.randrange(9)
        a, b = _ev((hi_a << 32) | lo, ua, ctx), _ev((hi_b << 32) | lo, ub, ctx)
        if i % 3 == 0:
            half = first if i % 2 else second
            put(a, half), put(b, half)
        elif i % 3 == 1:
            put(a, first), put(b, second)
        else:
            put(b, first), put(a, second)
    rng.shuffle(first)
    rng.shuffle(second)
    # two pops (both at ts 0) put a front on the host, whose bound lies inside the block at ts 1; the second half
    # then lands on both sides of it, and every block meets again in one run of pops
    return [("insert", first), ("peek",), ("pop", 2), ("insert", second), ("peek",), ("pop", 400), ("peek",),
            ("drain",)]


FRONT_BATCHES = (0, 1, 2, 255, 256, 257)


def _front_case(batch, seed):
    b = batch or 256      # batch 0 (the adaptive front) replays the script aimed at 256: only its pop order is claimed
    rng = random.Random(seed)
    m = SchedPlacement(b)
    ops = []

    def do(*op):
        ops.append(op)
        if op[0] == "pop":
            return [m.next(True) for _ in range(op[1])][-1]
        return m.replay([op])

    def live(seq):
        return [e for e in seq if e[1] not in m.removed]

    n0 = 3 * b + 40
    uids = list(range(1000, 1000 + 10 * n0, 10))       # gaps: a uid just below or above any of them is free
    rng.shuffle(uids)
    evs = [_ev(1000 + 5 * (i // 2), uids[i], i % 7) for i in range(n0)]   # every ts twice
    rng.shuffle(evs)
    do("insert", evs)
    fresh = iter(range(1000000, 2000000))
    last = None
    for _ in range(max(1, b // 2)):                    # leave the front half-consumed
        do("peek")
        last = do("pop", 1)
    do("peek")                                         # (refills a front that ran dry: the host holds keys again)
    assert m.active()
    bts, buid = m.bound
    if last[0] < bts:
        do("insert", [_ev(last[0], next(fresh), 1)])   # at the last popped ts, below the bound: heap
    do("insert", [_ev(bts, buid - 1, 2)])              # at front_bound.ts with a smaller uid: heap
    do("insert", [_ev(bts, buid + 1, 3)])              # ... with a larger uid: stage
    do("insert", [_ev(10 ** 9 + rng.randrange(1000), next(fresh), 4) for _ in range(5)])   # far above: stage
    for place in ("heap", "stage", "device", "front"):
        seq = {"heap": m.heap, "stage": m.stage, "device": m.dev[m.dh:], "front": m.front[m.fi:]}[place]
        cand = live(seq)
        victim = cand[len(cand) // 2]
        do("peek")
        do("remove", victim[1])
        do("peek")
    # more inserts around the moving bound while the front is consumed, then the rest one pop at a time
    step = 0
    while m.size:
        do("peek")
        do("pop", 1)
        step += 1
        if m.size:
            do("peek")
        if step % 37 == 5 and step < 6 * b and m.active():
            bts, buid = m.bound
            do("insert", [_ev(bts, next(fresh), 5), _ev(max(bts, 1) - 1, next(fresh), 6), _ev(bts + 3, next(fresh), 6)])
    return ops


def _refill_case(batch, seed):
    rng = random.Random(seed)
    ops = []
    uid = 4
    base = 0
    for size in (700, 2500, TILE, TILE + 1, 100, 5000, 1, 2 * TILE + 1):   # below and above one tile, alternating
        evs = []
        for _ in range(size):
            evs.append(_ev(base + rng.randrange(3000), uid, uid % 4))
            uid += 1
        rng.shuffle(evs)
        ops += [("insert", evs), ("peek",), ("drain",)]
        base += 2500
    return ops


@functools.lru_cache(maxsize=None)
def sched_cases():
    cases = []
    seed = 5000
    for batch in TILE_BATCHES:
        for live in TILE_LIVE:
            for size in TILE_INSERTS:
                seed += 1
                cases.append((f"tiles/b{batch}/live{live}/ins{size}", batch, _tiles_case(batch, live, size, seed)))
    for batch in (64, 4096):
        for s in (1, 2):
            cases.append((f"keys/b{batch}/s{s}", batch, _keys_case(batch, 6000 + s)))
    for batch in FRONT_BATCHES:
        cases.append((f"front/b{batch}", batch, _front_case(batch, 7000 + (batch or 256))))
    for batch in (512, 4096):
        cases.append((f"refill/b{batch}", batch, _refill_case(batch, 8000 + batch)))
    return cases


# ---------------- sim ----------------
def sim_scripts():
    return [(f"burst/s{seed}/b{batch}", seed, batch) for seed in (3, 17) for batch in (1, 64, 0)]
