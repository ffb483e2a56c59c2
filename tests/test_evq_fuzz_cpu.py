"""The event-queue fuzz on the CPU: the C++ oracle against the Python restatement on every hold case, the new Sim
script on the oracle, and proof on the cases and models alone that the cases reach the edges their names claim
(tests/evq_fuzz_cases.py, tests/evq_fuzz_model.py).  tests/test_gpu_evq_fuzz.py runs the same cases on the device."""
import numpy as np
import pytest

import nsref
from evq_fuzz_cases import (FRONT_BATCHES, TILE_BATCHES, TILE_INSERTS, TILE_LIVE, hold_cases, sched_cases,
                            sim_scripts)
from evq_fuzz_model import (HOLD_BATCH, HOLD_MAX_PENDING, TILE, SchedPlacement, digest_of_log, digest_term,
                            hold_model, hold_rounds, sched_expected, script_calls)
from sim_scripts import burst_script

W = 1 << 31
FAMILIES = ("wide_big", "wide_mixed", "packed_edges", "zeros", "ties", "short_log")


def family(name):
    return name.split("/")[0]


def test_digest_restatement():
    # the vectorised sum equals the scalar definition, and the scalar one the oracle's (through churn_run below)
    ts = np.array([0, 1, (1 << 32) + 7, (1 << 62) - 1], dtype=np.uint64)
    uid = np.array([4, 0xfffffffe, 77, 5], dtype=np.uint32)
    want = sum(digest_term(k, int(ts[k]), int(uid[k])) for k in range(4)) & ((1 << 64) - 1)
    assert digest_of_log(ts, uid) == want


@pytest.mark.parametrize("fam", FAMILIES)
def test_oracle_equals_python_model(fam):
    n_cases = 0
    for name, dist, total, _cap in hold_cases():
        if family(name) != fam:
            continue
        n_cases += 1
        want = hold_model(dist, total)
        res, lts, luid = nsref.churn_run(dist, total, log_cap=want.dispatched)
        assert want.dispatched == dist.size + total + 1, name
        assert np.array_equal(lts, want.log_ts) and np.array_equal(luid, want.log_uid), name
        assert (res.dispatched, res.holds, res.final_ts, res.next_uid, res.digest) == \
            (want.dispatched, want.holds, want.final_ts, want.next_uid, want.digest), name
    assert n_cases >= 2


def test_hold_cases_are_what_the_issue_lists():
    cases = hold_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    assert {family(n) for n in names} == set(FAMILIES)
    for name, dist, total, cap in cases:
        n = dist.size
        assert dist.dtype == np.uint64 and 1 <= n <= HOLD_MAX_PENDING and int(dist.max()) < 1 << 62, name
        assert cap == n + total + 1 or family(name) == "short_log", name
    by = {}
    for name, dist, total, _ in cases:
        by.setdefault(family(name), []).append((dist, total))
    assert {(d.size, t) for d, t in by["wide_big"]} == \
        {(n, t) for n in (1025, 2049, 10000, 11264) for t in (n // 3, 3000, 20000)}
    assert {d.size for d, _ in by["wide_mixed"]} == {1500, 11264}
    for dist, _ in by["wide_mixed"]:
        wide = dist[dist >= W]
        assert 0.004 < wide.size / dist.size < 0.03
        assert set(wide.tolist()) == {W, W + 1, 1 << 40}
        small = dist[dist < W]
        assert int(small.max()) < 1000 and {0, 1, 2, 5} <= set(small.tolist())
    want = set()
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 11263, 11264):
        want |= {(n, min(t, 30000)) for t in (0, 1, n - 1, n, n + 1, 4 * n)}
    assert {(d.size, t) for d, t in by["packed_edges"]} == want
    for dist, _ in by["packed_edges"]:
        assert int(dist.max()) < W
        if dist.size >= 1023:
            assert 0.005 < np.mean(dist == W - 1) < 0.04 and 0.005 < np.mean(dist == 0) < 0.04
    assert sorted((d.size, int(d.sum()), t) for d, t in by["zeros"]) == \
        sorted((n, s, 3 * n) for n in (1, 1024, 1025, 5000) for s in (0, 1))
    assert {d.size for d, _ in by["ties"]} == {2048, 11264}
    for dist, total in by["ties"]:
        assert len(set(dist.tolist())) == 3
        ts = hold_model(dist, total).log_ts
        assert np.mean(ts[1:] == ts[:-1]) >= 0.5          # at least half of all pops: the uid decided
    short = [(name, dist.size, total, cap) for name, dist, total, cap in cases if family(name) == "short_log"]
    assert len(short) == 9 and len({(n, t) for _, n, t, _ in short}) == 3
    for _, n, total, cap in short:
        assert cap in (1, n // 2, n + total) and 0 < cap < n + total + 1
    assert {family(name.split("/", 1)[1]) for name, _, _, _ in short} == {"wide_big", "packed_edges", "zeros"}


def test_hold_cases_reach_the_edges():
    cases = hold_cases()
    wide = [(name, dist, total) for name, dist, total, _ in cases if family(name) in ("wide_big", "wide_mixed")]
    assert all(int(dist.max()) >= W for _, dist, _ in wide)
    assert sum(1 for _, dist, total in wide if dist.size > HOLD_BATCH and total > 0) >= 3
    # both kernels at the capacity, below the generation (children stop while first-generation events pend), no hold
    for kernel_is_wide in (False, True):
        mine = [(dist, total) for _, dist, total, _ in cases if (int(dist.max()) >= W) == kernel_is_wide]
        assert any(dist.size == HOLD_MAX_PENDING for dist, _ in mine)
        assert any(0 < total < dist.size and dist.size > HOLD_BATCH for dist, total in mine)
    assert any(total == 0 for _, _, total, _ in cases)
    assert any(total == 0 and dist.size == HOLD_MAX_PENDING for _, dist, total, _ in cases)


@pytest.mark.parametrize("fam", ("zeros", "ties", "wide_mixed"))
def test_hold_rounds(fam):
    """(K, P, p, m) of every device round, recomputed: the round shapes the kernels have to get right."""
    seen = set()
    for name, dist, total, _ in hold_cases():
        if family(name) != fam:
            continue
        n = dist.size
        rounds, log = hold_rounds(dist, total)
        want = hold_model(dist, total)
        assert [e[0] for e in log] == want.log_ts.tolist() and [e[1] for e in log] == want.log_uid.tolist(), name
        max_p = max(r[2] for r in rounds)
        if fam == "zeros":
            if "/all/" in name and n >= HOLD_BATCH:
                # every candidate's child lands at the current ts for a whole 1,024-event round
                full = [r for r in rounds if r[2] == HOLD_BATCH and r[3] == HOLD_BATCH]
                assert full and not dist.any() and not want.log_ts.any(), name
                assert max_p == HOLD_BATCH
            elif n > HOLD_BATCH:
                assert max_p == HOLD_BATCH, name
            elif n == HOLD_BATCH:
                # 1,023 events at ts 0 and one at ts 1: a child at ts 0 always precedes the last candidate, so no
                # round of this case can commit all 1,024
                assert max_p == HOLD_BATCH - 1, name
            else:
                assert max_p == 1, name
        if any(r[1] > HOLD_BATCH and r[2] == HOLD_BATCH for r in rounds):
            seen.add("full round below P")             # B = HOLD_BATCH < P, every candidate commits
        if any(r[3] < r[2] and r[1] - r[2] > 0 for r in rounds):
            seen.add("m < p with survivors")           # the children stop inside a round
        if any(r[3] == 0 and r[1] > HOLD_BATCH for r in rounds):
            seen.add("no children above one batch")
        if any(r[2] < 16 and r[1] > HOLD_BATCH for r in rounds):
            seen.add("small commit far below P")
    assert {"full round below P", "m < p with survivors", "no children above one batch"} <= seen
    if fam == "wide_mixed":
        assert "small commit far below P" in seen


# ---------------- sched ----------------
def test_sched_cases_shape():
    cases = sched_cases()
    assert len({c[0] for c in cases}) == len(cases)
    assert {family(c[0]) for c in cases} == {"tiles", "keys", "front", "refill"}
    for name, batch, ops in cases:
        assert script_calls(ops) < 40000, name
        uids = [ev[1] for op in ops if op[0] == "insert" for ev in op[1]]
        assert len(set(uids)) == len(uids) and max(uids) < 0xffffffff, name
        assert all(ev[3] == ev[1] * 8 and 0 <= ev[0] < 1 << 63 for op in ops if op[0] == "insert" for ev in op[1])
        out = sched_expected(ops)                      # runs: no pop or peek on an empty queue, no double remove
        assert out[-1][-1] == 0, name
    tiles = {(b, len(ops[0][1]) - 1, len(ops[2][1])) for name, b, ops in cases if family(name) == "tiles"}
    assert tiles == {(b, lv, s) for b in TILE_BATCHES for lv in TILE_LIVE for s in TILE_INSERTS}
    assert set(TILE_INSERTS) == {1, 2047, 2048, 2049, 4096, 4097, 3 * 2048, 5 * 2048 + 1, 20000}
    assert {b for name, b, _ in cases if family(name) == "front"} == set(FRONT_BATCHES) == {0, 1, 2, 255, 256, 257}


def test_tiles_stage_sizes():
    """With a front of one event every bulk insert is staged whole: the device sorts and merges exactly the sizes
    listed, against live arrays of every listed size; the larger fronts split the insert between heap and stage."""
    stages = set()
    for name, batch, ops in sched_cases():
        if family(name) != "tiles" or batch != 1:
            continue
        m = SchedPlacement(batch)
        m.replay(ops[:4])
        live, size = len(ops[0][1]) - 1, len(ops[2][1])
        assert m.refill_log[1] == (size, live, 1), name
        stages.add((live, size))
        keys = [ev[0] for ev in ops[0][1]]
        bulk = [ev[0] for ev in ops[2][1]]
        if size >= 2047:
            assert min(bulk) < min(keys) and max(bulk) > max(keys)
            assert bulk != sorted(bulk)
    assert stages == {(lv, s) for lv in TILE_LIVE for s in TILE_INSERTS}
    # a run count that is no power of two: the last merge pass has a tail run without a partner
    assert any(-(-s // TILE) in (3, 11) for _, s in stages)
    split = 0
    for name, batch, ops in sched_cases():
        if family(name) == "tiles" and batch == 4096 and len(ops[0][1]) - 1 == TILE:
            m = SchedPlacement(batch)
            places = [p for p, _, _ in m.replay(ops[:3])[2]]
            split += "heap" in places and "stage" in places
    assert split >= 5


def test_keys_decide_by_high_word_and_by_uid():
    lo = (1 << 32) - 1
    for name, batch, ops in sched_cases():
        if family(name) != "keys":
            continue
        evs = [ev for op in ops if op[0] == "insert" for ev in op[1]]
        ts_set = {ev[0] for ev in evs}
        assert {0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 5, (1 << 63) - 1} <= ts_set
        assert sum(1 for ev in evs if (1 << 32) - 300 <= ev[1] <= (1 << 32) - 2) >= 50
        pops = [ev for o in sched_expected(ops) if o[0] in ("pop", "drain") for ev in o[1]]
        assert len(pops) == len(evs)
        # consecutive pops whose order only the high word of ts gives: equal low words, uids the other way round
        by_low = {}
        for ev in evs:
            by_low.setdefault(ev[0] & lo, []).append(ev)
        high = sum(1 for g in by_low.values() for a in g for b in g
                   if a[0] < b[0] and a[1] > b[1] and a[2] == b[2])
        assert high >= 300, name
        # ... and only the uid: runs of 300 and more equal ts, inserted in shuffled uid order
        runs, i = [], 0
        while i < len(pops):
            j = i
            while j < len(pops) and pops[j][0] == pops[i][0]:
                j += 1
            runs.append(pops[i:j])
            i = j
        long_runs = [r for r in runs if len(r) >= 300]
        assert len(long_runs) >= 4, name
        order = {ev[1]: k for k, ev in enumerate(evs)}
        for r in long_runs:
            u = [ev[1] for ev in r]
            assert u == sorted(u) and [order[x] for x in u] != sorted(order[x] for x in u)
        # both halves span more than one tile, so tile sort, merge pass and the merge with the device array all see them
        assert all(len(op[1]) > TILE for op in ops if op[0] == "insert"), name
        m = SchedPlacement(batch)
        second = [p for p, _, _ in m.replay(ops[:4])[3]]
        assert "heap" in second and (batch > TILE or second.count("stage") > TILE), name


def test_front_placements():
    for name, batch, ops in sched_cases():
        if family(name) != "front" or batch == 0:
            continue
        m = SchedPlacement(batch)
        notes = m.replay(ops)
        removes = [n for op, n in zip(ops, notes) if op[0] == "remove"]
        assert set(removes) == {"front", "heap", "stage", "device"}, name
        below = above = far = near = 0
        for op, note in zip(ops, notes):
            if op[0] != "insert":
                continue
            for place, ev, bound in note:
                if bound is None:
                    continue
                if ev[0] == bound[0] and ev[1] < bound[1]:
                    assert place == "heap"
                    below += 1
                if ev[0] == bound[0] and ev[1] > bound[1]:
                    assert place == "stage"
                    above += 1
                far += place == "stage" and ev[0] > bound[0] + 1000
                near += place == "heap" and ev[0] < bound[0]
        assert below and above and far and (near or batch == 1), (name, below, above, far, near)
        # a peek before and after every pop and remove
        for i, op in enumerate(ops):
            if op[0] in ("pop", "remove"):
                assert ops[i - 1] == ("peek",), name
                assert i + 1 == len(ops) or ops[i + 1] == ("peek",), name
        # the front was half-consumed when the aimed inserts came
        first_aimed = next(i for i, op in enumerate(ops) if op[0] == "insert" and i > 0)
        m2 = SchedPlacement(batch)
        m2.replay(ops[:first_aimed])
        assert m2.fi < len(m2.front) and (m2.fi > 0 or batch == 1), name
    front = {b: ops for name, b, ops in sched_cases() if family(name) == "front"}
    assert front[0] == front[256]


def test_refill_family():
    for name, batch, ops in sched_cases():
        if family(name) != "refill":
            continue
        m = SchedPlacement(batch)
        m.replay(ops)
        assert sum(1 for op in ops if op[0] == "drain") == 8 and m.size == 0
        stages = [ns for ns, _, _ in m.refill_log if ns]
        assert len(stages) == 8
        assert [s > TILE for s in stages] == [False, True, False, True, False, True, False, True]
        assert any(ns == 0 and take > 0 for ns, _, take in m.refill_log), name


# ---------------- sim ----------------
def test_burst_script_on_the_oracle():
    assert {(s, b) for _, s, b in sim_scripts()} == {(s, b) for s in (3, 17) for b in (1, 64, 0)}
    for seed in sorted({s for _, s, _ in sim_scripts()}):
        o = nsref.Sim(nsref.SCHED_MAP)
        log = burst_script(o, seed)
        marks = [i for i, e in enumerate(log) if e[0] == "stopped"]
        assert len(marks) == 1 and 100 < marks[0] < len(log) - 100       # a Stop in mid-run, a second Run after it
        events = [e for e in log if e[0] != "stopped"]
        assert len(events) > 10000 and o.dispatched() >= len(events)
        assert sum(1 for e in events if e[0] >= 1 << 32) > 100
        assert [e[0] for e in events] == sorted(e[0] for e in events)
        assert sum(1 for e in events if e[2] in (-100, -200)) == 2       # both 5,000-event bursts ran
        o2 = nsref.Sim(nsref.SCHED_MAP)
        assert burst_script(o2, seed) == log                             # a function of the seed alone
