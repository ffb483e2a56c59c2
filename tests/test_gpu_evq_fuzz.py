"""The event queue on the device against its plain references, at the structural edges of the kernels.

* every hold case of tests/evq_fuzz_cases.py through nsgpu.HoldRun (csrc/nsgpu_hold.hip, both kernels): the pop log,
  counters, final time, next uid and digest equal the oracle's, which tests/test_evq_fuzz_cpu.py holds to the Python
  restatement on the same cases;
* every sched script through nsgpu.Sched (csrc/nsgpu_sched.hip): each pop and peek equals the heapq model's, the
  size after every op, and the refills the merge kernels ran;
* sim_scripts.burst_script on nsgpu.Sim against nsref.Sim.
Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import nsref
from evq_fuzz_cases import hold_cases, sched_cases, sim_scripts
from evq_fuzz_model import HOLD_BATCH, HOLD_MAX_PENDING, SchedPlacement, hold_rounds, sched_expected
from sim_scripts import burst_script

pytestmark = pytest.mark.gpu

W = 1 << 31
HOLD = {c[0]: c for c in hold_cases()}
SCHED = {c[0]: c for c in sched_cases()}


def family(name):
    return name.split("/")[0]


@functools.lru_cache(maxsize=None)
def oracle(name):
    _, dist, total, _ = HOLD[name]
    res, lts, luid = nsref.churn_run(dist, total, log_cap=dist.size + total + 1)
    lts.setflags(write=False)
    luid.setflags(write=False)
    return res, lts, luid


def counters(st):
    return (st.dispatched, st.holds, st.final_ts, st.next_uid, st.digest)


def check_hold(name, st, gts, guid):
    _, dist, total, cap = HOLD[name]
    res, lts, luid = oracle(name)
    assert res.dispatched == dist.size + total + 1
    assert counters(st) == counters(res), name
    assert np.array_equal(gts, lts[:cap]) and np.array_equal(guid, luid[:cap]), name


def run_hold(name):
    import nsgpu
    _, dist, total, cap = HOLD[name]
    h = nsgpu.HoldRun(dist, total, log_cap=cap)
    h.launch()
    return h


@pytest.mark.parametrize("name", list(HOLD))
def test_hold_case(name):
    _, dist, total, cap = HOLD[name]
    st, gts, guid = run_hold(name).result()
    check_hold(name, st, gts, guid)
    if family(name) == "zeros":
        # the largest commit the round structure allows: 1,024 wherever 1,024 candidates can commit together
        # (test_evq_fuzz_cpu.py::test_hold_rounds shows where that is: all but the one-delay case at n = 1024)
        want = max(r[2] for r in hold_rounds(dist, total)[0])
        assert st.max_batch == want, name
        if dist.size >= HOLD_BATCH and ("/all/" in name or dist.size > HOLD_BATCH):
            assert st.max_batch == HOLD_BATCH, name


@pytest.mark.parametrize("name", ["packed_edges/n11264/t30000", "wide_big/n11264/t3000", "ties/wide/n2048",
                                  "short_log/zeros/all/n1025/cap512"])
def test_hold_second_launch(name):
    # the packed kernel leaves its histogram all-zero; the wide kernel's final_ts is an atomicMax onto a memset
    h = run_hold(name)
    first = h.result()
    check_hold(name, *first)
    h.launch()
    second = h.result()
    check_hold(name, *second)
    assert first[0].rounds == second[0].rounds and first[0].max_batch == second[0].max_batch


def test_hold_packed_after_wide():
    for name in ("packed_edges/n1025/t4100", "wide_mixed/n11264/t20000", "packed_edges/n1025/t4100",
                 "wide_big/n2049/t683", "packed_edges/n11264/t11265"):
        assert (int(HOLD[name][1].max()) >= W) == name.startswith("wide")
        check_hold(name, *run_hold(name).result())


def test_hold_refuses_one_past_capacity():
    import nsgpu
    ok = nsgpu.HoldRun(np.ones(HOLD_MAX_PENDING, dtype=np.uint64), 1)
    ok.launch()
    assert ok.result()[0].dispatched == HOLD_MAX_PENDING + 2
    h = nsgpu.HoldRun(np.ones(HOLD_MAX_PENDING + 1, dtype=np.uint64), 1)
    with pytest.raises(nsgpu.NsgpuError, match="n=11265 outside"):
        h.launch()


# ---------------- sched ----------------
class FastSched:
    """nsgpu.Sched with pops and peeks written into one preallocated array (a pop is one C call)."""

    def __init__(self, batch, cap):
        import nsgpu
        self.s = nsgpu.Sched(batch=batch)
        self.lib = nsgpu.lib()
        self.check = nsgpu.check
        self.out = np.zeros(cap + 1, nsgpu.EVENT_DTYPE)
        self.base = self.out.ctypes.data
        self.n = 0

    def take(self, f, k):
        lo = self.n
        for i in range(lo, lo + k):
            rc = f(self.s.h, self.base + 24 * i)
            if rc:
                self.check(rc)
        self.n += k
        return self.out[lo:lo + k]


def as_array(events):
    import nsgpu
    return np.array(events, dtype=nsgpu.EVENT_DTYPE).reshape(len(events))


def run_sched_script(name):
    _, batch, ops = SCHED[name]
    want = sched_expected(ops)
    calls = sum(len(w[1]) if w[0] in ("pop", "drain") else 1 for w in want)
    q = FastSched(batch, calls)
    by_uid = {ev[1]: ev for op in ops if op[0] == "insert" for ev in op[1]}
    model = SchedPlacement(batch) if batch else None
    staged_at = None                                   # refills when a bulk insert was staged, until a pop flushed it
    for i, (op, w) in enumerate(zip(ops, want)):
        kind = op[0]
        if kind == "insert":
            q.s.insert(op[1])
        elif kind == "remove":
            q.s.remove(by_uid[op[1]])
        elif kind == "peek":
            got = q.take(q.lib.nsgpu_sched_peek_next, 1)
            assert got.tolist() == [w[1]], (name, i)
        else:
            got = q.take(q.lib.nsgpu_sched_remove_next, len(w[1]))
            exp = as_array(w[1])
            if not np.array_equal(got, exp):
                bad = int(np.nonzero(got != exp)[0][0])
                raise AssertionError(f"{name} op {i} ({kind}) pop {bad}: got {got[bad]}, want {exp[bad]}")
        assert q.s.size() == w[-1], (name, i)
        refills = q.s.stats()[0]
        if model:
            model.replay([op])
            assert refills == model.refills, (name, i)
            if kind == "insert" and model.stage and staged_at is None:
                staged_at = refills
            elif staged_at is not None and not model.stage:
                assert refills > staged_at, (name, i)  # the stage was sorted and merged on the device
                staged_at = None
    assert q.s.is_empty() and q.s.size() == 0
    assert q.s.stats()[0] >= 1
    return q


@pytest.mark.parametrize("name", list(SCHED))
def test_sched_case(name):
    run_sched_script(name)


# ---------------- sim ----------------
@functools.lru_cache(maxsize=None)
def sim_oracle(seed):
    o = nsref.Sim(nsref.SCHED_MAP)
    log = burst_script(o, seed)
    return log, o.next_uid(), o.dispatched()


@pytest.mark.parametrize("name,seed,batch", sim_scripts())
def test_burst_script_matches_oracle(name, seed, batch):
    import nsgpu
    want, next_uid, dispatched = sim_oracle(seed)
    g = nsgpu.Sim(batch=batch)
    got = burst_script(g, seed)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (name, i)
    assert g.next_uid() == next_uid and g.dispatched() == dispatched
    assert len(want) > 10000 and any(e[0] != "stopped" and e[0] >= 1 << 32 for e in want)
    refills = (C.c_uint64(), C.c_uint64(), C.c_double())
    nsgpu.check(nsgpu.lib().nsgpu_sim_sched_stats(g.h, *(C.byref(x) for x in refills)))
    assert refills[0].value >= 1
