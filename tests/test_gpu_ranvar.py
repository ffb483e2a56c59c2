"""Random OnOff times (Uniform, Exponential) on the GPU engine, each run compared with the Python model
(tests/p2p_ranvar_pyref.py, pinned by tests/test_ranvar_cpu.py, which also asserts that no scenario here has an
ambiguous draw): digest, dispatch count, next uid, the full pop log, device and application counters, UdpServer and
error-model records, the sorted trace records, the draw counts, and an empty ambiguous log.  Everything is integer
state: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import nsgpu
import p2p
import p2p_flowmon_pyref as FM
import p2p_ranvar_pyref as RV
import ranvar_cases as RC
from p2p_model_compare import assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
_models = {}


def model(name, *args):
    """The model's run of scenario RC.<name> (*args), computed once."""
    if (name, args) not in _models:
        sc = getattr(RC, name)(*args)
        m = RV.run_monitored(sc, ALL_KINDS) if sc.flowmon else RV.run(sc, ALL_KINDS)
        assert len(m["ambiguous"]) == 0
        _models[(name, args)] = (sc, m)
    return _models[(name, args)]


def assert_draws(eng, m, label=""):
    assert np.array_equal(eng.onoff_draws(), m["draws"]), "draw counts " + label
    rec, over = eng.ambiguous_draws()
    assert len(rec) == 0 and over == 0, "ambiguous draws " + label


def run_engine(sc, m, traced=False, want_wide=None, again=False, label=""):
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    if want_wide is not None:
        assert eng.wide() == want_wide
    if traced:
        eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    for _ in range(2 if again else 1):  # (run = reset + launch: the second run starts from the reset image)
        st, devc, appc, log = eng.run(n)
        assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(),
                            eng.trace() if traced else None, label=label)
        assert_draws(eng, m, label)
    return eng


# ---------------- the variable on the device ----------------
def constructed():
    u = RC.first_u()
    return [p2p.Exponential(RC.ambiguous_mean(u), RC.AMBIGUOUS_STREAM),
            p2p.Exponential(0.003, RC.AMBIGUOUS_STREAM, bound=RC.ambiguous_bound(u))]


def test_variable_on_the_device_equals_the_host():
    """nsgpu_ranvar_run in a one-thread kernel against the same function on the host: seconds, ns, the other
    candidate and the flags, bit for bit, over 4,096 draws; the constructed ambiguous draws keep their flag."""
    cases = [(p2p.Uniform(0.001, 0.005, 0), 1, 1), (p2p.Uniform(0.0, 1.0, 5), 12345, 7), (p2p.Uniform(0.5, 0.5, 2), 1, 3),
             (p2p.Exponential(0.003, 0), 1, 1), (p2p.Exponential(1.0, 3), 12345, 7),
             (p2p.Exponential(0.003, 1, bound=0.001), 1, 1), (p2p.Exponential(2.5, 40, bound=0.4), 99, 2)]
    cases += [(v, RC.AMBIGUOUS_SEED, RC.AMBIGUOUS_RUN) for v in constructed()]
    for var, seed, run in cases:
        host = p2p.ranvar_run(var, seed, run, 4096)
        dev = p2p.ranvar_run(var, seed, run, 4096, on_device=True)
        assert [x.hex() for x in dev[0].tolist()] == [x.hex() for x in host[0].tolist()], var
        for h, d in zip(host[1:], dev[1:]):
            assert np.array_equal(h, d), var
    for var in constructed():
        assert p2p.ranvar_run(var, RC.AMBIGUOUS_SEED, RC.AMBIGUOUS_RUN, 1, on_device=True)[3][0]


def test_constructed_ambiguous_draw_is_logged_and_does_not_stop_the_run():
    """The two-node scenario whose OnTime variable's first draw is the constructed one: the run goes on with -mean *
    hi, the log holds the record with both timestamps, check_ambiguous decides it for this host."""
    u = RC.first_u()
    mean = RC.ambiguous_mean(u)
    sc = RC.two_nodes("exp", rng_seed=RC.AMBIGUOUS_SEED, rng_run=RC.AMBIGUOUS_RUN)
    sc.apps[1]["on_var"] = p2p.Exponential(mean, RC.AMBIGUOUS_STREAM)
    sc.stop_ns = 100_000_000
    want = RV.exponential_attempt(mean, 0.0, u)
    m = RV.run(sc)
    eng = p2p.Engine(sc)
    st = eng.run()[0]
    rec, over = eng.ambiguous_draws()
    assert over == 0 and len(rec) >= 1
    first = rec[(rec["app"] == 1) & (rec["which"] == 0) & (rec["ordinal"] == 0)]
    assert len(first) == 1
    assert (int(first[0]["ns"]), int(first[0]["ns_other"])) == (want["dev_ns"], want["dev_other"])
    assert int(first[0]["k"]) == int(round(u * 4294967088.0))
    d = eng.onoff_draws()
    assert d["ambiguous"][1] == len(rec) == len(m["ambiguous"])
    assert np.array_equal(np.sort(rec, order=["app", "which", "ordinal"]),
                          np.sort(m["ambiguous"], order=["app", "which", "ordinal"]))
    bad = p2p.check_ambiguous(rec, sc)
    if len(bad) == 0:  # (this host's libm agrees with the device on every listed draw: the run is the model's)
        assert st.digest == m["stats"]["digest"] and st.dispatched == m["stats"]["dispatched"]
    else:
        assert st.digest != m["stats"]["digest"]
    eng.close()


# ---------------- two nodes, one link ----------------
@pytest.mark.parametrize("kind", ["uniform", "exp", "bounded"])
def test_two_nodes(kind, monkeypatch):
    """Several hundred random transitions on one link: wide, narrow and traced."""
    sc, m = model("two_nodes", kind)
    run_engine(sc, m, want_wide=True).close()
    run_engine(sc, m, traced=True, label="traced").close()
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    run_engine(sc, m, want_wide=False, label="narrow").close()


def test_sources_that_stop(monkeypatch):
    """A MaxBytes source that stops itself in a burst and one stopped by its Stop time while on."""
    sc, m = model("stops")
    run_engine(sc, m, want_wide=True).close()
    run_engine(sc, m, traced=True, label="traced").close()
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    run_engine(sc, m, want_wide=False, label="narrow").close()


# ---------------- the 4 x 4 ports grid ----------------
def test_grid_wide_narrow_and_traced(monkeypatch):
    sc, m = model("grid4")
    run_engine(sc, m, want_wide=True, label="wide").close()
    run_engine(sc, m, traced=True, label="traced").close()
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    run_engine(sc, m, want_wide=False, label="narrow").close()
    run_engine(sc, m, traced=True, want_wide=False, label="narrow traced").close()


def test_grid_on_two_loopback_ranks():
    sc, m = model("grid4")
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, 2, log_cap=n, trace_cap=len(m["trace"]) + 64, trace_kinds=ALL_KINDS)
    for _ in range(2):
        st, devc, appc, log = grp.run(n)
        assert_equals_model(m, st, devc, appc, log, grp.udp_servers(), grp.frag_stats(), grp.error_models(), grp.trace(),
                            label="two ranks")
        assert_draws(grp, m, "two ranks")
    # each rank drew for its own nodes' applications only
    own = grp.owner
    for r, mem in enumerate(grp.members):
        d = mem.onoff_draws()
        for a, A in enumerate(sc.apps):
            if own[A["node"]] != r:
                assert d["on_draws"][a] == d["off_draws"][a] == 0


def test_grid_with_flow_statistics():
    """flowmon on the single engine: the flow records equal p2p_flowmon_pyref's monitor fed by the same model."""
    sc, m = model("grid4", True)
    eng = run_engine(sc, m, label="flowmon")
    for d in (FM.MAX_PER_HOP_DELAY_NS,):
        got, want = eng.flow_stats(d), m["flows"][d]
        assert len(got) == len(want) > 0
        for f in p2p.FLOW_STATS_DTYPE.names:
            assert np.array_equal(got[f], want[f]), f
    eng.close()
    plain = model("grid4")[1]
    assert plain["stats"] == m["stats"]  # (the monitor changes nothing else)


# ---------------- reset ----------------
@pytest.mark.parametrize("name,args", [("two_nodes", ("bounded",)), ("grid4", ())])
def test_reset_and_rerun_reproduces_the_run(name, args):
    sc, m = model(name, *args)
    run_engine(sc, m, again=True).close()


# ---------------- runtime refusals ----------------
def test_refusals_that_need_an_engine():
    sc, _m = model("two_nodes", "uniform")
    eng = p2p.Engine(sc)
    sim = nsgpu.Sim()
    with pytest.raises(nsgpu.NsgpuError, match="a scenario with a random OnOff time cannot be attached to a host-closure "
                                               "runtime"):
        sim.attach_p2p(eng)
    with pytest.raises(nsgpu.NsgpuError, match="random OnOff time cannot be attached"):
        sim.adopt_p2p(eng)
    uid, seq = C.c_uint32(100), C.c_uint32(0)
    with pytest.raises(nsgpu.NsgpuError, match="nsgpu_p2p_inject_send: not available in a scenario with a random OnOff "
                                               "time"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_inject_send(eng.h, 1, 0, 4, 0, C.byref(uid), C.byref(seq), None))
    with pytest.raises(nsgpu.NsgpuError, match="nsgpu_p2p_onoff_draws: the engine has 2 applications"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_onoff_draws(eng.h, None, 0, None))
    eng.close()
    # an engine without a random variable answers zeros
    eng = p2p.Engine(p2p.first_cc())
    eng.run()
    rec, over = eng.ambiguous_draws()
    assert not eng.onoff_draws().view(np.uint8).any() and len(rec) == 0 and over == 0
    eng.close()
