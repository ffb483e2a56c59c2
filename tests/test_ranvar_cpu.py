"""Random OnOff times without a GPU: the shared variable code on the host (nsgpu_ranvar_run, nsgpu_ranvar_log) against
the Python formulas and decimal, the C ABI's refusals and layout, and the conditions the scenarios of
tests/test_gpu_ranvar.py must meet (asserted on the Python model alone, tests/p2p_ranvar_pyref.py)."""
import ctypes as C
import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

import nsgpu
import nsref
import p2p
import p2p_errmodel_pyref as E
import p2p_ranvar_pyref as RV
import ranvar_cases as RC

M1 = E.M1
_runs = {}


def run(name, *args):
    if (name, args) not in _runs:
        sc = getattr(RC, name)(*args)
        _runs[(name, args)] = (sc, (RV.run_monitored if sc.flowmon else RV.run)(sc))
    return _runs[(name, args)]


def plan(sc):
    return p2p.dist_plan(sc, None, 0, 1)


# ---------------- Uniform ----------------
@pytest.mark.parametrize("lo,hi", [(0.001, 0.005), (0.0, 1.0), (0.5, 0.5), (0.0, 0.0), (0.25, 1.5), (1e-9, 3e-9)])
def test_uniform_on_the_host_equals_the_formula(lo, hi):
    """m_min + RandU01 () * (m_max - m_min): the product and the sum rounded separately; seconds and ns, bit for bit."""
    for seed, run_, stream in ((1, 1, 0), (1, 3, 5), (12345, 7, 2), (99, 2, 40)):
        sec, ns, other, amb = p2p.ranvar_run(p2p.Uniform(lo, hi, stream), seed, run_, 4096)
        g = E.RngStream(seed, run_, stream)
        want = [lo + g.u01() * (hi - lo) for _ in range(4096)]
        assert [x.hex() for x in sec.tolist()] == [x.hex() for x in want]
        assert ns.tolist() == [nsref.seconds(x) for x in want]
        assert np.array_equal(other, ns) and not amb.any()


def test_constant_draws_nothing():
    sec, ns, _other, amb = p2p.ranvar_run(p2p.Constant(0.25), 1, 1, 8)
    assert sec.tolist() == [0.25] * 8 and ns.tolist() == [250_000_000] * 8 and not amb.any()


# ---------------- the log ----------------
def log_arguments():
    rng = np.random.default_rng(20261021)
    ks = [rng.integers(1, M1 + 1, 100_000), np.arange(1, 65), np.arange(M1 - 63, M1 + 1)]
    for e in range(1, 33):
        ks.append(np.arange(2 ** e - 8, 2 ** e + 9))
    ks = np.concatenate(ks)
    return np.unique(ks[(ks >= 1) & (ks <= M1)])


def test_log_accuracy_against_decimal():
    """Over 100,000 random k, the 64 smallest, the 64 largest and the values around every power of two: hi is the
    correctly rounded logarithm of the double u = k * norm; hi + lo is within the stated bound (2^-40 ulp of hi, inside
    the 2^-20 the scheme needs) of the logarithm at 60 digits; and this host's math.log is hi or the neighbour on lo's
    side — the assumption the two-candidate rule rests on."""
    getcontext().prec = 60
    ks = log_arguments()
    assert len(ks) >= 100_000
    u = ks.astype(np.float64) * p2p.RNG_NORM
    hi, lo = p2p.ranvar_log(u)
    worst, neighbour = 0.0, 0
    for i in range(len(u)):
        ui, h, l = float(u[i]), float(hi[i]), float(lo[i])
        t = Decimal(ui).ln()
        assert h == float(t), (int(ks[i]), h, float(t))
        ulp = math.ulp(h)
        assert abs(l) <= ulp / 2
        err = float(abs(Decimal(h) + Decimal(l) - t) / Decimal(ulp))
        worst = max(worst, err)
        ml = math.log(ui)
        if ml != h:
            assert l != 0 and ml == math.nextafter(h, math.inf if l > 0 else -math.inf), (int(ks[i]), ml, h, l)
            neighbour += 1
    print("log: %d arguments, worst error %.3g ulp, math.log is the neighbour %d times" % (len(u), worst, neighbour))
    assert worst < RV.LOG_ERR < 2.0 ** -20


def test_log_refuses_arguments_outside_its_range():
    for bad in (0.0, 1.0, -0.5, 2.0 ** -34):
        with pytest.raises(nsgpu.NsgpuError, match="nsgpu_ranvar_log: u\\[0\\] outside"):
            p2p.ranvar_log([bad])


# ---------------- Exponential ----------------
@pytest.mark.parametrize("mean,bound", [(0.003, 0.0), (1.0, 0.0), (0.003, 0.004), (0.003, 0.001), (2.5, 0.4)])
def test_exponential_on_the_host_equals_the_model(mean, bound):
    """Draw for draw: the flags agree, the draw consumes the model's number of U01 values, and wherever the model calls
    the draw unambiguous the host function's timestamp is the one math.log gives."""
    for seed, run_, stream in ((1, 1, 0), (12345, 7, 3)):
        n = 4096
        sec, ns, other, amb = p2p.ranvar_run(p2p.Exponential(mean, stream, bound), seed, run_, n)
        v = RV.Variable(p2p.Exponential(mean, stream, bound), seed, run_)
        clean = 0
        for i in range(n):
            before = len(v.ambiguous)
            r = v.get_value()
            flagged = len(v.ambiguous) > before
            assert bool(amb[i]) == flagged, i
            if not flagged:
                assert int(ns[i]) == nsref.seconds(r) == int(other[i]), i
                assert bound == 0 or float(sec[i]) <= bound
                clean += 1
        assert clean >= n - 4
        # the streams are in step after the last draw: the attempts were the same
        u_next = E.RngStream(seed, run_, stream)
        for _ in range(v.attempts):
            u_next.u01()
        assert v.g.cg == u_next.cg


def test_constructed_ambiguous_timestamp():
    """A mean for which -mean * hi and -mean * neighbour fall on either side of a whole nanosecond: the flag is set
    and both timestamps are reported, by the single attempt and by the variable's first draw."""
    for stream in (0, 1, 2):
        u = RC.first_u(stream=stream)
        k = int(round(u * (M1 + 1.0)))
        mean = RC.ambiguous_mean(u)
        want = RV.exponential_attempt(mean, 0.0, u)
        assert want["ambiguous"] and want["dev_ns"] != want["dev_other"]
        got = p2p.ranvar_exponential(mean, 0.0, k)
        assert got["ambiguous"] and (got["ns"], got["ns_other"]) == (want["dev_ns"], want["dev_other"])
        assert abs(got["ns"] - got["ns_other"]) == 1
        sec, ns, other, amb = p2p.ranvar_run(p2p.Exponential(mean, stream), RC.AMBIGUOUS_SEED, RC.AMBIGUOUS_RUN, 16)
        assert amb.tolist() == [True] + [False] * 15
        assert (int(ns[0]), int(other[0])) == (want["dev_ns"], want["dev_other"]) and np.array_equal(ns[1:], other[1:])
        # a mean one part in a thousand away: the same draw is unambiguous
        assert not p2p.ranvar_exponential(mean * 1.001, 0.0, k)["ambiguous"]


def test_constructed_ambiguous_bound():
    """A bound between -mean * hi and -mean * neighbour: the two candidates disagree about the redraw."""
    u = RC.first_u()
    k = int(round(u * (M1 + 1.0)))
    bound = RC.ambiguous_bound(u)
    want = RV.exponential_attempt(0.003, bound, u)
    got = p2p.ranvar_exponential(0.003, bound, k)
    assert want["ambiguous"] and got["ambiguous"] and got["accept"] == want["dev_accept"]
    assert got["ns"] == got["ns_other"] == want["dev_ns"]  # (the timestamps agree: only the bound decides)
    _sec, _ns, _other, amb = p2p.ranvar_run(p2p.Exponential(0.003, RC.AMBIGUOUS_STREAM, bound), RC.AMBIGUOUS_SEED,
                                            RC.AMBIGUOUS_RUN, 4)
    assert amb[0]
    assert not p2p.ranvar_exponential(0.003, bound * 1.01, k)["ambiguous"]


def test_check_ambiguous_decides_for_this_host():
    """A listed record whose host timestamp equals the device's is dropped; one that differs is returned."""
    u = RC.first_u()
    k = int(round(u * (M1 + 1.0)))
    mean = RC.ambiguous_mean(u)
    sc = RC.two_nodes("exp")
    sc.apps[1]["on_var"] = p2p.Exponential(mean, 0)
    t = p2p.ranvar_exponential(mean, 0.0, k)
    host = nsref.seconds(-mean * math.log(u))
    assert host in (t["ns"], t["ns_other"])
    rec = np.array([(1, 0, 0, k, t["ns"], t["ns_other"]), (1, 0, 0, k, t["ns_other"], t["ns"])], p2p.AMBIGUOUS_DRAW_DTYPE)
    bad = p2p.check_ambiguous(rec, sc)
    assert len(bad) == 1 and int(bad[0]["ns"]) != host
    assert p2p.seconds_to_ns(-mean * math.log(u)) == host
    for x in (0.0, 1e-9, 0.003, 0.9999999995, 1.0, 22.18, 1234.000000001):
        assert p2p.seconds_to_ns(x) == nsref.seconds(x)


def test_attempt_limit_is_an_error_return():
    """A bound far below the mean (create refuses it; nsgpu_ranvar_run does not): 1,024 rejections end the call."""
    with pytest.raises(nsgpu.NsgpuError, match="nsgpu error 5: nsgpu_ranvar_run: a bounded ExponentialVariable was "
                                               "rejected 1024 times"):
        p2p.ranvar_run(p2p.Exponential(1.0, 0, bound=1e-9), 1, 1, 4)


# ---------------- create's refusals (plan_engine: no device) ----------------
def two(on=None, off=None, **kw):
    sc = RC.two_nodes("uniform", **kw)
    sc.apps[1]["on_var"], sc.apps[1]["off_var"] = on, off
    return sc


REFUSALS = [
    (lambda: two(p2p.Uniform(-0.001, 0.002, 0)), "app 1: OnTime: Uniform with min < 0"),
    (lambda: two(None, p2p.Uniform(0.003, 0.002, 0)), "app 1: OffTime: Uniform with max < min"),
    (lambda: two(p2p.Uniform(0.0, math.inf, 0)), "app 1: OnTime: Uniform with a non-finite parameter"),
    (lambda: two(p2p.Uniform(math.nan, 1.0, 0)), "app 1: OnTime: Uniform with a non-finite parameter"),
    (lambda: two(p2p.Exponential(0.0, 0)), "app 1: OnTime: Exponential with mean <= 0"),
    (lambda: two(p2p.Exponential(-1.0, 0)), "app 1: OnTime: Exponential with mean <= 0"),
    (lambda: two(p2p.Exponential(math.inf, 0)), "app 1: OnTime: Exponential with a non-finite mean"),
    (lambda: two(p2p.Exponential(math.nan, 0)), "app 1: OnTime: Exponential with a non-finite mean"),
    (lambda: two(p2p.Exponential(4.1e8, 0)), "app 1: OnTime: Exponential whose mean overflows the timestamp"),
    (lambda: two(None, p2p.Exponential(0.003, 0, bound=-0.001)), "app 1: OffTime: Exponential with bound < 0"),
    (lambda: two(p2p.Exponential(0.008, 0, bound=0.0009)), "app 1: OnTime: Exponential with a bound below mean / 8"),
    (lambda: two(p2p.Uniform(0.001, 0.002, 4), p2p.Exponential(0.003, 4)),
     "app 1 OnTime and app 1 OffTime name the same RngStream 4"),
    (lambda: two(p2p.RanVar(p2p.RV_OTHER, 0, 1.0)), "app 1: OnTime: only Constant, Uniform and Exponential variables are "
                                                    "modelled"),
    (lambda: two(p2p.RanVar(17, 0, 1.0)), "app 1: OnTime: unknown random variable kind 17"),
    (lambda: two(p2p.Uniform(0.001, 0.002, 0), rng_seed=4294944443), "rng_seed 4294944443 is not a seed "
                                                                      "RngStream::CheckSeed accepts"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_create_refuses(i):
    make, msg = REFUSALS[i]
    with pytest.raises(nsgpu.NsgpuError, match=msg):
        plan(make())


def test_create_refuses_a_variable_on_another_kind_and_shared_streams():
    sc = RC.two_nodes("uniform")
    sc.apps[0]["on_var"] = p2p.Uniform(0.001, 0.002, 7)  # (the PacketSink)
    with pytest.raises(nsgpu.NsgpuError, match="app 0: OnTime: a random variable on an application that is not an OnOff"):
        plan(sc)
    sc = RC.stops()
    sc.apps[2]["off_var"] = p2p.Exponential(0.002, 5)  # (application 1's OnTime stream)
    with pytest.raises(nsgpu.NsgpuError, match="app 1 OnTime and app 2 OffTime name the same RngStream 5"):
        plan(sc)
    sc = RC.grid4()
    (dev,) = sc.error_models
    sc.error_models[dev]["stream"] = 6
    with pytest.raises(nsgpu.NsgpuError, match="app 10: OnTime names RngStream 6, which a Rate error model names too"):
        plan(sc)
    sc.error_models[dev]["enabled"] = False  # (a disabled model draws nothing: no stream is used)
    plan(sc)


def test_acceptance_at_the_limits():
    plan(two(p2p.Exponential(0.008, 0, bound=0.001)))  # (bound == mean / 8)
    plan(two(p2p.Uniform(0.0, 0.0, 0), p2p.Uniform(0.002, 0.002, 1)))
    plan(two(p2p.Exponential(3.9e8, 0)))
    plan(two(p2p.Constant(0.002), p2p.Constant(0.001)))


# ---------------- layout ----------------
def test_struct_sizes_and_a_short_ext():
    """nsgpu_p2p_scenario keeps its 368 bytes; the extension record grew by two pointers, and a caller compiled against
    the shorter record (size 24) is served as before: its trace entries are read, the variables behind them are not."""
    assert C.sizeof(p2p.ScenarioStruct) == 368
    assert C.sizeof(p2p.ScenarioExtV2) == 40 and p2p.ScenarioExtV2.app_on_var.offset == 24 and C.sizeof(p2p.ScenarioExt) == 24
    assert p2p.RANVAR_DTYPE.itemsize == 24 and p2p.ONOFF_DRAWS_DTYPE.itemsize == 16
    assert p2p.AMBIGUOUS_DRAW_DTYPE.itemsize == 32
    sc = RC.two_nodes("uniform")
    bad = two(p2p.Uniform(-1.0, 0.0, 0))
    s, x = bad.c_struct(), bad.c_ext()
    pl = p2p.Plan()
    with pytest.raises(nsgpu.NsgpuError, match="Uniform with min < 0"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan_ex(C.byref(s), C.byref(x), None, 0, 1, 0, C.byref(pl)))
    x.size = 24  # (the record before the variables were appended: they are not looked at)
    nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan_ex(C.byref(s), C.byref(x), None, 0, 1, 0, C.byref(pl)))
    assert sc.c_ext() is not None and p2p.first_cc().c_ext() is None
    # a trace client through the short record, and with a random OnOff beside it through the long one
    import udp_trace_cases as UT
    tsc = UT.known_answer()
    s, x = tsc.c_struct(), tsc.c_ext()
    assert isinstance(x, p2p.ScenarioExt) and x.size == 24  # (a scenario without a variable travels in the short record)
    want = p2p.dist_plan(tsc, None, 0, 1)
    x.size = 24
    nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan_ex(C.byref(s), C.byref(x), None, 0, 1, 0, C.byref(pl)))
    assert pl.uid_init == want["uid_init"] and list(pl.lookahead)[:pl.n_kinds] == want["lookahead"]
    x.size = 16  # (not even the trace entries)
    with pytest.raises(nsgpu.NsgpuError, match="no trace entries"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan_ex(C.byref(s), C.byref(x), None, 0, 1, 0, C.byref(pl)))


def test_null_arrays_and_constant_entries_mean_the_constants():
    """A scenario whose variables are all Constant builds no extension record at all: add_onoff folds a Constant into
    on_s / off_s, and beside a random variable the other one's entry is NSGPU_RV_CONSTANT with no value of its own
    (the library reads app_on_s / app_off_s for it; tests/test_gpu_ranvar.py's grid runs such entries)."""
    a = RC.two_nodes("uniform")
    a.apps.pop()
    a.setup.pop(-2)  # (the application's setup entry: Simulator::Stop's is the last)
    a.add_onoff(0, 1, 1_000_000, 0, on_var=p2p.Constant(0.002), off_var=p2p.Constant(0.001))
    assert a.c_ext() is None and a.apps[1]["on_var"] is None and a.apps[1]["off_var"] is None
    s = a.c_struct()
    assert s._keep["app_on_s"].tolist() == [0.0, 0.002] and s._keep["app_off_s"].tolist() == [0.0, 0.001]
    plan(a)
    b = RC.grid4()
    x = b.c_ext()
    on, off = x._keep[2], x._keep[3]
    first = next(i for i, A in enumerate(b.apps) if A["kind"] == p2p.APP_ONOFF)
    assert (on[first]["kind"], on[first]["p0"], off[first]["kind"]) == (p2p.RV_CONSTANT, 0.0, p2p.RV_UNIFORM)
    assert b.c_struct()._keep["app_on_s"][first] == 0.004
    with pytest.raises(TypeError):
        a.add_onoff(0, 1, 0, 0, on_var=0.5)


def test_lookaheads_do_not_depend_on_the_variables():
    sc = RC.two_nodes("exp")
    want = plan(sc)
    sc.apps[1]["on_var"] = sc.apps[1]["off_var"] = None
    assert plan(sc) == want


# ---------------- the conditions on the GPU tests' inputs ----------------
@pytest.mark.parametrize("name,args", RC.CASES)
def test_no_case_has_an_ambiguous_draw(name, args):
    """The GPU tests compare everything exactly, which holds only where the model (math.log) and the engine (the
    double-double log) must agree: no attempt of any case may be ambiguous.  A later edit of the cases cannot slip one
    in."""
    sc, m = run(name, *args)
    assert len(m["ambiguous"]) == 0 and not m["draws"]["ambiguous"].any()
    assert m["draws"]["on_draws"].sum() + m["draws"]["off_draws"].sum() > 30


def test_two_nodes_conditions():
    """Several hundred transitions; bursts cut by a random stop (a send cancelled while running: residual bits); on
    times shorter than the first packet's interval; the bounded variables redraw."""
    for kind in ("uniform", "exp", "bounded"):
        sc, m = run("two_nodes", kind)
        d = m["draws"][1]
        assert d["on_draws"] + d["off_draws"] >= 380
        assert d["off_draws"] - d["on_draws"] in (0, 1)
        assert m["stats"]["cancelled"] >= 150  # (cancelled sends are dispatched too)
        assert 0 < m["appc"]["rx_packets"][0] <= m["appc"]["tx_packets"][1]
    on, off = run("two_nodes", "bounded")[1]["model"].var[1]
    assert on.attempts > on.draws and off.attempts > 2 * off.draws
    on, _off = run("two_nodes", "exp")[1]["model"].var[1]
    assert on.attempts == on.draws
    # the three kinds are three different runs
    assert len({run("two_nodes", k)[1]["stats"]["digest"] for k in ("uniform", "exp", "bounded")}) == 3


def test_stops_conditions():
    sc, m = run("stops")
    mod = m["model"]
    assert m["appc"]["tx_bytes"][1] == 30_000 and mod.app[1]["tot"] >= sc.apps[1]["maxb"]
    assert mod.on_at_stop == {1: False, 2: True}  # (1: from its own last SendPacket; 2: Stop while a send is pending)
    # application 1 stopped itself in a burst: the StopSending it had scheduled was cancelled with it, and nothing was
    # drawn after: one on draw for every off draw
    assert m["draws"]["on_draws"][1] == m["draws"]["off_draws"][1] > 3
    assert m["draws"]["on_draws"][2] == m["draws"]["off_draws"][2] > 3
    assert m["appc"]["tx_packets"][2] > 100 and m["log"][0][-2] < 310_000_000  # (silent soon after the Stop at 300 ms)


def test_grid4_conditions():
    sc, m = run("grid4")
    d = m["draws"]
    onoff = [a for a, A in enumerate(sc.apps) if A["kind"] == p2p.APP_ONOFF]
    assert len(onoff) == 6
    for a in onoff:
        A = sc.apps[a]
        assert (d["on_draws"][a] > 0) == (A["on_var"] is not None) and (d["off_draws"][a] > 0) == (A["off_var"] is not None)
        assert m["appc"]["tx_packets"][a] > 0
    kinds = {(A["on_var"].kind if A["on_var"] else 0, A["off_var"].kind if A["off_var"] else 0)
             for A in (sc.apps[a] for a in onoff)}
    assert len(kinds) == 6
    assert 0 < m["em"]["corrupted"].sum() < m["em"]["invoked"].sum()
    assert m["servers"]["received"].sum() > 100 and m["servers"]["lost"].sum() > 0
    assert p2p.dist_plan(sc, None, 0, 1)["wide"] == 1
    own = p2p.owner_blocks(sc.n_nodes, 2)
    assert len({int(own[sc.apps[a]["node"]]) for a in onoff}) == 2  # (both ranks own drawing applications)
    mon = run("grid4", True)[1]
    assert mon["stats"] == m["stats"] and len(mon["flows"][next(iter(mon["flows"]))]) == 7
