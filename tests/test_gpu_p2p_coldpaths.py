"""The handlers' out-of-line paths (nsgpu_p2p_dev.h "cold paths"): k2_handle inlines only the
node parts of a TransmitComplete, a forwarded Receive and a PacketSink delivery; every other kind, the trace records, the
compressed route table and the window scan of a crowded node are functions it calls, which read a device-resident
copy of the engine descriptor.  What can go wrong is a call made from a wave whose other lanes stay on the inlined
path: state handed across the call comes back wrong, or side effects land in another order.  So every scenario
(tests/coldpaths_cases.py; tests/test_p2p_coldpaths_cpu.py asserts that none is vacuous) is small enough that one or
two holder waves hold a window and mixes both kinds of lanes in it, and every case compares the full (ts, uid, context)
pop log, the device and application counters, the stats fields and the digest with the oracle, bit for bit; traced
cases compare the trace records too."""
import pytest

import coldpaths_cases as CC
import nsgpu
import p2p
import p2p_errmodel_pyref
import trace
from p2p_model_compare import assert_equals_model
from test_gpu_p2p_partials import assert_same_untraced
from test_gpu_trace import assert_same_run, oracle_full

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
LOG = 40_000
_cache = {}


def scenario(name, *args):
    """(scenario, the oracle's run with every trace sink recorded), computed once and never modified."""
    if (name, args) not in _cache:
        sc = getattr(CC, name)(*args)
        o = oracle_full(sc, LOG, kinds=ALL_KINDS)
        assert 0 < o[0].dispatched <= LOG  # (the whole pop log is compared)
        _cache[(name, args)] = (sc, o)
    return _cache[(name, args)]


def run_untraced(sc, o, want_wide=None, runs=1):
    eng = p2p.Engine(sc, log_cap=LOG)
    if want_wide is not None:
        assert eng.wide() == want_wide
    for _ in range(runs):
        assert_same_untraced(o, eng.run(log_n=LOG))
    eng.close()


def run_traced(sc, o):
    eng = p2p.Engine(sc, log_cap=LOG)
    eng.set_trace(len(o[4]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(log_n=LOG)
    assert_same_run(sc, o, (st, devc, appc, log, trace.sort_records(eng.trace())))
    eng.close()


def test_mixed_kinds_wide_deferred_engine():
    sc, o = scenario("mixed")
    assert sc.stop_ns <= 600_000_000
    run_untraced(sc, o, want_wide=True)


def test_mixed_kinds_same_engine_twice():
    sc, o = scenario("mixed")
    run_untraced(sc, o, want_wide=True, runs=2)


def test_mixed_kinds_traced():
    """set_trace runs the scanning pipeline, k2_handle<true, false, false>, and every trace record is an out-of-line
    call."""
    sc, o = scenario("mixed")
    run_traced(sc, o)


def test_tracing_turned_on_after_an_untraced_run():
    """The device-resident descriptor follows the host's: the first run equals the oracle untraced, the second, after
    set_trace on the same engine, equals it traced (a stale copy would hold a null trace buffer)."""
    sc, o = scenario("mixed")
    eng = p2p.Engine(sc, log_cap=LOG)
    assert_same_untraced(o, eng.run(log_n=LOG))
    eng.set_trace(len(o[4]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(log_n=LOG)
    assert_same_run(sc, o, (st, devc, appc, log, trace.sort_records(eng.trace())))
    eng.close()


def test_trace_kinds_changed_between_runs():
    """nsgpu_p2p_set_trace_kinds alone changes a descriptor field too: device sinks first, then every sink."""
    sc, o = scenario("mixed")
    odev = oracle_full(sc, LOG)
    eng = p2p.Engine(sc, log_cap=LOG)
    eng.set_trace(len(o[4]) + 64)
    st, devc, appc, log = eng.run(log_n=LOG)
    assert_same_run(sc, odev, (st, devc, appc, log, trace.sort_records(eng.trace())))
    nsgpu.check(nsgpu.lib().nsgpu_p2p_set_trace_kinds(eng.h, ALL_KINDS))
    st, devc, appc, log = eng.run(log_n=LOG)
    assert_same_run(sc, o, (st, devc, appc, log, trace.sort_records(eng.trace())))
    eng.close()


def test_mixed_kinds_narrow_kernel(monkeypatch):
    """The narrow kernel keeps the whole node part inline (the dumbbell lost with the split) and calls the trace,
    route and window-scan functions."""
    sc, o = scenario("mixed")
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    run_untraced(sc, o, want_wide=False)


@pytest.mark.parametrize("icmp", [False, True])
def test_no_route(icmp):
    sc, o = scenario("no_route", icmp)
    assert o[0].no_route_drops > 0
    run_untraced(sc, o)
    run_traced(sc, o)


def test_more_than_nslot_events_on_one_node():
    sc, o = scenario("crowded_node")
    run_untraced(sc, o, want_wide=False)


def test_star_with_echo_through_the_hub():
    """hub_node's serial node parts call the shared out-of-line functions."""
    sc, o = scenario("star_with_echo")
    run_untraced(sc, o, want_wide=True)
    run_traced(sc, o)


def test_star_with_echo_narrow(monkeypatch):
    sc, o = scenario("star_with_echo")
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    run_untraced(sc, o, want_wide=False)


def test_extended_handlers():
    """k2_handle<..., PORTS = true> through the same functions, against the Python model (the oracle has no ports):
    untraced, then traced."""
    sc = CC.extended()
    m = p2p_errmodel_pyref.run(sc, ALL_KINDS)
    n = m["stats"]["dispatched"]
    for traced in (False, True):
        eng = p2p.Engine(sc, log_cap=n)
        if traced:
            eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
        st, devc, appc, log = eng.run(n)
        assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(),
                            eng.trace() if traced else None)
        eng.close()


def test_two_loopback_ranks():
    """The partitioned instantiation, k2_handle<true, true, false>."""
    sc, o = scenario("mixed")
    grp = p2p.LoopbackGroup(sc, 2, log_cap=LOG)
    assert_same_untraced(o, grp.run(log_n=LOG))
