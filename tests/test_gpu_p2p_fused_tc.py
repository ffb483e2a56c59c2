"""The holder's fused TransmitComplete (nsgpu_p2p_win.h, handle_node2): a local record that is
its node's next event and finds its device's queue empty is run where it is made (its slot's counts and busy = 0)
instead of going through the lane's queue and a second trip round the holder's loop.  What can go wrong is a
condition of the fused step that lets through a record another event should have preceded: an event of the node
between, one at the record's ts, a second busy device, a packet queued behind it, a leaf waiting for its ts group's
end.  Every scenario (tests/fused_tc_cases.py; tests/test_p2p_fused_tc_cpu.py asserts that none is vacuous) aims at
one of them, and every case compares the full (ts, uid, context) pop log, the device and application counters, the
stats fields and the digest with the oracle, bit for bit; traced cases compare the trace records too."""
import numpy as np
import pytest

import fused_tc_cases as FC
import nsgpu
import p2p
import p2p_errmodel_pyref
import trace
from p2p_model_compare import assert_equals_model
from test_gpu_mixed import run_oracle
from test_gpu_p2p_partials import assert_same_untraced
from test_gpu_trace import assert_same_run, oracle_full

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
LOG = 40_000
SOME = ("alone", "equal_ts", "queued_behind")  # cases 1, 3 and 5
_cache = {}


def scenario(name):
    """(scenario, the oracle's run with every trace sink recorded), computed once and never modified."""
    if name not in _cache:
        sc = getattr(FC, name)()
        o = oracle_full(sc, LOG, kinds=ALL_KINDS)
        assert 0 < o[0].dispatched <= LOG  # (the whole pop log is compared)
        _cache[name] = (sc, o)
    return _cache[name]


def run_untraced(sc, o, want_wide, runs=1):
    eng = p2p.Engine(sc, log_cap=LOG)
    assert eng.wide() == want_wide
    gst = None
    for _ in range(runs):
        g = eng.run(log_n=LOG)
        assert_same_untraced(o, g)
        gst = g[0]
    eng.close()
    return gst


@pytest.mark.parametrize("name", FC.CASES)
def test_wide_deferred_engine(name):
    sc, o = scenario(name)
    gst = run_untraced(sc, o, want_wide=True)
    if name == "start_burst":
        assert gst.refits > 0  # (a sorted run happened)


@pytest.mark.parametrize("name", SOME)
def test_same_engine_twice(name):
    sc, o = scenario(name)
    run_untraced(sc, o, want_wide=True, runs=2)


@pytest.mark.parametrize("name", SOME)
def test_traced(name):
    """set_trace runs the scanning pipeline, k2_handle<true, false, false>; a fused TransmitComplete makes no trace
    record, a queued one that starts a transmission makes its Dequeue."""
    sc, o = scenario(name)
    eng = p2p.Engine(sc, log_cap=LOG)
    eng.set_trace(len(o[4]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(log_n=LOG)
    assert_same_run(sc, o, (st, devc, appc, log, trace.sort_records(eng.trace())))
    eng.close()


@pytest.mark.parametrize("name", SOME)
def test_narrow_kernel(name, monkeypatch):
    """The narrow engine makes no local record: it stays as it was."""
    sc, o = scenario(name)
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    run_untraced(sc, o, want_wide=False)


@pytest.mark.parametrize("name", SOME)
def test_two_loopback_ranks(name):
    """The partitioned instantiation, k2_handle<true, true, false>."""
    sc, o = scenario(name)
    grp = p2p.LoopbackGroup(sc, 2, log_cap=LOG)
    assert_same_untraced(o, grp.run(log_n=LOG))


def test_host_closures_cut_windows():
    """Case 3 with a host probe every 5.3 ms (test_gpu_p2p_partials' harness): each pauses the deferred pipeline and
    cuts a window short, and injects a Send of the column flow out of step with the flow's own."""
    sc = FC.equal_ts()
    app_send = FC.onoffs(sc)[0]
    app_obs = [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_SINK][0]
    t0, period, count = 150_000_000, 5_300_001, 30
    st, devc, appc, olog, _otr, osamp = run_oracle(sc, t0, period, count, app_send, app_obs, LOG)
    assert st.dispatched <= LOG
    eng = p2p.Engine(sc, log_cap=LOG)
    assert eng.wide()
    eng.reset()
    sim = nsgpu.Sim()
    sim.attach_p2p(eng)
    sim.set_log(LOG)
    samples = []

    def probe():
        samples.append(eng.counters()[1][app_obs].copy())
        sim.p2p_send(app_send)
        if len(samples) < count:
            sim.schedule(period, probe)

    sim.schedule(t0, probe)
    sim.run()
    gst, gdevc, gappc, (lts, luid, lctx) = eng.results(log_n=LOG)
    host_n, _host_c, host_d = sim.host_stats()
    assert host_n == count
    m = sim.log[1] != 0  # (the host dispatches' ranks)
    lts, luid, lctx = lts.copy(), luid.copy(), lctx.copy()
    lts[m], luid[m], lctx[m] = sim.log[0][m], sim.log[1][m], sim.log[2][m]
    assert sim.dispatched() == st.dispatched
    assert (int(gst.digest) + host_d) & ((1 << 64) - 1) == st.digest
    assert sim.next_uid() == st.next_uid
    assert np.array_equal(gdevc, devc)
    assert np.array_equal(gappc, appc)
    n = int(min(st.dispatched, len(olog[0])))
    for a, b, name in zip((lts, luid, lctx), olog, ("ts", "uid", "ctx")):
        assert np.array_equal(a[:n], b[:n]), name
    gsamp = np.array(samples)
    assert len(gsamp) == len(osamp)
    for f in ("tx_packets", "rx_packets", "tx_bytes", "rx_bytes"):
        assert np.array_equal(gsamp[f], osamp[f]), f


def test_ports_instantiation_with_a_lossless_error_model():
    """k2_handle<..., PORTS = true>: case 5 with UDP ports on the device and, on the congested link's receiving device,
    a ReceiveListErrorModel with an empty list (it corrupts nothing), against the Python model (the oracle has no
    ports) and, since nothing is lost, against the oracle's pop log of the plain scenario as well."""
    sc = FC.queued_behind()
    sc.ports = True
    down = [d for d, r in enumerate(sc.dev) if r[0] == FC.CROSS and sc.dev[r[1]][0] == FC.CROSS + FC.COLS][0]
    sc.set_receive_list_error_model(sc.dev[down][1], [])
    m = p2p_errmodel_pyref.run(sc, ALL_KINDS)
    n = m["stats"]["dispatched"]
    _plain, o = scenario("queued_behind")
    assert n == o[0].dispatched
    eng = p2p.Engine(sc, log_cap=n)
    assert eng.wide()
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models())
    for a, b, name in zip(log, o[3], ("ts", "uid", "ctx")):
        assert np.array_equal(a[:n], b[:n]), name
    eng.close()
