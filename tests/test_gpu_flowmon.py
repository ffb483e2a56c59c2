"""Per-flow statistics (FlowMonitor's FlowStats, accumulated on the device) on the GPU engine, each run compared with
the Python model (tests/p2p_flowmon_pyref.py, pinned by tests/test_flowmon_cpu.py, which also asserts that the
scenarios here are not vacuous): the full existing result set — digest, counts, the pop log, device and application
counters, UdpServer and error-model records, the sorted trace records — and the flow records field by field, for the
reference's 10 s MaxPerHopDelay and for 1 ms.  Everything is integer state: no tolerances."""
import ctypes as C

import numpy as np
import pytest

import flowmon_cases as FMC
import nsgpu
import p2p
import p2p_flowmon_pyref as FM
from p2p_model_compare import assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
DELAYS = (FM.MAX_PER_HOP_DELAY_NS, FMC.SMALL_DELAY_NS)
_models = {}


def model(name, *args):
    """The model's run of scenario FMC.<name> (*args), computed once."""
    if (name, args) not in _models:
        sc = getattr(FMC, name)(*args)
        _models[(name, args)] = (sc, FM.run(sc, ALL_KINDS, DELAYS))
    return _models[(name, args)]


def assert_flows(eng, m, label=""):
    """Engine.flow_stats against the model for both delays, asked twice in alternation: the sweep changes nothing."""
    for d in DELAYS + DELAYS:
        got, want = eng.flow_stats(d), m["flows"][d]
        assert len(got) == len(want), "flows (max_delay %d) %s" % (d, label)
        for f in p2p.FLOW_STATS_DTYPE.names:
            assert np.array_equal(got[f], want[f]), "%s (max_delay %d) %s: %s != %s" % (f, d, label, got[f], want[f])
    assert np.array_equal(eng.flow_stats(), m["flows"][FM.MAX_PER_HOP_DELAY_NS])  # (the default: 10 s)


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
        assert_flows(eng, m, label)
    eng.close()
    return st


@pytest.mark.parametrize("name,args", FMC.GPU_CASES)
def test_flow_stats_equal_the_model(name, args):
    """first.cc, the chain, incast (3) with queue drops at the senders, the mixed 4-leaf dumbbell in ports mode, the
    3x3 grid with a TTL expiry and a missing route (icmp off and on), the chain with two error models: untraced (the
    default pipeline of a monitored engine) and traced."""
    sc, m = model(name, *args)
    run_engine(sc, m)
    run_engine(sc, m, traced=True)


def test_wide_against_narrow_windows(monkeypatch):
    """The dumbbell and the icmp-less grid are granted wide windows; NSGPU_P2P_NARROW=1 runs the same scenarios
    through the narrow kernels.  Both equal the model."""
    for name, args in (("dumbbell4", ()), ("grid3", (False,)), ("incast3", ()), ("star15", ())):
        sc, m = model(name, *args)
        run_engine(sc, m, want_wide=True)
        monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
        run_engine(sc, m, want_wide=False, label="narrow")
        run_engine(sc, m, traced=True, want_wide=False, label="narrow traced")
        monkeypatch.delenv("NSGPU_P2P_NARROW")


def test_second_launch_after_reset_equals_the_first():
    for name, args in (("dumbbell4", ()), ("chain_errmodel", ()), ("grid3", (True,))):
        sc, m = model(name, *args)
        run_engine(sc, m, again=True)


def test_fuzz_seeds_with_the_monitor_on():
    """The seeds of p2p_fuzz_cases' mesh that draw no fragmenting flow, frag off and the monitor on (ports, icmp, error
    models, echo, OnOff and UdpClient flows at once); a seed with a fragmenting flow is left out, and at least half run."""
    ran = 0
    for seed in FMC.FUZZ_SEEDS:
        sc = FMC.fuzz(seed)
        if sc is None:
            continue
        m = FM.run(sc, ALL_KINDS, DELAYS)
        run_engine(sc, m, label="mesh %d" % seed)
        run_engine(sc, m, traced=True, label="mesh %d traced" % seed)
        ran += 1
    assert 2 * ran >= len(FMC.FUZZ_SEEDS)


@pytest.mark.parametrize("name,args", [("dumbbell4", ()), ("grid3", (True,)), ("chain_errmodel", ())])
def test_the_monitor_changes_nothing_else(name, args):
    """The same scenario with flowmon off and on: equal pop log, counters and digest; the unmonitored engine's flow
    records are all zeros."""
    sc, m = model(name, *args)
    n = m["stats"]["dispatched"]
    res = []
    for on in (False, True):
        sc.flowmon = on
        try:
            eng = p2p.Engine(sc, log_cap=n)
        finally:
            sc.flowmon = True
        st, devc, appc, log = eng.run(n)
        res.append((st.digest, st.dispatched, st.next_uid, devc, appc, log, eng.udp_servers(), eng.error_models()))
        if not on:
            raw = eng.flow_records()
            assert len(raw) == 2 * len(sc.apps) and not raw.view(np.uint8).any()
            assert len(eng.flow_stats(0)) == 0
        eng.close()
    off, on = res
    assert off[:3] == on[:3]
    for a, b in zip(off[3:5] + off[6:], on[3:5] + on[6:]):
        assert np.array_equal(a, b)
    for a, b in zip(off[5], on[5]):
        assert np.array_equal(a, b)


def test_identification_limit_is_an_error_return():
    """65,537 datagrams from one node: the 65,537th's identification is outside the node's table (the 16-bit
    identification would wrap): the run ends with the sticky NSGPU_ERANGE."""
    eng = p2p.Engine(FMC.id_limit(65537))
    with pytest.raises(nsgpu.NsgpuError, match="nsgpu error 5: nsgpu_p2p: a monitored node's IPv4 identification "
                                               "reached the size of its tracked-packet table"):  # (5: NSGPU_ERANGE)
        eng.run()
    with pytest.raises(nsgpu.NsgpuError, match="identification reached the size"):  # (sticky until the reset)
        eng.results()
    eng.close()


def test_one_datagram_below_the_identification_limit_runs_clean():
    eng = p2p.Engine(FMC.id_limit(65535))
    st, _devc, appc, _log = eng.run()
    (r,) = eng.flow_stats()
    assert r["tx_packets"] == r["rx_packets"] == 65535 == appc["tx_packets"][1]
    assert r["tx_bytes"] == 65535 * 40 and r["lost_packets"] == 0 and r["jitter_sum_ns"] == 0
    assert r["time_last_tx_ns"] == 1_000_000 + 65534 * 100
    eng.close()


def test_refusals_that_need_an_engine():
    eng = p2p.Engine(FMC.chain3(1))
    with pytest.raises(nsgpu.NsgpuError, match="nsgpu_p2p_flow_stats: negative max_delay_ns"):
        eng.flow_stats(-1)
    sim = nsgpu.Sim()
    with pytest.raises(nsgpu.NsgpuError, match="per-flow statistics \\(flowmon\\) cannot be attached to a host-closure "
                                               "runtime"):
        sim.attach_p2p(eng)
    eng.close()
    eng = p2p.Engine(FMC.incast3())  # (an OnOff flow: application 1)
    uid, seq = C.c_uint32(100), C.c_uint32(0)
    with pytest.raises(nsgpu.NsgpuError, match="nsgpu_p2p_inject_send: not available in a scenario with per-flow "
                                               "statistics"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_inject_send(eng.h, 1, 0, 4, 0, C.byref(uid), C.byref(seq), None))
    eng.close()
