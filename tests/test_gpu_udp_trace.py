"""UdpTraceClient on the GPU engine, each run compared with the Python model (tests/p2p_trace_client_pyref.py, pinned
by tests/test_udp_trace_cpu.py, which also asserts that the scenarios here contain what their names say): digest,
dispatch count, next uid, the full pop log, device and application counters, UdpServer records, trace_clients () and
the sorted trace records."""
import numpy as np
import pytest

import p2p
import p2p_pyref
import p2p_trace_client_pyref as T
import trace
import udp_ports_cases
import udp_trace_cases as U

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
TRACE_FIELDS = ("ts", "uid", "seq", "kind", "dev", "app", "ipid", "size", "ttl")
_models = {}


def model(name, *args, monitored=False):
    """The model's run of scenario U.<name> (*args), computed once."""
    key = (name, args, monitored)
    if key not in _models:
        sc = getattr(U, name)(*args)
        _models[key] = (sc, (T.run_monitored if monitored else T.run)(sc, ALL_KINDS))
    return _models[key]


def assert_equals_model(m, st, devc, appc, log, servers, clients, tr=None):
    for k, v in m["stats"].items():
        assert int(getattr(st, k)) == v, k
    for name, a, b in zip(("ts", "uid", "ctx"), log, m["log"]):
        assert np.array_equal(a, b), "log " + name
    assert np.array_equal(devc, m["devc"])
    assert np.array_equal(appc, m["appc"])
    for f in ("received", "lost", "last_max_seq"):
        assert np.array_equal(servers[f], m["servers"][f]), f
    if clients is not None:
        for f in ("sent", "current_entry", "sends"):
            assert np.array_equal(clients[f], m["clients"][f]), f
    if tr is not None:
        tr, want = trace.sort_records(tr), trace.sort_records(m["trace"])
        assert len(tr) == len(want)
        for f in TRACE_FIELDS:
            assert np.array_equal(tr[f], want[f]), "trace " + f


def run_traced(sc, m):
    """A traced single engine (the scanning pipeline) against the model, trace records included."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.trace_clients(), eng.trace())
    return eng


def run_untraced(sc, m, want_wide=None):
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    if want_wide is not None:
        assert eng.wide() == want_wide
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.trace_clients())
    return eng


def both(name, *args):
    sc, m = model(name, *args)
    run_traced(sc, m).close()
    run_untraced(sc, m).close()
    return m


def test_known_answer_247_received_0_lost():
    m = both("known_answer")
    srv = m["servers"][0]
    assert (int(srv["received"]), int(srv["lost"])) == (247, 0)


def test_burst_overflows_the_senders_queue():
    m = both("overflow")
    assert m["devc"]["drop_packets"][0] > 0 and m["servers"]["lost"][0] > 0


def test_forwarded_and_ttl_expiry_with_icmp():
    m = both("forwarded_ttl")
    assert m["stats"]["ttl_drops"] > 0 and m["stats"]["icmp_sent"] == m["stats"]["ttl_drops"]


def test_wrong_remote_port_with_icmp():
    m = both("wrong_port")
    assert m["stats"]["unreach_drops"] > 0 and m["stats"]["icmp_sent"] == m["stats"]["unreach_drops"]


def test_exact_multiple_and_tiny_frames():
    m = both("exact_and_tiny")
    # the 12-byte datagrams on the wire: 12 + 8 + 20 + 2 bytes
    enq = m["trace"][m["trace"]["kind"] == p2p_pyref.TR_ENQUEUE]
    assert np.count_nonzero(enq["size"] == 42) == m["tc_diag"]["header_only"] > 0


def test_stop_in_mid_cycle():
    m = both("stop_mid_cycle")
    assert m["stats"]["cancelled"] == 1


def test_no_route():
    m = both("no_route")
    assert int(m["clients"]["sent"][2]) == 0 and int(m["clients"]["sends"][2]) > 1


def test_every_pipeline():
    sc, m = model("grid_pipelines")
    run_untraced(sc, m, want_wide=True).close()  # the default engine: deferred, wide windows
    run_traced(sc, m).close()                    # the scanning pipeline
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, 2, log_cap=n, trace_cap=len(m["trace"]) + 64, trace_kinds=ALL_KINDS)
    st, devc, appc, log = grp.run(n)
    assert_equals_model(m, st, devc, appc, log, grp.udp_servers(), grp.trace_clients(), grp.trace())


def test_hub_forwards_bursts():
    sc, m = model("hub_forwards_bursts")
    run_untraced(sc, m).close()
    run_traced(sc, m).close()


def test_hub_hosts_the_client():
    sc, m = model("hub_hosts_client")
    run_untraced(sc, m).close()
    run_traced(sc, m).close()


@pytest.mark.parametrize("name", ["known_answer", "overflow"])
def test_flowmon(name):
    """flow_stats () equals the model's: the varying datagram sizes in the byte sums, the queue drops by reason; the
    run itself is the unmonitored one."""
    sc, m = model(name, True, monitored=True)
    _sc0, m0 = model(name)
    assert m["stats"] == m0["stats"]
    eng = run_untraced(sc, m)
    got, want = eng.flow_stats(), m["flows"][p2p.MAX_PER_HOP_DELAY_NS]
    assert len(got) == len(want) == 1
    for f in p2p.FLOW_STATS_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f
    eng.close()
    if name == "overflow":
        assert int(want["packets_dropped"][0][p2p.FLOW_DROP_QUEUE]) > 0
        assert int(want["tx_bytes"][0]) == int(m["appc"]["tx_bytes"][1]) + 28 * int(want["tx_packets"][0])


def test_rate_error_model_by_each_datagrams_own_size():
    sc, m = model("rate_error_model", monitored=True)
    eng = run_traced(sc, m)
    em = eng.error_models()
    assert np.array_equal(em, m["em"]) and int(em["corrupted"][1]) > 0
    eng.close()
    run_untraced(sc, m).close()


def test_extended_handlers_without_a_trace_client_are_unchanged():
    """A scenario without a trace client on the extended handlers: the log and digest the model without the new kind
    computes (recomputed here, not stored)."""
    sc = udp_ports_cases.grid_pipelines()
    m = p2p_pyref.run(sc, ALL_KINDS)
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    st, devc, appc, log = eng.run(n)
    for k, v in m["stats"].items():
        assert int(getattr(st, k)) == v, k
    for a, b in zip(log, m["log"]):
        assert np.array_equal(a, b)
    assert np.array_equal(devc, m["devc"]) and np.array_equal(appc, m["appc"])
    assert not eng.trace_clients()["sends"].any()
    eng.close()
