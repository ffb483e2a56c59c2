"""UDP ports, several endpoints a node, UdpClient and UdpServer on the GPU engine, each run compared with the Python
model of the p2p subset (tests/p2p_pyref.py, itself pinned to the oracle by tests/test_udp_ports_cpu.py, which also
asserts that the scenarios here are not vacuous): digest, dispatch count, next uid, the full pop log, device and
application counters, UdpServer records and the sorted trace records."""
import numpy as np
import pytest

import nsgpu
import p2p
import p2p_pyref
import trace
import udp_ports_cases as U

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
TRACE_FIELDS = ("ts", "uid", "seq", "kind", "dev", "app", "ipid", "size", "ttl")
_models = {}


def model(name, *args):
    """The model's run of scenario U.<name> (*args), computed once."""
    if (name, args) not in _models:
        sc = getattr(U, name)(*args)
        _models[(name, args)] = (sc, p2p_pyref.run(sc, ALL_KINDS))
    return _models[(name, args)]


def assert_equals_model(m, st, devc, appc, log, servers, tr=None):
    for k, v in m["stats"].items():
        assert int(getattr(st, k)) == v, k
    for name, a, b in zip(("ts", "uid", "ctx"), log, m["log"]):
        assert np.array_equal(a, b), "log " + name
    assert np.array_equal(devc, m["devc"])
    assert np.array_equal(appc, m["appc"])
    for f in ("received", "lost", "last_max_seq"):
        assert np.array_equal(servers[f], m["servers"][f]), f
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
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.trace())
    eng.close()
    return st


def run_untraced(sc, m, want_wide=None):
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    if want_wide is not None:
        assert eng.wide() == want_wide
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers())
    eng.close()


def test_udp_client_server():
    """UdpClientServerTestCase with the real kinds: received 8, lost 0."""
    sc, m = model("udp_client_server")
    run_traced(sc, m)
    run_untraced(sc, m)
    assert tuple(m["servers"][0])[:2] == (8, 0)


def test_three_endpoints_on_one_node():
    sc, m = model("three_endpoints")
    run_traced(sc, m)
    run_untraced(sc, m)


@pytest.mark.parametrize("icmp", [False, True])
def test_port_mismatch(icmp):
    sc, m = model("port_mismatch", icmp)
    st = run_traced(sc, m)
    run_untraced(sc, m)
    assert st.unreach_drops == 6 and st.icmp_sent == (6 if icmp else 0)


@pytest.mark.parametrize("window", [8, 32])
def test_loss_and_reordering(window):
    sc, m = model("loss_reorder", window)
    run_traced(sc, m)
    run_untraced(sc, m)


def test_stopped_server_and_client_without_route():
    sc, m = model("stopped_server_no_route")
    run_traced(sc, m)
    run_untraced(sc, m)


def test_every_pipeline():
    sc, m = model("grid_pipelines")
    run_untraced(sc, m, want_wide=True)  # the default engine: deferred, wide windows
    run_traced(sc, m)                    # the scanning pipeline
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, 2, log_cap=n, trace_cap=len(m["trace"]) + 64, trace_kinds=ALL_KINDS)
    st, devc, appc, log = grp.run(n)
    assert_equals_model(m, st, devc, appc, log, grp.udp_servers(), grp.trace())


def test_hub_blocks():
    sc, m = model("incast_hub")
    run_untraced(sc, m)
    run_traced(sc, m)


def test_icmp_errors_back_to_a_node_with_two_endpoints():
    """Port-unreachable and time-exceeded errors delivered to a sender that hosts two bound endpoints."""
    sc, m = model("icmp_back_to_endpoints")
    run_traced(sc, m)
    run_untraced(sc, m)
    grp = p2p.LoopbackGroup(sc, 2, log_cap=m["stats"]["dispatched"])
    st, devc, appc, log = grp.run(m["stats"]["dispatched"])
    assert_equals_model(m, st, devc, appc, log, grp.udp_servers())


def test_hub_forwards_sequence_numbered_datagrams():
    """The hub blocks' stateless forwarders with UdpClient datagrams, one flow's TTL expiring at the hub."""
    sc, m = model("hub_forwarding")
    run_traced(sc, m)
    run_untraced(sc, m, want_wide=False)


@pytest.mark.parametrize("build", [lambda: p2p.grid(8, 8), lambda: p2p.dumbbell(16)], ids=["grid8x8", "dumbbell16"])
def test_ports_equal_legacy_where_both_apply(build):
    res = []
    for ports in (False, True):
        sc = build()
        sc.ports = ports
        eng = p2p.Engine(sc, log_cap=1 << 17)
        st, devc, appc, log = eng.run(1 << 17)
        assert st.dispatched <= 1 << 17 and st.dispatched > 100
        res.append((p2p.stats_to_dict(st), devc, appc, log))
        eng.close()
    (s0, d0, a0, l0), (s1, d1, a1, l1) = res
    for k in ("dispatched", "digest", "next_uid", "final_ts", "cancelled", "unreach_drops"):
        assert s0[k] == s1[k], k
    assert np.array_equal(d0, d1) and np.array_equal(a0, a1)
    assert all(np.array_equal(x, y) for x, y in zip(l0, l1))


# ---------------- PacketLossCounter in its one-thread kernel ----------------
def test_loss_counter_known_answers_kernel():
    window, seq, cp, want = U.loss_counter_kat()
    dev = U.library_losses(window, seq, on_device=True)
    assert [int(dev[i]) for i in cp] == want
    assert np.array_equal(dev, U.library_losses(window, seq, on_device=False))


@pytest.mark.parametrize("window", [8, 32, 256])
def test_loss_counter_random_sequences_kernel(window):
    seq = U.random_sequences(window, window)
    c = p2p_pyref.PacketLossCounter(window)
    lit = []
    for s in seq:
        c.notify_received(int(s))
        lit.append(c.m_lost)
    # (the limit only keeps a runaway loop from passing: a loop of the gap's length over 10^6 is ~0.1 s in one thread and
    # would not trip it.  What pins the bounded loop is the host test with the 4 x 10^9 gap, tests/test_udp_ports_cpu.py:
    # the host and the kernel run one NSGPU_HD function)
    dev = U.library_losses(window, seq, on_device=True, limit_s=2.0)
    assert np.array_equal(dev, np.array(lit, np.uint32))
    assert np.array_equal(dev, U.library_losses(window, seq, on_device=False))


# ---------------- nsgpu_p2p_create's refusals (each message: tests/test_udp_ports_cpu.py, through the host-only plan) ----------------
def test_create_refuses_and_accepts():
    def refused(sc):
        sc.route_bfs()
        with pytest.raises(nsgpu.NsgpuError) as e:
            p2p.Engine(sc)
        return str(e.value)

    sc = U.line(2, [(5_000_000, 2 * U.MS)])
    sc.ports = False
    sc.add_sink(1, 0, 0, port=9)
    sc.add_echo_server(1, 0, 0, port=7)
    assert "node 1 has two bound endpoints" in refused(sc)
    sc = U.line(2, [(5_000_000, 2 * U.MS)])
    sc.ports = False
    sc.add_udp_server(1, 0, 0)
    assert "UdpClient / UdpServer need UDP ports" in refused(sc)
    sc = U.line(2, [(5_000_000, 2 * U.MS)])
    sc.add_sink(1, 0, 0, port=9)
    sc.add_udp_server(1, 0, 0, port=9)
    assert "two applications bound to port 9" in refused(sc)
    # a port 50000 sink on a node without a sender stays legal (p2p.dumbbell's)
    sc = U.line(2, [(5_000_000, 2 * U.MS)])
    sc.add_sink(1, 0, 0, port=50000)
    sc.add_onoff(0, 1, 0, 0, remote_port=50000)
    sc.route_bfs()
    p2p.Engine(sc).close()
