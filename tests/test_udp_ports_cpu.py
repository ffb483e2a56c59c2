"""UDP ports, UdpClient and UdpServer on the CPU: the Python model of the p2p subset (tests/p2p_pyref.py) against
the oracle where the oracle applies, PacketLossCounter's known answers, and the conditions the GPU scenarios of
tests/test_gpu_udp_ports.py must meet so that none of them passes vacuously — asserted on the model alone."""
import numpy as np
import pytest

import nsgpu
import nsref
import p2p
import p2p_pyref
import reference_fixtures as RF
import udp_ports_cases as U

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS


def icmp_scenario():
    """icmp = 1 with TTL expiries (TTL 2 on a sparse 12-node topology) and datagrams to unbound nodes (sinks bound
    from 20 ms to 300 ms only)."""
    return p2p.random_topology(12, 13, 8, 2, icmp=True, ttl=2, sink_window=(20_000_000, 300_000_000))


ORACLE_SCENARIOS = {
    "first_cc": p2p.first_cc,
    "drop_tail_queue": RF.drop_tail_queue_scenario,
    "udp_client_server_echo": RF.udp_client_server_scenario,
    "grid3x3": lambda: p2p.grid(3, 3),
    "incast8": lambda: p2p.incast(8),
    "random1": lambda: p2p.random_topology(8, 10, 5, 1),
    "random7": lambda: p2p.random_topology(10, 14, 6, 7),
    "icmp": icmp_scenario,
}


def oracle_run(sc):
    s = sc.c_struct()
    st = p2p.P2PStats()
    devc = np.zeros(s.n_devices, p2p.DEV_COUNTERS_DTYPE)
    appc = np.zeros(s.n_apps, p2p.APP_COUNTERS_DTYPE)
    nsref.p2p_run(s, st, devc, appc, 0)
    _secs, log, tr = nsref.p2p_run_trace(s, st, devc, appc, int(st.dispatched), ALL_KINDS)
    return st, devc, appc, log, tr


def model_differences(sc, m):
    """What differs between the oracle's run of `sc` and the model's result m ([]: nothing)."""
    st, devc, appc, log, tr = oracle_run(sc)
    bad = [k for k, v in m["stats"].items() if int(getattr(st, k)) != v]
    if not np.array_equal(devc, m["devc"]):
        bad.append("devc")
    if not np.array_equal(appc, m["appc"]):
        bad.append("appc")
    for name, a, b in zip(("log_ts", "log_uid", "log_ctx"), log, m["log"]):
        if not np.array_equal(a, b):
            bad.append(name)
    if len(tr) != len(m["trace"]) or any(not np.array_equal(tr[f], m["trace"][f]) for f in tr.dtype.names):
        bad.append("trace")
    return bad


@pytest.mark.parametrize("name", sorted(ORACLE_SCENARIOS))
def test_model_equals_oracle(name):
    sc = ORACLE_SCENARIOS[name]()
    m = p2p_pyref.run(sc, ALL_KINDS)
    assert m["stats"]["dispatched"] > 0
    if name == "icmp":
        assert m["stats"]["ttl_drops"] > 0 and m["stats"]["unreach_drops"] > 0 and m["stats"]["icmp_sent"] > 0
        assert (m["trace"]["kind"] == 6).any()  # NSGPU_TR_IP_DROP
    assert model_differences(sc, m) == []


def test_nudged_model_is_caught():
    """The positive control: the echo client's next Send scheduled before its socket's device children."""
    sc = RF.udp_client_server_scenario()
    bad = model_differences(sc, p2p_pyref.run(sc, ALL_KINDS, nudge="send_before_children"))
    assert "log_uid" in bad and "digest" in bad


# ---------------- PacketLossCounter ----------------
def literal_losses(window, seq):
    c = p2p_pyref.PacketLossCounter(window)
    out = []
    for s in seq:
        c.notify_received(int(s))
        out.append(c.m_lost)
    return np.array(out, np.uint32)


def test_loss_counter_known_answers_host():
    window, seq, cp, want = U.loss_counter_kat()
    lit = literal_losses(window, seq)
    assert [int(lit[i]) for i in cp] == want
    host = U.library_losses(window, seq, on_device=False)
    assert [int(host[i]) for i in cp] == want
    assert np.array_equal(host, lit)


@pytest.mark.parametrize("window", [8, 32, 256])
def test_loss_counter_random_sequences_host(window):
    seq = U.random_sequences(window, window)
    gaps = np.diff(np.maximum.accumulate(seq.astype(np.int64)))
    assert gaps.max() == 1_000_000 and (seq[1:] < np.maximum.accumulate(seq)[:-1]).any()
    # (the time limit is sized for the bounded loop: at most `window` iterations a call)
    assert np.array_equal(U.library_losses(window, seq, on_device=False, limit_s=1.0), literal_losses(window, seq))


def test_loss_counter_huge_gap_host():
    """A gap of 4 x 10^9: the loop as written would run for seconds here; the bounded one runs `window` iterations.
    Closed form: after 5 on a fresh counter the bits of 1 .. 4 are clear, so the next `window` iterations count 4
    and the other gap - window one each."""
    window, gap = 32, 4_000_000_000
    got = U.library_losses(window, np.array([5, 5 + gap], np.uint64).astype(np.uint32), on_device=False, limit_s=0.5)
    assert got.tolist() == [0, 4 + gap - window]


# ---------------- the GPU scenarios are not vacuous ----------------
def test_conditions_udp_client_server():
    m = p2p_pyref.run(U.udp_client_server())
    assert tuple(m["servers"][0])[:2] == (8, 0)


def test_conditions_three_endpoints():
    sc = U.three_endpoints()
    m = p2p_pyref.run(sc)
    a = m["appc"]
    assert a["rx_packets"][0] == a["tx_packets"][3] > 0       # the sink: the OnOff flow alone
    assert a["rx_packets"][1] == a["tx_packets"][4] == 20      # the UdpServer: the UdpClient's
    assert a["rx_packets"][2] == a["tx_packets"][5] == 5 and a["rx_packets"][5] == 5   # the echo pair
    assert len({int(a["rx_bytes"][k] // a["rx_packets"][k]) for k in range(3)}) == 3   # three payload sizes
    assert m["stats"]["unreach_drops"] == 0


@pytest.mark.parametrize("icmp", [False, True])
def test_conditions_port_mismatch(icmp):
    m = p2p_pyref.run(U.port_mismatch(icmp), ALL_KINDS)
    assert m["stats"]["unreach_drops"] == 6 and m["servers"]["received"][0] == 6
    assert m["stats"]["icmp_sent"] == (6 if icmp else 0)
    if icmp:  # the errors are forwarded back; their offending TTL is the low byte (32 after one hop) whatever the
        # sequence number above it, which is non-zero for the later datagrams
        e = m["trace"][(m["trace"]["app"] & p2p_pyref.PKT_ICMP) != 0]
        assert len(e) and set((e["ttl"] >> 8) & 0xFF) == {32} and set(e["ttl"] & 0xFF) <= {64, 63}
        d = m["trace"][(m["trace"]["app"] == 2)]
        assert (d["ttl"] >> 8).max() == 5


@pytest.mark.parametrize("window", [8, 32])
def test_conditions_loss_reorder(window):
    m = p2p_pyref.run(U.loss_reorder(window))
    assert m["servers"]["lost"][0] > 0
    assert m["diag"]["reordered"] >= 1   # an arrival with seq < lastMaxSeq at the server two clients feed
    assert m["diag"]["wide_gaps"] >= 1   # a loss counted through the gap > window branch


def test_conditions_stopped_server_no_route():
    m = p2p_pyref.run(U.stopped_server_no_route())
    assert m["diag"]["after_stop"] >= 3 and m["diag"]["noroute_attempts_at_zero"] >= 3
    assert m["appc"]["tx_packets"][2] == 0 and m["stats"]["no_route_drops"] >= 3
    assert m["stats"]["unreach_drops"] == 0 and m["stats"]["icmp_sent"] == 0
    assert m["servers"]["received"][0] < m["appc"]["tx_packets"][1]


def test_conditions_icmp_back_to_endpoints():
    sc = U.icmp_back_to_endpoints()
    m = p2p_pyref.run(sc, ALL_KINDS)
    assert m["stats"]["unreach_drops"] == 5 and m["stats"]["ttl_drops"] == 4 and m["stats"]["icmp_sent"] == 9
    tr = m["trace"]
    # every error reaches node 0 (MacRx on its device 0), which hosts two bound endpoints and the senders
    back = tr[(tr["kind"] == p2p_pyref.TR_RX) & (tr["dev"] == 0) & ((tr["app"] & p2p_pyref.PKT_ICMP) != 0)]
    assert len(back) == 9 and (back["app"] & p2p_pyref.PKT_ICMP_UNREACH != 0).sum() == 5
    assert sum(a["node"] == 0 and a["kind"] in p2p.BOUND for a in sc.apps) == 2
    assert m["servers"]["received"][1] == 6 and m["appc"]["rx_packets"][0] > 0  # its endpoints count their own flows


def test_conditions_hub_forwarding():
    sc = U.hub_forwarding()
    m = p2p_pyref.run(sc, ALL_KINDS)
    assert m["stats"]["ttl_drops"] == 5 and m["stats"]["icmp_sent"] == 0
    tr = m["trace"]
    d = tr[tr["kind"] == p2p_pyref.TR_IP_DROP]  # the expired datagrams as received: TTL 1 under sequence numbers 0 .. 4
    assert sorted(d["ttl"].tolist()) == [1 | (k << 8) for k in range(5)]
    # the hub (node 0) receives 24 datagrams at one time, more than a holder thread takes (16): its hub block's
    rx = tr[(tr["kind"] == p2p_pyref.TR_RX) & (np.array([sc.dev[x][0] for x in tr["dev"]]) == 0)]
    assert np.unique(rx["ts"], return_counts=True)[1].max() == 24 and (rx["ttl"] >> 8).max() == 4
    assert m["servers"]["received"][0] == 23 * 5


def test_conditions_grid_and_hub():
    m = p2p_pyref.run(U.grid_pipelines())
    srv = m["servers"][m["servers"]["received"] > 0]
    assert len(srv) == 4 and (srv["received"] == 25).all()
    assert (m["appc"]["rx_packets"][1:8:2] > 0).all()  # the sinks beside them
    m = p2p_pyref.run(U.incast_hub())
    assert m["servers"]["received"][1] == 16 * 6 and m["appc"]["rx_packets"][0] > 0


def test_legacy_struct_unchanged():
    """ports=False passes no port array: the struct every existing scenario builds."""
    s = p2p.grid(3, 3).c_struct()
    assert s.app_port is None and s.app_remote_port is None and s.app_loss_window is None
    sc = p2p.grid(3, 3)
    sc.ports = True
    assert sc.c_struct().app_port is not None


# ---------------- nsgpu_p2p_create's refusals (its validation runs before any device call: the host-only plan) ----------------
def refused(sc):
    with pytest.raises(nsgpu.NsgpuError) as e:
        p2p.dist_plan(sc, None, 0, 1)
    return str(e.value)


def two_node(ports=True):
    sc = U.line(2, [(5_000_000, 2 * U.MS)])
    sc.ports = ports
    return sc


def test_refusals_legacy_mode():
    sc = two_node(ports=False)
    sc.add_sink(1, 0, 0, port=9)
    sc.add_echo_server(1, 0, 0, port=7)
    sc.route_bfs()
    assert "node 1 has two bound endpoints" in refused(sc)
    for add in (lambda s: s.add_udp_server(1, 0, 0), lambda s: s.add_udp_client(0, 1, 0, 0)):
        sc = two_node(ports=False)
        add(sc)
        sc.route_bfs()
        assert "UdpClient / UdpServer need UDP ports" in refused(sc)


def test_refusals_ports_mode():
    def case(build):
        sc = two_node()
        build(sc)
        sc.route_bfs()
        return refused(sc)

    assert "two applications bound to port 9" in case(lambda s: (s.add_sink(1, 0, 0, port=9),
                                                                   s.add_udp_server(1, 0, 0, port=9)))
    assert "bound port 0" in case(lambda s: s.add_sink(1, 0, 0, port=0))
    assert "ephemeral range" in case(lambda s: (s.add_sink(1, 0, 0, port=50000),
                                                s.add_onoff(1, 0, 0, 0, remote_port=9)))
    assert "PacketSize 11 outside [12, 1472]" in case(lambda s: s.add_udp_client(0, 1, 0, 0, size=11))
    assert "PacketSize 1473 outside [12, 1472]" in case(lambda s: s.add_udp_client(0, 1, 0, 0, size=1473))
    assert "above 2^24" in case(lambda s: s.add_udp_client(0, 1, 0, 0, count=(1 << 24) + 1))
    for w in (0, 12, 264):
        assert "PacketWindowSize" in case(lambda s: s.add_udp_server(1, 0, 0, window=w))
    assert "holds no SeqTsHeader" in case(lambda s: (s.add_udp_server(1, 0, 0, port=100),
                                                     s.add_onoff(0, 1, 0, 0, size=8, remote_port=100)))
    # a port 50000 sink on a node without a sender stays legal (p2p.dumbbell's)
    sc = two_node()
    sc.add_sink(1, 0, 0, port=50000)
    sc.add_onoff(0, 1, 0, 0, remote_port=50000)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0


# ---------------- the trace codecs refuse SeqTsHeader datagrams ----------------
def test_codecs_refuse_udp_client_records():
    import trace
    sc = U.three_endpoints()
    tr = trace.sort_records(p2p_pyref.run(sc, ALL_KINDS)["trace"])
    mine = tr[(tr["app"] & p2p_pyref.PKT_APP) == 4]  # the UdpClient's flow
    other = tr[(tr["app"] & p2p_pyref.PKT_APP) != 4]
    assert len(mine) and len(other)
    py, lib = trace.Codec(sc), p2p.TraceCodec(sc)
    assert py.ascii(other) == lib.ascii(other)  # (the other flows of a ports scenario are written as before)
    assert py.pcaps(other) == lib.pcaps(other, py.ifindex)
    with pytest.raises(ValueError, match="UdpClient datagram"):
        py.ascii(mine[:1])
    with pytest.raises(ValueError, match="UdpClient datagram"):
        py.pcaps(tr)
    for call in (lambda: lib.ascii(tr), lambda: lib.line(mine[0]), lambda: lib.packet(mine[0]),
                 lambda: lib.pcap(tr, 0)):
        with pytest.raises(nsgpu.NsgpuError, match="UdpClient datagram"):
            call()
