"""IPv4 fragmentation and reassembly on the CPU: DoFragmentation's arithmetic and the Fragments class of the Python
model (tests/p2p_frag_pyref.py) on derived answers, the reference's own known answers as two-node scenarios, the
model's identity with the oracle and tests/p2p_pyref.py off the new path, the conditions the GPU scenarios of
tests/test_gpu_frag.py must meet so that none of them passes vacuously — asserted on the model alone —, create's
refusals through the host-only plan, and a positive control."""
import numpy as np
import pytest

import frag_cases as F
import nsgpu
import nsref
import p2p
import p2p_frag_pyref as R
import p2p_pyref
import reference_fixtures as RF
import udp_ports_cases as U

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
_models = {}


def model(name, *args):
    if (name, args) not in _models:
        _models[(name, args)] = R.run(getattr(F, name)(*args), ALL_KINDS)
    return _models[(name, args)]


# ---------------- DoFragmentation (ipv4-l3-protocol.cc:1116-1206), answers derived by hand ----------------
def test_do_fragmentation_arithmetic():
    assert R.fragment_lengths(1472) == [1500]              # 1472 + 8 + 20: fits the MTU, one packet
    assert R.fragment_lengths(1473) == [1500, 21]          # L = 1481: 1480 and 1 byte of IP payload
    assert R.fragment_lengths(2000) == [1500, 548]         # L = 2008: 1480 + 528
    big = R.fragment_lengths(65507)                        # L = 65515 = 44 x 1480 + 395
    assert big == [1500] * 44 + [415] and len(big) == 45
    fr = R.do_fragmentation(20 + 65515)
    assert [o for o, _p, _m in fr] == [1480 * i for i in range(45)] and all(o % 8 == 0 for o, _p, _m in fr)
    assert [m for _o, _p, m in fr] == [True] * 44 + [False]  # all but the last carry MF
    assert sum(p for _o, p, _m in fr) == 65515


# ---------------- Fragments (:1259-1389) on hand-made lists ----------------
def filled(entries, nudge=None):
    f = R.Fragments(nudge)
    for size, offset, more, tag in entries:
        f.add_fragment(size, offset, more, tag)
    return f


def test_fragments_in_order_completion():
    f = filled([(1480, 0, True, "a"), (1480, 1480, True, "b")])
    assert not f.is_entire()
    f.add_fragment(40, 2960, False, "c")
    assert f.is_entire() and f.get_packet() == 3000 and f.get_partial_packet() == 3000


def test_fragments_missing_middle():
    f = filled([(1480, 0, True, "a"), (40, 2960, False, "c")])
    assert not f.m_moreFragment and not f.is_entire()  # the last one is there, the hole is found by the offsets
    assert f.get_partial_packet() == 1480               # the contiguous prefix
    f.add_fragment(1480, 1480, True, "b")               # inserted in the middle: m_moreFragment stays false
    assert not f.m_moreFragment and f.is_entire() and f.get_packet() == 3000


def test_fragments_equal_offsets_keep_arrival_order():
    f = filled([(1480, 0, True, "first"), (1480, 0, True, "second"), (1480, 0, True, "third")])
    assert [t for _s, _o, t in f.m_fragments] == ["first", "second", "third"]
    f = filled([(1480, 1480, True, "x"), (1480, 0, True, "first"), (1480, 0, True, "second")])
    assert [t for _s, _o, t in f.m_fragments] == ["first", "second", "x"]
    f = filled([(1480, 0, True, "first"), (1480, 0, True, "second")], nudge="before_equal")  # (the control's nudge)
    assert [t for _s, _o, t in f.m_fragments] == ["second", "first"]


def test_fragments_last_arrives_first():
    f = filled([(40, 2960, False, "c")])
    assert not f.m_moreFragment and not f.is_entire()  # lastEndOffset 0 < 2960
    assert f.get_partial_packet() == 0                 # no entry at offset 0: empty
    f.add_fragment(1480, 0, True, "a")                 # not at the end: m_moreFragment is not touched
    assert not f.m_moreFragment and not f.is_entire()
    f.add_fragment(1480, 1480, True, "b")
    assert f.is_entire() and f.get_packet() == 3000
    # a fragment with MF that goes to the end sets m_moreFragment again
    g = filled([(1480, 0, True, "a"), (40, 2960, False, "c"), (1480, 4440, True, "d")])
    assert g.m_moreFragment and not g.is_entire()


def test_fragments_overlap_rule():
    # a later entry contributes only what lies beyond lastEndOffset; one that ends before it nothing
    f = filled([(1480, 0, True, "a"), (1480, 0, True, "a2"), (1480, 1480, True, "b"), (40, 2960, False, "c")])
    assert f.is_entire() and f.get_packet() == 3000
    f = filled([(1480, 0, True, "a"), (1000, 1000, False, "tail")])  # 480 bytes overlap: 1480 + 520
    assert f.is_entire() and f.get_packet() == 2000 and f.get_partial_packet() == 2000
    f = filled([(1480, 0, True, "a"), (100, 200, True, "inside"), (40, 1480, False, "c")])
    assert f.is_entire() and f.get_packet() == 1520


def test_fragments_partial_packet():
    assert filled([(1480, 1480, True, "b")]).get_partial_packet() == 0
    assert filled([(1480, 0, True, "a")]).get_partial_packet() == 1480
    # a hole ends the prefix; an entry beyond it adds nothing
    assert filled([(1480, 0, True, "a"), (1480, 2960, True, "c")]).get_partial_packet() == 1480
    assert filled([(8, 0, True, "a")]).get_partial_packet() == 8  # (not more than 8 bytes: no ICMP error)


# ---------------- the reference's known answers (ipv4-fragmentation-test.cc:312-398) ----------------
@pytest.mark.parametrize("size", [1000, 2000, 5000, 10000, 65000])
def test_reference_datagrams_arrive_whole(size):
    sc = F.reference_whole(size)
    m = R.run(sc, ALL_KINDS)
    sink = m["appc"][0]
    assert int(sink["rx_bytes"]) == size and int(sink["rx_packets"]) == 1
    n = len(R.fragment_lengths(size))
    assert m["frag"]["fragments_sent"] == (n if n > 1 else 0) and m["frag"]["reassembled"] == (1 if n > 1 else 0)
    assert int(m["devc"]["drop_packets"].sum()) == 0


def test_reference_lost_fragment_times_out_with_an_icmp_error():
    sc = F.reference_lost_fragment()
    m = R.run(sc, ALL_KINDS)
    server, client = m["appc"][0], m["appc"][1]
    assert int(server["rx_packets"]) == 0 and int(client["rx_packets"]) == 0
    assert int(m["devc"]["drop_packets"][0]) == 2  # four fragments: one transmitting, one queued, two dropped
    assert m["frag"]["timeouts"] == 1 and m["stats"]["icmp_sent"] == 1
    # the time-exceeded error reaches the client's node: a 56-byte ICMP packet received on device 0
    rx = m["trace"][(m["trace"]["kind"] == p2p_pyref.TR_RX) & (m["trace"]["dev"] == 0)]
    assert len(rx) == 1 and int(rx["app"][0]) & p2p_pyref.PKT_ICMP and not int(rx["app"][0]) & p2p_pyref.PKT_ICMP_UNREACH
    assert int(rx["size"][0]) == 56
    drop = m["trace"][m["trace"]["kind"] == p2p_pyref.TR_IP_DROP]
    assert len(drop) == 1 and int(drop["dev"][0]) == 1  # DROP_FRAGMENT_TIMEOUT on the captured input device


# ---------------- identity off the new path ----------------
def oracle_run(sc):
    s = sc.c_struct()
    st = p2p.P2PStats()
    devc = np.zeros(s.n_devices, p2p.DEV_COUNTERS_DTYPE)
    appc = np.zeros(s.n_apps, p2p.APP_COUNTERS_DTYPE)
    nsref.p2p_run(s, st, devc, appc, 0)
    _secs, log, tr = nsref.p2p_run_trace(s, st, devc, appc, int(st.dispatched), ALL_KINDS)
    return st, devc, appc, log, tr


def same_result(a, b):
    return (a["stats"] == b["stats"] and np.array_equal(a["devc"], b["devc"]) and np.array_equal(a["appc"], b["appc"])
            and np.array_equal(a["servers"], b["servers"]) and all(np.array_equal(x, y) for x, y in zip(a["log"], b["log"]))
            and np.array_equal(a["trace"], b["trace"]))


NON_PORTS = {"first_cc": p2p.first_cc, "udp_client_server_echo": RF.udp_client_server_scenario,
             "grid3x3": lambda: p2p.grid(3, 3), "incast8": lambda: p2p.incast(8),
             "icmp": lambda: p2p.random_topology(12, 13, 8, 2, icmp=True, ttl=2, sink_window=(20_000_000, 300_000_000))}
PORTS = {"three_endpoints": U.three_endpoints, "loss_reorder": lambda: U.loss_reorder(8),
         "port_mismatch_icmp": lambda: U.port_mismatch(True)}


@pytest.mark.parametrize("name", sorted(NON_PORTS))
def test_frag_on_changes_nothing_where_the_oracle_applies(name):
    sc = NON_PORTS[name]()
    sc.frag = True
    m = R.run(sc, ALL_KINDS)
    assert m["stats"]["dispatched"] > 0 and m["frag"] == dict.fromkeys(p2p.FRAG_STATS_FIELDS, 0)
    sc.frag = False  # (the oracle knows no fragmentation: it runs the scenario as it always did)
    assert same_result(m, p2p_pyref.run(sc, ALL_KINDS) | {"frag": None})
    st, devc, appc, log, tr = oracle_run(sc)
    assert all(int(getattr(st, k)) == v for k, v in m["stats"].items())
    assert np.array_equal(devc, m["devc"]) and np.array_equal(appc, m["appc"])
    assert all(np.array_equal(x, y) for x, y in zip(log, m["log"]))
    assert len(tr) == len(m["trace"]) and all(np.array_equal(tr[f], m["trace"][f]) for f in tr.dtype.names)


@pytest.mark.parametrize("name", sorted(PORTS))
def test_frag_on_changes_nothing_in_ports_scenarios(name):
    sc = PORTS[name]()
    sc.frag = True
    m = R.run(sc, ALL_KINDS)
    assert m["stats"]["dispatched"] > 0 and m["frag"] == dict.fromkeys(p2p.FRAG_STATS_FIELDS, 0)
    assert same_result(m, p2p_pyref.run(sc, ALL_KINDS))


# ---------------- the GPU scenarios are not vacuous ----------------
@pytest.mark.parametrize("name,args", F.LOSS_CASES)
def test_conditions_loss_cases(name, args):
    m = model(name, *args)
    f = m["frag"]
    assert f["timeouts"] >= 1            # a timer fired
    assert f["cancelled_timers"] >= 1    # a cancelled timer was dispatched
    assert m["diag"]["mixed"] >= 1       # a datagram reassembled from a list longer than its own fragment count
    assert f["reassembled"] >= 1 and 3 < f["max_list"] <= p2p.FRAG_CAP
    assert int(m["devc"]["drop_packets"].sum()) > 0
    assert (m["stats"]["icmp_sent"] > 0) == args[0]
    assert (m["trace"]["kind"] == p2p_pyref.TR_IP_DROP).sum() == f["timeouts"]


def test_conditions_of_the_other_gpu_scenarios():
    m = model("echo_2000")
    assert m["frag"]["fragmented"] == 6 and m["frag"]["fragments_sent"] == 12 and m["frag"]["reassembled"] == 6
    assert [int(x) for x in m["appc"]["rx_packets"]] == [3, 3] and [int(x) for x in m["appc"]["rx_bytes"]] == [6000, 6000]
    m = model("forwarding_4000")
    assert m["frag"]["reassembled"] == m["frag"]["fragmented"] > 3 and int(m["devc"]["tx_packets"][2]) == 3 * m["frag"]["fragmented"]
    m = model("largest")
    assert m["frag"]["fragments_sent"] == 45 and m["frag"]["max_list"] == 45 and int(m["appc"]["rx_bytes"][0]) == 65507
    m = model("sender_overflow")  # per datagram: one fragment transmitting, two queued, two dropped
    assert int(m["devc"]["drop_packets"][0]) == 4 and int(m["devc"]["enq_packets"][0]) == 6
    assert m["frag"]["timeouts"] == 2 and m["frag"]["reassembled"] == 0 and int(m["appc"]["rx_packets"][0]) == 0
    m = model("ttl_expiry")
    assert m["stats"]["ttl_drops"] == 9 and m["stats"]["icmp_sent"] == 9 and m["frag"]["fragments_sent"] == 9
    m = model("port_unreachable")
    assert m["stats"]["unreach_drops"] == 3 and m["stats"]["icmp_sent"] == 3 and m["frag"]["reassembled"] == 3
    icmp = m["trace"][(m["trace"]["kind"] == p2p_pyref.TR_IP_TX) & ((m["trace"]["app"] & p2p_pyref.PKT_ICMP) != 0) &
                      (m["trace"]["dev"] == 3)]  # (as node 2 sends them; node 1 forwards them)
    assert len(icmp) == 3 and all(int(t) >> 16 == 548 for t in icmp["ttl"])  # the offending header: the last fragment's
    m = model("udp_client_1500")
    srv = m["servers"][0]
    assert 0 < int(srv["received"]) < 40 and int(srv["lost"]) > 0 and int(srv["last_max_seq"]) > int(srv["received"])
    assert m["frag"]["fragmented"] == 40 and m["frag"]["fragments_sent"] == 80 and m["frag"]["timeouts"] >= 1
    m = model("grid_pipelines")
    assert m["frag"]["reassembled"] == m["frag"]["fragmented"] >= 8 and m["stats"]["dispatched"] > 1000
    m = model("hub_forwards")
    assert m["frag"]["reassembled"] == 36 and m["stats"]["dispatched"] > 400
    m = model("hub_echo_server")
    assert m["frag"]["fragmented"] == 6 and m["frag"]["reassembled"] >= 4  # three echoes, each way
    assert int(m["appc"]["rx_packets"][0]) == 3 and int(m["appc"]["rx_packets"][2]) >= 1


def test_hub_echo_reply_shares_its_window_with_a_hub_burst():
    """The hub's three-fragment reply (its Ipv4 Tx records on the hub's device towards leaf 1) is followed, within less
    than the smallest frame's time, by 22 same-time Receives at the hub that are all forwarded to that device: one
    window (its bound is the Receives' time: their lookahead is 0), one hub, every device step on one device."""
    sc = F.hub_echo_server()
    m = model("hub_echo_server")
    tr = m["trace"]
    hub_dev = 1  # (link (1, 0): device 0 on leaf 1, device 1 on the hub)
    ftx = tr[(tr["kind"] == p2p_pyref.TR_IP_TX) & (tr["dev"] == hub_dev) & ((tr["ipid"] >> 16) != 0) &
             ((tr["app"] & p2p_pyref.PKT_ICMP) == 0)]
    assert len(ftx) == 9 and len(set(int(u) for u in ftx["uid"])) == 3  # three replies of three fragments
    tx_min = p2p.dist_plan(sc, None, 0, 1)["tx_min"]
    ts, _uid, ctx = m["log"]
    hub_ts, counts = np.unique(ts[ctx == 0], return_counts=True)
    for t in sorted(set(int(x) for x in ftx["ts"]))[:2]:
        after = [(int(a), int(c)) for a, c in zip(hub_ts, counts) if t < a <= t + tx_min]
        assert len(after) == 1 and after[0][1] == 22
        fwd = tr[(tr["kind"] == p2p_pyref.TR_IP_TX) & (tr["ts"] == after[0][0])]
        assert len(fwd) == 22 and (fwd["dev"] == hub_dev).all()


def test_hub_timeout_fires_inside_a_single_device_hub_window():
    """The timer fires at the very time of 22 Receives at the hub, all forwarded to the hub's device towards leaf 1,
    where the time-exceeded error goes too; the Drop record follows the error's Send, on the captured input device
    with the captured TTL.  No event of that time has an inline child (nothing is delivered at the hub then)."""
    m = model("hub_timeout")
    assert m["frag"]["timeouts"] == 1 and m["stats"]["icmp_sent"] == 1 and m["frag"]["reassembled"] == 0
    tr = m["trace"]
    drop = tr[tr["kind"] == p2p_pyref.TR_IP_DROP]
    assert len(drop) == 1 and int(drop["dev"][0]) == 1 and int(drop["ttl"][0]) == 64 and int(drop["size"][0]) == 1500
    t, uid = int(drop["ts"][0]), int(drop["uid"][0])
    ts, _uid, ctx = m["log"]
    assert int(((ts == t) & (ctx == 0)).sum()) == 23  # the timer and the burst's 22 Receives
    tx = tr[(tr["ts"] == t) & (tr["kind"] == p2p_pyref.TR_IP_TX)]
    assert len(tx) == 23 and (tx["dev"] == 1).all()
    mine = tr[(tr["ts"] == t) & (tr["uid"] == uid)]
    assert int(mine["kind"][0]) == p2p_pyref.TR_IP_TX and int(mine["app"][0]) & p2p_pyref.PKT_ICMP
    assert int(mine["kind"][-1]) == p2p_pyref.TR_IP_DROP and int(mine["seq"][-1]) == len(mine) - 1
    assert not ((tr["ts"] == t) & (tr["kind"] == p2p_pyref.TR_RX) & (tr["dev"] == 1)).any()  # no fragment then


def test_list_overflow_is_an_error_not_a_truncation():
    with pytest.raises(OverflowError):
        R.run(F.list_overflow())


def test_hub_scenarios_make_hub_windows():
    """More than 16 same-time events of one node in a window make it a hub: 23 leaves send at once here."""
    for name in ("hub_forwards", "hub_echo_server"):
        m = model(name)
        ts, _uid, ctx = m["log"]
        hub = ts[ctx == 0]
        _v, counts = np.unique(hub, return_counts=True)
        assert counts.max() >= (12 if name == "hub_forwards" else 20)


# ---------------- nsgpu_p2p_create's refusals (the host-only plan) ----------------
def refused(sc):
    with pytest.raises(nsgpu.NsgpuError) as e:
        p2p.dist_plan(sc, None, 0, 1)
    return str(e.value)


def test_refusals_and_acceptance():
    def two_node(frag, **kw):
        sc = F.line(2, [(5_000_000, 2 * F.MS)], **kw)
        sc.frag = frag
        sc.add_sink(1, 0, 0)
        return sc

    sc = two_node(True)
    sc.add_onoff(0, 1, 0, 0, size=65508)
    sc.route_bfs()
    assert "65508-byte payload is above the largest UDP datagram" in refused(sc)
    sc = two_node(True)
    sc.add_onoff(0, 1, 0, 0, size=65507)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0
    sc = two_node(False)  # frag off: today's message
    sc.add_onoff(0, 1, 0, 0, size=2000)
    sc.route_bfs()
    assert "app 1: 2000-byte payload needs IPv4 fragmentation" in refused(sc)
    sc = two_node(True)  # a negative timeout, whatever the flows
    sc.frag_timeout_ns = -1
    sc.add_onoff(0, 1, 0, 0, size=100)
    sc.route_bfs()
    assert "negative frag_timeout_ns" in refused(sc)
    # two fragmenting flows into one node
    sc = F.line(3, [(5_000_000, F.MS), (5_000_000, F.MS)])
    sc.add_sink(2, 0, 0)
    sc.add_onoff(0, 2, 0, 0, size=2000)
    sc.add_onoff(1, 2, 0, 0, size=1473)
    sc.route_bfs()
    assert "node 2 receives fragments of 2 fragmenting flows" in refused(sc)
    # ... one of them small: accepted
    sc = F.line(3, [(5_000_000, F.MS), (5_000_000, F.MS)])
    sc.add_sink(2, 0, 0)
    sc.add_onoff(0, 2, 0, 0, size=2000)
    sc.add_onoff(1, 2, 0, 0, size=1472)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0
    # an echo client's reply fragments return to its own node: a second flow into that node is refused
    sc = F.line(2, [(5_000_000, F.MS)])
    sc.add_echo_server(1, 0, 0)
    sc.add_sink(0, 0, 0)
    sc.add_echo_client(0, 1, 0, 0, size=3000)
    sc.add_onoff(1, 0, 0, 0, size=3000)
    sc.ports = True
    for a, port in zip(sc.apps, (7, 9, 0, 0)):
        a["port"] = port
    sc.apps[2]["remote_port"], sc.apps[3]["remote_port"] = 7, 9
    sc.route_bfs()
    assert "node 0 receives fragments of 2 fragmenting flows" in refused(sc)
    # UdpClient: [12, 1500] with frag, [12, 1472] without (today's message)
    for frag, size, msg in ((True, 1501, "PacketSize 1501 outside [12, 1500]"), (True, 11, "PacketSize 11 outside [12, 1500]"),
                            (False, 1473, "PacketSize 1473 outside [12, 1472]")):
        sc = F.line(2, [(5_000_000, F.MS)], ports=True)
        sc.frag = frag
        sc.add_udp_server(1, 0, 0)
        sc.add_udp_client(0, 1, 0, 0, size=size)
        sc.route_bfs()
        assert msg in refused(sc)
    sc = F.line(2, [(5_000_000, F.MS)], ports=True)
    sc.add_udp_server(1, 0, 0)
    sc.add_udp_client(0, 1, 0, 0, size=1500)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0


def test_lookahead_takes_the_smallest_fragment():
    """A 1473-byte payload leaves a 21-byte last fragment: 23 bytes on the wire bound tx_min, not 1503."""
    sc = F.line(2, [(8_000_000, F.MS)])
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 0, 0, size=1473)
    sc.route_bfs()
    pl = p2p.dist_plan(sc, None, 0, 1)
    tx = nsref.seconds(float(21 + 2) * 8 / float(8_000_000))  # 23 bytes at 8 Mbit/s
    assert tx < 24_000 and pl["tx_min"] == tx and pl["lx"] == tx + F.MS
    assert pl["lookahead"][0] == tx  # the timeout kind's entry: it may send an ICMP error from its node
    sc.frag_timeout_ns = 10_000  # a timeout below the smallest frame's time bounds the Receive that schedules it
    assert p2p.dist_plan(sc, None, 0, 1)["lookahead"][10] == 10_000


# ---------------- the trace codecs refuse fragments ----------------
def test_codecs_refuse_fragment_records():
    import trace
    sc = F.echo_2000()
    tr = trace.sort_records(model("echo_2000")["trace"])
    frags = tr[(tr["ipid"] >> 16) != 0]
    assert len(frags) == len(tr) > 0  # every datagram of this scenario is fragmented
    py, lib = trace.Codec(sc), p2p.TraceCodec(sc)
    with pytest.raises(ValueError, match="an IPv4 fragment"):
        py.ascii(frags[:1])
    with pytest.raises(ValueError, match="an IPv4 fragment"):
        py.pcaps(tr)
    for call in (lambda: lib.ascii(tr), lambda: lib.line(frags[0]), lambda: lib.packet(frags[0]),
                 lambda: lib.pcap(tr, 0)):
        with pytest.raises(nsgpu.NsgpuError, match="an IPv4 fragment"):
            call()
    # an ICMP error about a fragment (its descriptor has no MF / offset for the embedded header) is refused as well
    sc = F.ttl_expiry()
    tr = trace.sort_records(model("ttl_expiry")["trace"])
    icmp = tr[(tr["app"] & p2p_pyref.PKT_ICMP) != 0]
    assert len(icmp) > 0
    py, lib = trace.Codec(sc), p2p.TraceCodec(sc)
    with pytest.raises(ValueError, match="an ICMP error about an IPv4 fragment"):
        py.ascii(icmp[:1])
    with pytest.raises(ValueError, match="an ICMP error about an IPv4 fragment"):
        py.pcaps(icmp)
    for call in (lambda: lib.ascii(icmp), lambda: lib.line(icmp[0]), lambda: lib.packet(icmp[0])):
        with pytest.raises(nsgpu.NsgpuError, match="an ICMP error about one"):
            call()
    # a frag scenario's unfragmented datagrams are written as before
    sc = U.three_endpoints()
    other = trace.sort_records(p2p_pyref.run(sc, ALL_KINDS)["trace"])
    other = other[(other["app"] & p2p_pyref.PKT_APP) != 4]
    want = trace.Codec(sc).ascii(other)
    sc.frag = True
    assert trace.Codec(sc).ascii(other) == want and p2p.TraceCodec(sc).ascii(other) == want


# ---------------- positive control ----------------
@pytest.mark.parametrize("nudge,name,args", [("before_equal", "udp_client_1500", (36,)),
                                             ("timer_left_running", "loss_at_forwarder", (True,))])
def test_nudged_model_is_caught(nudge, name, args):
    """Insertion before equal offsets changes which entry is first, and with it the sequence number a mixed list
    delivers (a UdpClient's datagrams differ in nothing else; with 36 of them the last delivery is a mixed one, so
    the server's last sequence number shows it); a timer left uncancelled fires on the next buffer."""
    good = model(name, *args)
    bad = R.run(getattr(F, name)(*args), ALL_KINDS, nudge=nudge)
    assert not same_result(good, bad)
