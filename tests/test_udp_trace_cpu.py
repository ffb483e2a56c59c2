"""UdpTraceClient without a GPU: the Python model (tests/p2p_trace_client_pyref.py) against answers derived by hand
from udp-trace-client.cc and against the reference's own known answer, the two trace loaders against each other, the
model pinned to tests/p2p_pyref.py where no trace client exists and caught when nudged, what the GPU scenarios must
contain, nsgpu_p2p_create's refusals through the host-only plan, and the C ABI that must not move."""
import ctypes as C

import numpy as np
import pytest

import nsgpu
import nsref
import p2p
import p2p_pyref
import p2p_trace_client_pyref as T
import udp_ports_cases
import udp_trace_cases as U

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
MS, S = U.MS, U.S


class SendLog(T.Model):
    """The model, recording every Send's time and its datagrams' UDP payload sizes."""

    def __init__(self, sc):
        super().__init__(sc)
        self.sends = []

    def tc_send(self, a):
        self.sends.append((self.now, []))
        super().tc_send(a)

    def tc_send_packet(self, a, size):
        sent = self.app[a]["sent"]
        super().tc_send_packet(a, size)
        if self.app[a]["sent"] > sent:
            self.sends[-1][1].append(size if size > 12 else 12)


def two_node(bps=100_000_000):
    return U.line(2, [(bps, 1 * MS)])


def send_log(entries, mps, start=1 * S, stop=3 * S):
    sc = two_node()
    sc.add_udp_server(1, 0, 0, port=100)
    sc.add_udp_trace_client(0, 1, start, 0, entries=entries, max_packet_size=mps, remote_port=100)
    sc.stop(stop)
    sc.route_bfs()
    m = SendLog(sc)
    m.setup()
    m.run()
    return m


# ---------------- derived answers ----------------
def test_default_trace_entries():
    assert T.load_default_trace() == list(p2p.DEFAULT_TRACE) == p2p.default_trace()
    assert [t for t, _z in p2p.DEFAULT_TRACE] == [0, 40, 0, 0, 200, 0, 0, 120, 0, 0]
    assert [z for _t, z in p2p.DEFAULT_TRACE] == [534, 1542, 134, 390, 765, 407, 504, 903, 421, 587]


def test_default_trace_send_times_and_sizes():
    m = send_log(None, 1024)
    t0 = 1 * S
    times = [t - t0 for t, _d in m.sends]
    assert times[:7] == [0, 40 * MS, 240 * MS, 360 * MS, 400 * MS, 600 * MS, 720 * MS]
    for k in range(1, len(times) - 3):  # period 360 ms from +40 ms
        assert times[k + 3] - times[k] == 360 * MS
    sizes = [d for _t, d in m.sends]
    assert sizes[0] == [534]
    cycle = [[1024, 518, 134, 390], [765, 407, 504], [903, 421, 587, 534]]
    for k in range(1, len(sizes)):
        assert sizes[k] == cycle[(k - 1) % 3], k
    assert sum(len(c) for c in cycle) == 11 and sum(sum(c) for c in cycle) == 6187


def test_reference_known_answer():
    """udp-client-server-test.cc:169-180: 247 received, 0 lost (1 + 22 x 11 + 4)."""
    r = T.run(U.known_answer())
    assert tuple(r["servers"][0])[:2] == (247, 0)
    assert tuple(r["clients"][1])[:3] == (247, 4, 68)
    assert r["stats"]["cancelled"] == 1  # the Send pending at 10 s


def test_exact_multiple_adds_a_header_only_datagram():
    m = send_log([(20, 2048), (50, 1024), (50, 1000)], 1024, stop=1 * S + 110 * MS)
    assert [d for _t, d in m.sends[:3]] == [[1024, 1024, 12], [1024, 12], [1000]]


def test_tiny_frames_give_a_12_byte_payload():
    m = send_log([(10, 0), (10, 5), (10, 12), (10, 13)], 1024, stop=1 * S + 35 * MS)
    assert [d for _t, d in m.sends[:4]] == [[12], [12], [12], [13]]
    assert m.app[1]["c"]["tx_bytes"] == 12 + 12 + 12 + 13


# ---------------- the loaders ----------------
@pytest.mark.parametrize("name", U.GOLDEN_FILES)
def test_loaders_agree(name):
    assert p2p.load_trace_file(U.golden(name)) == T.load_trace(U.golden(name))


def test_loader_quirks():
    with_nl, without = (p2p.load_trace_file(U.golden(f)) for f in ("udp_trace_newline.txt", "udp_trace_no_newline.txt"))
    assert without == [(0, 600), (40, 1300), (0, 90), (120, 700)]
    assert with_nl == without + [(0, 700)]  # the last entry twice, the copy with timeToSend 0
    dec = p2p.load_trace_file(U.golden("udp_trace_decreasing.txt"))
    assert dec[1] == ((60 - 100) & 0xFFFFFFFF, 300) and dec[2] == (140, 500)  # time - prevTime is unsigned
    assert dec[3] == (0, 80)  # (a B frame does not move prevTime)
    assert dec[4] == ((150 - 200) & 0xFFFFFFFF, 200)
    tail = p2p.load_trace_file(U.golden("udp_trace_b_tail.txt"))
    assert [t for t, _z in tail] == [0, 50, 0, 0, 0] and len(tail) == 5
    assert p2p.load_trace_file(U.golden("udp_trace_one_line.txt")) == [(30, 1000)]
    assert p2p.load_trace_file(U.golden("no_such_file.txt")) == list(p2p.DEFAULT_TRACE)  # unreadable: the default trace
    assert T.load_trace(U.golden("no_such_file.txt")) == list(p2p.DEFAULT_TRACE)


# ---------------- the model is p2p_pyref where there is no trace client, and is caught when wrong ----------------
@pytest.mark.parametrize("name", ["three_endpoints", "loss_reorder", "stopped_server_no_route"])
def test_model_equals_p2p_pyref_without_a_trace_client(name):
    args = (32,) if name == "loss_reorder" else ()
    a = p2p_pyref.run(getattr(udp_ports_cases, name)(*args), ALL_KINDS)
    b = T.run(getattr(udp_ports_cases, name)(*args), ALL_KINDS)
    assert a["stats"] == b["stats"]
    assert all(np.array_equal(x, y) for x, y in zip(a["log"], b["log"]))
    assert np.array_equal(a["devc"], b["devc"]) and np.array_equal(a["appc"], b["appc"])
    assert np.array_equal(a["servers"], b["servers"]) and np.array_equal(a["trace"], b["trace"])
    assert not b["clients"]["sends"].any()


def differs(a, b):
    return a["stats"] != b["stats"] or any(not np.array_equal(x, y) for x, y in zip(a["log"], b["log"]))


def test_nudged_models_are_caught():
    sc = U.exact_and_tiny()
    assert differs(T.run(sc), T.run(U.exact_and_tiny(), nudge="drop_zero_remainder"))
    assert differs(T.run(U.known_answer()), T.run(U.known_answer(), nudge="no_wrap_join"))
    # (and the nudges change nothing where they do not apply: no exact multiple, no wrap before the stop)
    assert not differs(T.run(U.stop_mid_cycle()), T.run(U.stop_mid_cycle(), nudge="drop_zero_remainder"))
    assert not differs(T.run(U.stop_mid_cycle()), T.run(U.stop_mid_cycle(), nudge="no_wrap_join"))


# ---------------- the GPU scenarios contain what their names say ----------------
def test_gpu_scenarios_are_not_vacuous():
    r = T.run(U.overflow())
    assert r["devc"]["drop_packets"][0] > 0 and r["servers"]["lost"][0] > 0 and r["tc_diag"]["bursts_over_one"] > 0
    r = T.run(U.forwarded_ttl())
    assert r["stats"]["ttl_drops"] == r["stats"]["icmp_sent"] > 0 and r["servers"]["received"][0] > 0
    assert r["devc"]["tx_packets"][2] > 0  # (node 1 forwards)
    r = T.run(U.wrong_port())
    assert r["stats"]["unreach_drops"] == r["stats"]["icmp_sent"] > 0 and r["servers"]["received"][1] > 0
    r = T.run(U.exact_and_tiny())
    assert r["tc_diag"]["zero_remainder"] > 0 and r["tc_diag"]["header_only"] > r["tc_diag"]["zero_remainder"]
    r = T.run(U.stop_mid_cycle())
    assert r["stats"]["cancelled"] == 1 and tuple(r["clients"][1])[:3] == (8, 7, 3)
    r = T.run(U.no_route())
    assert r["clients"]["sent"][2] == 0 and r["clients"]["sends"][2] > 1 and r["stats"]["no_route_drops"] > 0
    assert r["tc_diag"]["noroute_sends"] == r["stats"]["no_route_drops"]
    r = T.run(U.grid_pipelines())
    kinds = {a["kind"] for a in U.grid_pipelines().apps}
    assert {p2p.APP_UDP_TRACE_CLIENT, p2p.APP_UDP_CLIENT, p2p.APP_ONOFF} <= kinds
    assert r["tc_diag"]["wrap_joined"] > 0 and 1000 < r["stats"]["dispatched"] < 5000
    assert p2p.dist_plan(U.grid_pipelines(), None, 0, 1)["wide"] == 1
    for name in ("hub_forwards_bursts", "hub_hosts_client"):
        sc = getattr(U, name)()
        r = T.run(sc)
        # a hub block: more than 16 same-window events at node 0 — 24 same-time arrivals
        ts, _uid, ctx = r["log"]
        at_hub = ts[ctx == 0]
        assert np.max(np.unique(at_hub, return_counts=True)[1]) >= 24, name
        assert r["tc_diag"]["bursts_over_one"] > 0
        if name == "hub_hosts_client":  # every Send of the hub's client shares its timestamp with 24 Receives there
            for k in range(5):
                assert np.count_nonzero(at_hub == 1 * S + U.HUB_ARRIVAL + k * 4 * MS) >= 25, k
    r = T.run_monitored(U.rate_error_model())
    assert 0 < r["em"]["corrupted"][1] < r["em"]["invoked"][1]
    assert len({int(p[2]) for _d, p in r["dropped"]} | {0}) > 2  # corrupt frames of several sizes
    for name in ("known_answer", "overflow"):
        a, b = T.run(getattr(U, name)()), T.run_monitored(getattr(U, name)(True))
        assert a["stats"] == b["stats"]  # the monitor only observes
    f = T.run_monitored(U.overflow(True))["flows"][p2p.MAX_PER_HOP_DELAY_NS]
    assert f["packets_dropped"][0][p2p.FLOW_DROP_QUEUE] > 0 and f["tx_packets"][0] > f["rx_packets"][0]


# ---------------- refusals (create's validation runs before any device call: the host-only plan) ----------------
def refused(sc):
    sc.route_bfs()
    with pytest.raises(nsgpu.NsgpuError) as e:
        p2p.dist_plan(sc, None, 0, 1)
    return str(e.value)


def client(entries=None, mps=1024, ports=True, frag=False, server=True, **kw):
    sc = two_node()
    sc.ports, sc.frag = ports, frag
    if server:
        sc.add_udp_server(1, 0, 0, port=100)
    sc.add_udp_trace_client(0, 1, 0, 0, entries=entries, max_packet_size=mps, remote_port=100, **kw)
    return sc


def test_refusals():
    assert "UdpTraceClient needs UDP ports" in refused(client(ports=False, server=False))
    assert "no trace entries" in refused(client(entries=[]))
    assert "every entry's timeToSend is 0" in refused(client(entries=[(0, 100), (0, 200)]))
    assert "MaxPacketSize 0 outside [1, 1472]" in refused(client(mps=0))
    assert "MaxPacketSize 1473 outside [1, 1472]" in refused(client(mps=1473))
    assert "MaxPacketSize 1473 outside [1, 1472]" in refused(client(mps=1473, frag=True))
    assert "packet_size 65536 above 65535" in refused(client(entries=[(10, 65536)]))
    assert "a Send of 257 datagrams" in refused(client(entries=[(10, 256)], mps=1))
    assert "a Send of 258 datagrams" in refused(client(entries=[(10, 100)] + [(0, 100)] * 128, mps=100))
    assert "a 12-byte payload" in refused(client(entries=[(10, 2048)], server=False))
    sc = client(entries=[(10, 5)], server=False)
    sc.add_sink(1, 0, 0, port=100)
    assert "a 12-byte payload" in refused(sc)
    assert "bad destination/ttl/source slot" in refused(client(ttl=0))
    # without an extension record the kind has no entries
    sc = client()
    sc.route_bfs()
    s, pl = sc.c_struct(), p2p.Plan()
    with pytest.raises(nsgpu.NsgpuError, match="no trace entries"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan(C.byref(s), None, 0, 1, 0, C.byref(pl)))
    # what is accepted: the cap itself, a trace client in a frag scenario beside other flows, a sink for payloads above 12
    sc = client(entries=[(10, 255)], mps=1)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0
    sc = client(frag=True)
    sc.add_onoff(0, 1, 0, 0, size=3000, remote_port=100)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0
    sc = client(entries=[(10, 500)], server=False)
    sc.add_sink(1, 0, 0, port=100)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["n_init"] > 0
    assert p2p.UDP_TRACE_MAX_BURST == 256 >= 64


def tx_time(frame, bps=100_000_000):
    return nsref.seconds(float(frame) * 8 / float(bps))  # Seconds (m_bps.CalculateTxTime (bytes)), data-rate.cc:224-227


def test_lookahead_takes_the_flows_smallest_frame():
    """tx_min is the transmission time of the smallest frame a trace client can put on a wire: 12 + 8 + 20 + 2 bytes
    for a trace with a tiny frame, whatever MaxPacketSize says."""
    sc = client(entries=[(10, 1000), (0, 3)], mps=1024)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["tx_min"] == tx_time(42)
    sc = client(entries=[(10, 1000), (0, 300)], mps=1024)
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["tx_min"] == tx_time(330)
    sc = client(entries=[(10, 1000), (0, 300)], mps=400)  # 1000 = 400 + 400 + 200
    sc.route_bfs()
    assert p2p.dist_plan(sc, None, 0, 1)["tx_min"] == tx_time(230)


# ---------------- the C ABI that must not move ----------------
def test_abi():
    assert C.sizeof(p2p.ScenarioStruct) == 368 and p2p.ScenarioStruct.rng_run.offset == 364
    assert C.sizeof(p2p.ScenarioExt) == 24 and p2p.ScenarioExt.trace_entries.offset == 16
    assert p2p.APP_UDP_TRACE_CLIENT == 6
    assert p2p.UDP_TRACE_ENTRY_DTYPE.itemsize == 8 and p2p.UDP_TRACE_CLIENT_DTYPE.itemsize == 16
    # ext == NULL through _ex is the old entry point, for every field of the plan, single and partitioned
    for sc in (udp_ports_cases.grid_pipelines(), p2p.grid(4, 4), p2p.dumbbell(4)):
        for owner, nranks in ((None, 1), (p2p.owner_blocks(sc.n_nodes, 2), 2)):
            s, a, b = sc.c_struct(), p2p.Plan(), p2p.Plan()
            own = owner.ctypes.data if owner is not None else None
            nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan(C.byref(s), own, 0, nranks, 0, C.byref(a)))
            nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan_ex(C.byref(s), None, own, 0, nranks, 0, C.byref(b)))
            assert bytes(a) == bytes(b)
    # every rank of a partitioned trace-client scenario gets the same plan
    sc = U.grid_pipelines()
    own = p2p.owner_blocks(sc.n_nodes, 2)
    assert p2p.plan_mismatch([p2p.dist_plan(sc, own, r, 2) for r in range(2)]) == {}


def test_codecs_refuse_trace_client_records():
    import trace
    sc = U.wrong_port()
    tr = trace.sort_records(T.run(sc, ALL_KINDS)["trace"])
    mine = tr[((tr["app"] & p2p_pyref.PKT_APP) == 2) & ((tr["app"] & p2p_pyref.PKT_ICMP) == 0)]
    assert len(mine)
    py, lib = trace.Codec(sc), p2p.TraceCodec(sc)
    with pytest.raises(ValueError, match="UdpTraceClient datagram"):
        py.ascii(mine[:1])
    for call in (lambda: lib.ascii(mine), lambda: lib.line(mine[0]), lambda: lib.packet(mine[0])):
        with pytest.raises(nsgpu.NsgpuError, match="UdpTraceClient"):
            call()
