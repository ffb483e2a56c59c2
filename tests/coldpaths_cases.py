"""Scenarios for the handlers' out-of-line paths (nsgpu_p2p_dev.h "cold paths"): every one is small
enough that one or two holder waves of k2_handle hold a whole window, and mixed enough that lanes on the inlined path
(forwarded Receives, PacketSink deliveries, TransmitCompletes) share a wave with lanes that leave it (Sends, the
application start / stop kinds, echo applications, ICMP errors, TTL expiry, a missing route or endpoint).
tests/test_p2p_coldpaths_cpu.py asserts with the oracle alone that each really produces the kinds it is meant to."""
import p2p

MS = 1_000_000


def nid(y, x, cols=8):
    return y * cols + x


def mixed():
    """8 x 8 grid, ICMP on, Stop at 0.6 s.  The link delay is 200 us so that the engine is wide with ICMP's 58-byte
    frames (create: Lx <= 8 tx_min).  Flows:
      * column OnOff flows 0..4 (row 0 -> row 7): the inlined path;
      * an OnOff flow with 4 ms on / 3 ms off: StartSending / StopSending and cancelled Sends;
      * a UdpEchoClient / UdpEchoServer pair corner to corner: queued DoForwardUps and reply routing;
      * a flow with TTL 3 on an 11-hop path: time-exceeded errors travelling back;
      * a flow to a node with no PacketSink: port-unreachable errors;
      * a PacketSink that stops at 0.3 s under a flow that goes on: an application stopping mid-run, then unreachable."""
    g = p2p.grid(8, 8, delay_ns=200_000, n_flows=5, icmp=True, stop_ns=500 * MS, sim_stop_ns=600 * MS)
    g.add_sink(nid(7, 6), 0, 0)
    g.add_onoff(nid(0, 6), nid(7, 6), 120 * MS, 450 * MS, rate_bps=2_000_000, size=256, on_s=0.004, off_s=0.003)
    g.add_echo_server(nid(7, 7), 50 * MS, 550 * MS)
    g.add_echo_client(nid(0, 7), nid(7, 7), 110 * MS, 500 * MS, count=30, interval_ns=10 * MS, size=300)
    g.add_onoff(nid(0, 0), nid(7, 4), 130 * MS, 400 * MS, rate_bps=300_000, size=200, on_s=1e9, off_s=0.0, ttl=3)
    g.add_onoff(nid(1, 0), nid(1, 7), 140 * MS, 400 * MS, rate_bps=300_000, size=200, on_s=1e9, off_s=0.0)
    g.add_sink(nid(7, 5), 0, 300 * MS)
    g.add_onoff(nid(0, 5), nid(7, 5), 150 * MS, 450 * MS, rate_bps=400_000, size=300, on_s=1e9, off_s=0.0)
    g.route_bfs()
    return g


def mixed_apps(g):
    """Indices of mixed()'s applications by role."""
    k = [a["kind"] for a in g.apps]
    return {"echo_client": k.index(p2p.APP_ECHO_CLIENT), "echo_server": k.index(p2p.APP_ECHO_SERVER)}


def no_route(icmp):
    """Two components, 0 - 1 - 2 and 3 - 4, with flows towards the other one: node 0 has a single link, so global
    routing gives it a default route and its datagrams reach node 1, whose Receive finds no route; node 1's own flow
    finds none at its Send.  A flow inside the first component keeps forwarded Receives in the same windows."""
    sc = p2p.Scenario(5, icmp=icmp)
    links = [sc.link(0, 1, 5_000_000, 200_000), sc.link(1, 2, 5_000_000, 200_000), sc.link(3, 4, 5_000_000, 200_000)]
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.1.0.0") + (k << 8))
    sc.add_sink(4, 0, 0)
    sc.add_sink(2, 0, 0)
    sc.add_onoff(0, 4, 50 * MS, 250 * MS, rate_bps=400_000, size=200, on_s=1e9, off_s=0.0)
    sc.add_onoff(1, 4, 60 * MS, 250 * MS, rate_bps=300_000, size=300, on_s=0.02, off_s=0.01)
    sc.add_onoff(0, 2, 55 * MS, 250 * MS, rate_bps=500_000, size=256, on_s=1e9, off_s=0.0)
    sc.stop(300 * MS)
    sc.route_bfs()
    return sc


def crowded_node():
    """A node of degree 4 fed by four saturated neighbours, 5 x 5 grid: each neighbour of the centre sends at its link's
    rate through the centre to the neighbour opposite, so in every span of one transmission time the centre has four
    Receives and its own four TransmitCompletes: more than NSLOT = 7 window events (the holder's scan of the window
    for the rest) and at most CH = 16 (no hub block).  1 ms of link delay keeps the engine narrow (create: Lx > 8
    tx_min), so that a window is one transmission time long."""
    fl = [(nid(2, 1, 5), nid(2, 3, 5)), (nid(2, 3, 5), nid(2, 1, 5)), (nid(1, 2, 5), nid(3, 2, 5)),
          (nid(3, 2, 5), nid(1, 2, 5))]
    return p2p.grid(5, 5, bps=10_000_000, delay_ns=1_000_000, flows=fl, rate_bps=10_000_000, size=64,
                    start_ns=100 * MS, stop_ns=130 * MS, sim_stop_ns=150 * MS)


def star_with_echo():
    """incast(15) with ICMP on and 130-byte frames (about 35 Receives at the hub in a wide window: a hub block), plus an echo pair between two leaves through the hub, plus a leaf flow to a leaf without
    a PacketSink (port unreachable through the hub): the hub block's serial node parts call the out-of-line code."""
    sc = p2p.Scenario(16, icmp=True)
    for i in range(1, 16):
        sc.link(i, 0, 10_000_000, 200_000, 100)
    sc.install_stack()
    for i in range(15):
        sc.assign_link(2 * i, 2 * i + 1, p2p.ip("10.0.0.0") + (i << 8))
    sc.add_sink(0, 0, 0)
    for i in range(1, 16):
        sc.add_onoff(i, 0, 100 * MS, 130 * MS, rate_bps=10_000_000, size=100, on_s=1.0, off_s=0.0,
                     remote_addr=sc.dev_addr[1])
    sc.add_echo_server(15, 50 * MS, 0)
    sc.add_echo_client(1, 15, 101 * MS, 140 * MS, count=20, interval_ns=1 * MS, size=200)
    sc.add_onoff(2, 14, 102 * MS, 130 * MS, rate_bps=1_000_000, size=100, on_s=1.0, off_s=0.0)
    sc.stop(150 * MS)
    sc.route_bfs()
    return sc


def extended():
    """The extended handlers (ports, fragmentation, a receive error model) beside plain column flows on a 4 x 4 grid:
    a UdpClient / UdpServer pair, an OnOff flow whose 3000-byte datagrams fragment, a ReceiveListErrorModel on the
    server's device (lost fragments: reassembly timeouts 20 ms later; the other timers are dispatched cancelled), and a
    flow to a port nobody is bound to."""
    g = p2p.Scenario(0, icmp=True, ports=True, frag=True, frag_timeout_ns=20 * MS)
    rows = cols = 4
    dev_of = {}
    for y in range(rows):
        for x in range(cols):
            g.add_node()
            if x > 0:
                dev_of[(nid(y, x - 1, 4), nid(y, x, 4))] = g.link(nid(y, x - 1, 4), nid(y, x, 4), 10_000_000, 200_000)
            if y > 0:
                dev_of[(nid(y - 1, x, 4), nid(y, x, 4))] = g.link(nid(y - 1, x, 4), nid(y, x, 4), 10_000_000, 200_000)
    g.install_stack()
    for k, (da, db) in enumerate(dev_of.values()):
        g.assign_link(da, db, p2p.ip("10.2.0.0") + (k << 8))

    for x in range(3):  # plain column flows
        g.add_sink(nid(3, x, 4), 0, 0, port=9)
        g.add_onoff(nid(0, x, 4), nid(3, x, 4), 100 * MS, 300 * MS, rate_bps=500_000, size=512, on_s=1e9, off_s=0.0,
                    remote_port=9)
    srv = nid(3, 3, 4)
    g.add_udp_server(srv, 50 * MS, 350 * MS, port=100)
    g.add_udp_client(nid(0, 3, 4), srv, 100 * MS, 300 * MS, count=40, interval_ns=4 * MS, size=400,
                     remote_port=100)
    g.add_sink(srv, 0, 0, port=9)
    g.add_onoff(nid(0, 0, 4), srv, 110 * MS, 300 * MS, rate_bps=1_000_000, size=3000, on_s=1e9, off_s=0.0,
                remote_port=9)
    g.add_onoff(nid(1, 0, 4), srv, 120 * MS, 300 * MS, rate_bps=200_000, size=100, on_s=1e9, off_s=0.0,
                remote_port=77)
    g.set_receive_list_error_model(dev_of[(nid(2, 3, 4), srv)][1], [1, 4, 9, 10, 30, 31, 50, 77])
    g.stop(400 * MS)
    g.route_bfs()
    return g
