"""Scenarios of the UDP-ports tests, shared by tests/test_udp_ports_cpu.py (the conditions each must meet, asserted
on the model alone) and tests/test_gpu_udp_ports.py (the engine against the model)."""
import numpy as np

import p2p

MS, S = 1_000_000, 1_000_000_000


def line(n, links, icmp=False, qmax=100):
    """n nodes in a line; links[i] = (bps, delay_ns) of link i -> i + 1; a ports-mode scenario with addresses."""
    sc = p2p.Scenario(n, icmp=icmp, ports=True)
    ld = [sc.link(i, i + 1, bps, dl, qmax) for i, (bps, dl) in enumerate(links)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.1.1.0") + (k << 8))
    return sc


def udp_client_server():
    """UdpClientServerTestCase (udp-client-server-test.cc:65-112) on a point-to-point link: UdpServer (port 4000) on
    node 1 from 1 s to 10 s, UdpClient (MaxPackets 10, Interval 1 s, PacketSize 1024) on node 0 from 2 s to 10 s:
    the server receives 8 (the sends at 2 .. 9 s), loses 0."""
    sc = line(2, [(5_000_000, 2 * MS)])
    sc.add_udp_server(1, 1 * S, 10 * S, port=4000)
    sc.add_udp_client(0, 1, 2 * S, 10 * S, count=10, interval_ns=1 * S, size=1024, remote_port=4000)
    sc.route_bfs()
    return sc


def three_endpoints():
    """Node 1: a PacketSink (port 9), a UdpServer (4000) and a UdpEchoServer (7); node 0: an OnOff, a UdpClient and
    a UdpEchoClient, one to each port."""
    sc = line(2, [(5_000_000, 2 * MS)])
    sc.add_sink(1, 0, 0, port=9)
    sc.add_udp_server(1, 0, 0, port=4000)
    sc.add_echo_server(1, 0, 0, port=7)
    sc.add_onoff(0, 1, 100 * MS, 400 * MS, rate_bps=500_000, size=200, on_s=1.0, off_s=0.0, remote_port=9)
    sc.add_udp_client(0, 1, 100 * MS, 400 * MS, count=20, interval_ns=7 * MS, size=100, remote_port=4000)
    sc.add_echo_client(0, 1, 100 * MS, 400 * MS, count=5, interval_ns=31 * MS, size=64, remote_port=7)
    sc.stop(500 * MS)
    sc.route_bfs()
    return sc


def port_mismatch(icmp):
    """A 3-node line: node 2's UdpServer binds port 4000; one UdpClient of node 0 sends there, another to port 4001,
    which nobody binds (RX_ENDPOINT_UNREACH; with icmp the port-unreachable error travels back over node 1)."""
    sc = line(3, [(5_000_000, 1 * MS), (5_000_000, 1 * MS)], icmp=icmp)
    sc.add_udp_server(2, 0, 0, port=4000)
    sc.add_udp_client(0, 2, 10 * MS, 0, count=6, interval_ns=5 * MS, size=64, remote_port=4000)
    sc.add_udp_client(0, 2, 12 * MS, 0, count=6, interval_ns=5 * MS, size=80, remote_port=4001, ttl=33)
    sc.stop(100 * MS)
    sc.route_bfs()
    return sc


def loss_reorder(window):
    """A 3-node line with a slow second link (200 kbit/s) and a 2-packet queue: two UdpClients feed one UdpServer on
    node 2.  Client A (node 0) sends a 100-byte datagram every ms, five times what the link carries, so most are
    dropped at node 1 (losses).  Client B (node 1) joins at 150 ms with a few 1400-byte datagrams: its low sequence
    numbers arrive below lastMaxSeq, and each holds the link for 57 ms, a gap of more than 32 of A's numbers."""
    sc = line(3, [(10_000_000, 1 * MS), (200_000, 2 * MS)], qmax=2)
    sc.add_udp_server(2, 0, 0, port=100, window=window)
    sc.add_udp_client(0, 2, 10 * MS, 0, count=400, interval_ns=1 * MS, size=100, remote_port=100)
    sc.add_udp_client(1, 2, 150 * MS, 0, count=8, interval_ns=40 * MS, size=1400, remote_port=100)
    sc.stop(600 * MS)
    sc.route_bfs()
    return sc


def stopped_server_no_route():
    """The two semantics that differ from the echo pair: node 1's UdpServer stops at 50 ms while node 0's client
    keeps sending (the datagrams still find the endpoint: a DoForwardUp each, nothing counted, no ICMP); node 2 is
    not linked to anything, so its UdpClient's Send fails every Interval with m_sent staying 0, until it is stopped."""
    sc = p2p.Scenario(3, icmp=True, ports=True)
    da, db = sc.link(0, 1, 5_000_000, 1 * MS)
    sc.install_stack()
    sc.assign_link(da, db, p2p.ip("10.1.1.0"))
    sc.add_udp_server(1, 0, 50 * MS, port=100)
    sc.add_udp_client(0, 1, 10 * MS, 0, count=12, interval_ns=8 * MS, size=50, remote_port=100)
    sc.add_udp_client(2, 1, 10 * MS, 60 * MS, count=5, interval_ns=10 * MS, size=50, remote_port=100)
    sc.stop(200 * MS)
    sc.route_bfs()
    return sc


def icmp_back_to_endpoints():
    """ICMP errors returning to a node that is a sender and hosts two bound endpoints (its Receives go through the
    per-flow endpoint table; an error's descriptor holds flag bits above its flow and must find no endpoint): a
    3-node line with icmp; node 0 hosts a PacketSink (port 9), a UdpServer (port 100) and two UdpClients towards
    node 2 — one to a port nobody binds (port unreachable, sent back from node 2), one with TTL 1 (time exceeded,
    sent back from node 1); node 2's own UdpClient and OnOff feed node 0's two endpoints meanwhile."""
    sc = line(3, [(5_000_000, 1 * MS), (5_000_000, 1 * MS)], icmp=True)
    sc.add_sink(0, 0, 0, port=9)
    sc.add_udp_server(0, 0, 0, port=100, window=8)
    sc.add_udp_server(2, 0, 0, port=4000)
    sc.add_udp_client(0, 2, 10 * MS, 0, count=5, interval_ns=3 * MS, size=40, remote_port=4001)
    sc.add_udp_client(0, 2, 11 * MS, 0, count=4, interval_ns=3 * MS, size=60, remote_port=4000, ttl=1)
    sc.add_udp_client(2, 0, 10 * MS, 0, count=6, interval_ns=2 * MS, size=30, remote_port=100)
    sc.add_onoff(2, 0, 10 * MS, 30 * MS, rate_bps=400_000, size=100, on_s=1.0, off_s=0.0, remote_port=9)
    sc.stop(60 * MS)
    sc.route_bfs()
    return sc


def hub_forwarding(n_src=24):
    """A star whose hub only forwards: n_src leaves each run a UdpClient, all started at once, towards a UdpServer
    on one more leaf, so every window holds n_src same-time Receives at the hub that IpForward sends on (the hub
    blocks' stateless forwarders, with datagrams that carry sequence numbers).  Leaf 3's datagrams leave with TTL 1
    and expire at the hub (icmp off: counted and traced, the Drop record with the TTL word as received)."""
    sc = p2p.Scenario(n_src + 2, ports=True)
    dst = n_src + 1
    ld = [sc.link(i, 0, 10_000_000, 1 * MS, 100) for i in range(1, n_src + 2)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.0.0.0") + (k << 8))
    sc.add_udp_server(dst, 0, 0, port=100, window=32)
    for i in range(1, n_src + 1):
        sc.add_udp_client(i, dst, 1 * S, 0, count=5, interval_ns=4 * MS, size=256, remote_port=100,
                          ttl=1 if i == 3 else 64)
    sc.stop(1 * S + 40 * MS)
    sc.route_bfs()
    return sc


def grid_pipelines(rows=4, cols=4):
    """p2p.grid's 4x4 topology (PointToPointGridHelper, its addresses) in ports mode: every bottom-row node hosts a
    UdpServer (port 100) and a PacketSink (port 9); a UdpClient column flow per column runs from the top row to its
    server, an OnOff flow from the top of the next column to the sink beside it (XY routes by route_bfs)."""
    sc = p2p.grid(rows, cols, flows=[])  # (no flows: the topology, stack and addresses)
    sc.ports = True
    sc.setup = [e for e in sc.setup if e[0] != p2p.SETUP_STOP]  # (Simulator::Stop comes after the applications)
    nid = lambda y, x: y * cols + x  # noqa: E731
    for x in range(cols):
        sc.add_udp_server(nid(rows - 1, x), 0, 0, port=100, window=16)
        sc.add_sink(nid(rows - 1, x), 0, 0, port=9)
    for x in range(cols):
        sc.add_udp_client(nid(0, x), nid(rows - 1, x), 10 * MS + x * 100_000, 0, count=25, interval_ns=2 * MS,
                          size=200 + 8 * x, remote_port=100)
        sc.add_onoff(nid(0, (x + 1) % cols), nid(rows - 1, x), 10 * MS, 60 * MS, rate_bps=2_000_000, size=300,
                     on_s=1.0, off_s=0.0, remote_port=9)
    sc.stop(100 * MS)
    sc.route_bfs()
    return sc


def incast_hub(n_src=32):
    """p2p.incast (32) with ports: the hub hosts a PacketSink (port 9) and a UdpServer (port 100); the odd sources
    are OnOff flows to the sink, the even ones UdpClients to the server, all started at once (hub blocks)."""
    sc = p2p.Scenario(n_src + 1, ports=True)
    for i in range(1, n_src + 1):
        sc.link(i, 0, 10_000_000, 1 * MS, 100)
    sc.install_stack()
    for i in range(n_src):
        sc.assign_link(2 * i, 2 * i + 1, p2p.ip("10.0.0.0") + (i << 8))
    sc.add_sink(0, 0, 0, port=9)
    sc.add_udp_server(0, 0, 0, port=100, window=32)
    for i in range(1, n_src + 1):
        if i % 2:
            sc.add_onoff(i, 0, 1 * S, 1 * S + 20 * MS, rate_bps=1_000_000, size=512, on_s=1.0, off_s=0.0,
                         remote_port=9)
        else:
            sc.add_udp_client(i, 0, 1 * S, 0, count=6, interval_ns=4 * MS, size=512, remote_port=100)
    sc.stop(1 * S + 40 * MS)
    sc.route_bfs()
    return sc


def loss_counter_kat():
    """PacketLossCounterTestCase (udp-client-server-test.cc:208-257): (window, the sequence numbers it notifies in
    order, the index of the last one before each NS_TEST_ASSERT, the GetLost () each assert expects: 0, 1, 7, 7
    again after the reordering without loss, 9)."""
    seq, cp = [32], []                          # "out of order"
    seq += range(0, 64)
    cp.append(len(seq) - 1)                     # 0
    seq += range(65, 128)                       # drop (1) seqNum 64
    cp.append(len(seq) - 1)                     # 1
    seq += range(134, 200)                      # drop seqNum 128 .. 133
    cp.append(len(seq) - 1)                     # 7
    seq += [205, 206, 207, 200, 201, 202, 203, 204]   # reordering without loss
    seq += range(205, 250)
    cp.append(len(seq) - 1)                     # 7
    seq += [255, 252, 253, 254]                 # reordering with loss: drop (2) seqNum 250, 251
    seq += range(256, 300)
    cp.append(len(seq) - 1)                     # 9
    return 32, np.array(seq, np.uint32), cp, [0, 1, 7, 7, 9]


def random_sequences(window, seed, n=300):
    """Sequence numbers with small forward gaps on both sides of the window, reordering, and two large gaps (5 x 10^4
    and 10^6: a loop that ran the gap's length would show), for the three counters to agree on after every element."""
    rng = np.random.default_rng(seed)
    cur, out = 0, []
    for k in range(n):
        r = rng.random()
        if k in (n // 3, 2 * n // 3):
            cur += 50_000 if k == n // 3 else 1_000_000
        elif r < 0.55:
            cur += 1
        elif r < 0.80:
            cur += int(rng.integers(2, 2 * window + 3))
        else:  # an older one again
            out.append(max(0, cur - int(rng.integers(1, 3 * window))))
            continue
        out.append(cur)
    return np.array(out, np.uint32)


def library_losses(window, seq, on_device, limit_s=None):
    """nsgpu_loss_counter_run: GetLost () after every element, by the library's function on the host or in its
    one-thread kernel.  limit_s: a time limit for the call, sized for the bounded loop."""
    import ctypes as C
    import time

    import nsgpu
    seq = np.ascontiguousarray(seq, np.uint32)
    out = np.zeros(len(seq), np.uint32)
    t0 = time.perf_counter()
    nsgpu.check(nsgpu.lib().nsgpu_loss_counter_run(window, seq.ctypes.data, len(seq), out.ctypes.data,
                                                   1 if on_device else 0, C.c_void_p(None)))
    if limit_s is not None:
        assert time.perf_counter() - t0 < limit_s
    return out
