"""Scenarios of the UdpTraceClient tests, shared by tests/test_udp_trace_cpu.py (what each must contain, asserted on
the model alone) and tests/test_gpu_udp_trace.py (the engine against the model).  Every one is a few hundred to a few
thousand events."""
import os

import nsref
import p2p
import p2p_trace_client_pyref as T
from udp_ports_cases import MS, S, line

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILES = ("udp_trace_newline.txt", "udp_trace_no_newline.txt", "udp_trace_decreasing.txt",
                "udp_trace_b_tail.txt", "udp_trace_one_line.txt", "udp_trace_exact_tiny.txt")


def golden(name):
    return os.path.join(GOLDEN, name)


def known_answer(flowmon=False):
    """UdpTraceClientServerTestCase (udp-client-server-test.cc:126-180) on a point-to-point link: UdpServer on node 1
    from 1 s to 10 s, UdpTraceClient (the default trace, MaxPacketSize 1400 - 28 = 1372) on node 0 from 2 s to 10 s:
    247 received, 0 lost."""
    sc = line(2, [(5_000_000, 2 * MS)])
    sc.flowmon = flowmon
    sc.add_udp_server(1, 1 * S, 10 * S, port=4000)
    sc.add_udp_trace_client(0, 1, 2 * S, 10 * S, max_packet_size=1372, remote_port=4000)
    sc.route_bfs()
    return sc


def overflow(flowmon=False):
    """A 400 kbit/s link with a 2-packet queue: the default trace's bursts of three and four datagrams overflow the
    sender's own DropTail inside one Send event, so the server sees gaps in the sequence numbers."""
    sc = line(2, [(400_000, 2 * MS)], qmax=2)
    sc.flowmon = flowmon
    sc.add_udp_server(1, 0, 0, port=100, window=32)
    sc.add_udp_trace_client(0, 1, 10 * MS, 0, max_packet_size=512, remote_port=100)
    sc.stop(2500 * MS)
    sc.route_bfs()
    return sc


def forwarded_ttl():
    """A three-node line with icmp: node 0's trace client sends over node 1 to node 2's server; a second trace client
    of node 0 has TTL 1, so each of its datagrams expires at node 1 and a time-exceeded error comes back."""
    sc = line(3, [(5_000_000, 1 * MS), (2_000_000, 1 * MS)], icmp=True)
    sc.add_udp_server(2, 0, 0, port=100, window=16)
    sc.add_udp_trace_client(0, 2, 10 * MS, 0, max_packet_size=1024, remote_port=100)
    sc.add_udp_trace_client(0, 2, 15 * MS, 0, entries=[(0, 300), (30, 700), (0, 80), (50, 1300)],
                            max_packet_size=600, remote_port=100, ttl=1)
    sc.stop(900 * MS)
    sc.route_bfs()
    return sc


def wrong_port():
    """A wrong remote port with icmp: node 1 binds port 100 only, node 0's trace client sends to 4001; the
    port-unreachable errors return to node 0, which hosts a bound UdpServer of its own (fed by node 1's client)."""
    sc = line(2, [(5_000_000, 1 * MS)], icmp=True)
    sc.add_udp_server(1, 0, 0, port=100)
    sc.add_udp_server(0, 0, 0, port=200, window=8)
    sc.add_udp_trace_client(0, 1, 10 * MS, 0, max_packet_size=1024, remote_port=4001)
    sc.add_udp_client(1, 0, 10 * MS, 0, count=8, interval_ns=50 * MS, size=40, remote_port=200)
    sc.stop(800 * MS)
    sc.route_bfs()
    return sc


def exact_and_tiny():
    """The golden trace with a frame MaxPacketSize divides exactly (2048 and 1024 at 1024: a 12-byte datagram after
    the full ones) and frames of 0, 5, 12 and 13 bytes."""
    sc = line(2, [(5_000_000, 1 * MS)])
    sc.add_udp_server(1, 0, 0, port=100)
    sc.add_udp_trace_client(0, 1, 10 * MS, 0, entries=T.load_trace(golden("udp_trace_exact_tiny.txt")),
                            max_packet_size=1024, remote_port=100)
    sc.stop(700 * MS)
    sc.route_bfs()
    return sc


def stop_mid_cycle():
    """The client stops 300 ms after its start, between the Sends at +240 and +360 ms: the cancelled Send is still
    dispatched at +360 ms and counted."""
    sc = line(2, [(5_000_000, 1 * MS)])
    sc.add_udp_server(1, 0, 0, port=100)
    sc.add_udp_trace_client(0, 1, 100 * MS, 400 * MS, max_packet_size=1024, remote_port=100)
    sc.stop(1 * S)
    sc.route_bfs()
    return sc


def no_route():
    """Node 2 is linked to nothing: its trace client's every SendPacket fails, m_sent stays 0 and the Send events go
    on until it is stopped; node 0's client works meanwhile."""
    sc = p2p.Scenario(3, ports=True)
    da, db = sc.link(0, 1, 5_000_000, 1 * MS)
    sc.install_stack()
    sc.assign_link(da, db, p2p.ip("10.1.1.0"))
    sc.add_udp_server(1, 0, 0, port=100)
    sc.add_udp_trace_client(0, 1, 10 * MS, 0, max_packet_size=1024, remote_port=100)
    sc.add_udp_trace_client(2, 1, 10 * MS, 700 * MS, max_packet_size=300, remote_port=100)
    sc.stop(1 * S)
    sc.route_bfs()
    return sc


def grid_pipelines(rows=4, cols=4):
    """p2p.grid's 4x4 topology in ports mode: every bottom-row node hosts two UdpServers (ports 100, 101) and a
    PacketSink (port 9); per column a trace client from the top row to the server on port 100 (MaxPacketSize 450 and
    1472 in turn, so some columns split frames and some do not), a UdpClient to port 101 of the next column and an OnOff
    flow to the sink.  No frame is below 180 bytes on the wire, which keeps the engine's windows wide (the deferred
    pipeline)."""
    sc = p2p.grid(rows, cols, flows=[])
    sc.ports = True
    sc.setup = [e for e in sc.setup if e[0] != p2p.SETUP_STOP]
    nid = lambda y, x: y * cols + x  # noqa: E731
    entries = [(0, 600), (8, 1300), (0, 400), (0, 1100), (12, 700)]
    for x in range(cols):
        sc.add_udp_server(nid(rows - 1, x), 0, 0, port=100, window=16)
        sc.add_udp_server(nid(rows - 1, x), 0, 0, port=101, window=16)
        sc.add_sink(nid(rows - 1, x), 0, 0, port=9)
    for x in range(cols):
        sc.add_udp_trace_client(nid(0, x), nid(rows - 1, x), 10 * MS + x * 100_000, 0, entries=entries[x:] + entries[:x],
                                max_packet_size=450 if x % 2 == 0 else 1472, remote_port=100)
        sc.add_udp_client(nid(0, x), nid(rows - 1, (x + 1) % cols), 11 * MS, 0, count=12, interval_ns=5 * MS,
                          size=150, remote_port=101)
        sc.add_onoff(nid(0, (x + 1) % cols), nid(rows - 1, x), 10 * MS, 60 * MS, rate_bps=1_000_000, size=300,
                     on_s=1.0, off_s=0.0, remote_port=9)
    sc.stop(100 * MS)
    sc.route_bfs()
    return sc


def _star(n_leaves, extra=0):
    sc = p2p.Scenario(n_leaves + 1 + extra, ports=True)
    ld = [sc.link(i, 0, 10_000_000, 1 * MS, 100) for i in range(1, n_leaves + 1 + extra)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.0.0.0") + (k << 8))
    return sc


# a 256-byte UdpClient datagram's frame (286 bytes) over a star link: Seconds (CalculateTxTime) + the channel's delay
HUB_ARRIVAL = nsref.seconds(float(286) * 8 / float(10_000_000)) + 1 * MS


def hub_forwards_bursts(n_src=24):
    """A star whose hub only forwards: 24 leaves each run a trace client (the default trace, MaxPacketSize 400: bursts
    of up to eight datagrams), all started at once, towards a UdpServer on one more leaf — every window holds the
    bursts' same-time Receives at the hub (a hub block)."""
    sc = _star(n_src, 1)
    dst = n_src + 1
    sc.add_udp_server(dst, 0, 0, port=100, window=64)
    for i in range(1, n_src + 1):
        sc.add_udp_trace_client(i, dst, 1 * S, 0, max_packet_size=400, remote_port=100)
    sc.stop(1 * S + 300 * MS)
    sc.route_bfs()
    return sc


def hub_hosts_client(n_src=24):
    """The same star, the other way: the hub hosts a trace client towards leaf 1's server while 24 leaves' UdpClients
    send to the hub's own server at once.  The client starts when the leaves' first datagrams arrive (286 bytes at 10
    Mbit/s and 1 ms: HUB_ARRIVAL after their start) and its Sends keep the leaves' 4 ms period, so every Send shares
    its timestamp with 24 Receives at the hub and runs inside a hub block (its serial node part, then the burst's
    device steps)."""
    sc = _star(n_src)
    sc.add_udp_server(0, 0, 0, port=100, window=64)
    sc.add_udp_server(1, 0, 0, port=100, window=16)
    sc.add_udp_trace_client(0, 1, 1 * S + HUB_ARRIVAL, 0, entries=[(0, 900), (4, 700), (0, 300), (0, 100), (4, 1200)],
                            max_packet_size=400, remote_port=100)
    for i in range(1, n_src + 1):
        sc.add_udp_client(i, 0, 1 * S, 0, count=12, interval_ns=4 * MS, size=256, remote_port=100)
    sc.stop(1 * S + 60 * MS)
    sc.route_bfs()
    return sc


def rate_error_model():
    """A byte-unit Rate error model on the receiving device of a link that carries a trace client's datagrams of many
    sizes: the threshold is looked up by each frame's own size."""
    sc = line(2, [(5_000_000, 1 * MS)])
    sc.add_udp_server(1, 0, 0, port=100, window=32)
    sc.add_udp_trace_client(0, 1, 10 * MS, 0, max_packet_size=700, remote_port=100)
    sc.set_rate_error_model(1, 0.0004, unit="byte", stream=0)
    sc.stop(1500 * MS)
    sc.route_bfs()
    return sc
