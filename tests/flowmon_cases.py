"""Scenarios of the per-flow statistics tests, shared by tests/test_flowmon_cpu.py (hand-computed answers, and the
conditions the scenarios must meet, asserted on the Python model alone: tests/p2p_flowmon_pyref.py) and
tests/test_gpu_flowmon.py (the engine against the model).  Every scenario is small: a model run takes well under a
second."""
import errmodel_cases as EC
import p2p
import p2p_fuzz_cases as FC

MS, US = 1_000_000, 1_000
SMALL_DELAY_NS = 1 * MS  # the second max_delay of every comparison (the first: the reference's 10 s)


def monitored(sc):
    sc.flowmon = True
    return sc


def first_cc():
    return monitored(p2p.first_cc())


def chain3(count=1):
    """Three nodes in a line (10 Mb/s, 1 ms; 5 Mb/s, 3 ms): one UdpClient datagram of 100 bytes from node 0 to a
    UdpServer on node 2."""
    sc = EC.line(3, [(10_000_000, 1 * MS), (5_000_000, 3 * MS)], ports=True)
    sc.add_udp_server(2, 0, 0, port=100, window=8)
    sc.add_udp_client(0, 2, 1 * MS, 0, count=count, interval_ns=1 * MS, size=100, remote_port=100)
    sc.stop(50 * MS)
    sc.route_bfs()
    return monitored(sc)


def incast3():
    """p2p.incast (3): every leaf offers 4 Mb/s to its own 1 Mb/s link with a 3-packet queue: the sender's own
    DropTail queue drops (DROP_QUEUE before the first hop), and the delays of what passes grow (jitter)."""
    return monitored(p2p.incast(3, bps=1_000_000, delay_ns=1 * MS, qmax=3, rate_bps=4_000_000, size=200,
                                start_ns=1 * MS, stop_ns=40 * MS, sim_stop_ns=45 * MS))


def dumbbell4():
    """A 4-leaf dumbbell in ports mode with one flow of every kind from left leaf i to right leaf i: OnOff to a
    PacketSink, UdpEchoClient to a UdpEchoServer (a reply flow), UdpClient to a UdpServer, and a UdpClient to a port
    nothing is bound to (its datagrams still count as received).  The 1 Mb/s router link with a 4-packet queue drops
    at a forwarder (both ways) and spreads the delays; Simulator::Stop comes while datagrams are in flight."""
    n = 4
    sc = p2p.Scenario(2 * n + 2, ports=True)
    r1, r2 = n, n + 1
    links = [sc.link(r1, r2, 1_000_000, 2 * MS, 4)]
    links += [sc.link(i, r1, 10_000_000, 500 * US, 20) for i in range(n)]
    links += [sc.link(n + 2 + i, r2, 10_000_000, 500 * US, 20) for i in range(n)]
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.1.0.0") + (k << 8))
    right = lambda i: n + 2 + i  # noqa: E731
    sc.add_sink(right(0), 0, 0, port=9)
    sc.add_echo_server(right(1), 0, 0, port=9)
    sc.add_udp_server(right(2), 0, 0, port=100, window=32)
    sc.add_udp_server(right(3), 0, 0, port=100, window=32)
    sc.add_onoff(0, right(0), 1 * MS, 0, rate_bps=2_000_000, size=300, on_s=0.004, off_s=0.002, remote_port=9)
    sc.add_echo_client(1, right(1), 1 * MS + 100 * US, 0, count=12, interval_ns=1500 * US, size=150, remote_port=9)
    sc.add_udp_client(2, right(2), 2 * MS, 0, count=30, interval_ns=700 * US, size=120, remote_port=100)
    sc.add_udp_client(3, right(3), 2 * MS + 50 * US, 0, count=10, interval_ns=2 * MS, size=64, remote_port=77)
    sc.stop(24 * MS)
    sc.route_bfs()
    return monitored(sc)


def grid3(icmp):
    """A 3x3 grid with three flows: 0 -> 8 with TTL 2 (it expires at the second forwarder; with icmp the
    time-exceeded error goes back), 3 -> 5 whose route the forwarder between them lacks (DROP_NO_ROUTE at node 4),
    and 2 -> 6, which arrives."""
    sc = p2p.grid(3, 3, flows=[(0, 8), (3, 5), (2, 6)], start_ns=1 * MS, stop_ns=12 * MS, sim_stop_ns=30 * MS,
                  rate_bps=2_000_000, size=256, on_s=1.0, off_s=0.0, ttl=64, icmp=icmp)
    flow = {(a["node"], a["dst"]): i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_ONOFF}
    sc.apps[flow[(0, 8)]]["ttl"] = 2
    sc.route[4, sc.dst_slot[5]] = p2p.NO_ROUTE
    return monitored(sc)


def chain_errmodel():
    """A three-node chain, UdpClients both ways between UdpServers on the ends: a ReceiveList on the forwarder's
    incoming device (1) and a Rate EU_PKT 0.3 model on node 2's device (3) eat frames, whose datagrams stay tracked
    and are lost by timeout only."""
    sc = EC.line(3, [(10_000_000, 500 * US), (10_000_000, 500 * US)], ports=True, rng_seed=1, rng_run=2)
    sc.add_udp_server(2, 0, 0, port=100, window=8)
    sc.add_udp_server(0, 0, 0, port=100, window=8)
    sc.add_udp_client(0, 2, 1 * MS, 0, count=24, interval_ns=500 * US, size=100, remote_port=100)
    sc.add_udp_client(2, 0, 1 * MS + 30 * US, 0, count=10, interval_ns=1 * MS, size=60, remote_port=100)
    sc.stop(40 * MS)
    sc.route_bfs()
    sc.set_receive_list_error_model(1, [1, 5, 6])
    sc.set_rate_error_model(3, 0.3, unit="pkt", stream=0)
    return monitored(sc)


def hub_dumbbell(n_leaves=40):
    """p2p.dumbbell with n_leaves leaves a side, two 512-byte datagrams a leaf, all leaves alike: router 1 takes
    n_leaves same-time Receives (more than CH = 16 events of one node in a window: a hub block, whose forwarding
    lanes report ReportForwarding and whose serial device pass reports the bottleneck's 8-packet queue's drops)."""
    return monitored(p2p.dumbbell(n_leaves, qmax=8, max_bytes=1024, compressed=False))


def star15():
    """15 leaves on a hub with identical links and a bottleneck to a far node (16 devices: the largest degree a wide
    engine takes), every leaf sending three 1000-byte datagrams back to back: a wide window holds several of the
    hub's same-time Receive groups."""
    L = 15
    hub, far = L, L + 1
    sc = p2p.Scenario(L + 2, ports=True)
    links = [sc.link(i, hub, 10_000_000, 2 * MS, 20) for i in range(L)]
    links.append(sc.link(hub, far, 20_000_000, 1 * MS, 12))
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.1.0.0") + (k << 8))
    sc.add_sink(far, 0, 0, port=9)
    for i in range(L):
        sc.add_onoff(i, far, 1 * MS, 0, rate_bps=100_000_000, size=1000, on_s=1.0, off_s=0.0, max_bytes=3000,
                     remote_port=9)
    sc.stop(30 * MS)
    sc.route_bfs()
    return monitored(sc)


def id_limit(count):
    """Two nodes on a 10 Gb/s link with a 1 ms delay: one UdpClient sends `count` minimum-size datagrams 100 ns
    apart (a 42-byte frame takes 34 ns), so a window holds thousands of events."""
    sc = EC.line(2, [(10_000_000_000, 1 * MS)], ports=True)
    sc.add_udp_server(1, 0, 0, port=100, window=8)
    sc.add_udp_client(0, 1, 1 * MS, 0, count=count, interval_ns=100, size=12, remote_port=100)
    sc.stop(20 * MS)
    sc.route_bfs()
    return monitored(sc)


# mesh seeds of tests/p2p_fuzz_cases.py: the first six draw no fragmenting flow (found by scanning the generator,
# which tests/test_flowmon_cpu.py repeats for them), the last two do and are skipped
FUZZ_SEEDS = (70, 71, 88, 444, 914, 1537, 0, 5)


def fuzz(seed):
    """p2p_fuzz_cases' mesh (seed) with the monitor on and frag off, or None when the seed draws a fragmenting flow
    (flowmon with frag is refused)."""
    sc = FC.build("mesh", seed)
    if FC.fragmenting_flows(sc):
        return None
    sc.frag = False
    return monitored(sc)


# (name, args) of the scenarios tests/test_gpu_flowmon.py compares with the model
GPU_CASES = (("first_cc", ()), ("chain3", (3,)), ("incast3", ()), ("dumbbell4", ()), ("grid3", (False,)),
             ("grid3", (True,)), ("chain_errmodel", ()), ("hub_dumbbell", ()), ("star15", ()))
