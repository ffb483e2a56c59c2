"""Scenarios of the IPv4 fragmentation tests, shared by tests/test_frag_cpu.py (the conditions each must meet,
asserted on the model alone) and tests/test_gpu_frag.py (the engine against the model, tests/p2p_frag_pyref.py)."""
import p2p

MS, US, S = 1_000_000, 1_000, 1_000_000_000


def line(n, links, icmp=False, ports=False, qmax=100, timeout_ns=0):
    """n nodes in a line with frag on; links[i] = (bps, delay_ns) or (bps, delay_ns, qmax) of link i -> i + 1."""
    sc = p2p.Scenario(n, icmp=icmp, ports=ports, frag=True, frag_timeout_ns=timeout_ns)
    ld = [sc.link(i, i + 1, l[0], l[1], l[2] if len(l) > 2 else qmax) for i, l in enumerate(links)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.1.1.0") + (k << 8))
    return sc


def echo_2000():
    """UdpEchoClient with PacketSize 2000 on two nodes: two fragments each way, three datagrams."""
    sc = line(2, [(5_000_000, 2 * MS)])
    sc.add_echo_server(1, 0, 0)
    sc.add_echo_client(0, 1, 1 * MS, 0, count=3, interval_ns=9 * MS, size=2000)
    sc.stop(60 * MS)
    sc.route_bfs()
    return sc


def forwarding_4000():
    """A 4000-byte OnOff over a 3-node line: node 1 forwards the three fragments of every datagram."""
    sc = line(3, [(10_000_000, 1 * MS), (10_000_000, 1 * MS)])
    sc.add_sink(2, 0, 0)
    sc.add_onoff(0, 2, 1 * MS, 30 * MS, rate_bps=8_000_000, size=4000, on_s=1.0, off_s=0.0)
    sc.stop(50 * MS)
    sc.route_bfs()
    return sc


def largest():
    """One 65507-byte datagram (MAX_IPV4_UDP_DATAGRAM_SIZE), qmax 100: 45 fragments."""
    sc = line(2, [(100_000_000, 1 * MS)], qmax=100)
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=100_000_000, size=65507, on_s=1.0, off_s=0.0, max_bytes=65507)
    sc.stop(20 * MS)
    sc.route_bfs()
    return sc


def sender_overflow():
    """A 5-fragment datagram (7000 bytes) into the sender's own 2-packet queue: the first fragment starts
    transmitting, two queue, two are dropped; the receiver's buffer never completes and its timer fires (4 ms)."""
    sc = line(2, [(10_000_000, 1 * MS)], qmax=2, timeout_ns=4 * MS)
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=4_000_000, size=7000, on_s=1.0, off_s=0.0, max_bytes=14000)
    sc.stop(40 * MS)
    sc.route_bfs()
    return sc


def loss_at_forwarder(icmp):
    """A 3-node line with a slow second link (5 Mbit/s) and a 3-packet queue at the forwarder, an 8 ms timeout: node 0
    sends 4000-byte datagrams (three fragments) faster than the second link carries them, in two bursts.  Fragments
    are lost at node 1, so node 2's one buffer mixes consecutive datagrams (entire with a list longer than a
    datagram's own three fragments), timers fire on what never completes (with icmp: a time-exceeded error back to
    node 0 whenever the prefix at offset 0 is there), and the timers of the completed ones are dispatched cancelled."""
    sc = line(3, [(20_000_000, 200 * US), (5_000_000, 300 * US, 3)], icmp=icmp, timeout_ns=8 * MS)
    sc.add_sink(2, 0, 0)
    sc.add_onoff(0, 2, 1 * MS, 0, rate_bps=10_000_000, size=4000, on_s=0.02, off_s=0.03)
    sc.stop(110 * MS)
    sc.route_bfs()
    return sc


def ttl_expiry():
    """Fragments with TTL 1 expire at the forwarder of a 3-node line with icmp: one time-exceeded error a fragment."""
    sc = line(3, [(10_000_000, 1 * MS), (10_000_000, 1 * MS)], icmp=True)
    sc.add_sink(2, 0, 0)
    sc.add_onoff(0, 2, 1 * MS, 0, rate_bps=8_000_000, size=3000, on_s=1.0, off_s=0.0, max_bytes=9000, ttl=1)
    sc.stop(30 * MS)
    sc.route_bfs()
    return sc


def port_unreachable():
    """Ports and icmp: 2000-byte datagrams to a port nobody binds.  The reassembled datagram is RX_ENDPOINT_UNREACH
    and the error's offending header is the last-arrived fragment's (length 548, not the datagram's)."""
    sc = line(3, [(10_000_000, 1 * MS), (10_000_000, 1 * MS)], icmp=True, ports=True)
    sc.add_sink(2, 0, 0, port=9)
    sc.add_onoff(0, 2, 1 * MS, 0, rate_bps=4_000_000, size=2000, on_s=1.0, off_s=0.0, max_bytes=6000, remote_port=10)
    sc.stop(30 * MS)
    sc.route_bfs()
    return sc


def udp_client_1500(count=40):
    """UdpClient with PacketSize 1500 (what its checker allows, udp-client.cc:70) to a UdpServer, with ports: every
    datagram is a 1500-byte and a 48-byte fragment.  The second link's 4-packet queue loses some fragments, so the
    server's received / lost counts and the sequence numbers that survive reassembly are all exercised."""
    sc = line(3, [(10_000_000, 500 * US), (3_000_000, 500 * US, 4)], ports=True, timeout_ns=5 * MS)
    sc.add_udp_server(2, 0, 0, port=100, window=32)
    sc.add_udp_client(0, 2, 1 * MS, 0, count=count, interval_ns=2 * MS, size=1500, remote_port=100)
    sc.stop(120 * MS)
    sc.route_bfs()
    return sc


def grid_pipelines(rows=8, cols=8):
    """p2p.grid's 8x8 topology with one fragmenting flow a destination: a 4352-byte OnOff flow down every column
    (fragments of 1500, 1500 and 1420 bytes: the smallest frame is large enough for create to grant wide windows, so
    the default engine runs the deferred pipeline with local records)."""
    sc = p2p.grid(rows, cols, start_ns=1 * MS, stop_ns=14 * MS, sim_stop_ns=60 * MS, rate_bps=8_000_000, size=4352,
                  on_s=1.0, off_s=0.0)
    sc.frag = True
    return sc


def hub_forwards(n_src=24):
    """A star whose hub only forwards fragments: n_src leaves, the first half each send 2500-byte datagrams (two
    fragments) to its partner in the second half, all started at once (hub blocks, the stateless forwarders)."""
    sc = p2p.Scenario(n_src + 1, frag=True)
    ld = [sc.link(i, 0, 10_000_000, 1 * MS, 100) for i in range(1, n_src + 1)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.0.0.0") + (k << 8))
    half = n_src // 2
    for i in range(1, half + 1):
        sc.add_sink(half + i, 0, 0)
    for i in range(1, half + 1):
        sc.add_onoff(i, half + i, 1 * S, 0, rate_bps=4_000_000, size=2500, on_s=1.0, off_s=0.0, max_bytes=7500)
    sc.stop(1 * S + 30 * MS)
    sc.route_bfs()
    return sc


def hub_echo_server(n_src=24):
    """A star whose hub hosts a UdpEchoServer: leaf 1 sends it 3000-byte echoes (reassembly at the hub, and the reply a
    three-fragment send from it), the leaves 3 .. n_src send 200-byte datagrams through the hub to a sink on leaf 1.
    Their start is timed so that their same-time Receives reach the hub 10 us after an echo's last fragment does:
    less than the smallest frame's 56 us, so the window of the server's queued DoForwardUp — the multi-fragment
    send — ends at those Receives and holds them too (a Receive's lookahead is 0 with an echo application).  That is a
    hub window whose device steps are all on the hub's device towards leaf 1: what the parallel device scan takes,
    and must decline here for the serial pass."""
    sc = p2p.Scenario(n_src + 1, ports=True, frag=True)
    ld = [sc.link(i, 0, 10_000_000, 1 * MS, 100) for i in range(1, n_src + 1)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.0.0.0") + (k << 8))
    sc.add_echo_server(0, 0, 0, port=7)
    sc.add_sink(1, 0, 0, port=9)
    sc.add_echo_client(1, 0, 1 * S, 0, count=3, interval_ns=8 * MS, size=3000, remote_port=7)
    # the request's fragments (1502, 1502 and 70 bytes on the wire at 10 Mbit/s) and the link's 1 ms: the last one is at
    # the hub 3459.2 us after the Send; a leaf's first datagram (232 bytes on the wire) 1.6 ms + 185.6 us + 1 ms after
    # its start
    start = 1 * S + 3_459_200 + 10 * US - (1_600_000 + 185_600 + 1 * MS)
    for i in range(3, n_src + 1):
        sc.add_onoff(i, 1, start, 0, rate_bps=1_000_000, size=200, on_s=1.0, off_s=0.0, max_bytes=3000, remote_port=9)
    sc.stop(1 * S + 40 * MS)
    sc.route_bfs()
    return sc


def hub_timeout(n_src=24, timeout_ns=3_982_400):
    """A star whose hub is the destination of a fragmenting flow, with icmp: leaf 1 sends it one 3000-byte datagram
    through its own 1-packet queue, which drops the last fragment, so the hub's buffer never completes and its timer
    fires.  The leaves 3 .. n_src burst 200-byte datagrams through the hub to a sink on leaf 1 every 1.6 ms, and the
    timeout is chosen so that the timer fires at the very time of one burst's Receives (the first fragment is at the
    hub 1 s + 3 ms + 1201.6 us + 1 ms after the start, the fifth burst 1.6 ms + 184 us + 1 ms + 4 x 1.6 ms; to the
    nanosecond as the model's log has them, which tests/test_frag_cpu.py asserts).  That window is a
    hub window whose device steps — 22 forwards and the time-exceeded error — are all on the hub's device towards
    leaf 1: what the parallel device scan takes, and must decline for the Drop record that follows the error."""
    sc = p2p.Scenario(n_src + 1, icmp=True, ports=True, frag=True, frag_timeout_ns=timeout_ns)
    ld = [sc.link(i, 0, 10_000_000, 1 * MS, 100) for i in range(1, n_src + 1)]
    sc.dev[0][5] = 1  # leaf 1's own DropTail queue: MaxPackets 1
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.0.0.0") + (k << 8))
    sc.add_sink(0, 0, 0, port=9)
    sc.add_sink(1, 0, 0, port=9)
    sc.add_onoff(1, 0, 1 * S, 0, rate_bps=8_000_000, size=3000, on_s=1.0, off_s=0.0, max_bytes=3000, remote_port=9)
    for i in range(3, n_src + 1):
        sc.add_onoff(i, 1, 1 * S, 0, rate_bps=1_000_000, size=200, on_s=1.0, off_s=0.0, max_bytes=2000, remote_port=9)
    sc.stop(1 * S + 30 * MS)
    sc.route_bfs()
    return sc


def list_overflow():
    """The reassembly list's limit: 7000-byte datagrams into the sender's 2-packet queue lose their last two fragments
    every time, and with the default 30 s timeout the receiver's one buffer keeps the three that arrive of each:
    the 43rd datagram's third fragment would be entry 129."""
    sc = line(2, [(10_000_000, 1 * MS)], qmax=2)
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=4_000_000, size=7000, on_s=1.0, off_s=0.0, max_bytes=7000 * 44)
    sc.stop(700 * MS)
    sc.route_bfs()
    return sc


def reference_whole(size):
    """Ipv4FragmentationTest (ipv4-fragmentation-test.cc:312-398), the datagrams that arrive whole: one `size`-byte
    datagram between two nodes."""
    sc = line(2, [(5_000_000, 2 * MS)])
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=50_000_000, size=size, on_s=1.0, off_s=0.0, max_bytes=size)
    sc.stop(400 * MS)
    sc.route_bfs()
    return sc


def reference_lost_fragment():
    """... and the one with a fragment lost: a 1-packet queue at the sender loses fragments of a 5000-byte echo, the
    server receives nothing, and with icmp the timeout's time-exceeded error reaches the client's node."""
    sc = line(2, [(5_000_000, 2 * MS)], icmp=True, qmax=1, timeout_ns=20 * MS)
    sc.add_echo_server(1, 0, 0)
    sc.add_echo_client(0, 1, 1 * MS, 0, count=1, interval_ns=1 * S, size=5000)
    sc.stop(100 * MS)
    sc.route_bfs()
    return sc


LOSS_CASES = (("loss_at_forwarder", (False,)), ("loss_at_forwarder", (True,)))
GPU_CASES = (("echo_2000", ()), ("forwarding_4000", ()), ("largest", ()), ("sender_overflow", ()),
             ("ttl_expiry", ()), ("port_unreachable", ()), ("udp_client_1500", ()), ("grid_pipelines", ()),
             ("hub_forwards", ()), ("hub_echo_server", ()), ("hub_timeout", ())) + LOSS_CASES
