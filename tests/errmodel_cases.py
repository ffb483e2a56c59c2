"""Scenarios of the receive error model tests, shared by tests/test_errmodel_cpu.py (the conditions each must meet,
asserted on the model alone) and tests/test_gpu_errmodel.py (the engine against the model,
tests/p2p_errmodel_pyref.py)."""
import p2p

MS, US, S = 1_000_000, 1_000, 1_000_000_000


def line(n, links, icmp=False, ports=False, frag=False, qmax=100, timeout_ns=0, rng_seed=0, rng_run=0):
    """n nodes in a line; links[i] = (bps, delay_ns) of link i -> i + 1.  Link i's devices are 2 i (on node i) and
    2 i + 1 (on node i + 1)."""
    sc = p2p.Scenario(n, icmp=icmp, ports=ports, frag=frag, frag_timeout_ns=timeout_ns, rng_seed=rng_seed,
                      rng_run=rng_run)
    ld = [sc.link(i, i + 1, l[0], l[1], qmax) for i, l in enumerate(links)]
    sc.install_stack()
    for k, (da, db) in enumerate(ld):
        sc.assign_link(da, db, p2p.ip("10.1.1.0") + (k << 8))
    return sc


def udp_list(model="list"):
    """Two nodes, one link: a UdpClient sends 20 datagrams to a UdpServer (PacketWindowSize 8, so that the loss counter
    passes the early losses).  model: "list" = ReceiveList [0, 3, 3, 19, 25] on the server's device (duplicates, and an
    ordinal that never arrives); "none"; "rate0" / "rate1" = Rate EU_PKT 0.0 / 1.0; "disabled" = the list, disabled."""
    sc = line(2, [(5_000_000, 2 * MS)], ports=True)
    sc.add_udp_server(1, 0, 0, port=100, window=8)
    sc.add_udp_client(0, 1, 1 * MS, 0, count=20, interval_ns=1 * MS, size=100, remote_port=100)
    sc.stop(60 * MS)
    sc.route_bfs()
    if model in ("list", "disabled"):
        sc.set_receive_list_error_model(1, [0, 3, 3, 19, 25], enabled=model == "list")
    elif model in ("rate0", "rate1"):
        sc.set_rate_error_model(1, 0.0 if model == "rate0" else 1.0, unit="pkt", stream=0)
    return sc


def chain_echo():
    """A three-node chain with icmp: a UdpEchoClient on node 0 sends 16 echoes to a UdpEchoServer on node 2 that stops
    at 20 ms (later requests are port-unreachable: ICMP errors travel back).  ReceiveList on the forwarder's incoming
    device (1), Rate EU_PKT 0.3 on the destination's (3), and a ReceiveList on the client's device (0) that drops
    replies and an ICMP error on the way back."""
    sc = line(3, [(10_000_000, 500 * US), (10_000_000, 500 * US)], icmp=True, rng_seed=1, rng_run=1)
    sc.add_echo_server(2, 0, 20 * MS)
    sc.add_echo_client(0, 2, 1 * MS, 0, count=16, interval_ns=2 * MS, size=200)
    sc.stop(60 * MS)
    sc.route_bfs()
    sc.set_receive_list_error_model(1, [2, 7, 11])
    sc.set_rate_error_model(3, 0.3, unit="pkt", stream=0)
    sc.set_receive_list_error_model(0, [1, 4, 8])
    return sc


def frag_loss(icmp):
    """Frag plus loss: node 0 sends 4000-byte datagrams (three fragments: arrival ordinals 3 k, 3 k + 1, 3 k + 2 at
    the destination's device) in bursts; a ReceiveList at the destination drops the middle fragment of some.  The
    node's one buffer then mixes datagrams, a buffer left incomplete at a burst's end times out (8 ms; with icmp a
    time-exceeded error), and the timers of the completed ones are dispatched cancelled."""
    sc = line(2, [(20_000_000, 200 * US)], icmp=icmp, frag=True, timeout_ns=8 * MS)
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=10_000_000, size=4000, on_s=0.02, off_s=0.03)
    sc.stop(110 * MS)
    sc.route_bfs()
    sc.set_receive_list_error_model(1, [4, 13, 16, 3 * 7 - 2, 40, 58])
    return sc


def rate_both_ends(streams, rng_run):
    """Rate models on both ends of one link, 200 small datagrams each way between UdpClients and UdpServers: EU_PKT 0.25
    on node 0's device, EU_BYTE 2e-3 on node 1's (130-byte frames: about 0.23)."""
    sc = line(2, [(10_000_000, 300 * US)], ports=True, rng_seed=1, rng_run=rng_run)
    sc.add_udp_server(0, 0, 0, port=100, window=32)
    sc.add_udp_server(1, 0, 0, port=100, window=32)
    sc.add_udp_client(0, 1, 1 * MS, 0, count=200, interval_ns=150 * US, size=100, remote_port=100)
    sc.add_udp_client(1, 0, 1 * MS + 40 * US, 0, count=200, interval_ns=150 * US, size=100, remote_port=100)
    sc.stop(50 * MS)
    sc.route_bfs()
    sc.set_rate_error_model(0, 0.25, unit="pkt", stream=streams[0])
    sc.set_rate_error_model(1, 2e-3, unit="byte", stream=streams[1])
    return sc


def mixed_sizes():
    """EU_BYTE and EU_BIT with mixed frame sizes on one link: each way a 1700-byte OnOff flow (frames of 1502 and 250
    bytes) beside a 30-byte one (60-byte frames).  EU_BYTE 5e-4 on node 1's device (thresholds about 0.53, 0.12, 0.03),
    EU_BIT 6e-5 on node 0's (about 0.51, 0.11, 0.03)."""
    sc = line(2, [(20_000_000, 200 * US)], frag=True, timeout_ns=3 * MS, rng_seed=12345, rng_run=7)
    sc.add_sink(0, 0, 0)
    sc.add_sink(1, 0, 0)
    for a, b in ((0, 1), (1, 0)):
        sc.add_onoff(a, b, 1 * MS, 0, rate_bps=8_000_000, size=1700, on_s=1.0, off_s=0.0, max_bytes=1700 * 40)
        sc.add_onoff(a, b, 1 * MS + 100 * US, 0, rate_bps=200_000, size=30, on_s=1.0, off_s=0.0, max_bytes=30 * 60)
    sc.stop(120 * MS)
    sc.route_bfs()
    sc.set_rate_error_model(1, 5e-4, unit="byte", stream=2)
    sc.set_rate_error_model(0, 6e-5, unit="bit", stream=5)
    return sc


def hub_dumbbell(n_leaves):
    """p2p.dumbbell with a Rate model (EU_PKT 0.4) on router 2's bottleneck incoming device and a ReceiveList on two of
    router 1's leaf-side devices: router 1 takes n_leaves same-time Receives (a hub block), of which those on the
    modelled devices must run in the serial pass."""
    sc = p2p.dumbbell(n_leaves, max_bytes=1024, compressed=False)  # (two datagrams a leaf)
    sc.rng_seed, sc.rng_run = 1, 3
    sc.set_rate_error_model(1, 0.4, unit="pkt", stream=1)       # device 1: router 2's end of the router link
    sc.set_receive_list_error_model(2 + 2 * 5 + 1, [0])          # router 1's device towards left leaf 5
    sc.set_receive_list_error_model(2 + 2 * 11 + 1, [1, 2])      # ... and leaf 11 (ordinal 2 never arrives)
    return sc


def grid_wide(rows=8, cols=8):
    """p2p.grid's 8x8 topology with a 4352-byte fragmenting flow down every column (frames large enough for create to
    grant wide windows) and Rate EU_BYTE models on every device of rows 3 and 6 that a flow arrives on."""
    sc = p2p.grid(rows, cols, start_ns=1 * MS, stop_ns=40 * MS, sim_stop_ns=90 * MS, rate_bps=8_000_000, size=4352,
                  on_s=1.0, off_s=0.0)
    sc.frag = True
    sc.frag_timeout_ns = 6 * MS
    sc.rng_seed, sc.rng_run = 1, 1
    k = 0
    for d, (node, peer, *_r) in enumerate(sc.dev):
        y, x = divmod(node, cols)
        py = sc.dev[peer][0] // cols
        if y in (3, 6) and py == y - 1:  # the device towards the node above: where the column's flow arrives
            sc.set_rate_error_model(d, 2.5e-4, unit="byte", stream=k)
            k += 1
    return sc


def without_models(sc):
    """The same scenario object with its error models taken off (for the digest comparison)."""
    sc.error_models = {}
    return sc


GPU_CASES = (("udp_list", ("list",)), ("chain_echo", ()), ("frag_loss", (False,)), ("frag_loss", (True,)),
             ("rate_both_ends", ((0, 1), 1)), ("rate_both_ends", ((1, 0), 1)), ("rate_both_ends", ((0, 1), 3)),
             ("rate_both_ends", ((1, 0), 3)), ("mixed_sizes", ()), ("hub_dumbbell", (40,)), ("hub_dumbbell", (2000,)),
             ("grid_wide", ()))
