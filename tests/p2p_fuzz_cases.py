"""Seeded scenarios with every p2p device feature on at once, shared by tests/test_p2p_fuzz_cpu.py (the conditions
the cases must meet, asserted on the Python model alone) and tests/test_gpu_p2p_fuzz.py (the engine against the model,
tests/p2p_errmodel_pyref.py, through four pipelines).  A scenario is a function of (family, seed) alone.

  mesh (seed)  10 nodes on a random spanning tree plus extra links (13 links), drawn rates, delays and queue lengths;
               ports, frag, icmp drawn.  A UdpServer and a PacketSink on one node (the endpoint is found by flow), a
               UdpEchoServer that may stop mid-run, a PacketSink that may start late; UdpClients (some to an unbound
               port), UdpEchoClients (some with TTL 2) and OnOff flows, of sizes on both sides of the MTU; six devices
               with a ReceiveList or a Rate model.
  star (seed, large)
               24 leaves on a hub with identical links, all starting at one instant, so that the hub takes 24
               same-time Receives (more than CH = 16: a hub block); a bottleneck from the hub to a far node; an echo
               server on the hub; one leaf's flow fragments; ReceiveList / Rate models on five of the hub's leaf-side
               devices and a byte-unit Rate model on the far node's.  large: every leaf flow carries 1000-byte payloads
               or more.

A 24-leaf star is never granted wide windows, whatever its frames: create asks for a largest node degree of at most
LQ = 16 (nsgpu_p2p_win.h: a node's pending local records are its busy devices'), and a node takes more than CH = 16
same-time Receives only through more than 16 devices.  So a hub block of same-time Receives runs in the scanning
pipelines only.  star_wide is the nearest star that is wide: 15 leaves (a hub of LQ devices), large frames, a seed
that draws no icmp.  Its hub still has more than CH events at one timestamp (15 Receives and the echo server's
zero-delay deliveries), but with an echo endpoint a Receive's lookahead is 0, so a window ends at the Receives' time
and the model cannot say whether one window holds more than CH of them; the family is there for the deferred pipeline
on a crowded node, not as a proven hub block.  tests/test_p2p_fuzz_cpu.py asserts which family is wide.

What nsgpu_p2p_create refuses and the model does not, the generators avoid: two fragmenting flows into one node (an
echo client's own node counts, for its replies), a UdpClient PacketSize outside [12, 1500], a payload below 12 bytes to
a UdpServer, bound ports from 49152 up, two applications of a node on one port, a PacketWindowSize that is no multiple
of 8 in [8, 256], two enabled Rate models on one RngStream, more than 16 distinct (unit, rate) pairs.
"""
import numpy as np

import p2p

MS, US = 1_000_000, 1_000
CH = 16  # events of one node above which a hub block runs them (nsgpu_p2p_dev.h)
LQ = 16  # the largest node degree of a wide engine (nsgpu_p2p_win.h)
MAX_PAYLOAD = 1472  # above it a datagram is fragmented (MTU 1500)
STAR_LEAVES = 24
RATE_OF_UNIT = {"pkt": 0.2, "byte": 3e-4, "bit": 4e-5}  # (two threshold tables: well below the 16 create allows)


def mesh(seed, n_nodes=10, n_links=13):
    rng = np.random.default_rng(seed)
    icmp = bool(rng.integers(0, 2))
    sc = p2p.Scenario(n_nodes, icmp=icmp, ports=True, frag=True, frag_timeout_ns=int(rng.choice([3, 8, 20])) * MS,
                      rng_seed=int(rng.choice([1, 12345])), rng_run=int(rng.integers(1, 8)))
    edges = set()
    for n in range(1, n_nodes):  # a random spanning tree, then extra links
        edges.add((int(rng.integers(0, n)), n))
    while len(edges) < n_links:
        a, b = sorted(rng.choice(n_nodes, 2, replace=False).tolist())
        edges.add((a, b))
    links = [sc.link(a, b, int(rng.choice([5_000_000, 10_000_000, 20_000_000])),
                     int(rng.choice([100 * US, 500 * US, 1 * MS])), int(rng.choice([4, 20, 100])))
             for a, b in sorted(edges)]
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.1.0.0") + (k << 8))
    takes_fragments = set()  # nodes that already receive one fragmenting flow's fragments

    def size_for(choices, src, dst, echo=False):
        """A drawn payload size; a fragmenting one only where create accepts it (the smallest choice otherwise)."""
        z = int(rng.choice(choices))
        if z > MAX_PAYLOAD:
            nodes = [dst] + ([src] if echo else [])
            if any(n in takes_fragments for n in nodes):
                return int(min(choices))
            takes_fragments.update(nodes)
        return z

    def other_than(node):
        return int(rng.choice([x for x in range(n_nodes) if x != node]))

    srv_udp, srv_echo, srv_sink = rng.permutation(n_nodes).tolist()[:3]
    sc.add_udp_server(srv_udp, 0, 0, port=100, window=int(rng.choice([8, 32])))
    sc.add_echo_server(srv_echo, 0, int(rng.choice([0, 30 * MS])), port=9)
    sc.add_sink(srv_sink, int(rng.choice([0, 5 * MS])), 0, port=9)
    sc.add_sink(srv_udp, 0, 0, port=9)  # the second endpoint of the UdpServer's node
    for _ in range(3):
        s = other_than(srv_udp)
        sc.add_udp_client(s, srv_udp, int(rng.integers(1, 5)) * MS, 0, count=int(rng.integers(10, 40)),
                          interval_ns=int(rng.choice([200 * US, 1 * MS])),
                          size=size_for([100, 1472, 1500], s, srv_udp),
                          remote_port=int(rng.choice([100, 100, 100, 77])))  # (nothing is bound to port 77)
    for _ in range(2):
        s = other_than(srv_echo)
        sc.add_echo_client(s, srv_echo, int(rng.integers(1, 5)) * MS, 0, count=int(rng.integers(5, 20)),
                           interval_ns=2 * MS, size=size_for([200, 2000, 5000], s, srv_echo, True),
                           ttl=int(rng.choice([64, 64, 2])))
    for dst in (srv_sink, srv_udp):
        s = other_than(dst)
        sc.add_onoff(s, dst, int(rng.integers(1, 5)) * MS, 0, rate_bps=int(rng.choice([2_000_000, 8_000_000])),
                     size=size_for([64, 1700, 4352], s, dst), on_s=float(rng.choice([0.005, 0.02])),
                     off_s=float(rng.choice([0.0, 0.01])), max_bytes=int(rng.choice([0, 40000])), remote_port=9)
    sc.stop(60 * MS)
    sc.route_bfs()
    stream = 0
    for d in rng.permutation(len(sc.dev)).tolist()[:6]:
        if int(rng.integers(0, 3)) == 0:
            sc.set_receive_list_error_model(d, sorted(rng.integers(0, 30, size=4).tolist()))
        else:
            unit = ["pkt", "byte", "bit"][int(rng.integers(0, 3))]
            sc.set_rate_error_model(d, RATE_OF_UNIT[unit], unit=unit, stream=stream)  # (a stream of its own each)
            stream += 1
    return sc


def star(seed, large=False, n_leaves=STAR_LEAVES):
    """Leaf i is node i, the hub node n_leaves, the far node n_leaves + 1; link i's devices are 2 i (on the leaf) and
    2 i + 1 (on the hub), the bottleneck's 2 n_leaves (hub) and 2 n_leaves + 1 (far)."""
    rng = np.random.default_rng(seed)
    L = n_leaves
    hub, far = L, L + 1
    small = 1000 if large else 200
    sc = p2p.Scenario(L + 2, icmp=bool(rng.integers(0, 2)), ports=True, frag=True, frag_timeout_ns=5 * MS,
                      rng_seed=1, rng_run=int(rng.integers(1, 6)))
    links = [sc.link(i, hub, 10_000_000, 500 * US, 20) for i in range(L)]
    links.append(sc.link(hub, far, int(rng.choice([20_000_000, 100_000_000])), 200 * US, int(rng.choice([8, 100]))))
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.1.0.0") + (k << 8))
    sc.add_udp_server(far, 0, 0, port=100, window=32)
    sc.add_echo_server(hub, 0, 0, port=9)
    sc.add_sink(far, 0, 0, port=9)
    big = int(rng.integers(0, L))  # the leaf whose flow fragments (the far node's one fragmenting flow)
    for i in range(L):  # every leaf starts at 2 ms: equal frames on identical links reach the hub together
        c = int(rng.integers(0, 3))
        if i == big:
            sc.add_onoff(i, far, 2 * MS, 0, rate_bps=4_000_000, size=4000, on_s=0.01, off_s=0.005, remote_port=9)
        elif c == 0:
            sc.add_udp_client(i, far, 2 * MS, 0, count=12, interval_ns=1 * MS, size=small,
                              remote_port=int(rng.choice([100, 100, 55])))  # (nothing is bound to port 55)
        elif c == 1:
            sc.add_echo_client(i, hub, 2 * MS, 0, count=10, interval_ns=1 * MS, size=small)
        else:
            sc.add_onoff(i, far, 2 * MS, 0, rate_bps=8 * small * 1000, size=small, on_s=1.0, off_s=0.0,
                         max_bytes=12 * small, remote_port=9)  # (a datagram a millisecond, twelve of them)
    sc.stop(40 * MS)
    sc.route_bfs()
    stream = 0
    for k, i in enumerate(rng.permutation(L)[:5].tolist()):
        d = 2 * i + 1  # the hub's device towards leaf i
        if k % 2:
            sc.set_receive_list_error_model(d, [0, 2, 5])
        else:
            sc.set_rate_error_model(d, 0.3, unit="pkt", stream=stream)
            stream += 1
    sc.set_rate_error_model(2 * L + 1, 4e-4, unit="byte", stream=stream)
    return sc


FAMILIES = {"mesh": mesh, "star": lambda seed: star(seed, False), "star_large": lambda seed: star(seed, True),
            "star_wide": lambda seed: star(seed, True, n_leaves=LQ - 1)}


def build(family, seed):
    return FAMILIES[family](seed)


def star_hub(sc):
    return sc.n_nodes - 2


# ---------------- what a scenario holds (for the conditions and for a failure's message) ----------------
def fragmenting_flows(sc):
    return [a for a, A in enumerate(sc.apps) if A["kind"] in p2p.SENDERS and A["size"] > MAX_PAYLOAD]


def path_devices(sc, src, dst):
    """The devices a datagram from node src to node dst leaves by, in order."""
    out, n = [], src
    while n != dst:
        d = sc.next_hop(n, sc.dst_slot[dst])
        if d == p2p.NO_ROUTE or len(out) > sc.n_nodes:
            return None
        out.append(d)
        n = sc.dev[sc.dev[d][1]][0]
    return out


def owner_interleaved(sc, nranks=3):
    return (np.arange(sc.n_nodes) % nranks).astype(np.uint32)


def describe_node(sc, node):
    """A node's application kinds and its devices' models, for an assertion's message."""
    kinds = {p2p.APP_SINK: "PacketSink", p2p.APP_ONOFF: "OnOff", p2p.APP_ECHO_SERVER: "UdpEchoServer",
             p2p.APP_ECHO_CLIENT: "UdpEchoClient", p2p.APP_UDP_CLIENT: "UdpClient", p2p.APP_UDP_SERVER: "UdpServer"}
    apps = ["%d:%s" % (a, kinds[A["kind"]]) for a, A in enumerate(sc.apps) if A["node"] == node]
    models = []
    for d, D in enumerate(sc.dev):
        if D[0] == node and d in sc.error_models:
            e = sc.error_models[d]
            models.append("dev %d: %s" % (d, "ReceiveList %s" % e["packets"] if e["kind"] == "list" else
                                          "Rate %s %g stream %d" % (e["unit"], e["rate"], e["stream"])))
    return "node %d apps [%s] models [%s]" % (node, ", ".join(apps), "; ".join(models) or "none")


# (family, seed): chosen on the model so that the conditions of tests/test_p2p_fuzz_cpu.py hold
FUZZ_CASES = (
    ("mesh", 0), ("mesh", 5), ("mesh", 6), ("mesh", 7), ("mesh", 9), ("mesh", 12), ("mesh", 14), ("mesh", 26),
    ("mesh", 27),
    ("mesh", 10), ("mesh", 11), ("mesh", 15),  # (the narrow plans)
    ("star", 0), ("star", 1), ("star", 3), ("star", 6), ("star_large", 0), ("star_large", 6),
    ("star_wide", 1), ("star_wide", 6),  # (15 leaves, no icmp: wide plans)
)
