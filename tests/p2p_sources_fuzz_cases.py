"""The second seeded set: tests/p2p_fuzz_cases.py's scenarios with the two newer kinds of source added, shared by
tests/test_p2p_sources_fuzz_cpu.py (the conditions, asserted on the composed Python model alone:
tests/p2p_full_pyref.py) and tests/test_gpu_p2p_sources_fuzz.py (the engine against that model through every
pipeline).  A scenario is FZ.<family> (seed), untouched and with its draws in their order, and what a second generator,
np.random.default_rng (K + seed), adds to it:

  mesh (seed)        one or two UdpTraceClients towards the UdpServer's node (one of them sometimes to a port nothing
                     is bound to), with drawn start and stop times (some stop in mid-cycle), a drawn MaxPacketSize and a
                     drawn trace of 4 to 8 entries: timeToSend 0 to 5 ms, sizes that give header-only datagrams, exact
                     multiples of MaxPacketSize and frames cut into several datagrams; some traces begin with timeToSend
                     0, so that a cycle's last burst joins the next cycle's first.  Every OnOff flow of the mesh gets
                     drawn OnTime / OffTime variables (Constant, Uniform, Exponential, some bounded; means 1 to 6 ms),
                     each with an RngStream of its own from FIRST_VAR_STREAM up (the error models' count from 0), and
                     one in three a Stop time.  The OnOff sizes stay as FZ drew them: a random source may fragment.
  star / star_large / star_wide (seed)
                     three leaves additionally host a trace client towards the far node's UdpServer, so their bursts
                     cross the hub and the bottleneck; half of the non-fragmenting OnOff leaves get random times.
                     star_wide (15 leaves: FZ's nearest star with wide windows) draws its traces from frames whose every
                     datagram carries 1000 bytes or more, since one small frame makes a plan narrow.

monitored (family, seed) is the same scenario with frag off and the monitor on, every payload above MAX_PAYLOAD
replaced by the smallest choice of its draw (the star's one fragmenting leaf: by the star's small size), or None where
create still refuses it.

What create refuses, the generator avoids: a trace whose every timeToSend is 0, more than 256 datagrams a Send (at most
8 entries of at most 2048 bytes at a MaxPacketSize of 200 or more: 88), a MaxPacketSize above 1472, a variable on an
RngStream a Rate model or another variable has.
"""
import numpy as np

import nsgpu
import p2p
import p2p_fuzz_cases as FZ
from p2p_fuzz_cases import CH, LQ, MAX_PAYLOAD, MS, US  # noqa: F401  (for the tests that import this module alone)

K = 90_000  # the second generator's seed offset
FIRST_VAR_STREAM = 20
UNBOUND_PORT = 78  # (nothing is bound to it; FZ's unbound ports are 77 and 55)
MAX_PACKET_SIZES = (200, 1024, 1472)
FRAME_SIZES = (12, 134, 200, 400, 1024, 1542, 2048)


def _trace(rng, sizes, times):
    """4 to 8 entries; the first has timeToSend 0 in about half of the traces; never all 0."""
    n = int(rng.integers(4, 9))
    ent = [(int(rng.choice(times)), int(rng.choice(sizes))) for _ in range(n)]
    if int(rng.integers(0, 2)):
        ent[0] = (0, ent[0][1])
    if all(t == 0 for t, _z in ent):
        ent[-1] = (int(rng.integers(1, 6)), ent[-1][1])
    return ent


def _variable(rng, stream, mean_ms):
    """(a Constant, Uniform or Exponential of mean mean_ms, the next free stream)."""
    mean = mean_ms * 1e-3
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return p2p.Constant(mean), stream
    if kind in (1, 2):
        half = mean * float(rng.choice([0.25, 0.5, 1.0]))
        return p2p.Uniform(mean - half, mean + half, stream), stream + 1
    bound = 0.0 if kind == 3 else mean * float(rng.choice([0.125, 0.5, 2.0]))
    return p2p.Exponential(mean, stream, bound=bound), stream + 1


def set_variables(app, on, off):
    """What add_onoff (on_var=, off_var=) does, on an application that exists."""
    for key, const, v in (("on_var", "on", on), ("off_var", "off", off)):
        if v.kind == p2p.RV_CONSTANT:
            app[const], app[key] = v.p0, None
        else:
            app[key] = v


def mesh_src(seed, trace_clients=True):
    sc = FZ.mesh(seed)
    rng = np.random.default_rng(K + seed)
    srv = next(A["node"] for A in sc.apps if A["kind"] == p2p.APP_UDP_SERVER)
    stream = FIRST_VAR_STREAM
    for A in sc.apps:
        if A["kind"] == p2p.APP_ONOFF:
            on, stream = _variable(rng, stream, int(rng.integers(1, 7)))
            off, stream = _variable(rng, stream, int(rng.integers(1, 7)))
            set_variables(A, on, off)
            if int(rng.integers(0, 3)) == 0:  # (FZ's sources never stop; some of these do, perhaps while on)
                A["stop"] = int(rng.integers(20, 46)) * MS + 300 * US
    n_clients = int(rng.integers(1, 3))
    unbound = int(rng.integers(0, 3)) == 0  # the last client's port
    for i in range(n_clients):
        src = int(rng.choice([x for x in range(sc.n_nodes) if x != srv]))
        start = int(rng.integers(1, 6)) * MS + int(rng.integers(0, 10)) * 100 * US
        stop = 0 if int(rng.integers(0, 2)) else start + int(rng.integers(12, 40)) * MS + 500 * US
        mps = int(rng.choice(MAX_PACKET_SIZES))
        ent = _trace(rng, FRAME_SIZES, range(0, 6))
        port = UNBOUND_PORT if unbound and i == n_clients - 1 else 100
        if port != 100:  # (create refuses a header-only datagram to anything but a UdpServer)
            ent = [(t, z if z % mps > 12 else z + 100) for t, z in ent]
        if trace_clients:
            sc.add_udp_trace_client(src, srv, start, stop, entries=ent, max_packet_size=mps, remote_port=port)
    sc.route_bfs()
    return sc


def star_src(seed, large=False, n_leaves=FZ.STAR_LEAVES, trace_clients=True, wide_frames=False):
    sc = FZ.star(seed, large, n_leaves)
    rng = np.random.default_rng(K + seed)
    L = n_leaves
    far = L + 1
    small = 1000 if large else 200
    stream = FIRST_VAR_STREAM
    plain = [a for a, A in enumerate(sc.apps) if A["kind"] == p2p.APP_ONOFF and A["size"] <= MAX_PAYLOAD]
    for a in rng.permutation(plain)[:(len(plain) + 1) // 2].tolist():
        # (a constant OffTime of 0 keeps the first burst in step with the other leaves: its datagrams reach the hub
        # among theirs; on times of a few datagrams, so that twelve datagrams take several draws)
        on, stream = _variable(rng, stream, float(rng.choice([1.5, 2.0, 3.0])))
        if on.kind == p2p.RV_CONSTANT:
            on, stream = p2p.Uniform(0.001, 0.003, stream), stream + 1
        off = p2p.Constant(0.0)
        if int(rng.integers(0, 2)):
            off, stream = _variable(rng, stream, int(rng.integers(1, 4)))
        set_variables(sc.apps[a], on, off)
    # the frame of `small` bytes in one datagram reaches the hub together with the leaves' own (equal frames on
    # identical links), the others do not
    sizes = (small, small, small, 12, 400, 1024, 1542, 2048)
    for leaf in rng.permutation(L)[:3].tolist():
        mps = int(rng.choice(MAX_PACKET_SIZES[1:] if wide_frames else MAX_PACKET_SIZES))
        if wide_frames:  # no datagram below 1000 bytes: full ones and a remainder of 1000
            sizes = (small, small, mps + small, 2 * mps + small)
        ent = _trace(rng, sizes, (0, 1, 1, 2, 3))
        stop = 0 if int(rng.integers(0, 2)) else 2 * MS + int(rng.integers(10, 30)) * MS + 500 * US
        if trace_clients:
            sc.add_udp_trace_client(leaf, far, 2 * MS, stop, entries=ent, max_packet_size=mps, remote_port=100)
    sc.route_bfs()
    return sc


def star_wide_src(seed, trace_clients=True):
    return star_src(seed, True, LQ - 1, trace_clients, wide_frames=True)


FAMILIES = {"mesh": mesh_src, "star": lambda seed, **kw: star_src(seed, False, **kw),
            "star_large": lambda seed, **kw: star_src(seed, True, **kw), "star_wide": star_wide_src}
# the smallest choice of each kind's size draw in FZ.mesh; a star's fragmenting leaf gets the star's small size
_SMALLEST = {p2p.APP_UDP_CLIENT: 100, p2p.APP_ECHO_CLIENT: 200, p2p.APP_ONOFF: 64}
_STAR_SMALL = {"star": 200, "star_large": 1000, "star_wide": 1000}


def build(family, seed, trace_clients=True):
    return FAMILIES[family](seed, trace_clients=trace_clients)


def monitored(family, seed):
    sc = build(family, seed)
    for A in sc.apps:
        if A["kind"] in _SMALLEST and A["size"] > MAX_PAYLOAD:
            A["size"] = _SMALLEST[A["kind"]] if family == "mesh" else _STAR_SMALL[family]
    sc.frag, sc.flowmon = False, True
    try:
        p2p.dist_plan(sc, None, 0, 1)
    except nsgpu.NsgpuError:
        return None
    return sc


# ---------------- variants for the sensitivity checks ----------------
def random_sources(sc):
    return [a for a, A in enumerate(sc.apps) if A["kind"] == p2p.APP_ONOFF and
            (A.get("on_var") is not None or A.get("off_var") is not None)]


def trace_client_apps(sc):
    return [a for a, A in enumerate(sc.apps) if A["kind"] == p2p.APP_UDP_TRACE_CLIENT]


def with_swapped_streams(sc):
    """The first source whose two variables both draw gets them on each other's stream; None without such a source."""
    for a in random_sources(sc):
        on, off = sc.apps[a]["on_var"], sc.apps[a]["off_var"]
        if on is not None and off is not None:
            on.stream, off.stream = off.stream, on.stream
            return sc
    return None


def variable_mean(v):
    return (v.p0 + v.p1) / 2 if v.kind == p2p.RV_UNIFORM else v.p0


def with_constant_means(sc):
    for a in random_sources(sc):
        A = sc.apps[a]
        set_variables(A, p2p.Constant(variable_mean(A["on_var"]) if A["on_var"] is not None else A["on"]),
                      p2p.Constant(variable_mean(A["off_var"]) if A["off_var"] is not None else A["off"]))
    return sc


def signature(sc):
    """Everything a scenario is made of, comparable with == (a variable by its record)."""
    apps = [{k: (v.record() if isinstance(v, p2p.RanVar) else v) for k, v in A.items()} for A in sc.apps]
    return (sc.dev, apps, sc.error_models, sc.setup, sc.icmp, sc.frag, sc.flowmon, sc.frag_timeout_ns, sc.rng_seed,
            sc.rng_run, sc.stop_ns)


# ---------------- what a scenario holds (for a failure's message) ----------------
_KINDS = {p2p.APP_SINK: "PacketSink", p2p.APP_ONOFF: "OnOff", p2p.APP_ECHO_SERVER: "UdpEchoServer",
          p2p.APP_ECHO_CLIENT: "UdpEchoClient", p2p.APP_UDP_CLIENT: "UdpClient", p2p.APP_UDP_SERVER: "UdpServer",
          p2p.APP_UDP_TRACE_CLIENT: "UdpTraceClient"}


def _describe_variable(v):
    if v.kind == p2p.RV_UNIFORM:
        return "Uniform (%g, %g) stream %d" % (v.p0, v.p1, v.stream)
    return "Exponential (%g%s) stream %d" % (v.p0, ", bound %g" % v.p1 if v.p1 else "", v.stream)


def describe_node(sc, node):
    """FZ.describe_node's text, which also names a trace client's entries and MaxPacketSize and a source's variables."""
    apps = []
    for a, A in enumerate(sc.apps):
        if A["node"] != node:
            continue
        s = "%d:%s" % (a, _KINDS[A["kind"]])
        if A["kind"] == p2p.APP_UDP_TRACE_CLIENT:
            s += " (%d entries %s, MaxPacketSize %d, port %d)" % (len(A["entries"]), A["entries"], A["size"],
                                                                   A["remote_port"])
        elif A["kind"] == p2p.APP_ONOFF:
            s += " (%d bytes" % A["size"]
            for name, v in (("on", A.get("on_var")), ("off", A.get("off_var"))):
                if v is not None:
                    s += ", %s %s" % (name, _describe_variable(v))
            s += ")"
        apps.append(s)
    models = []
    for d, D in enumerate(sc.dev):
        if D[0] == node and d in sc.error_models:
            e = sc.error_models[d]
            models.append("dev %d: %s" % (d, "ReceiveList %s" % e["packets"] if e["kind"] == "list" else
                                          "Rate %s %g stream %d" % (e["unit"], e["rate"], e["stream"])))
    return "node %d apps [%s] models [%s]" % (node, ", ".join(apps), "; ".join(models) or "none")


# (family, seed): chosen on the model so that the conditions of tests/test_p2p_sources_fuzz_cpu.py hold
SRC_FUZZ_CASES = (
    ("mesh", 1), ("mesh", 4), ("mesh", 5), ("mesh", 6), ("mesh", 9), ("mesh", 13), ("mesh", 26), ("mesh", 27),
    ("mesh", 10), ("mesh", 11),  # (the narrow plans)
    ("star", 0), ("star", 1), ("star", 3), ("star_large", 1), ("star_large", 3),
    ("star_wide", 9), ("star_wide", 11),  # (15 leaves, no icmp, large frames: wide plans)
)
# the cases whose single-engine plan is wide (tests/test_p2p_sources_fuzz_cpu.py asserts that these are the ones): they
# also run through the narrow kernels
WIDE_CASES = (("mesh", 1), ("mesh", 4), ("mesh", 5), ("mesh", 6), ("mesh", 9), ("mesh", 13), ("mesh", 26), ("mesh", 27),
              ("star_wide", 9), ("star_wide", 11))
