"""The third seeded set, the "band" families: every p2p device feature in windows several holder blocks wide.  Shared
by tests/test_p2p_wide_fuzz_cpu.py (the conditions, asserted on the Python models alone) and
tests/test_gpu_p2p_wide_fuzz.py (the engine against the model through every pipeline).  A scenario is a function of
(family, seed) alone.

A band is R = 3 rows x C columns of independent column chains: node (r, c) is r C + c (C is 1 modulo 3, so that both
two block ranks and owner = node % 3 cut every column), column c's devices are 4 c (row 0), 4 c + 1 and 4 c + 2 (row 1,
up and down) and 4 c + 3 (row 2).  Every link has 10 Mb/s and 1 ms; every flow goes down its column and starts at
START.  A column whose sender puts one 1000-byte datagram a millisecond on the wire is "in lockstep": its Send,
TransmitCompletes and Receives fall on the same timestamps as every other such column's, so that one timestamp holds
two events of every lockstep column (a row's TransmitComplete and the next row's Receive) and a window several holder
blocks of HB events.

What a column carries is drawn with np.random.default_rng (seed), column by column, nine draws a column in this order
(every draw is made whether or not it is used):

  1  kind        an index into the family's kinds by its weights (KINDS_WIDE / KINDS_NARROW):
                   udp      UdpClient -> UdpServer, 1000 bytes every ms                                   (lockstep)
                   onoff    OnOff -> PacketSink, 1000 bytes at 8 Mb/s, always on                          (lockstep)
                   unbound  UdpClient, 1000 bytes every ms, to port UNBOUND_PORT, which nothing binds     (lockstep)
                   fast     UdpClient -> UdpServer, 1000 bytes every 500 us into a short queue: the queue
                            overflows and the server counts losses
                   frag     OnOff -> PacketSink whose datagrams fragment (FRAG_SIZES_WIDE / _NARROW at 8 Mb/s)
                   fragudp  (narrow) UdpClient -> UdpServer of 1500 bytes every 2 ms: two fragments each
                   echo     (narrow) UdpEchoClient -> UdpEchoServer, 1000 bytes every ms
                   small    (narrow) OnOff -> PacketSink, 64 bytes at 512 kb/s
  2  size        an index into the kind's size choices (frag only; drawn for all)
  3  queue       an index into QUEUES: the queue length of the column's row-0 device (fast: of SHORT_QUEUES; frag,
                 fragudp: of FRAG_QUEUES, where 1 drops a datagram's last fragment at its own sender)
  4  modelled    integers (0, 5): 0 puts a receive error model on the column (frag, fragudp: 0 or 1)
  5  which       integers (0, 12): below 9 a ReceiveList model, 9 / 10 / 11 a Rate model per packet / byte / bit
                 (RATE_OF_UNIT) on the next free RngStream (one model in four, so that the MAX_RATE_MODELS streams
                 last over the band's whole width); once they are taken, a ReceiveList model
  6  where       integers (0, 3): 0 / 2 the row-1 device that receives from row 0, 1 the row-2 device; 2 on a narrow
                 family's echo or unbound column: the row-1 device that receives from row 2 (replies and ICMP errors
                 on their way back); a collected column: 0 the row-1 device, else the collector's device for it
  7-9 list       three integers (0, 12): the ReceiveList model's ordinals

Families:

  band_wide        no ICMP, no echo, every frame 1000 bytes or more (a fragmenting datagram's last fragment too):
                   tx_min = 824 us, Lx = 1.824 ms, so create grants wide windows (Lx > tx_min, Lx <= LKD tx_min): the
                   deferred pipeline with local records in many holder regions at once.  The columns COLLECT_AT ..
                   COLLECT_AT + LQ - 2 (15 of them; kinds udp, onoff and unbound only, since a node takes one
                   fragmenting flow) send to a collector node linked to their row-2 nodes: a node of degree LQ - 1,
                   which create still grants wide windows.  It takes 15 same-time Receives and, at the same
                   timestamp, their zero-delay deliveries (DoForwardUp events on the same node): up to 29 events of
                   one node at one timestamp, more than CH (a hub block's serial pass), inside a wide window.  The
                   collector sends nothing (no ICMP, no echo), so it has no TransmitCompletes to add.
  band_narrow      ICMP on, echo and small columns: tx_min is at most an ICMP error's 46.4 us (18.4 us where a
                   1473-byte datagram's one-byte last fragment is drawn) and Lx above LKD tx_min, so the plan is
                   narrow, and with an echo endpoint lookahead[K_RECEIVE] is 0.
  band_hub         band_narrow with the row-2 nodes of HUB_COLUMNS = 24 neighbouring columns linked to a collector
                   that hosts their UdpServer and PacketSink: more than CH same-time Receives on one node (a hub
                   block), some on modelled devices, inside a timestamp that spans several holder blocks.
  band_src_wide, band_src_narrow
                   band_wide (without its collector) / band_narrow with tests/p2p_sources_fuzz_cases.py's additions,
                   drawn by a second generator, default_rng (K + seed), after the first has finished: a permutation of
                   the onoff columns, of which the first half get OnTime / OffTime variables (SF._variable; a Constant
                   OnTime is replaced by Uniform (1 ms, 3 ms); OffTime is Constant 0 or, one in two, a variable of mean
                   1 to 3 ms), each on its own stream from FIRST_VAR_STREAM up; then a permutation of the udp columns,
                   of which the first TRACE_CLIENTS have their UdpClient replaced by a UdpTraceClient (SF._trace; the
                   wide family's frames give datagrams of 1000 bytes or more).  These families are wider (C_SRC), so
                   that the constant-time columns alone keep the width.
                   monitored (family, seed): the same scenario with frag off and the monitor on, every payload above
                   MAX_PAYLOAD replaced by 1000 bytes (the smallest choice that keeps a wide plan wide).

What create refuses, the generator avoids: what tests/p2p_fuzz_cases.py lists, so at most MAX_RATE_MODELS = 18 Rate
models (FIRST_VAR_STREAM is 20) with three (unit, rate) pairs, one fragmenting flow a node, and a band_wide collector of
degree LQ - 1.  The chains are shallow: three rows, and only the few fast / frag columns keep a queue busy.  (The
holder-region fill limit that tests/test_gpu_p2p_span.py::test_region_guard documents, error 32, was not met by any
shape tried here.)

What the models measured for each case (tests/test_p2p_wide_fuzz_cpu.py asserts the floors; these figures say how far
a case is from them): the largest same-time group after START, the groups above WIDTH = 512, the events, the trace
records and the seconds of the model's run on a CPU host (the scenario's build takes 0.1 s: route_bfs visits three
nodes a destination).  The second line of a band_src case is its monitored variant.

  band_wide        0   largest  788   groups above  39   events  47105   trace records  73144   model 0.7 s
  band_wide        1   largest  845   groups above  39   events  47320   trace records  73004   model 0.5 s
  band_wide        2   largest  814   groups above  39   events  45995   trace records  71164   model 0.4 s
  band_narrow      0   largest  784   groups above  35   events  46700   trace records  73748   model 0.4 s
  band_narrow      1   largest  825   groups above  35   events  46189   trace records  71894   model 0.5 s
  band_narrow      2   largest  819   groups above  35   events  47345   trace records  74579   model 0.5 s
  band_hub         0   largest  778   groups above  35   events  47223   trace records  75181   model 0.5 s
  band_hub         2   largest  820   groups above  35   events  47816   trace records  76054   model 0.7 s
  band_hub         4   largest  793   groups above  35   events  47077   trace records  74569   model 0.6 s
  band_src_wide    0   largest  838   groups above  32   events  52401   trace records  72438   model 1.3 s
                       largest 1042   groups above  32   events  55346   trace records  76136   model 1.4 s   479 flows
  band_src_wide    1   largest  864   groups above  32   events  51798   trace records  71375   model 1.2 s
                       largest 1034   groups above  32   events  54337   trace records  74551   model 1.4 s   480 flows
  band_src_narrow  0   largest  849   groups above  28   events  50745   trace records  72672   model 1.0 s
                       largest  974   groups above  28   events  51130   trace records  72307   model 1.1 s   511 flows
  band_src_narrow  1   largest  842   groups above  27   events  50759   trace records  72157   model 1.2 s
                       largest  957   groups above  28   events  51066   trace records  71817   model 1.4 s   504 flows
"""
import numpy as np

import p2p
import p2p_sources_fuzz_cases as SF
from p2p_fuzz_cases import CH, LQ, MAX_PAYLOAD, MS, RATE_OF_UNIT, US  # noqa: F401
from p2p_sources_fuzz_cases import FIRST_VAR_STREAM, K  # noqa: F401

HB = 64      # window events of one holder block (nsgpu_p2p_dev.h)
NHB = 64     # holder blocks (nsgpu_p2p_dev.h)
LR = 128     # local records of one holder block's region (nsgpu_p2p_win.h)
RKC = 64     # columns of a rank tile (nsgpu_p2p_win.h)
RKCW = 256   # columns of a rel-ts-only rank tile (nsgpu_p2p_win.h)
NHUB = 32    # hub blocks (nsgpu_p2p_win.h)
LKD = 8      # chain levels kept: create grants wide windows up to Lx = LKD tx_min (nsgpu_p2p_dev.h)
WIDTH = 512  # the floor of a wide same-time group: 8 holder blocks of HB, two RKCW tiles, eight RKC tiles
assert WIDTH == 8 * HB == 2 * RKCW == 8 * RKC

R = 3
C_BAND, C_SRC = 361, 481  # (1 modulo 3)
BPS, DELAY = 10_000_000, 1 * MS
# band_hub's links to the collector: 2 ms less two transmissions of a 1030-byte frame (823999 ns each, as the reference
# rounds them), so that the collector's Receives fall on the timestamp of the lockstep columns' row-1 Receives (a group
# above WIDTH), not between two of them
HUB_DELAY = 2 * MS - 2 * 823_999
START = 2 * MS
STOP = {"band_wide": 24 * MS, "band_narrow": 22 * MS, "band_hub": 22 * MS, "band_src_wide": 20 * MS,
        "band_src_narrow": 18 * MS}
FRAG_TIMEOUT = 5 * MS
UNBOUND_PORT = 77
HUB_COLUMNS = 24
COLLECT_AT = 100  # band_wide's collected columns begin here; band_hub's at a drawn column
MAX_RATE_MODELS = 18
TRACE_CLIENTS = 6
QUEUES, SHORT_QUEUES, FRAG_QUEUES = (20, 100), (2, 4), (1, 2, 100)
FRAG_SIZES_WIDE = (2500, 4352)           # last fragments of 1028 and 1400 bytes
FRAG_SIZES_NARROW = (1473, 2000, 4352)   # 1473: a last fragment of one byte
KINDS_WIDE = (("udp", 0.30), ("onoff", 0.40), ("unbound", 0.08), ("fast", 0.08), ("frag", 0.14))
KINDS_NARROW = (("udp", 0.28), ("onoff", 0.36), ("unbound", 0.07), ("fast", 0.07), ("frag", 0.08), ("fragudp", 0.04),
                ("echo", 0.05), ("small", 0.05))
COLLECTED_KINDS = ("udp", "onoff", "unbound")  # what a collected column may carry; others become onoff
LOCKSTEP = ("udp", "onoff", "unbound")


def band(seed, family, C, narrow, collected=0):
    rng = np.random.default_rng(seed)
    kinds_w = KINDS_NARROW if narrow else KINDS_WIDE
    names, weights = [k for k, _w in kinds_w], [w for _k, w in kinds_w]
    draws = [(int(rng.choice(len(names), p=weights)), int(rng.integers(0, 3)), int(rng.integers(0, 6)),
              int(rng.integers(0, 5)), int(rng.integers(0, 12)), int(rng.integers(0, 3)),
              sorted(rng.integers(0, 12, size=3).tolist())) for _c in range(C)]
    first = 0
    if collected:
        first = COLLECT_AT if not narrow else int(rng.integers(0, C - collected))  # (the generator's last draw)
    sc = p2p.Scenario(R * C + (1 if collected else 0), icmp=narrow, ports=True, frag=True, frag_timeout_ns=FRAG_TIMEOUT,
                      rng_seed=1, rng_run=1 + seed % 5)
    collector = R * C if collected else None
    links = []
    for c in range(C):
        q = draws[c][2]
        kind = names[draws[c][0]]
        q0 = (SHORT_QUEUES[q % 2] if kind == "fast" else FRAG_QUEUES[q % 3] if kind in ("frag", "fragudp")
              else QUEUES[q % 2])
        links.append(sc.link(c, C + c, BPS, DELAY, q0))
        links.append(sc.link(C + c, 2 * C + c, BPS, DELAY, 100))
    hub_dev = {}
    for c in range(first, first + collected):
        links.append(sc.link(2 * C + c, collector, BPS, HUB_DELAY if narrow else DELAY, 100))
        hub_dev[c] = links[-1][1]
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.1.0.0") + (k << 8))
    if collected:
        sc.add_udp_server(collector, 0, 0, port=100, window=8)
        sc.add_sink(collector, 0, 0, port=9)
    col_kind, stream = [], 0
    for c in range(C):
        ki, zi, _q, modelled, which, where, lst = draws[c]
        kind = names[ki]
        src, dst = c, 2 * C + c
        if c in hub_dev:
            dst = collector
            if kind not in COLLECTED_KINDS:
                kind = "onoff"
        elif kind in ("udp", "fast", "fragudp"):
            sc.add_udp_server(dst, 0, 0, port=100, window=8)
            sc.add_sink(dst, 0, 0, port=9)  # (a second endpoint: the datagrams find theirs by flow)
        elif kind == "echo":
            sc.add_echo_server(dst, 0, 0, port=7)
        else:
            sc.add_sink(dst, 0, 0, port=9)
        col_kind.append(kind)
        if kind in ("udp", "unbound"):
            sc.add_udp_client(src, dst, START, 0, count=1000, interval_ns=1 * MS, size=1000,
                              remote_port=100 if kind == "udp" else UNBOUND_PORT)
        elif kind == "fast":
            sc.add_udp_client(src, dst, START, 0, count=1000, interval_ns=500 * US, size=1000, remote_port=100)
        elif kind == "fragudp":
            sc.add_udp_client(src, dst, START, 0, count=1000, interval_ns=2 * MS, size=1500, remote_port=100)
        elif kind == "echo":
            sc.add_echo_client(src, dst, START, 0, count=1000, interval_ns=1 * MS, size=1000, remote_port=7)
        elif kind == "small":
            sc.add_onoff(src, dst, START, 0, rate_bps=512_000, size=64, on_s=1.0, off_s=0.0, remote_port=9)
        else:
            sizes = FRAG_SIZES_NARROW if narrow else FRAG_SIZES_WIDE
            size = sizes[zi % len(sizes)] if kind == "frag" else 1000
            sc.add_onoff(src, dst, START, 0, rate_bps=8_000_000, size=size, on_s=1.0, off_s=0.0, remote_port=9)
        if modelled == 0 or (kind in ("frag", "fragudp") and modelled == 1):
            if c in hub_dev:
                d = hub_dev[c] if where else 4 * c + 1
            elif where == 2 and narrow and kind in ("echo", "unbound"):
                d = 4 * c + 2  # (the way back: echo replies, ICMP errors)
            else:
                d = 4 * c + 1 if where % 2 == 0 else 4 * c + 3
            if which < 9 or stream >= MAX_RATE_MODELS:
                sc.set_receive_list_error_model(d, lst)
            else:
                unit = ("pkt", "byte", "bit")[which - 9]
                sc.set_rate_error_model(d, RATE_OF_UNIT[unit], unit=unit, stream=stream)
                stream += 1
    sc.stop(STOP[family])
    sc.route_bfs()
    sc.band = dict(family=family, C=C, kinds=col_kind, collector=collector,
                   collected=list(range(first, first + collected)))
    return sc


def band_src(seed, family, narrow, trace_clients=True):
    sc = band(seed, family, C_SRC, narrow)
    rng = np.random.default_rng(K + seed)
    C, kinds = sc.band["C"], sc.band["kinds"]
    sender_of = {A["node"]: a for a, A in enumerate(sc.apps) if A["kind"] in p2p.SENDERS}
    stream = FIRST_VAR_STREAM
    plain = [c for c in range(C) if kinds[c] == "onoff"]
    for c in rng.permutation(plain)[:(len(plain) + 1) // 2].tolist():
        on, stream = SF._variable(rng, stream, float(rng.choice([1.5, 2.0, 3.0])))
        if on.kind == p2p.RV_CONSTANT:
            on, stream = p2p.Uniform(0.001, 0.003, stream), stream + 1
        off = p2p.Constant(0.0)
        if int(rng.integers(0, 2)):
            off, stream = SF._variable(rng, stream, int(rng.integers(1, 4)))
        SF.set_variables(sc.apps[sender_of[c]], on, off)
        kinds[c] = "onoff_random"
    udp = [c for c in range(C) if kinds[c] == "udp"]
    for c in rng.permutation(udp)[:TRACE_CLIENTS].tolist():
        mps = int(rng.choice(SF.MAX_PACKET_SIZES if narrow else SF.MAX_PACKET_SIZES[1:]))
        sizes = SF.FRAME_SIZES if narrow else (1000, 1000, mps + 1000, 2 * mps + 1000)
        ent = SF._trace(rng, sizes, (0, 1, 1, 2, 3))
        if trace_clients:  # in the UdpClient's place: the same application index, node and setup call
            A = sc.apps[sender_of[c]]
            A.update(kind=p2p.APP_UDP_TRACE_CLIENT, size=mps, count=0, interval=0, entries=ent)
            kinds[c] = "trace"
    return sc


FAMILIES = {
    "band_wide": lambda seed: band(seed, "band_wide", C_BAND, False, collected=LQ - 1),
    "band_narrow": lambda seed: band(seed, "band_narrow", C_BAND, True),
    "band_hub": lambda seed: band(seed, "band_hub", C_BAND, True, collected=HUB_COLUMNS),
    "band_src_wide": lambda seed, **kw: band_src(seed, "band_src_wide", False, **kw),
    "band_src_narrow": lambda seed, **kw: band_src(seed, "band_src_narrow", True, **kw),
}
SRC_FAMILIES = ("band_src_wide", "band_src_narrow")
WIDE_FAMILIES = ("band_wide", "band_src_wide")


def build(family, seed):
    return FAMILIES[family](seed)


def monitored(family, seed):
    """A band_src scenario with frag off and the monitor on, every fragmenting payload replaced by 1000 bytes."""
    assert family in SRC_FAMILIES
    sc = build(family, seed)
    for A in sc.apps:
        if A["kind"] in (p2p.APP_ONOFF, p2p.APP_UDP_CLIENT) and A["size"] > MAX_PAYLOAD:
            A["size"] = 1000
    sc.frag, sc.flowmon = False, True
    p2p.dist_plan(sc, None, 0, 1)  # (create's checks: a refusal raises)
    return sc


# ---------------- what a scenario holds (for the conditions and for a failure's message) ----------------
def columns_of(sc, *kinds):
    return [c for c, k in enumerate(sc.band["kinds"]) if k in kinds]


def column_of_device(sc, d):
    """The column a device belongs to (a collector's device: the column it is linked to)."""
    C = sc.band["C"]
    n = sc.dev[d][0]
    if n == sc.band["collector"]:
        n = sc.dev[sc.dev[d][1]][0]
    return n % C


def modelled_columns(sc, kind, unit=None):
    return sorted({column_of_device(sc, d) for d, e in sc.error_models.items()
                   if e["kind"] == kind and (unit is None or e["unit"] == unit)})


def with_swapped_rate_streams(sc):
    """The first two Rate models of different units get each other's stream."""
    rates = [e for _d, e in sorted(sc.error_models.items()) if e["kind"] == "rate"]
    a = rates[0]
    b = next(e for e in rates if e["unit"] != a["unit"])
    a["stream"], b["stream"] = b["stream"], a["stream"]
    return sc


def without_one_list_entry(sc, used):
    """The first ReceiveList model that `used` (device -> bool) accepts loses its smallest ordinal."""
    for d, e in sorted(sc.error_models.items()):
        if e["kind"] == "list" and used(d):
            e["packets"] = e["packets"][1:]
            return sc
    return None


def describe_node(sc, node):
    """Where the node lies in the band and what its column carries, then SF.describe_node's text."""
    C = sc.band["C"]
    if node == sc.band["collector"]:
        where = "the collector of columns %d..%d" % (sc.band["collected"][0], sc.band["collected"][-1])
    else:
        where = "row %d column %d (%s)" % (node // C, node % C, sc.band["kinds"][node % C])
    return where + " | " + SF.describe_node(sc, node)


# (family, seed): chosen on the models so that the conditions of tests/test_p2p_wide_fuzz_cpu.py hold
WIDE_FUZZ_CASES = (
    ("band_wide", 0), ("band_wide", 1), ("band_wide", 2),
    ("band_narrow", 0), ("band_narrow", 1), ("band_narrow", 2),
    ("band_hub", 0), ("band_hub", 2), ("band_hub", 4),
    ("band_src_wide", 0), ("band_src_wide", 1),
    ("band_src_narrow", 0), ("band_src_narrow", 1),
)
