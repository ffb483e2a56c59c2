"""Scenarios of the random OnOff time tests, shared by tests/test_ranvar_cpu.py (the conditions the scenarios must
meet, asserted on the Python model alone: tests/p2p_ranvar_pyref.py) and tests/test_gpu_ranvar.py (the engine against
the model).  Every scenario is small: a model run takes about a second at most.  The seeds are chosen so that the
model lists no ambiguous draw in any of them (test_ranvar_cpu.py asserts it for every entry of CASES)."""
import errmodel_cases as EC
import p2p

MS, US = 1_000_000, 1_000


def two_nodes(kind, rng_seed=1, rng_run=1):
    """Two nodes, one 5 Mb/s / 1 ms link, one OnOff (2 Mb/s, 200-byte datagrams: 0.8 ms apart) into a PacketSink, until
    Simulator::Stop at 1.2 s: several hundred transitions, most bursts cut by a random stop (the residual bits), and
    on times below one packet interval (a cancelled send and nothing sent).
      "uniform"  Uniform (1 ms, 5 ms) on and off times
      "exp"      Exponential (mean 3 ms) both
      "bounded"  Exponential (mean 3 ms, bound 4 ms) on, Exponential (mean 3 ms, bound 1 ms) off"""
    sc = EC.line(2, [(5_000_000, 1 * MS)], rng_seed=rng_seed, rng_run=rng_run)
    sc.add_sink(1, 0, 0)
    if kind == "uniform":
        on, off = p2p.Uniform(0.001, 0.005, 0), p2p.Uniform(0.001, 0.005, 1)
    elif kind == "exp":
        on, off = p2p.Exponential(0.003, 0), p2p.Exponential(0.003, 1)
    else:
        on, off = p2p.Exponential(0.003, 0, bound=0.004), p2p.Exponential(0.003, 1, bound=0.001)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=2_000_000, size=200, on_var=on, off_var=off)
    sc.stop(1200 * MS)
    sc.route_bfs()
    return sc


def stops():
    """The same link with two sources: application 1 has MaxBytes 30,000 and stops itself in the middle of a burst
    (ScheduleNextTx's StopApplication draws nothing, and its pending StopSending still fires and draws), application 2
    is stopped by its Stop time (300 ms) while it is on; both have long on times (Uniform (20 ms, 40 ms)) and short
    Exponential off times, and streams given out of order."""
    sc = EC.line(2, [(5_000_000, 1 * MS)], rng_seed=7, rng_run=3)
    sc.add_sink(1, 0, 0)
    sc.add_onoff(0, 1, 1 * MS, 0, rate_bps=1_000_000, size=250, max_bytes=30_000,
                 on_var=p2p.Uniform(0.020, 0.040, 5), off_var=p2p.Exponential(0.002, 2))
    sc.add_onoff(0, 1, 2 * MS, 300 * MS, rate_bps=1_500_000, size=300,
                 on_var=p2p.Uniform(0.020, 0.040, 9), off_var=p2p.Exponential(0.002, 0))
    sc.stop(600 * MS)
    sc.route_bfs()
    return sc


def grid4(flowmon=False):
    """A 4 x 4 grid in ports mode (10 Mb/s, 200 us links): six OnOff sources with Constant / Uniform / Exponential on
    and off times in every pairing, into PacketSinks; a UdpClient / UdpServer pair across the grid; a RateErrorModel
    (EU_PKT 0.1) on one device of a path, whose stream (11) is none of the variables'."""
    n = 4
    sc = p2p.Scenario(n * n, ports=True, rng_seed=3, rng_run=2, flowmon=flowmon)
    links = []
    for y in range(n):
        for x in range(n):
            if x > 0:
                links.append(sc.link(y * n + x - 1, y * n + x, 10_000_000, 200 * US, 50))
            if y > 0:
                links.append(sc.link((y - 1) * n + x, y * n + x, 10_000_000, 200 * US, 50))
    sc.install_stack()
    for k, (da, db) in enumerate(links):
        sc.assign_link(da, db, p2p.ip("10.0.0.0") + (k << 8))
    for node in (15, 12, 3, 0, 10):
        sc.add_sink(node, 0, 0, port=9)
    sc.add_udp_server(13, 0, 0, port=100, window=32)
    C, U, E = p2p.Constant, p2p.Uniform, p2p.Exponential
    src = [(0, 15, C(0.004), U(0.001, 0.003, 0)),
           (3, 12, U(0.002, 0.006, 1), C(0.002)),
           (12, 3, E(0.003, 2), U(0.0, 0.004, 3)),
           (15, 0, U(0.003, 0.003, 4), E(0.002, 5)),
           (5, 10, E(0.004, 6, bound=0.008), E(0.001, 7, bound=0.004)),
           (6, 10, C(0.003), E(0.0015, 8))]
    for i, (s, d, on, off) in enumerate(src):
        sc.add_onoff(s, d, 1 * MS + i * 37 * US, 0 if i % 2 else 150 * MS, rate_bps=1_500_000 + 250_000 * i,
                     size=180 + 40 * i, on_var=on, off_var=off, remote_port=9, max_bytes=40_000 if i == 2 else 0)
    sc.add_udp_client(1, 13, 2 * MS, 0, count=150, interval_ns=1 * MS, size=120, remote_port=100)
    sc.stop(200 * MS)
    sc.route_bfs()
    # the device on which node 13 receives from node 9 (the UdpClient's last hop, and nothing else's)
    dev = next(d for d, r in enumerate(sc.dev) if r[0] == 13 and sc.dev[r[1]][0] == 9)
    sc.set_rate_error_model(dev, 0.1, unit="pkt", stream=11)
    return sc


# (name, args) of every scenario a GPU test compares with the model: the model must list no ambiguous draw in them
CASES = (("two_nodes", ("uniform",)), ("two_nodes", ("exp",)), ("two_nodes", ("bounded",)), ("stops", ()),
         ("grid4", ()), ("grid4", (True,)))

# A constructed ambiguous draw (test_ranvar_cpu.py finds the mean; the value is pinned there): the first draw of
# stream 0 with seed 1, run 1
AMBIGUOUS_SEED, AMBIGUOUS_RUN, AMBIGUOUS_STREAM = 1, 1, 0


def first_u(seed=AMBIGUOUS_SEED, run=AMBIGUOUS_RUN, stream=AMBIGUOUS_STREAM):
    import p2p_errmodel_pyref
    return p2p_errmodel_pyref.RngStream(seed, run, stream).u01()


def ambiguous_mean(u, target_ns=3_000_000, span=8, targets=256):
    """A mean near target_ns / (|log u| * 1e9) for which -mean * hi and -mean * hi's neighbour (the two values a libm
    log below 1 ulp can give) fall on either side of a whole nanosecond: a search over a few ulps of the mean around
    K / (|hi| * 1e9), for K = target_ns and, where the products step over that boundary's two doubles, the next ones."""
    import math

    import nsref
    import p2p_ranvar_pyref as RV
    hi, nb, _frac = RV.exact_log(u)
    assert nb != hi
    for K in range(target_ns, target_ns + targets):
        lo_m = up_m = K / (abs(hi) * 1e9)
        for _ in range(span):
            for m in (lo_m, up_m):
                if nsref.seconds(-m * hi) != nsref.seconds(-m * nb):
                    return m
            lo_m, up_m = math.nextafter(lo_m, 0.0), math.nextafter(up_m, math.inf)
    raise AssertionError("no ambiguous mean")


def ambiguous_bound(u, mean=0.003):
    """A bound that -mean * hi meets and -mean * neighbour does not, or the other way round."""
    import p2p_ranvar_pyref as RV
    hi, nb, _frac = RV.exact_log(u)
    r1, r2 = -mean * hi, -mean * nb
    assert r1 != r2
    return min(r1, r2)
