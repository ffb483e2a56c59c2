"""The cost of UdpTraceClient sources: a 32 x 32 grid in ports mode, one flow per column from the top
row to a UdpServer in the bottom row.  Variant "trace": every source is a UdpTraceClient with the default trace
(MaxPacketSize 1024: 11 datagrams and 6,187 bytes every 360 ms, in bursts of 4, 3 and 4).  Variant "client": every
source is a UdpClient of the same mean rate (562-byte datagrams, one every 360 / 11 ms).  Interleaved runs; the figure
is events a second of each and the time a datagram costs end to end.  The lookaheads follow a flow's smallest frame
(the default trace's 134-byte frame keeps this grid's windows narrow where 562-byte datagrams let them be wide), so a
third variant, "client_small", runs UdpClients with 134-byte datagrams: the window effect without the bursts.  No
threshold: a first measurement.

  python scripts/p2p_trace_client_cost.py [n] [runs] [sim seconds] > cost.json
"""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "ns-3-dev-dnemu_amd")]
import p2p  # noqa: E402

MS, S = 1_000_000, 1_000_000_000


def scenario(n, trace, sim_s, size=562):
    sc = p2p.grid(n, n, flows=[])
    sc.ports = True
    sc.setup = [e for e in sc.setup if e[0] != p2p.SETUP_STOP]
    for x in range(n):
        sc.add_udp_server((n - 1) * n + x, 0, 0, port=100, window=32)
    for x in range(n):
        start = 100 * MS + x * 1_000_003  # (the columns out of step, as independent video sources are)
        if trace:
            sc.add_udp_trace_client(x, (n - 1) * n + x, start, 0, max_packet_size=1024, remote_port=100)
        else:
            sc.add_udp_client(x, (n - 1) * n + x, start, 0, count=1 << 24, interval_ns=360 * MS // 11, size=size,
                              remote_port=100)
    sc.stop(int(sim_s * S))
    sc.route_bfs()
    return sc


def once(eng):
    eng.reset()
    eng.results()  # (waits for the reset's copies)
    t0 = time.perf_counter()
    eng.launch()
    st = eng.results()[0]
    return (time.perf_counter() - t0) * 1e3, st


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sim_s = float(sys.argv[3]) if len(sys.argv) > 3 else 10.0
    engs = {}
    for k, trace, size in (("client", False, 562), ("client_small", False, 134), ("trace", True, 0)):
        engs[k] = p2p.Engine(scenario(n, trace, sim_s, size))
        engs[k].run()  # warm-up
    ms = {k: [] for k in engs}
    st = {}
    for _ in range(runs):  # interleaved
        for k, eng in engs.items():
            t, st[k] = once(eng)
            ms[k].append(t)
    out = dict(grid=n, sim_s=sim_s)
    for k, eng in engs.items():
        med = statistics.median(ms[k])
        srv = eng.udp_servers()
        out[k] = dict(ms=[round(x, 3) for x in ms[k]], median_ms=round(med, 3), wide=eng.wide(),
                      events=int(st[k].dispatched), windows=int(st[k].windows),
                      mev_s=round(int(st[k].dispatched) / med / 1e3, 2), received=int(srv["received"].sum()),
                      lost=int(srv["lost"].sum()),
                      us_per_datagram=round(med * 1e3 / max(int(srv["received"].sum()), 1), 4))
    out["trace"]["sends"] = int(engs["trace"].trace_clients()["sends"].sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
