"""The cost of the per-flow statistics: a 32 x 32 grid in ports mode (p2p.grid (n, n), so the extended
handlers either way) with flowmon off and on, the same scenario both ways, interleaved; both runs dispatch the same
events (the digests are compared).  An unmonitored engine of this scenario runs the deferred pipeline, a monitored one
the scanning pipeline (a flow's first transmission records the event's uid), so a third variant runs the unmonitored
scenario traced into a one-record buffer, which also selects the scanning pipeline: on against that is the hooks' own
work.  Beside it the wall time of Engine.flow_records (the sweep kernel, the copies of the flows' records and a
synchronisation).

  python scripts/p2p_flowmon_cost.py [n] [runs] > cost.json
"""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "ns-3-dev-dnemu_amd")]
import p2p  # noqa: E402


def engine(n, flowmon, scanning):
    sc = p2p.grid(n, n)
    sc.ports = True
    sc.flowmon = flowmon
    eng = p2p.Engine(sc)
    if scanning:
        eng.set_trace(1, 0)  # (no kind recorded: the trace buffer only takes the engine off the deferred pipeline)
    eng.run()  # warm-up
    return eng


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
    variants = (("off", False, False), ("off_scanning", False, True), ("on", True, False))
    engs = {k: engine(n, fm, scan) for k, fm, scan in variants}
    ms = {k: [] for k in engs}
    st = {}
    for _ in range(runs):  # interleaved
        for k, eng in engs.items():
            t, st[k] = once(eng)
            ms[k].append(t)
    assert len({int(s.digest) for s in st.values()}) == 1
    sweep = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fl = engs["on"].flow_records()
        sweep.append((time.perf_counter() - t0) * 1e3)
    out = dict(grid=n, events=int(st["on"].dispatched), flows=int((fl["tx_packets"] > 0).sum()),
               tx_packets=int(fl["tx_packets"].sum()), rx_packets=int(fl["rx_packets"].sum()),
               forwards=int(fl["times_forwarded"].sum()), flow_records_ms=[round(x, 3) for x in sweep],
               flow_records_median_ms=round(statistics.median(sweep), 3))
    for k in engs:
        med = statistics.median(ms[k])
        out[k] = dict(ms=[round(x, 3) for x in ms[k]], median_ms=round(med, 3), wide=engs[k].wide(),
                      mev_s=round(out["events"] / med / 1e3, 2))
    reports = out["tx_packets"] + out["rx_packets"] + out["forwards"]
    out["ns_per_report"] = round((out["on"]["median_ms"] - out["off_scanning"]["median_ms"]) * 1e6 / reports, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
