"""The cost of random OnOff times: a 32 x 32 grid in ports mode, one OnOff flow per column from the
top row to a PacketSink in the bottom row (500 kb/s, 512-byte datagrams).  The same sources run with Constant 1 s / 1 s
on and off times, with Uniform (0.5, 1.5) both and with Exponential (1) both; the constant variant runs once more
with the variables given as NSGPU_RV_CONSTANT entries beside one far-away random one ("constant_ext": the extended
handlers and the draw function's constant branch, the same events).  Interleaved runs; the figures are events a second
and windows a run of each, and the Exponential run's ambiguous draws.  A transition event has lookahead 0 and ends its
window, and random times no longer coincide across applications: the window count is expected to rise.  No threshold:
a first measurement.

  python scripts/p2p_ranvar_cost.py [n] [runs] [sim seconds] > cost.json
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


def scenario(n, kind, sim_s):
    sc = p2p.grid(n, n, flows=[])
    sc.ports = True
    sc.rng_seed, sc.rng_run = 1, 1
    sc.setup = [e for e in sc.setup if e[0] != p2p.SETUP_STOP]
    for x in range(n):
        sc.add_sink((n - 1) * n + x, 0, 0, port=9)
    for x in range(n):
        start = 100 * MS + x * 1_000_003  # (the columns out of step)
        on = off = None
        if kind == "uniform":
            on, off = p2p.Uniform(0.5, 1.5, 2 * x), p2p.Uniform(0.5, 1.5, 2 * x + 1)
        elif kind == "exponential":
            on, off = p2p.Exponential(1.0, 2 * x), p2p.Exponential(1.0, 2 * x + 1)
        elif kind == "constant_ext" and x == 0:
            off = p2p.Uniform(1.0, 1.0, 0)  # (min == max: the constant's value, through a draw)
        sc.add_onoff(x, (n - 1) * n + x, start, 0, rate_bps=500_000, size=512, on_s=1.0, off_s=1.0, on_var=on,
                     off_var=off, remote_port=9)
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
    sim_s = float(sys.argv[3]) if len(sys.argv) > 3 else 20.0
    engs = {}
    for k in ("constant", "constant_ext", "uniform", "exponential"):
        engs[k] = p2p.Engine(scenario(n, k, sim_s))
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
        d = eng.onoff_draws()
        rec, over = eng.ambiguous_draws()
        out[k] = dict(ms=[round(x, 3) for x in ms[k]], median_ms=round(med, 3), wide=eng.wide(),
                      events=int(st[k].dispatched), windows=int(st[k].windows),
                      mev_s=round(int(st[k].dispatched) / med / 1e3, 2),
                      events_per_window=round(int(st[k].dispatched) / max(int(st[k].windows), 1), 1),
                      draws=int(d["on_draws"].sum() + d["off_draws"].sum()), ambiguous=len(rec), ambiguous_overflow=over)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
