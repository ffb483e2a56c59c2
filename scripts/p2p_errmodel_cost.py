"""The cost of a modelled Receive: config 4's grid (p2p.grid (n, n)) through the extended handlers
without error models (frag=True, nothing is fragmented) against the same scenario with a RateErrorModel at rate 0 on
every device — every frame draws, none is dropped, so both runs dispatch the same events (the digests are compared)
and the difference is the models' own work: EU_PKT (the draw) and EU_BYTE (the draw and the table lookup).

  python scripts/p2p_errmodel_cost.py [n] [runs] > cost.json
"""
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "ns-3-dev-dnemu_amd")]
import p2p  # noqa: E402


def measure(unit, n, runs):
    sc = p2p.grid(n, n)
    sc.frag = True
    if unit:
        for d in range(len(sc.dev)):
            sc.set_rate_error_model(d, 0.0, unit=unit, stream=d)
    eng = p2p.Engine(sc)
    eng.run()  # warm-up
    ms = []
    for _ in range(runs):
        eng.reset()
        eng.results()  # (waits for the reset's copies)
        t0 = time.perf_counter()
        eng.launch()
        st = eng.results()[0]
        ms.append((time.perf_counter() - t0) * 1e3)
    em = eng.error_models()
    out = dict(unit=unit or "none", ms=[round(x, 3) for x in ms], median_ms=round(statistics.median(ms), 3),
               events=int(st.dispatched), digest=int(st.digest), wide=eng.wide(),
               receives_modelled=int(em["invoked"].sum()), corrupted=int(em["corrupted"].sum()))
    out["mev_s"] = round(out["events"] / out["median_ms"] / 1e3, 2)
    eng.close()
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    res = [measure(u, n, runs) for u in (None, "pkt", "byte", None)]
    assert len({r["digest"] for r in res}) == 1 and all(r["corrupted"] == 0 for r in res)
    base = statistics.mean(r["median_ms"] for r in res if r["unit"] == "none")
    for r in res:
        if r["unit"] != "none":
            r["ns_per_modelled_receive"] = round((r["median_ms"] - base) * 1e6 / r["receives_modelled"], 3)
    print(json.dumps(dict(grid=n, runs=res)))


if __name__ == "__main__":
    main()
