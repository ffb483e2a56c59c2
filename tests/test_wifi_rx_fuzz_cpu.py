"""The seeded scenarios of the open-loop Wi-Fi receive engine (tests/wifi_rx_fuzz_cases.py) on the CPU alone:
the two restatements (oracle/nsref_wifi.cc, tests/wifi_pyref.py) agree on every case the Python model runs, no
committed case has a decision within 1e-9 of a threshold, each family reaches what it is there for (asserted on
the model's own instrumentation), and a case is a function of (family, seed) only."""
import functools

import numpy as np
import pytest

import wifi
import wifi_pyref
import wifi_rx_fuzz_cases as fc
from test_wifi_oracle import run_oracle

IDS = [fc.case_id(c) for c in fc.CASES]
MODEL_CASES = [c for c in fc.CASES if c[0] != "blocks"]


@functools.lru_cache(maxsize=None)
def case(family, seed):
    return fc.build(family, seed)


@functools.lru_cache(maxsize=None)
def model(family, seed):
    c = case(family, seed)
    info = {}
    return wifi_pyref.run(c["sc"], fc.durations(c["sc"]), info) + (info,)


@functools.lru_cache(maxsize=None)
def oracle_stats(family, seed):
    return run_oracle(case(family, seed)["sc"], rx_log=False)[0]


@pytest.mark.parametrize("family,seed", MODEL_CASES, ids=[fc.case_id(c) for c in MODEL_CASES])
def test_restatements_agree(family, seed):
    """The fields of test_oracle_matches_independent_restatement, on every case the Python model runs."""
    c = case(family, seed)
    assert c["model"]
    sc = c["sc"]
    st, phys, base, ends, log = run_oracle(sc)
    pst, plog, pends, pbase, pphy, _ = model(family, seed)
    assert pst["rx"] <= 60_000
    for f in ("dispatched", "tx", "rx", "sync", "drop_rx", "drop_tx", "drop_ed", "cca_evals", "cca_switches",
              "end", "end_cancelled", "final_ts", "next_uid"):
        assert getattr(st, f) == pst[f], f
    assert list(base) == pbase
    assert len(ends) == len(pends)
    pe = sorted(pends, key=lambda e: e["uid"])
    for a, b in zip(ends, pe):
        assert (a["ts"], a["sync_ts"], a["uid"], a["phy"], a["tx"], a["flags"]) == \
            (b["ts"], b["sync_ts"], b["uid"], b["phy"], b["tx"], b["flags"])
    n = sc.n_phy
    for (k, j), (ts, uid, outcome, flags, cca) in plog.items():
        r = log[k * n + j]
        assert (r["ts"], r["uid"], r["outcome"], r["flags"] & 3, r["cca_ns"]) == (ts, uid, outcome, flags, cca), (k, j)
    assert int((log["outcome"] != wifi.NOT_RUN).sum()) == st.rx
    for j in range(n):
        for f in ("rx", "sync", "drop_rx", "drop_tx", "drop_ed", "cca_switches", "end", "end_cancelled", "ni_max"):
            assert phys[j][f] == pphy[j][f], (j, f)
        assert phys[j]["ni_len"] == len(pphy[j]["ni_t"])
        assert phys[j]["first_power"] == pphy[j]["first"]


@pytest.mark.parametrize("family,seed", fc.CASES, ids=IDS)
def test_no_decision_near_a_threshold(family, seed):
    """The GPU's pow / log10 differ from glibc's in the last bits: a case with a power within 1e-9 of a threshold could
    differ legitimately, so none is committed."""
    st = oracle_stats(family, seed)
    assert st.near_threshold == 0 and st.rx > 0


def test_mixed_coverage():
    chains, stops, cut = set(), set(), 0
    for family, seed in fc.CASES:
        if family != "mixed":
            continue
        c = case(family, seed)
        st, info = model(family, seed)[0], model(family, seed)[5]
        for f in ("sync", "drop_rx", "drop_tx", "drop_ed", "cca_switches", "end_cancelled"):
            assert st[f] > 0, (seed, f)
        sc = c["sc"]
        assert 20 <= sc.n_phy <= 200 and 150 <= len(sc.tx) <= 400 and 1 <= len(set(sc.channel)) <= 3
        assert len(set(zip(sc.tx["modclass"], sc.tx["rate"], sc.tx["bw"]))) >= 5
        du = fc.durations(sc)
        assert min(du) < 100_000 and max(du) > 10_000_000
        assert sc.tx["size"].min() >= 14 and sc.tx["size"].max() <= 2304 and len(set(sc.tx["dbm"])) == len(sc.tx)
        assert sorted(sc.node) != list(range(sc.n_phy)) and len(set(sc.node)) == sc.n_phy
        chains.add(c["chain"])
        stops.add(c["stop"])
        cut += info["undispatched"] > 0
        if c["stop"] == "inside":  # receptions in flight at the Stop
            assert info["undispatched"] > 0 and any(not (e["flags"] & wifi.END_DISPATCHED) for e in model(family, seed)[2])
    assert chains == set(fc.CHAIN_KINDS) and stops == set(fc.STOPS) and cut >= 1


@pytest.mark.parametrize("seed", [s for f, s in fc.CASES if f == "near"])
def test_near_coverage(seed):
    info = model("near", seed)[5]
    for f in ("zero_delay", "tie_rr", "tie_re", "sync_at_tx", "rx_at_own_tx"):
        assert info[f] > 0, f


def test_near_runs_every_chain_kind():
    assert {case(f, s)["chain"] for f, s in fc.CASES if f == "near"} == set(fc.NEAR_CHAINS)


@pytest.mark.parametrize("seed", [s for f, s in fc.CASES if f == "burst"])
def test_burst_window(seed):
    c = case("burst", seed)
    assert fc.largest_window(c["sc"]) == c["window"] == fc.BURST_W[seed % 4] and c["sc"].n_phy >= 100
    assert c["expect"] == ("equal" if c["window"] <= fc.WSORT_MAX else "window")


def test_burst_windows_straddle_the_capacity():
    assert sorted(case(f, s)["window"] for f, s in fc.CASES if f == "burst") == [63, 64, 65, 80]


@pytest.mark.parametrize("seed", [s for f, s in fc.CASES if f == "pending"])
def test_pending_maxima(seed):
    c = case("pending", seed)
    pe = model("pending", seed)[5]["pe_max"]
    assert max(pe) == c["pe_max"] == fc.PENDING[seed % 4][0]
    assert all(pe[v] == c["pe_max"] for v in c["victims"]) and len(c["victims"]) == fc.PENDING[seed % 4][1]
    assert sum(1 for v in pe if v == c["pe_max"]) == len(c["victims"])
    assert c["expect"] == ("equal" if c["pe_max"] <= fc.PE_CAP else "pending")


def test_pending_reaches_the_capacity_and_one_more():
    got = sorted((case(f, s)["pe_max"], len(case(f, s)["victims"])) for f, s in fc.CASES if f == "pending")
    assert got == [(5, 1), (8, 1), (8, 3), (9, 1)] and fc.PE_CAP == 8


@pytest.mark.parametrize("seed", [s for f, s in fc.CASES if f == "queues"])
def test_queues_figures(seed):
    c = case("queues", seed)
    st, pphy, info = model("queues", seed)[0], model("queues", seed)[4], model("queues", seed)[5]
    ni_max = max(p["ni_max"] for p in pphy)
    if c["variant"] == "ni":  # the list reaches the capacity exactly, and the phy goes on receiving afterwards
        assert ni_max == c["ni_max"] == c["sc"].ni_cap == fc.ni_pow2(ni_max) in (16, 32)
        assert fc.ni_pow2(c["ni_below"]) == ni_max // 2
        full = [j for j, p in enumerate(pphy) if p["ni_max"] == ni_max]
        assert full and all(pphy[j]["rx"] > ni_max for j in full)
    elif c["variant"] == "deep":
        # (40 asked; 91 and more put 64 phys' end queues past the 160 KB of LDS a block of the MI355X may use)
        assert fc.overlap(c["sc"]) >= c["overlap_min"] == 91 and ni_max <= c["sc"].ni_cap
        assert fc.lds_plan(c["sc"], c["sc"].n_phy, 256, 160 * 1024)[2] < 64
    else:
        assert max(info["starts_max"]) == c["starts_max"] == 12 > fc.SCAP_LDS
        k = int(np.argmax(info["starts_max"]))
        assert k == 0 and 0 < st["tx"] - 30 == 18  # (15 frames before the two rings' 18, 15 after)
    assert {case(f, s)["variant"] for f, s in fc.CASES if f == "queues"} == {"ni", "deep", "overflow"}


def test_blocks_phy_counts():
    got = [case(f, s)["sc"].n_phy for f, s in fc.CASES if f == "blocks"]
    assert got == [1023, 1024, 1025, 2049, 4100, 9217, 65_600]
    for f, s in fc.CASES:
        if f == "blocks":
            sc = case(f, s)["sc"]
            assert 20 <= len(sc.tx) <= 40 and len(set(sc.channel)) == 2
            assert case(f, s)["rx_log"] == (sc.n_phy < 9000)


@pytest.mark.parametrize("family,seed", fc.CASES, ids=IDS)
def test_blocks_outcomes_and_families_seed_count(family, seed):
    if family == "blocks":
        st = oracle_stats(family, seed)
        assert st.sync > 0 and st.drop_ed > 0 and st.drop_rx + st.drop_tx > 0
    assert sum(1 for f, _ in fc.CASES if f == family) >= 4


@pytest.mark.parametrize("family,seed", fc.CASES, ids=IDS)
def test_cases_are_deterministic(family, seed):
    a, b = fc.build(family, seed)["sc"], fc.build(family, seed)["sc"]
    for f in ("x", "y", "z", "channel", "node", "tx"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.loss, a.ed, a.cca, a.uid_start, a.stop_ts, a.stop_uid, a.ni_cap) == \
        (b.loss, b.ed, b.cca, b.uid_start, b.stop_ts, b.stop_uid, b.ni_cap)
