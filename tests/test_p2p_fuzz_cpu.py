"""The seeded cross-feature scenarios (tests/p2p_fuzz_cases.py) without a GPU: every case is accepted by create's
checks (through the host-only plan, single and on three interleaved ranks) and is not vacuous, and the set as a whole
reaches every interaction tests/test_gpu_p2p_fuzz.py is there for.  All of it is asserted on the Python model's run
(tests/p2p_errmodel_pyref.py)."""
import numpy as np
import pytest

import errmodel_cases as EC
import nsgpu
import p2p
import p2p_errmodel_pyref as E
import p2p_frag_pyref
import p2p_fuzz_cases as FZ
from p2p_pyref import PKT_ICMP, PKT_ICMP_UNREACH, PKT_REPLY, TR_IP_TX, TR_RX

_runs = {}


def run(family, seed):
    if (family, seed) not in _runs:
        sc = FZ.build(family, seed)
        _runs[(family, seed)] = (sc, E.run(sc))
    return _runs[(family, seed)]


def features(sc, m):
    """What one case contributes to the set-level conditions (a dict of booleans and a few figures)."""
    f = {}
    st, fr, tr = m["stats"], m["frag"], m["trace"]
    own = FZ.owner_interleaved(sc, 3)
    f["wide"] = bool(p2p.dist_plan(sc, None, 0, 1)["wide"])
    f["dispatched"] = st["dispatched"]
    # same-timestamp events of the busiest node, and whether a frame passes a modelled device's Receive among them
    ts, _uid, ctx = m["log"]
    hub = int(np.bincount(ctx[ctx != 0xFFFFFFFF].astype(np.int64)).argmax())
    vals, counts = np.unique(ts[ctx == hub], return_counts=True)
    f["busiest_node"], f["hub_same_time"] = hub, int(counts.max())
    crowded = vals[counts > FZ.CH]
    hub_models = [d for d in sc.error_models if sc.dev[d][0] == hub]
    rx = tr[(tr["kind"] == TR_RX) & np.isin(tr["dev"], hub_models)]
    f["hub_block_with_modelled_receive"] = bool(np.isin(rx["ts"], crowded).any())
    # a fired timeout and a cancelled timer; with icmp the timeout's error: an event whose first sink call is the
    # Tx of a time-exceeded error (a Receive's first call is the device's Rx)
    first = tr[tr["seq"] == 0]
    timeout_errors = int(np.sum((first["kind"] == TR_IP_TX) & (first["app"] & PKT_ICMP != 0) &
                                (first["app"] & PKT_ICMP_UNREACH == 0)))
    f["timeout_and_cancelled"] = fr["timeouts"] >= 1 and fr["cancelled_timers"] >= 1 and \
        (timeout_errors >= 1 if sc.icmp else st["icmp_sent"] == 0)
    f["timeout_icmp"] = f["timeout_and_cancelled"] and sc.icmp
    dropped_fragment = any(not p[0] & PKT_ICMP and p[1] >> p2p_frag_pyref.FRAG_SHIFT for _d, p in m["dropped"])
    f["model_drops_fragment"] = dropped_fragment and fr["reassembled"] < fr["fragmented"]
    f["unreach_icmp"] = st["unreach_drops"] > 0 and sc.icmp
    f["unreach_no_icmp"] = st["unreach_drops"] > 0 and not sc.icmp
    f["ttl_expiry"] = st["ttl_drops"] > 0
    flows = FZ.fragmenting_flows(sc)
    f["queue_drop_of_fragments"] = any(
        int(m["devc"]["drop_packets"][FZ.path_devices(sc, sc.apps[a]["node"], sc.apps[a]["dst"])[0]]) > 0
        for a in flows)
    f["server_lost"] = bool((m["servers"]["lost"] > 0).any())
    f["drops_reply_or_icmp"] = any(p[0] & (PKT_REPLY | PKT_ICMP) for _d, p in m["dropped"])
    ranks = {int(own[sc.dev[d][0]]) for d, e in sc.error_models.items() if e["enabled"]}
    crossing = any(len({int(own[sc.dev[d][0]]) for d in FZ.path_devices(sc, sc.apps[a]["node"], sc.apps[a]["dst"])}
                       | {int(own[sc.apps[a]["dst"]])}) > 1 for a in flows)
    f["three_ranks_split"] = len(ranks) >= 2 and crossing
    return f


def cases_with(key, families=None):
    return [(fam, seed) for fam, seed in FZ.FUZZ_CASES if (families is None or fam in families) and
            features(*run(fam, seed))[key]]


# ---------------- every case ----------------
def test_the_case_list():
    fams = [fam for fam, _s in FZ.FUZZ_CASES]
    assert fams.count("mesh") >= 10 and fams.count("star") + fams.count("star_large") >= 6
    assert fams.count("star_large") >= 1 and fams.count("star_wide") >= 1
    assert len(set(FZ.FUZZ_CASES)) == len(FZ.FUZZ_CASES)


def test_generators_are_deterministic():
    for fam in FZ.FAMILIES:
        a, b = FZ.build(fam, 3), FZ.build(fam, 3)
        assert a.dev == b.dev and a.apps == b.apps and a.error_models == b.error_models and a.setup == b.setup
        assert (a.icmp, a.frag_timeout_ns, a.rng_seed, a.rng_run) == (b.icmp, b.frag_timeout_ns, b.rng_seed, b.rng_run)
        assert FZ.build(fam, 4).apps != a.apps


@pytest.mark.parametrize("family,seed", FZ.FUZZ_CASES)
def test_case_is_accepted_and_not_vacuous(family, seed):
    sc, m = run(family, seed)
    assert sc.ports and sc.frag and E.check_seed(sc.rng_seed)
    single = p2p.dist_plan(sc, None, 0, 1)
    assert single["n_init"] > 0
    own = FZ.owner_interleaved(sc, 3)
    plans = [p2p.dist_plan(sc, own, r, 3) for r in range(3)]
    assert not p2p.plan_mismatch(plans)
    assert 100 < m["stats"]["dispatched"] < 8000  # (a GPU test of a few seconds)
    assert m["frag"]["max_list"] < p2p.FRAG_CAP  # (the list overflow has its own test)
    assert any(0 < int(c) < int(i) for i, c in m["em"]), m["em"]
    m0 = E.run(EC.without_models(FZ.build(family, seed)))
    assert m0["stats"]["digest"] != m["stats"]["digest"]
    assert np.all(m0["em"]["invoked"] == 0)


# ---------------- the set as a whole ----------------
def test_mesh_cases_have_wide_and_narrow_plans():
    wide = cases_with("wide", ("mesh",))
    narrow = [c for c in FZ.FUZZ_CASES if c[0] == "mesh" and c not in wide]
    assert wide and narrow, (wide, narrow)


def test_star_cases_make_a_hub_block_with_modelled_receives():
    got = cases_with("hub_block_with_modelled_receive", ("star", "star_large"))
    assert got, "no star case has more than CH same-time events at the hub with a modelled Receive among them"
    for fam, seed in FZ.FUZZ_CASES:  # (the busiest node of every star is its hub: a Receive from every leaf at once)
        if fam == "mesh":
            continue
        sc, m = run(fam, seed)
        f = features(sc, m)
        assert f["busiest_node"] == FZ.star_hub(sc) and f["hub_same_time"] >= sc.n_nodes - 2, (fam, seed)
        assert fam == "star_wide" or sc.n_nodes - 2 == FZ.STAR_LEAVES > FZ.CH


def test_which_stars_are_wide():
    """create grants wide windows up to a node degree of LQ, and more than CH = LQ same-time Receives need more
    devices than that: a 24-leaf star is narrow whatever its frames; the 15-leaf star_wide (a hub of LQ devices, large
    frames, no icmp) is wide, and still has more than CH events at one timestamp at its hub."""
    assert FZ.CH >= FZ.LQ
    for fam, seed in FZ.FUZZ_CASES:
        if fam == "mesh":
            continue
        sc, m = run(fam, seed)
        f = features(sc, m)
        degree = sum(1 for D in sc.dev if D[0] == FZ.star_hub(sc))
        if fam == "star_wide":
            assert degree == FZ.LQ and not sc.icmp and f["wide"] and f["hub_same_time"] > FZ.CH, (fam, seed)
        else:
            assert degree == FZ.STAR_LEAVES + 1 > FZ.LQ and not f["wide"], (fam, seed)
    assert "star_wide" in [fam for fam, _s in FZ.FUZZ_CASES]


@pytest.mark.parametrize("key,what", [
    ("timeout_and_cancelled", "a fired fragment timeout and a cancelled timer"),
    ("timeout_icmp", "a fired fragment timeout whose ICMP error is sent"),
    ("model_drops_fragment", "an error model dropping a fragment (reassembled < fragmented)"),
    ("unreach_icmp", "port-unreachable drops with icmp"),
    ("unreach_no_icmp", "port-unreachable drops without icmp"),
    ("ttl_expiry", "a TTL expiry"),
    ("queue_drop_of_fragments", "queue drops on the device a fragmenting flow leaves by"),
    ("server_lost", "a UdpServer with lost > 0"),
    ("drops_reply_or_icmp", "a dropped echo reply or ICMP error"),
    ("three_ranks_split", "modelled devices on two of three interleaved ranks and a fragmenting flow across ranks"),
])
def test_some_case_has(key, what):
    got = cases_with(key)
    assert got, "no case of FUZZ_CASES has " + what
    print(key, got)


# ---------------- the layered models agree on composed input ----------------
@pytest.mark.parametrize("seed", [c[1] for c in FZ.FUZZ_CASES if c[0] == "mesh"][:2])
def test_model_without_error_models_equals_the_frag_model(seed):
    sc = EC.without_models(FZ.mesh(seed))
    a, b = E.run(sc), p2p_frag_pyref.run(sc)
    assert a["stats"] == b["stats"] and a["frag"] == b["frag"] and np.array_equal(a["trace"], b["trace"])
    assert a["frag"]["fragmented"] > 0 and a["stats"]["dispatched"] > 1000


def test_two_fragmenting_flows_into_one_node_are_what_the_generator_avoids():
    """The refusal the generators respect is create's, not the model's."""
    sc = FZ.mesh(0)
    a = FZ.fragmenting_flows(sc)[0]
    src = next(n for n in range(sc.n_nodes) if n not in (sc.apps[a]["dst"], sc.apps[a]["node"]))
    sc.add_onoff(src, sc.apps[a]["dst"], 1 * FZ.MS, 0, size=3000, remote_port=9)
    sc.route_bfs()
    with pytest.raises(nsgpu.NsgpuError, match="receives fragments of 2 fragmenting flows"):
        p2p.dist_plan(sc, None, 0, 1)
