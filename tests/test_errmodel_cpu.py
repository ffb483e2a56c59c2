"""Receive error models without a GPU: the RngStream restatements against values recorded from the reference, the
C ABI's refusals, layout and threshold tables, and the conditions the scenarios of tests/test_gpu_errmodel.py must
meet (asserted on the Python model alone, tests/p2p_errmodel_pyref.py)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import errmodel_cases as EC
import nsgpu
import p2p
import p2p_errmodel_pyref as E

CH = 16  # events of one node above which a hub block runs them (nsgpu_p2p_dev.h)
_runs = {}


def kat():
    with open(os.path.join(os.path.dirname(__file__), "golden", "rng_stream_kat.json")) as f:
        return json.load(f)


def run(name, *args, models=True):
    if (name, args, models) not in _runs:
        sc = getattr(EC, name)(*args)
        if not models:
            EC.without_models(sc)
        _runs[(name, args, models)] = (sc, E.run(sc))
    return _runs[(name, args, models)]


# ---------------- the generator ----------------
def test_python_generator_equals_the_reference():
    k = kat()
    assert [(c["seed"], c["run"]) for c in k["cases"]] == [(1, 1), (1, 3), (12345, 7)]
    for c in k["cases"]:
        assert sorted(c["streams"]) == ["0", "1", "2", "5"]
        for s, vals in c["streams"].items():
            g = E.RngStream(c["seed"], c["run"], int(s))
            assert [g.u01().hex() for _ in range(k["n"])] == vals, (c["seed"], c["run"], s)


def test_host_generator_equals_the_reference():
    """nsgpu_rng_stream_run on the host: the jump matrices (squared from the one-step matrices) and the step."""
    k = kat()
    for c in k["cases"]:
        for s, vals in c["streams"].items():
            got = p2p.rng_stream(c["seed"], c["run"], int(s), k["n"])
            assert [x.hex() for x in got.tolist()] == vals, (c["seed"], c["run"], s)


def test_seed_and_run_zero_select_the_defaults():
    assert np.array_equal(p2p.rng_stream(0, 0, 2, 8), p2p.rng_stream(1, 1, 2, 8))


def test_streams_far_apart():
    """Stream and run numbers with several bits set: the jumps composed by the bits equal the jumps one by one."""
    g = E.RngStream(7, 11, 37)
    assert [g.u01() for _ in range(4)] == p2p.rng_stream(7, 11, 37, 4).tolist()


def test_check_seed():
    for seed in (4294944443, 4294967087, 0xFFFFFFFF):
        with pytest.raises(nsgpu.NsgpuError, match="not a seed RngStream::CheckSeed accepts"):
            p2p.rng_stream(seed, 1, 0, 1)
        assert not E.check_seed(seed)
    assert len(p2p.rng_stream(4294944442, 1, 0, 1)) == 1


# ---------------- layout ----------------
def test_struct_layout_of_the_appended_fields():
    S = p2p.ScenarioStruct
    # (offsetof / sizeof of nsgpu_p2p_scenario in include/nsgpu_types.h, as a C compiler lays it out on x86-64)
    assert S.frag_timeout_ns.offset == 296  # the last field before this feature keeps its place
    want = 304
    for f in ("dev_em_kind", "dev_em_enabled", "dev_em_unit", "dev_em_rate", "dev_em_stream", "em_list_off", "em_list"):
        assert getattr(S, f).offset == want, f
        want += 8
    assert S.rng_seed.offset == 360 and S.rng_run.offset == 364
    assert C.sizeof(S) == 368
    assert p2p.ERROR_MODEL_DTYPE.itemsize == 8


def test_no_model_leaves_the_struct_fields_null():
    s = EC.udp_list("none").c_struct()
    assert not s.dev_em_kind and not s.em_list and s.rng_seed == 0


# ---------------- thresholds ----------------
@pytest.mark.parametrize("unit", ["byte", "bit"])
@pytest.mark.parametrize("rate", [1e-5, 0.01])
def test_threshold_table(unit, rate):
    t = p2p.error_model_thresholds(unit, rate)
    assert len(t) == 1503
    for n in range(1503):
        assert t[n] == 1 - math.pow(1 - rate, n if unit == "byte" else 8 * n), n
        assert t[n] == E.threshold(unit, rate, n)


# ---------------- refusals ----------------
def plan(sc):
    return p2p.dist_plan(sc, None, 0, 1)


def test_refusals_and_acceptance():
    assert plan(EC.udp_list("list"))["n_init"] > 0
    sc = EC.rate_both_ends((4, 4), 1)
    with pytest.raises(nsgpu.NsgpuError, match="devices 0 and 1 name the same RngStream 4"):
        plan(sc)
    sc = EC.rate_both_ends((4, 4), 1)
    sc.error_models[0]["enabled"] = False  # (a disabled model draws nothing: it uses no stream)
    assert plan(sc)["n_init"] > 0
    sc = EC.udp_list("rate0")
    sc.error_models[1]["rate"] = float("nan")
    with pytest.raises(nsgpu.NsgpuError, match="device 1: the Rate error model's ErrorRate is NaN"):
        plan(sc)
    for seed in (4294944443, 0xFFFFFFFF):
        sc = EC.udp_list("rate0")
        sc.rng_seed = seed
        with pytest.raises(nsgpu.NsgpuError, match="rng_seed %d is not a seed RngStream::CheckSeed accepts" % seed):
            plan(sc)
    sc = EC.udp_list("rate0")
    sc.rng_seed = 4294944442
    assert plan(sc)["n_init"] > 0
    with pytest.raises(NotImplementedError, match="ListErrorModel"):
        EC.udp_list("none").set_list_error_model(1, [5])
    with pytest.raises(ValueError, match="unit"):
        EC.udp_list("none").set_rate_error_model(1, 0.1, unit="word")


def test_list_error_model_and_unknown_kinds_are_refused_by_the_library():
    sc = EC.udp_list("list")
    for kind, msg in ((p2p.EM_LIST, "device 1: ListErrorModel is not modelled"), (9, "unknown error model kind 9")):
        s = sc.c_struct()
        s._keep["dev_em_kind"][1] = kind
        pl = p2p.Plan()
        with pytest.raises(nsgpu.NsgpuError, match=msg):
            nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan(C.byref(s), None, 0, 1, 0, C.byref(pl)))
    s = EC.udp_list("rate0").c_struct()
    s._keep["dev_em_unit"][1] = 3
    with pytest.raises(nsgpu.NsgpuError, match="unknown error unit 3"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan(C.byref(s), None, 0, 1, 0, C.byref(p2p.Plan())))


def test_threshold_table_cap():
    """NSGPU_EM_MAX_TABLES distinct (unit, rate) pairs are accepted (EU_PKT needs none, equal pairs share one); one
    more is refused."""
    def star(rates):
        sc = p2p.Scenario(len(rates) + 1)
        for i in range(len(rates)):
            sc.link(i + 1, 0, 1_000_000, 1_000_000)
        sc.install_stack()
        sc.add_sink(0, 0, 0)
        sc.add_onoff(1, 0, 0, 0)
        sc.stop(1_000_000)
        sc.route_bfs()
        for i, (unit, r) in enumerate(rates):
            sc.set_rate_error_model(2 * i + 1, r, unit=unit, stream=i)
        return sc
    ok = [("byte", 1e-4 * (i + 1)) for i in range(8)] + [("bit", 1e-4 * (i + 1)) for i in range(8)]
    assert len(ok) == p2p.EM_MAX_TABLES
    assert plan(star(ok + [("byte", 1e-4), ("pkt", 0.5), ("pkt", 0.25)]))["n_init"] > 0
    with pytest.raises(nsgpu.NsgpuError, match="more than 16 distinct \\(unit, rate\\) pairs"):
        plan(star(ok + [("bit", 0.5)]))


def test_lookahead_is_unchanged_by_a_model():
    a, b = plan(EC.udp_list("list")), plan(EC.udp_list("none"))
    assert a["lookahead"] == b["lookahead"] and a["lookw"] == b["lookw"] and a["wide"] == b["wide"]


# ---------------- the scenarios of the GPU tests are not vacuous ----------------
# (the deliberate rate-0 / rate-1 / disabled cases are test_degenerate_cases')
@pytest.mark.parametrize("name,args", EC.GPU_CASES)
def test_every_modelled_device_drops_and_passes(name, args):
    sc, m = run(name, *args)
    _sc0, m0 = run(name, *args, models=False)
    assert sc.error_models
    for d in sc.error_models:
        inv, cor = (int(x) for x in m["em"][d])
        assert inv == int(m["devc"]["rx_packets"][d]) > 0, d  # (every modelled device here sees traffic)
        assert 0 < cor < inv, (d, inv, cor)
    assert sum(1 for _ in m["dropped"]) == int(m["em"]["corrupted"].sum())
    assert m["stats"]["digest"] != m0["stats"]["digest"]
    assert np.all(m0["em"]["invoked"] == 0)


def test_udp_server_loss_equals_the_drops_inside_the_loss_window():
    """PacketLossCounter counts a missing sequence number once the window (8) has passed it, and never number 0: of
    the dropped 0, 3 and 19 that is number 3."""
    sc, m = run("udp_list", "list")
    seqs = sorted(p[3] >> 8 for _d, p in m["dropped"])
    assert seqs == [0, 3, 19]
    srv = m["servers"][0]
    inside = [s for s in seqs if s >= 1 and s + 8 <= int(srv["last_max_seq"])]
    assert int(srv["lost"]) == len(inside) == 1
    assert int(srv["received"]) == 17


def test_degenerate_cases():
    sc0, m0 = run("udp_list", "none")
    _s, r0 = run("udp_list", "rate0")
    assert tuple(r0["em"][1]) == (20, 0) and r0["stats"]["digest"] == m0["stats"]["digest"]
    _s, r1 = run("udp_list", "rate1")
    assert tuple(r1["em"][1]) == (20, 20) and int(r1["servers"][0]["received"]) == 0
    assert r1["stats"]["digest"] != m0["stats"]["digest"]
    _s, dis = run("udp_list", "disabled")
    assert tuple(dis["em"][1]) == (0, 0) and dis["stats"]["digest"] == m0["stats"]["digest"]
    assert np.array_equal(dis["devc"], m0["devc"]) and np.array_equal(dis["trace"], m0["trace"])


def test_chain_echo_drops_a_reply_and_an_icmp_error_on_the_way_back():
    sc, m = run("chain_echo")
    back = [p for d, p in m["dropped"] if d == 0]
    assert any(p[0] & 0x80000000 for p in back), "no echo reply dropped"
    assert any(p[0] & 0x40000000 for p in back), "no ICMP error dropped"
    assert m["stats"]["icmp_sent"] > 0 and m["stats"]["unreach_drops"] > 0
    assert {d for d, _p in m["dropped"]} == {0, 1, 3}


@pytest.mark.parametrize("icmp", [False, True])
def test_frag_loss_conditions(icmp):
    sc, m = run("frag_loss", icmp)
    # every dropped frame is a middle fragment (offset 1480, more fragments)
    for _d, p in m["dropped"]:
        assert (p[1] >> 16) & 0x1FFF == 1480 // 8 and p[1] & 0x20000000
    assert m["frag"]["timeouts"] >= 1 and m["frag"]["cancelled_timers"] >= 1 and m["diag"]["mixed"] >= 1
    assert (m["stats"]["icmp_sent"] >= 1) == icmp
    assert m["frag"]["reassembled"] < m["frag"]["fragmented"]


def test_the_two_stream_assignments_differ():
    for rng_run in (1, 3):
        a, b = run("rate_both_ends", (0, 1), rng_run)[1], run("rate_both_ends", (1, 0), rng_run)[1]
        assert a["stats"]["digest"] != b["stats"]["digest"]
        assert not np.array_equal(a["em"], b["em"])
    assert run("rate_both_ends", (0, 1), 1)[1]["stats"]["digest"] != run("rate_both_ends", (0, 1), 3)[1]["stats"]["digest"]


def test_mixed_sizes_thresholds_straddle_the_draws():
    """Both units see 1502-, 250- and 60-byte frames, and the large frames are dropped far more often than the small."""
    sc, m = run("mixed_sizes")
    for d, unit, rate in ((1, "byte", 5e-4), (0, "bit", 6e-5)):
        assert 0.45 < E.threshold(unit, rate, 1502) < 0.6 and E.threshold(unit, rate, 60) < 0.05
        sizes = [p[2] for dd, p in m["dropped"] if dd == d]
        assert sizes.count(1502) >= 5 and sizes.count(1502) > 3 * sizes.count(60)
    all_sizes = {int(s) + 2 for s in m["trace"]["size"][m["trace"]["kind"] == 3]}
    assert {1502, 250, 60} <= all_sizes
    assert m["frag"]["timeouts"] >= 1


@pytest.mark.parametrize("n_leaves", [40, 2000])
def test_hub_scenario_makes_a_hub_window_with_modelled_receives(n_leaves):
    """Router 1 (node n_leaves) takes n_leaves same-time Receives — more than CH events of one node in one window —
    and those on devices 13 and 25 are among them."""
    sc, m = run("hub_dumbbell", n_leaves)
    ts, _uid, ctx = m["log"]
    at = ts[ctx == n_leaves]
    vals, counts = np.unique(at, return_counts=True)
    assert counts.max() >= n_leaves > CH
    assert tuple(m["em"][13]) == (2, 1) and tuple(m["em"][25]) == (2, 1)
    assert sc.dev[13][0] == sc.dev[25][0] == n_leaves and sc.dev[1][0] == n_leaves + 1


def test_wide_and_narrow_plans():
    assert plan(EC.grid_wide())["wide"] == 1
    assert plan(EC.frag_loss(False))["wide"] == 1 and plan(EC.frag_loss(True))["wide"] == 0


def test_group_owners_split_the_modelled_devices():
    sc = EC.chain_echo()
    own = p2p.owner_blocks(sc.n_nodes, 2)
    assert {int(own[sc.dev[d][0]]) for d in sc.error_models} == {0, 1}
    sc = EC.rate_both_ends((0, 1), 3)
    own = p2p.owner_blocks(sc.n_nodes, 2)
    assert [int(own[sc.dev[d][0]]) for d in (0, 1)] == [0, 1]


def test_model_without_error_models_equals_the_frag_model():
    import frag_cases
    import p2p_frag_pyref
    sc = frag_cases.loss_at_forwarder(True)
    a, b = E.run(sc), p2p_frag_pyref.run(sc)
    assert a["stats"] == b["stats"] and a["frag"] == b["frag"] and np.array_equal(a["trace"], b["trace"])
