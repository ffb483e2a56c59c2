"""The second seeded set (tests/p2p_sources_fuzz_cases.py: trace clients and random OnOff times on top of the
cross-feature scenarios) without a GPU: the composed model (tests/p2p_full_pyref.py) equals the models it is made of
where their inputs coincide; every case is accepted by create's checks (through the host-only plan, single and on three
interleaved ranks) and is not vacuous; the set as a whole reaches every interaction tests/test_gpu_p2p_sources_fuzz.py
is there for; and the model's digest moves under every change a wrong kernel could amount to."""
import numpy as np
import pytest

import nsgpu
import p2p
import p2p_errmodel_pyref
import p2p_full_pyref as FULL
import p2p_fuzz_cases as FZ
import p2p_ranvar_pyref
import p2p_sources_fuzz_cases as SF
import p2p_trace_client_pyref
import ranvar_cases
import udp_trace_cases
from p2p_pyref import TR_DROP, TR_IP_RX, TR_RX


class Probe(FULL.Model):
    """The composed model with three tallies beside it (it changes nothing of the run): the datagrams of every Send,
    the nodes that reassembled a datagram, the bursts of a random source that sent nothing."""

    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self.send_sizes = {}      # trace client -> [datagrams of each Send]
        self.reassembled_at = {}  # node -> datagrams reassembled there
        self.empty_bursts = {}    # random source -> on periods in which it sent nothing
        self._tx_at_start = {}

    def tc_send(self, a):
        n0 = self.app[a]["sent"]
        super().tc_send(a)
        self.send_sizes.setdefault(a, []).append(self.app[a]["sent"] - n0)

    def process_fragment(self, n, p, iif):
        whole = super().process_fragment(n, p, iif)
        if whole is not None:
            self.reassembled_at[n] = self.reassembled_at.get(n, 0) + 1
        return whole

    def start_sending(self, a):
        self._tx_at_start[a] = self.app[a]["c"]["tx_packets"]
        super().start_sending(a)

    def stop_sending(self, a):
        if self._tx_at_start.get(a) == self.app[a]["c"]["tx_packets"]:
            self.empty_bursts[a] = self.empty_bursts.get(a, 0) + 1
        super().stop_sending(a)


_runs = {}


def run(family, seed):
    if (family, seed) not in _runs:
        sc = SF.build(family, seed)
        mod = Probe(sc)
        mod.setup()
        mod.run()
        _runs[(family, seed)] = (sc, FULL.results(mod))
    return _runs[(family, seed)]


def own_datagrams(tr, apps):
    """The records of `tr` that name a datagram of one of the applications `apps` itself (no reply, no ICMP error)."""
    return tr[np.isin(tr["app"], apps)] if len(apps) else tr[:0]


def features(family, sc, m):
    """What one case contributes to the set-level conditions (a dict of booleans and a few figures)."""
    f = {}
    mod, tr, st = m["model"], m["trace"], m["stats"]
    own = FZ.owner_interleaved(sc, 3)
    tcs, rnd = SF.trace_client_apps(sc), SF.random_sources(sc)
    node_of_dev = np.array([D[0] for D in sc.dev])
    wide = bool(p2p.dist_plan(sc, None, 0, 1)["wide"])
    f["wide_with_trace_client"] = wide and any(mod.app[a]["sent"] for a in tcs)
    f["wide_with_random_source"] = wide and any(m["draws"]["on_draws"][a] for a in rnd)
    f["narrow_mesh"] = not wide and family == "mesh"
    for k in ("wrap_joined", "zero_remainder", "header_only"):
        f[k] = m["tc_diag"][k] > 0
    # a client stopped between two Sends of a cycle: its pending Send was cancelled and then dispatched
    f["stopped_in_mid_cycle"] = any(
        sc.apps[a]["stop"] and mod.app[a]["current_entry"] != 0 and mod.app[a]["send_ev"].cancelled and
        (mod.app[a]["send_ev"].ts, mod.app[a]["send_ev"].uid) <= (mod.now, mod.cur_uid) for a in tcs)
    drops = tr[tr["kind"] == TR_DROP]
    f["burst_overflows_own_queue"] = any(
        len(own_datagrams(drops[drops["dev"] == FZ.path_devices(sc, sc.apps[a]["node"], sc.apps[a]["dst"])[0]], [a]))
        for a in tcs)
    f["rate_model_corrupts_trace_datagram"] = any(
        p[0] in tcs and sc.error_models[d]["kind"] == "rate" and sc.error_models[d]["unit"] in ("byte", "bit")
        for d, p in m["dropped"])
    iprx = tr[tr["kind"] == TR_IP_RX]
    at_dst = {a: len(own_datagrams(iprx[node_of_dev[iprx["dev"]] == sc.apps[a]["dst"]], [a])) for a in tcs}
    to_unbound = any(sc.apps[a]["remote_port"] == SF.UNBOUND_PORT and at_dst[a] for a in tcs)
    f["unbound_icmp"] = to_unbound and sc.icmp and st["icmp_sent"] > 0
    f["unbound_no_icmp"] = to_unbound and not sc.icmp
    # the hub's crowded timestamps (stars only), and whose Receives are among them
    f["hub_block_trace_client"] = f["hub_block_random_source"] = False
    if family != "mesh":
        hub = FZ.star_hub(sc)
        ts, _uid, ctx = m["log"]
        vals, counts = np.unique(ts[ctx == hub], return_counts=True)
        crowded = vals[counts > FZ.CH]
        rx = tr[(tr["kind"] == TR_RX) & (node_of_dev[tr["dev"]] == hub)]
        rx = rx[np.isin(rx["ts"], crowded)]
        f["hub_block_trace_client"] = len(own_datagrams(rx, tcs)) > 0
        f["hub_block_random_source"] = len(own_datagrams(rx, rnd)) > 0
    f["reassembles_and_takes_trace_datagrams"] = any(
        mod.reassembled_at.get(sc.apps[a]["dst"], 0) and at_dst[a] for a in tcs)
    f["fragmenting_random_source"] = any(
        sc.apps[a]["size"] > FZ.MAX_PAYLOAD and m["appc"]["tx_packets"][a] and m["draws"]["on_draws"][a] for a in rnd)
    f["bounded_redraw"] = any(v.kind == p2p.RV_EXPONENTIAL and v.p1 and v.attempts > v.draws
                              for a in rnd for v in mod.var[a])
    f["empty_burst"] = any(mod.empty_bursts.get(a, 0) for a in rnd)
    f["max_bytes_in_a_burst"] = any(sc.apps[a]["maxb"] and mod.app[a]["tot"] >= sc.apps[a]["maxb"] and
                                    mod.on_at_stop.get(a) is False for a in rnd)
    f["stopped_while_on"] = any(sc.apps[a]["stop"] and mod.on_at_stop.get(a) is True for a in rnd)
    f["variables_on_two_ranks"] = len({int(own[sc.apps[a]["node"]]) for a in rnd
                                       if m["draws"]["on_draws"][a] + m["draws"]["off_draws"][a]}) >= 2
    f["trace_client_across_ranks"] = any(own[sc.apps[a]["node"]] != own[sc.apps[a]["dst"]] and at_dst[a] for a in tcs)
    f["random_source_across_ranks"] = any(own[sc.apps[a]["node"]] != own[sc.apps[a]["dst"]] and
                                          m["appc"]["tx_packets"][a] for a in rnd)
    return f


def cases_with(key):
    return [(fam, seed) for fam, seed in SF.SRC_FUZZ_CASES if features(fam, *run(fam, seed))[key]]


# ---------------- the composition ----------------
def same_run(a, b, keys):
    assert a["stats"] == b["stats"]
    for x, y in zip(a["log"], b["log"]):
        assert np.array_equal(x, y)
    for k in keys:
        if isinstance(a[k], dict):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("family,seed", [("mesh", 0), ("star", 1)])
def test_without_clients_or_variables_it_is_the_error_model_model(family, seed):
    sc = FZ.build(family, seed)
    a, b = FULL.run(sc), p2p_errmodel_pyref.run(sc)
    same_run(a, b, ("devc", "appc", "servers", "frag", "em", "trace"))
    assert a["dropped"] == b["dropped"] and b["frag"]["fragmented"] > 0
    assert not a["clients"].view(np.uint8).any() and not a["draws"].view(np.uint8).any()


@pytest.mark.parametrize("name", ["grid_pipelines", "exact_and_tiny"])
def test_without_variables_frag_or_models_it_is_the_trace_client_model(name):
    sc = getattr(udp_trace_cases, name)()
    a, b = FULL.run(sc), p2p_trace_client_pyref.run(sc)
    same_run(a, b, ("devc", "appc", "servers", "clients", "tc_diag", "trace"))
    assert b["tc_diag"]["bursts_over_one"] > 0 and not a["em"].view(np.uint8).any()


@pytest.mark.parametrize("name", ["grid4", "stops"])
def test_without_trace_clients_it_is_the_random_times_model(name):
    sc = getattr(ranvar_cases, name)()
    a, b = FULL.run(sc), p2p_ranvar_pyref.run(sc)
    same_run(a, b, ("devc", "appc", "servers", "frag", "em", "trace", "draws", "ambiguous"))
    assert b["draws"]["on_draws"].sum() > 0 and not a["clients"].view(np.uint8).any()


def test_monitored_composition_equals_its_parts():
    """The same over the flowmon model: the flow records of the trace client's and of the random times' monitored
    models."""
    sc = udp_trace_cases.overflow(True)
    a, b = FULL.run_monitored(sc), p2p_trace_client_pyref.run_monitored(sc)
    same_run(a, b, ("devc", "appc", "servers", "clients", "em", "trace"))
    assert all(np.array_equal(a["flows"][d], b["flows"][d]) for d in b["flows"])
    sc = ranvar_cases.grid4(True)
    a, b = FULL.run_monitored(sc), p2p_ranvar_pyref.run_monitored(sc)
    same_run(a, b, ("devc", "appc", "servers", "em", "trace", "draws", "frag"))
    assert all(np.array_equal(a["flows"][d], b["flows"][d]) for d in b["flows"])


# ---------------- every case ----------------
def test_the_case_list():
    fams = [fam for fam, _s in SF.SRC_FUZZ_CASES]
    assert fams.count("mesh") >= 8 and fams.count("star") + fams.count("star_large") >= 4
    assert fams.count("star_large") >= 1 and fams.count("star_wide") >= 2
    assert len(set(SF.SRC_FUZZ_CASES)) == len(SF.SRC_FUZZ_CASES)


def test_which_cases_are_wide():
    wide = tuple(c for c in SF.SRC_FUZZ_CASES if p2p.dist_plan(run(*c)[0], None, 0, 1)["wide"])
    assert wide == SF.WIDE_CASES
    fams = {fam for fam, _s in wide}
    assert fams == {"mesh", "star_wide"} and all(c in wide for c in SF.SRC_FUZZ_CASES if c[0] == "star_wide")


def test_generators_are_deterministic_and_leave_the_first_set_alone():
    for fam in SF.FAMILIES:
        a, b = SF.build(fam, 3), SF.build(fam, 3)
        assert SF.signature(a) == SF.signature(b)
        assert SF.signature(SF.build(fam, 4)) != SF.signature(a)
        # FZ's scenario is a prefix of it: the same devices, models and applications but for the OnOff times
        base = FZ.build(fam, 3)
        assert a.dev == base.dev and a.error_models == base.error_models and len(a.apps) > len(base.apps)
        for A, B in zip(a.apps, base.apps):
            if B["kind"] != p2p.APP_ONOFF:
                assert A == B
            else:
                assert {k for k in A if A[k] != B[k]} <= {"on", "off", "on_var", "off_var", "stop"}
            assert (A["kind"], A["node"], A["dst"], A["size"], A["rate"]) == \
                (B["kind"], B["node"], B["dst"], B["size"], B["rate"])
        m = SF.monitored(fam, 3)
        if m is not None:
            assert m.flowmon and not m.frag and not FZ.fragmenting_flows(m)


@pytest.mark.parametrize("family,seed", SF.SRC_FUZZ_CASES)
def test_case_is_accepted_and_not_vacuous(family, seed):
    sc, m = run(family, seed)
    mod = m["model"]
    assert sc.ports and sc.frag and p2p_errmodel_pyref.check_seed(sc.rng_seed)
    single = p2p.dist_plan(sc, None, 0, 1)
    assert single["n_init"] > 0
    own = FZ.owner_interleaved(sc, 3)
    plans = [p2p.dist_plan(sc, own, r, 3) for r in range(3)]
    assert not p2p.plan_mismatch(plans)
    assert 100 < m["stats"]["dispatched"] < 8000  # (a GPU test of a few seconds)
    assert m["frag"]["max_list"] < p2p.FRAG_CAP
    assert len(m["ambiguous"]) == 0
    tcs = SF.trace_client_apps(sc)
    assert tcs and SF.random_sources(sc)
    for a in tcs:  # (every client starts: its start time is below the run's Stop)
        assert sum(1 for n in mod.send_sizes[a] if n > 1) >= 2, (a, mod.send_sizes[a])
    assert m["draws"]["on_draws"].sum() >= 10 and m["draws"]["off_draws"].sum() >= 10
    assert any(0 < int(c) < int(i) for i, c in m["em"]), m["em"]
    streams = [v.stream for A in sc.apps for v in (A.get("on_var"), A.get("off_var")) if v is not None]
    assert len(set(streams)) == len(streams) and min(streams) >= SF.FIRST_VAR_STREAM
    assert all(e["stream"] < SF.FIRST_VAR_STREAM for e in sc.error_models.values() if e["kind"] == "rate")


@pytest.mark.parametrize("family,seed", SF.SRC_FUZZ_CASES)
def test_monitored_variant_has_no_ambiguous_draw(family, seed):
    sc = SF.monitored(family, seed)
    if sc is None:
        return
    m = FULL.run_monitored(sc)
    assert len(m["ambiguous"]) == 0 and len(m["flows"][p2p.MAX_PER_HOP_DELAY_NS]) > 0
    assert m["stats"]["dispatched"] < 8000


def test_at_least_half_of_the_cases_have_a_monitored_variant():
    n = sum(1 for fam, seed in SF.SRC_FUZZ_CASES if SF.monitored(fam, seed) is not None)
    assert 2 * n >= len(SF.SRC_FUZZ_CASES)


# ---------------- the set as a whole ----------------
@pytest.mark.parametrize("key,what", [
    ("wide_with_trace_client", "a wide plan that holds a trace client"),
    ("wide_with_random_source", "a wide plan that holds a random source"),
    ("narrow_mesh", "a narrow mesh plan"),
    ("wrap_joined", "a cycle's last burst joined to the next cycle's first"),
    ("zero_remainder", "a frame that MaxPacketSize divides"),
    ("header_only", "a header-only datagram"),
    ("stopped_in_mid_cycle", "a trace client stopped in mid-cycle, with its Send cancelled"),
    ("burst_overflows_own_queue", "a burst that overflows the sender's own queue"),
    ("rate_model_corrupts_trace_datagram", "a trace client's datagram corrupted by a byte- or bit-unit Rate model"),
    ("unbound_icmp", "a trace client's datagrams to an unbound port, with icmp"),
    ("unbound_no_icmp", "a trace client's datagrams to an unbound port, without icmp"),
    ("hub_block_trace_client", "a trace client's Receive at the hub among more than CH same-time events"),
    ("hub_block_random_source", "a random source's Receive at the hub among more than CH same-time events"),
    ("reassembles_and_takes_trace_datagrams", "a node that reassembles fragments and receives trace-client datagrams"),
    ("fragmenting_random_source", "a fragmenting source with random times"),
    ("bounded_redraw", "a bounded Exponential with a redraw"),
    ("empty_burst", "an on time shorter than the packet interval (a burst that sends nothing)"),
    ("max_bytes_in_a_burst", "a random source ended by MaxBytes inside a burst"),
    ("stopped_while_on", "a random source ended by its Stop time while it is on"),
    ("variables_on_two_ranks", "variables on two of three interleaved ranks"),
    ("trace_client_across_ranks", "a trace client whose server is on another of three interleaved ranks"),
    ("random_source_across_ranks", "a random source whose sink is on another of three interleaved ranks"),
])
def test_some_case_has(key, what):
    got = cases_with(key)
    assert got, "no case of SRC_FUZZ_CASES has " + what
    print(key, got)


# ---------------- sensitivity: what a wrong kernel could amount to moves the digest ----------------
def digests_differ(variant):
    """The cases whose digest differs between the model's run and variant (family, seed) -> a results dict or None."""
    out = []
    for fam, seed in SF.SRC_FUZZ_CASES:
        v = variant(fam, seed)
        if v is not None and v["stats"]["digest"] != run(fam, seed)[1]["stats"]["digest"]:
            out.append((fam, seed))
    return out


@pytest.mark.parametrize("nudge", ["drop_zero_remainder", "no_wrap_join"])
def test_digest_moves_under_the_trace_clients_nudges(nudge):
    assert digests_differ(lambda fam, seed: FULL.run(SF.build(fam, seed), nudge=nudge))


def test_digest_moves_when_a_source_swaps_its_streams():
    def variant(fam, seed):
        sc = SF.with_swapped_streams(SF.build(fam, seed))
        return None if sc is None else FULL.run(sc)
    assert digests_differ(variant)


def test_digest_moves_when_every_variable_is_its_mean():
    got = digests_differ(lambda fam, seed: FULL.run(SF.with_constant_means(SF.build(fam, seed))))
    assert len(got) == len(SF.SRC_FUZZ_CASES)  # (every case draws)


def test_digest_moves_without_the_trace_clients():
    got = digests_differ(lambda fam, seed: FULL.run(SF.build(fam, seed, trace_clients=False)))
    assert len(got) == len(SF.SRC_FUZZ_CASES)


# ---------------- the refusals the generator respects are create's ----------------
def test_a_variable_on_a_rate_models_stream_is_refused():
    sc = SF.build("mesh", SF.SRC_FUZZ_CASES[0][1])
    rate = next(e for e in sc.error_models.values() if e["kind"] == "rate" and e["enabled"])
    A = next(A for A in sc.apps if A.get("on_var") is not None or A.get("off_var") is not None)
    (A["on_var"] if A["on_var"] is not None else A["off_var"]).stream = rate["stream"]
    with pytest.raises(nsgpu.NsgpuError,
                       match="names RngStream %d, which a Rate error model names too" % rate["stream"]):
        p2p.dist_plan(sc, None, 0, 1)


def test_a_max_packet_size_of_1473_is_refused():
    sc = SF.build("mesh", SF.SRC_FUZZ_CASES[0][1])
    sc.apps[SF.trace_client_apps(sc)[0]]["size"] = 1473
    with pytest.raises(nsgpu.NsgpuError, match="MaxPacketSize 1473 outside \\[1, 1472\\]"):
        p2p.dist_plan(sc, None, 0, 1)
