"""The third seeded set (tests/p2p_wide_fuzz_cases.py: the band families) without a GPU.  These conditions keep
tests/test_gpu_p2p_wide_fuzz.py from quietly testing nothing: every case is accepted by create's checks (through the
host-only plan: single, on two block ranks and on three interleaved ranks) with the plan its family means; it is wide
(at least MIN_GROUPS same-time groups of more than WIDTH events after the applications start); its feature events are
spread over the largest group; it reaches every interaction it is there for; and the model's digest moves when a
feature's state is changed.  All of it is asserted on the composed Python model (tests/p2p_full_pyref.py), which equals
tests/p2p_errmodel_pyref.py on a scenario without trace clients and variables (asserted here on one band too).

The spread is a proxy.  It slices the largest same-time group in the model's order, which is uid order within one
timestamp; the engine's slot order inside a window is its own, so "four slices" stands for "several holder blocks"
and proves nothing about which block handles which event."""
import copy

import numpy as np
import pytest

import p2p
import p2p_errmodel_pyref as E
import p2p_full_pyref as FULL
import p2p_fuzz_cases as FZ
import p2p_wide_fuzz_cases as WF
from p2p_frag_pyref import FRAG_SHIFT
from p2p_pyref import PKT_ICMP, PKT_ICMP_UNREACH, PKT_REPLY

MIN_GROUPS = 10  # same-time groups above WF.WIDTH
MIN_SLICES = 4   # slices of WF.HB events of the largest group that hold a feature event
SEVERAL = 3      # columns an item of the generator's list must occur on
K_RECEIVE = 10   # the event kind of PointToPointNetDevice::Receive (nsgpu_p2p_dev.h): the plan's lookahead index


class Tally:
    """Tallies beside a model (it changes nothing of the run): the events that are feature events (by uid: a Receive on
    a modelled device, of a fragment, of a datagram for an unbound port at its destination, of a UdpServer's datagram
    at its destination) and the nodes whose reassembly timed out."""

    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self.feature_events = {}  # uid -> set of names
        self.timeout_nodes = []
        self.modelled_receives = []  # (ts, device)

    def receive(self, d, p):
        sc, what = self.sc, set()
        if d in self.em:
            what.add("modelled")
            self.modelled_receives.append((self.now, d))
        if not p[0] & PKT_ICMP:
            if p[1] >> FRAG_SHIFT:
                what.add("fragment")
            A = sc.apps[p[0] & ~PKT_REPLY]
            if not p[0] & PKT_REPLY and sc.dev[d][0] == A["dst"]:
                if A["remote_port"] == WF.UNBOUND_PORT:
                    what.add("unbound")
                elif A["remote_port"] == 100:
                    what.add("server")
        if what:
            self.feature_events[self.cur_uid] = what
        return super().receive(d, p)

    def handle_fragments_timeout(self, key, ip, iif):
        self.timeout_nodes.append(key[0])
        return super().handle_fragments_timeout(key, ip, iif)


class Probe(Tally, FULL.Model):
    pass


_runs = {}


def run_model(sc):
    mod = Probe(sc)
    mod.setup()
    mod.run()
    return FULL.results(mod)


def run(family, seed):
    if (family, seed) not in _runs:
        sc = WF.build(family, seed)
        _runs[(family, seed)] = (sc, run_model(sc))
    return _runs[(family, seed)]


def groups(m):
    """(timestamps, counts) of the pop log's same-time groups after the first application start."""
    ts = m["log"][0]
    return np.unique(ts[ts > WF.START], return_counts=True)


def blocks_of(columns):
    """The 64-column blocks a list of columns touches."""
    return {c // WF.HB for c in columns}


ALL = pytest.mark.parametrize("family,seed", WF.WIDE_FUZZ_CASES)


# ---------------- the list and the generators ----------------
def test_the_case_list():
    fams = [fam for fam, _s in WF.WIDE_FUZZ_CASES]
    assert [fams.count(f) for f in ("band_wide", "band_narrow", "band_hub", "band_src_wide", "band_src_narrow")] == \
        [3, 3, 3, 2, 2]
    assert len(set(WF.WIDE_FUZZ_CASES)) == len(WF.WIDE_FUZZ_CASES) and set(fams) == set(WF.FAMILIES)


def test_the_layout_constants():
    assert WF.WIDTH == 8 * WF.HB == 2 * WF.RKCW == 8 * WF.RKC and WF.NHB * WF.HB == 4096 and WF.LR == 2 * WF.HB
    assert WF.C_BAND % 3 == 1 and WF.C_SRC % 3 == 1 and WF.HUB_COLUMNS > WF.CH and WF.LQ - 1 < WF.CH


def test_generators_are_deterministic():
    from p2p_sources_fuzz_cases import signature
    for fam in WF.FAMILIES:
        a, b = WF.build(fam, 3), WF.build(fam, 3)
        assert signature(a) == signature(b) and a.band == b.band
        assert signature(WF.build(fam, 4)) != signature(a)


def test_composed_model_equals_the_error_model_model_on_a_band():
    sc = WF.build("band_hub", WF.WIDE_FUZZ_CASES[6][1])
    a, b = run("band_hub", WF.WIDE_FUZZ_CASES[6][1])[1], E.run(sc)
    assert a["stats"] == b["stats"] and a["frag"] == b["frag"] and a["dropped"] == b["dropped"]
    for k in ("devc", "appc", "servers", "em", "trace"):
        assert np.array_equal(a[k], b[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a["log"], b["log"]))


# ---------------- every case ----------------
@ALL
def test_case_is_accepted_with_the_plan_meant(family, seed):
    sc, m = run(family, seed)
    assert sc.ports and sc.frag and E.check_seed(sc.rng_seed)
    single = p2p.dist_plan(sc, None, 0, 1)
    assert single["n_init"] > 0
    assert bool(single["wide"]) == (family in WF.WIDE_FAMILIES)
    if single["wide"]:
        assert single["tx_min"] < single["lx"] <= WF.LKD * single["tx_min"]
        assert max(np.bincount([D[0] for D in sc.dev])) <= WF.LQ
    C = sc.band["C"]
    for nranks, own in ((2, p2p.owner_blocks(sc.n_nodes, 2)), (3, FZ.owner_interleaved(sc, 3))):
        plans = [p2p.dist_plan(sc, own, r, nranks) for r in range(nranks)]
        assert not p2p.plan_mismatch(plans)
        assert all(bool(pl["wide"]) == (family in WF.WIDE_FAMILIES) for pl in plans)
        # every column's hops cross ranks
        assert all(len({int(own[r * C + c]) for r in range(WF.R)}) > 1 for c in range(C)), nranks
    own = FZ.owner_interleaved(sc, 3)
    assert all(len({int(own[r * C + c]) for r in range(WF.R)}) == 3 for c in range(C))
    assert 20_000 < m["stats"]["dispatched"] < 70_000  # (a GPU test of a few seconds)
    assert m["frag"]["max_list"] < p2p.FRAG_CAP
    streams = [e["stream"] for e in sc.error_models.values() if e["kind"] == "rate"]
    assert len(set(streams)) == len(streams) <= WF.MAX_RATE_MODELS < WF.FIRST_VAR_STREAM
    if family in WF.WIDE_FAMILIES:  # every frame is 1000 bytes or more
        assert not sc.icmp and all(A["size"] >= 1000 for A in sc.apps if A["kind"] in p2p.SENDERS)
    else:
        assert sc.icmp and WF.columns_of(sc, "echo") and WF.columns_of(sc, "small")
        assert single["lookahead"][K_RECEIVE] == 0  # (an echo endpoint: a window ends at a Receive's time)


@ALL
def test_every_item_is_on_several_columns_of_several_blocks(family, seed):
    """What the generator must put on several columns, and not all of them within one block of HB columns (the
    columns' events follow one another in uid order, so neighbouring columns share a slice of a group)."""
    sc, m = run(family, seed)
    mod, C = m["model"], sc.band["C"]
    frag_apps = FZ.fragmenting_flows(sc)
    items = {
        "UdpClient -> UdpServer": WF.columns_of(sc, "udp"),
        "short queue before a UdpServer": WF.columns_of(sc, "fast"),
        "OnOff -> PacketSink": WF.columns_of(sc, "onoff"),
        "fragmenting sender": [sc.apps[a]["node"] % C for a in frag_apps],
        "unbound port": WF.columns_of(sc, "unbound"),
        "ReceiveList model": WF.modelled_columns(sc, "list"),
        "Rate model per packet": WF.modelled_columns(sc, "rate", "pkt"),
        "Rate model per byte": WF.modelled_columns(sc, "rate", "byte"),
        "Rate model per bit": WF.modelled_columns(sc, "rate", "bit"),
        "reassembly timeout": sorted({n % C for n in mod.timeout_nodes}),
    }
    if sc.icmp:
        items["UdpEcho"] = WF.columns_of(sc, "echo")
        items["64-byte frames"] = WF.columns_of(sc, "small")
    for what, cols in items.items():
        assert len(cols) >= SEVERAL and len(blocks_of(cols)) >= 2, (what, cols)
    assert all(min(sc.apps[a]["size"] for a in frag_apps) >= 1473 and sc.apps[a]["size"] <= 4352 for a in frag_apps)
    # every item that is an event of the run occurs (the models are invoked, the servers take datagrams)
    for d in sc.error_models:
        assert m["em"]["invoked"][d] > 0, d


@ALL
def test_width(family, seed):
    _sc, m = run(family, seed)
    _ts, counts = groups(m)
    n = int((counts > WF.WIDTH).sum())
    print(family, seed, "largest same-time group", int(counts.max()), "groups above", WF.WIDTH, ":", n)
    assert n >= MIN_GROUPS, (int(counts.max()), n)


@ALL
def test_spread(family, seed):
    sc, m = run(family, seed)
    ts, counts = groups(m)
    t = ts[int(np.argmax(counts))]
    uids = m["log"][1][m["log"][0] == t]  # (the model's order: uid order within one timestamp)
    assert len(uids) == counts.max() > WF.WIDTH
    feats = m["model"].feature_events
    slices = {}
    for i, u in enumerate(uids.tolist()):
        for what in feats.get(u, ()):
            slices.setdefault(what, set()).add(i // WF.HB)
    every = set().union(*slices.values())
    print(family, seed, {k: sorted(v) for k, v in slices.items()})
    run_len = best = 0  # the longest run of consecutive slices that hold a feature event
    for s in range(len(uids) // WF.HB + 1):
        run_len = run_len + 1 if s in every else 0
        best = max(best, run_len)
    assert best >= MIN_SLICES, sorted(every)
    assert len(slices.get("modelled", ())) >= 2, slices  # (the kind of state a wrong block would lose)


@ALL
def test_reach(family, seed):
    sc, m = run(family, seed)
    st, fr, mod = m["stats"], m["frag"], m["model"]
    assert fr["fragmented"] > 0 and fr["reassembled"] > 0 and fr["timeouts"] > 0 and fr["cancelled_timers"] > 0
    assert fr["reassembled"] < fr["fragmented"]
    # a model or a full queue took a fragment of a datagram whose reassembly timed out
    frag_apps = FZ.fragmenting_flows(sc)
    model_took = {sc.dev[d][0] % sc.band["C"] for d, p in m["dropped"] if not p[0] & PKT_ICMP and p[1] >> FRAG_SHIFT}
    queue_took = {sc.apps[a]["node"] % sc.band["C"] for a in frag_apps
                  if m["devc"]["drop_packets"][FZ.path_devices(sc, sc.apps[a]["node"], sc.apps[a]["dst"])[0]] > 0}
    timed_out = {n % sc.band["C"] for n in mod.timeout_nodes}
    assert timed_out & model_took and timed_out & queue_took, (timed_out, model_took, queue_took)
    for kind, unit in (("list", None), ("rate", "pkt"), ("rate", "byte"), ("rate", "bit")):
        devs = [d for d, e in sc.error_models.items() if e["kind"] == kind and (unit is None or e["unit"] == unit)]
        assert sum(int(m["em"]["corrupted"][d]) for d in devs) > 0, (kind, unit)
        assert any(0 < int(m["em"]["corrupted"][d]) < int(m["em"]["invoked"][d]) for d in devs), (kind, unit)
    assert st["unreach_drops"] > 0
    if sc.icmp:
        tr = m["trace"]
        assert st["icmp_sent"] > 0 and np.any(tr["app"] & PKT_ICMP_UNREACH != 0)
        assert np.any((tr["app"] & PKT_ICMP != 0) & (tr["app"] & PKT_ICMP_UNREACH == 0))  # (a timeout's error)
        assert any(p[0] & (PKT_REPLY | PKT_ICMP) for _d, p in m["dropped"])  # a model took a reply or an error
    else:
        assert st["icmp_sent"] == 0
    lost = [a for a, A in enumerate(sc.apps) if A["kind"] == p2p.APP_UDP_SERVER and m["servers"]["lost"][a] > 0]
    assert len(lost) >= SEVERAL, lost
    # a queue overflow in front of a UdpServer that counts losses
    fast = [c for c in WF.columns_of(sc, "fast") if m["devc"]["drop_packets"][4 * c] > 0]
    assert fast and any(sc.apps[a]["node"] % sc.band["C"] in fast for a in lost)
    if sc.band["collector"] is not None:
        hub = sc.band["collector"]
        ts, _uid, ctx = m["log"]
        vals, counts = np.unique(ts[ctx == hub], return_counts=True)
        hub_models = {d for d in sc.error_models if sc.dev[d][0] == hub}
        assert hub_models
        if family == "band_hub":  # more than CH same-time events, one at least on a modelled device
            crowded = set(vals[counts > WF.CH].tolist())
            assert crowded and any(t in crowded and d in hub_models for t, d in mod.modelled_receives)
            # ... at a timestamp that is itself several holder blocks wide
            gts, gcounts = groups(m)
            assert any(t in crowded for t in gts[gcounts > WF.WIDTH].tolist())
        else:
            # band_wide's collector (degree LQ - 1 <= LQ, so the plan stays wide): at most LQ - 1 same-time Receives,
            # which with their zero-delay deliveries (DoForwardUp events of the same node and time) are more than CH
            # events at one timestamp, some of the Receives on modelled devices
            assert sum(1 for D in sc.dev if D[0] == hub) == WF.LQ - 1
            crowded = set(vals[counts > WF.CH].tolist())
            assert len(crowded) >= MIN_GROUPS
            assert any(t in crowded and d in hub_models for t, d in mod.modelled_receives)
    if family in WF.SRC_FAMILIES:
        rnd, tcs = WF.SF.random_sources(sc), WF.SF.trace_client_apps(sc)
        assert len(rnd) > 64 and len(tcs) == WF.TRACE_CLIENTS
        for a in rnd:
            assert m["draws"]["on_draws"][a] + m["draws"]["off_draws"][a] > 0, a
        assert len(m["ambiguous"]) == 0
        assert all(m["clients"]["sends"][a] > 0 for a in tcs)  # (every client sends bursts, some of several datagrams)
        assert sum(1 for a in tcs if m["clients"]["sent"][a] > m["clients"]["sends"][a]) >= 2
        streams = [v.stream for A in sc.apps for v in (A.get("on_var"), A.get("off_var")) if v is not None]
        assert len(set(streams)) == len(streams) and min(streams) >= WF.FIRST_VAR_STREAM
        # about half of the non-fragmenting OnOff columns draw, and they too lie in several blocks
        plain = len(WF.columns_of(sc, "onoff"))
        assert abs(len(rnd) - plain) <= 1 and len(blocks_of(WF.columns_of(sc, "onoff_random"))) >= 4


@pytest.mark.parametrize("family,seed", [c for c in WF.WIDE_FUZZ_CASES if c[0] in WF.SRC_FAMILIES])
def test_monitored_variant(family, seed):
    sc = WF.monitored(family, seed)  # (create's checks pass: a refusal raises)
    assert sc is not None and sc.flowmon and not sc.frag and not FZ.fragmenting_flows(sc)
    assert bool(p2p.dist_plan(sc, None, 0, 1)["wide"]) == (family in WF.WIDE_FAMILIES)
    m = FULL.run_monitored(sc)
    fl = m["flows"][p2p.MAX_PER_HOP_DELAY_NS]
    assert len(m["ambiguous"]) == 0 and m["stats"]["dispatched"] < 70_000
    assert len(fl) > 64 and int((fl["lost_packets"] > 0).sum()) >= SEVERAL and int((fl["packets_dropped"] > 0).sum())
    _ts, counts = groups(m)
    assert int((counts > WF.WIDTH).sum()) >= MIN_GROUPS


# ---------------- sensitivity: the comparison can see the features at this size ----------------
SENSITIVITY_CASES = (WF.WIDE_FUZZ_CASES[0], WF.WIDE_FUZZ_CASES[6])


@pytest.mark.parametrize("family,seed", SENSITIVITY_CASES)
def test_digest_moves_when_two_rate_models_swap_their_streams(family, seed):
    sc, m = run(family, seed)
    other = FULL.run(WF.with_swapped_rate_streams(copy.deepcopy(sc)))
    assert other["stats"]["digest"] != m["stats"]["digest"]


@pytest.mark.parametrize("family,seed", SENSITIVITY_CASES)
def test_digest_moves_without_one_receive_list_entry(family, seed):
    sc, m = run(family, seed)
    changed = WF.without_one_list_entry(copy.deepcopy(sc), lambda d: int(m["em"]["corrupted"][d]) > 0 and
                                        min(sc.error_models[d]["packets"]) < int(m["em"]["invoked"][d]))
    assert changed is not None
    other = FULL.run(changed)
    assert other["stats"]["digest"] != m["stats"]["digest"]
    assert int(other["em"]["corrupted"].sum()) != int(m["em"]["corrupted"].sum()) or \
        not np.array_equal(other["em"], m["em"])
