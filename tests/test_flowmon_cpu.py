"""Per-flow statistics without a GPU: the Python model (tests/p2p_flowmon_pyref.py) pinned to answers computed by
hand from the scenarios' link parameters, the proof that it leaves the base model's run untouched, the conditions the
scenarios of tests/test_gpu_flowmon.py must meet (asserted on the model alone), the record's layout and the refusals
of the host-only plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flowmon_cases as FMC
import nsgpu
import nsref
import p2p
import p2p_errmodel_pyref
import p2p_flowmon_pyref as FM
import p2p_fuzz_cases as FC

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
DELAYS = (FM.MAX_PER_HOP_DELAY_NS, FMC.SMALL_DELAY_NS)
_runs = {}


def run(name, *args):
    if (name, args) not in _runs:
        sc = getattr(FMC, name)(*args)
        _runs[(name, args)] = (sc, FM.run(sc, ALL_KINDS, DELAYS))
    return _runs[(name, args)]


def hop_ns(sc, dev, ip_len):
    """One hop of an IPv4 packet of ip_len bytes out of device dev: the frame's (PppHeader: 2 bytes) transmission time
    at the device's DataRate, as the device converts it, plus the channel's Delay."""
    _node, _peer, bps, _ifg, delay, _q = sc.dev[dev]
    return nsref.seconds(float(ip_len + 2) * 8 / float(bps)) + delay


# ---------------- known answers ----------------
def test_first_cc_known_answer():
    """first.cc: one 1024-byte echo and its reply over 5 Mb/s, 2 ms.  IPv4 length 1024 + 8 + 20 = 1052; the 1054-byte
    frame takes 1054 * 8 / 5e6 s = 1,686,400 ns, plus 2 ms: 3,686,400 ns each way."""
    sc, m = run("first_cc")
    assert sc.dev[0][2] == 5_000_000 and sc.dev[0][4] == 2_000_000
    one_way = hop_ns(sc, 0, 1052)
    assert one_way == 1_686_400 + 2_000_000 == 3_686_400
    fl = m["flows"][FM.MAX_PER_HOP_DELAY_NS]
    assert list(fl["flow_id"]) == [1, 2]
    assert list(fl["flow"]) == [1, len(sc.apps) + 1]  # application 1 is the client; the reply flow is n_apps + 1
    for r in fl:
        assert r["tx_packets"] == r["rx_packets"] == 1
        assert r["tx_bytes"] == r["rx_bytes"] == 1052
        assert r["delay_sum_ns"] == r["last_delay_ns"] == one_way
        assert r["jitter_sum_ns"] == 0 and r["times_forwarded"] == 0 and r["lost_packets"] == 0
        assert not r["packets_dropped"].any() and not r["bytes_dropped"].any()
    # the client sends at 2 s; the server answers when the request is delivered
    assert fl[0]["time_first_tx_ns"] == fl[0]["time_last_tx_ns"] == 2_000_000_000
    assert fl[0]["time_first_rx_ns"] == fl[1]["time_first_tx_ns"] == 2_000_000_000 + one_way
    assert fl[1]["time_last_rx_ns"] == 2_000_000_000 + 2 * one_way
    assert np.array_equal(m["flows"][FMC.SMALL_DELAY_NS], fl)


def test_three_node_chain_known_answer():
    """One 100-byte datagram (IPv4 length 128, a 130-byte frame) over 10 Mb/s + 1 ms, then 5 Mb/s + 3 ms: forwarded
    once; 104 us + 1 ms + 208 us + 3 ms, each transmission time converted as the device converts it."""
    sc, m = run("chain3", 1)
    delay = hop_ns(sc, 0, 128) + hop_ns(sc, 2, 128)
    assert abs(delay - (104_000 + 1_000_000 + 208_000 + 3_000_000)) <= 2  # (Seconds (double) truncates: 4,311,998)
    (r,) = m["flows"][FM.MAX_PER_HOP_DELAY_NS]
    assert (r["flow_id"], r["flow"]) == (1, 1)
    assert r["tx_packets"] == r["rx_packets"] == 1 and r["tx_bytes"] == r["rx_bytes"] == 128
    assert r["times_forwarded"] == 1
    assert r["delay_sum_ns"] == delay
    assert r["time_first_tx_ns"] == 1_000_000 and r["time_last_rx_ns"] == 1_000_000 + delay
    assert r["jitter_sum_ns"] == 0 and r["lost_packets"] == 0
    # three datagrams a millisecond apart never queue: three equal delays, no jitter
    (r3,) = run("chain3", 3)[1]["flows"][FM.MAX_PER_HOP_DELAY_NS]
    assert r3["rx_packets"] == 3 and r3["delay_sum_ns"] == 3 * delay and r3["times_forwarded"] == 3
    assert r3["jitter_sum_ns"] == 0


def test_incast_counts_add_up():
    """Every datagram is received, dropped by a queue, or still tracked at the stop."""
    sc, m = run("incast3")
    big, small = (m["flows"][d] for d in DELAYS)
    for r, s in zip(big, small):
        q = int(r["packets_dropped"][FM.DROP_QUEUE])
        assert q > 0 and r["bytes_dropped"][FM.DROP_QUEUE] == q * (200 + 28)
        assert r["lost_packets"] == q  # nothing is 10 s old at 45 ms
        in_flight = int(r["tx_packets"] - r["rx_packets"]) - q
        assert in_flight >= 1 and s["lost_packets"] == q + in_flight  # ... but everything in flight is 1 ms old


# ---------------- the model only observes ----------------
def all_cases():
    return [(n, a) for n, a in FMC.GPU_CASES] + [("fuzz", (s,)) for s in FMC.FUZZ_SEEDS if FMC.fuzz(s) is not None]


@pytest.mark.parametrize("name,args", all_cases())
def test_model_leaves_the_base_run_untouched(name, args):
    sc, m = run(name, *args)
    sc.flowmon = False
    try:
        b = p2p_errmodel_pyref.run(sc, ALL_KINDS)
    finally:
        sc.flowmon = True
    assert m["stats"] == b["stats"]
    for x, y in zip(m["log"], b["log"]):
        assert np.array_equal(x, y)
    assert np.array_equal(m["trace"], b["trace"])
    for k in ("devc", "appc", "servers", "em"):
        assert np.array_equal(m[k], b[k]), k
    assert m["dropped"] == b["dropped"]


# ---------------- the GPU scenarios are not vacuous ----------------
def test_gpu_scenarios_cover_every_report():
    diag = {}
    jitter = reply = in_flight = False
    for name, args in FMC.GPU_CASES:
        sc, m = run(name, *args)
        for k, v in m["fm_diag"].items():
            diag[k] = diag.get(k, 0) + v
        big, small = (m["flows"][d] for d in DELAYS)
        jitter = jitter or bool((big["jitter_sum_ns"] > 0).any())
        reply = reply or bool(((big["flow"] >= len(sc.apps)) & (big["rx_packets"] > 0)).any())
        # a packet still in flight at the stop, with no error model in the scenario: not lost under the default
        # delay, lost under the small one
        if not sc.error_models:
            in_flight = in_flight or bool((small["lost_packets"] > big["lost_packets"]).any())
    for k in ("queue_drop_at_sender", "queue_drop_at_forwarder", "ttl_drop_icmp", "ttl_drop_no_icmp", "no_route_drop",
              "unreachable_received", "tracked_eaten_by_error_model"):
        assert diag[k] > 0, k
    assert jitter and reply and in_flight
    # the loss by timeout where an error model ate the frame: tracked to the end, lost only under the small delay
    sc, m = run("chain_errmodel")
    big, small = (m["flows"][d] for d in DELAYS)
    assert m["fm_diag"]["tracked_eaten_by_error_model"] == int((small["lost_packets"] - big["lost_packets"]).sum()) > 0
    assert not big["packets_dropped"].any()
    # the unreachable port's datagrams are received, and counted nowhere else
    sc, m = run("dumbbell4")
    r = m["flows"][DELAYS[0]]
    r = r[r["flow"] == 7][0]
    assert r["rx_packets"] == m["fm_diag"]["unreachable_received"] > 0 and m["appc"]["rx_packets"][3] == 0


def test_hub_scenarios_crowd_one_node():
    """hub_dumbbell's router 1 and star15's hub take more than CH = 16 events at one timestamp (one window: a hub
    block); the dumbbell's router has more devices than a wide engine takes, the star is planned wide.  Both drop at
    the forwarder's bottleneck queue and forward what passes."""
    for name, hub, wide in (("hub_dumbbell", 40, 0), ("star15", 15, 1)):
        sc, m = run(name)
        ts, _uid, ctx = m["log"]
        _vals, counts = np.unique(ts[ctx == hub], return_counts=True)
        assert counts.max() > FC.CH, name
        assert p2p.dist_plan(sc, None, 0, 1)["wide"] == wide, name
        fl = m["flows"][DELAYS[0]]
        assert m["fm_diag"]["queue_drop_at_forwarder"] == int(fl["packets_dropped"][:, FM.DROP_QUEUE].sum()) > 0
        assert fl["times_forwarded"].sum() > 0 and (fl["rx_packets"] > 0).any()


def test_fuzz_seeds():
    """The seeds tests/test_gpu_flowmon.py runs: at least half draw no fragmenting flow, and only those are left out."""
    ran = [s for s in FMC.FUZZ_SEEDS if FMC.fuzz(s) is not None]
    assert 2 * len(ran) >= len(FMC.FUZZ_SEEDS)
    for s in FMC.FUZZ_SEEDS:
        assert (FMC.fuzz(s) is None) == bool(FC.fragmenting_flows(FC.build("mesh", s)))
    for s in ran:
        assert len(run("fuzz", s)[1]["flows"][DELAYS[0]]) >= 8  # (nine senders, replies besides)


# ---------------- layout ----------------
class FlowRecord(C.Structure):
    """nsgpu_flow_record (include/nsgpu_types.h), field for field."""
    _fields_ = [("tx_packets", C.c_uint64), ("tx_bytes", C.c_uint64), ("rx_packets", C.c_uint64),
                ("rx_bytes", C.c_uint64), ("delay_sum_ns", C.c_int64), ("jitter_sum_ns", C.c_int64),
                ("last_delay_ns", C.c_int64), ("time_first_tx_ns", C.c_int64), ("time_last_tx_ns", C.c_int64),
                ("time_first_rx_ns", C.c_int64), ("time_last_rx_ns", C.c_int64), ("times_forwarded", C.c_uint64),
                ("lost_packets", C.c_uint64), ("packets_dropped", C.c_uint64 * 4), ("bytes_dropped", C.c_uint64 * 4),
                ("first_tx_ts", C.c_uint64), ("first_tx_uid", C.c_uint32), ("pad_", C.c_uint32)]


def test_record_and_scenario_layout():
    assert C.sizeof(FlowRecord) == p2p.FLOW_RECORD_DTYPE.itemsize == 184  # (the library asserts the same 184)
    for name, _t in FlowRecord._fields_:
        assert getattr(FlowRecord, name).offset == p2p.FLOW_RECORD_DTYPE.fields[name][1], name
    assert FlowRecord.packets_dropped.offset == 104 and FlowRecord.first_tx_ts.offset == 168
    # the header declares the same fields in the same order
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "nsgpu_types.h")) as f:
        text = f.read()
    body = re.search(r"typedef struct nsgpu_flow_record \{(.*?)\} nsgpu_flow_record;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", x).strip() for x in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _t in FlowRecord._fields_]
    # flowmon is the word behind frag that was padding: no field moves and the struct keeps its size
    S = p2p.ScenarioStruct
    assert S.flowmon.offset == S.frag.offset + 4 == 292 and S.frag_timeout_ns.offset == 296
    assert C.sizeof(S) == S.rng_run.offset + 4 == 368
    s = FMC.first_cc().c_struct()
    assert s.flowmon == 1 and p2p.first_cc().c_struct().flowmon == 0


# ---------------- refusals (the host-only plan) ----------------
def plan(sc, owner=None, nranks=1):
    return p2p.dist_plan(sc, owner, 0, nranks)


def test_refusals_and_acceptance():
    for name, args in FMC.GPU_CASES:
        assert plan(getattr(FMC, name)(*args))["n_init"] > 0
    assert plan(FMC.id_limit(65537))["n_init"] > 0
    sc = FMC.chain3(1)
    sc.frag = True
    with pytest.raises(nsgpu.NsgpuError, match="flowmon with frag is not modelled \\(the reference classifies a "
                                               "non-first fragment by reading payload bytes as a UDP header"):
        plan(sc)
    sc = FMC.chain3(1)
    with pytest.raises(nsgpu.NsgpuError, match="flowmon on a partitioned engine is not modelled"):
        plan(sc, owner=[0, 0, 1], nranks=2)
    sc.flowmon = False  # (the same partition without the monitor is planned)
    assert plan(sc, owner=[0, 0, 1], nranks=2)["n_init"] > 0
    # the word was padding before: anything but 0 or 1 is refused, not taken for a request
    s = FMC.chain3(1).c_struct()
    s.flowmon = 0xA5A5A5A5
    with pytest.raises(nsgpu.NsgpuError, match="flowmon is 2779096485 \\(0 or 1"):
        nsgpu.check(nsgpu.lib().nsgpu_p2p_dist_plan(C.byref(s), None, 0, 1, 0, C.byref(p2p.Plan())))
    # a fuzz seed with a fragmenting flow, monitored as it stands
    sc = FC.build("mesh", 0)
    sc.flowmon = True
    with pytest.raises(nsgpu.NsgpuError, match="flowmon with frag"):
        plan(sc)
