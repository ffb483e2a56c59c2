"""The scenarios of tests/test_gpu_p2p_coldpaths.py really produce the kinds they are meant to (the oracle and the
Python model alone, no GPU): a case that silently had no event on an out-of-line path would test nothing."""
import numpy as np

import coldpaths_cases as CC
import p2p
import p2p_errmodel_pyref
from test_gpu_trace import oracle_full

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS


def test_mixed_has_every_cold_kind():
    g = CC.mixed()
    st, devc, appc, _log, tr = oracle_full(g, 0, kinds=ALL_KINDS)
    assert st.dispatched < 400_000
    assert st.cancelled > 0            # Sends cancelled by StopSending / StopApplication
    assert st.ttl_drops > 0            # the TTL 3 flow expires mid-path
    assert st.unreach_drops > 0        # no PacketSink, and the sink that stopped
    assert st.icmp_sent >= st.ttl_drops + st.unreach_drops > 0  # (icmp on: an error for each, all routed)
    assert st.no_route_drops == 0
    apps = CC.mixed_apps(g)
    assert appc["rx_packets"][apps["echo_client"]] == 30 == appc["tx_packets"][apps["echo_server"]]  # the replies
    kinds = [a["kind"] for a in g.apps]
    onoff = [i for i, k in enumerate(kinds) if k == p2p.APP_ONOFF]
    bursty = onoff[5]
    # the on/off flow was started and stopped many times: fewer datagrams than its rate over the whole interval
    assert 0 < appc["tx_packets"][bursty] < 0.7 * (0.33 * 2_000_000 / (256 * 8))
    stopped_sink = [i for i, a in enumerate(g.apps) if a["kind"] == p2p.APP_SINK and a["stop"] > 0][0]
    feeder = onoff[-1]
    assert 0 < appc["rx_packets"][stopped_sink] < appc["tx_packets"][feeder]  # it stopped under a running flow
    assert len(tr) > 0


def test_no_route_at_a_receive_and_at_a_send():
    for icmp in (False, True):
        sc = CC.no_route(icmp)
        st, _devc, appc, _log, _tr = oracle_full(sc, 0)
        onoff = [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_ONOFF]
        # every datagram of the two cross-component flows is dropped for want of a route: node 0's at node 1's
        # Receive, node 1's at its own Send
        assert appc["tx_packets"][onoff[0]] > 0 and appc["tx_packets"][onoff[1]] > 0
        assert st.no_route_drops == appc["tx_packets"][onoff[0]] + appc["tx_packets"][onoff[1]]
        assert st.cancelled > 0
        sinks = [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_SINK]
        assert appc["rx_packets"][sinks[0]] == 0 and appc["rx_packets"][sinks[1]] > 0


def test_crowded_node_passes_the_slot_table():
    """More than NSLOT = 7 and at most CH = 16 events of the centre node in the span of a narrow window: every pop-log
    entry of the centre is a Receive or a TransmitComplete (no flow ends there)."""
    sc = CC.crowded_node()
    st, _devc, _appc, log, _tr = oracle_full(sc, 200_000)
    n = int(st.dispatched)
    assert n <= 200_000
    ts, ctx = log[0][:n], log[2][:n]
    t = np.sort(ts[ctx == CC.nid(2, 2, 5)].astype(np.int64))
    span = (64 + 30) * 8 * 100  # the smallest frame's transmission time at 10 Mb/s, in ns: a narrow window's span
    most = max(np.searchsorted(t, t + span, side="left") - np.arange(len(t)))
    assert 7 < most <= 16, most


def test_star_with_echo_runs_cold_kinds_at_the_hub():
    sc = CC.star_with_echo()
    st, _devc, appc, _log, _tr = oracle_full(sc, 0)
    kinds = [a["kind"] for a in sc.apps]
    assert appc["rx_packets"][kinds.index(p2p.APP_ECHO_CLIENT)] > 0  # replies came back through the hub
    assert st.unreach_drops > 0 and st.icmp_sent > 0


def test_extended_has_ports_fragments_and_a_lossy_device():
    sc = CC.extended()
    m = p2p_errmodel_pyref.run(sc, ALL_KINDS)
    assert m["frag"]["fragmented"] > 0 and m["frag"]["reassembled"] > 0
    assert m["frag"]["timeouts"] > 0 and m["frag"]["cancelled_timers"] > 0  # K_FRAG_TIMEOUT, fired and cancelled
    assert m["em"]["corrupted"].sum() > 0
    srv = [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_UDP_SERVER][0]
    assert m["servers"]["received"][srv] > 0
    assert m["stats"]["icmp_sent"] > 0  # the flow to the unbound port
