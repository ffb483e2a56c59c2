"""The scenarios of tests/test_gpu_p2p_fused_tc.py really produce the TransmitCompletes they are meant to (the oracle
alone, no GPU): a case that silently exercised nothing would test nothing.

Every transmission shows in the oracle's device trace as a Dequeue (ts, device, size with the PPP header), made by
the event that started it; its TransmitComplete runs on the device's node at Dequeue ts + size x 8 / rate.  From
that and the pop log each TransmitComplete is put into the classes the fused step's conditions distinguish."""
import numpy as np
import pytest

import fused_tc_cases as FC
import p2p
import trace
from test_gpu_trace import oracle_full

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
LOG = 40_000
_cache = {}


def classes(name):
    """Counts of the scenario's TransmitCompletes by class (one TransmitComplete may be in several, or in `alone`):
      alone:   no other event of its node after the event that started the transmission and up to its ts;
      between: another event of the node after that event (in pop order) and before its ts;
      equal:   another event of the node at exactly its ts;
      queued:  a packet queued behind it (it starts the next transmission: a Dequeue of its device at its ts);
      leaf:    a delivered Receive (an Ipv4 Rx with no Tx: its DoForwardUp leaf) on the node at the parent's ts."""
    if name in _cache:
        return _cache[name]
    sc = getattr(FC, name)()
    st, _devc, _appc, log, tr = oracle_full(sc, LOG, kinds=ALL_KINDS)
    n = int(st.dispatched)
    assert 0 < n <= LOG  # (the whole pop log fits)
    ts, uid, ctx = (np.asarray(a[:n]).astype(np.int64) for a in log)
    index_of_uid = {int(u): i for i, u in enumerate(uid)}
    node_of_dev = np.array([d[0] for d in sc.dev])
    by_node = {}
    for i in range(n):
        by_node.setdefault(int(ctx[i]), []).append(i)
    deq = tr[tr["kind"] == trace.TR_DEQUEUE]
    deq_at = {(int(r["dev"]), int(r["ts"])) for r in deq}
    tx_uids = {int(r["uid"]) for r in tr[tr["kind"] == trace.TR_IP_TX]}
    delivered_at = {(int(node_of_dev[r["dev"]]), int(r["ts"])) for r in tr[tr["kind"] == trace.TR_IP_RX]
                    if int(r["uid"]) not in tx_uids}
    out = dict(alone=0, between=0, equal=0, queued=0, leaf=0, total=0)
    for r in deq:
        d, t0 = int(r["dev"]), int(r["ts"])
        # (the device's own arithmetic: Seconds (size * 8 / rate as a double), point-to-point-net-device.cc:236-253)
        t, c = t0 + p2p.seconds_to_ns(int(r["size"]) * 8 / float(sc.dev[d][2])), int(node_of_dev[d])
        if t >= ts[n - 1]:
            continue  # (after Stop: never dispatched)
        ip = index_of_uid[int(r["uid"])]
        mine = [i for i in by_node[c] if i > ip and ts[i] <= t]
        at_t = [i for i in mine if ts[i] == t]
        assert at_t, "no event of the node at the TransmitComplete's ts"
        between = any(ts[i] < t for i in mine)
        equal = len(at_t) > 1
        queued = (d, t) in deq_at
        leaf = (c, t0) in delivered_at
        out["total"] += 1
        out["between"] += between
        out["equal"] += equal
        out["queued"] += queued
        out["leaf"] += leaf
        out["alone"] += not (between or equal or queued or leaf)
    out["drops"] = int((tr["kind"] == trace.TR_DROP).sum())
    out["refits_possible"] = int((ts == 0).sum())
    _cache[name] = out
    return out


def test_alone_has_only_lone_transmit_completes():
    k = classes("alone")
    assert k["total"] > 500
    assert k["alone"] == k["total"]


def test_another_event_between():
    k = classes("another_between")
    assert k["between"] > 20 and k["equal"] == 0 and k["queued"] == 0


def test_equal_ts():
    sc = FC.equal_ts()
    a, b = FC.onoffs(sc)
    assert sc.apps[b]["start"] - sc.apps[a]["start"] == (512 + 30) * 8 * 100 == 433_600
    k = classes("equal_ts")
    assert k["equal"] > 20 and k["queued"] == 0


def test_two_busy_devices():
    """The first record of a pair has the second Receive behind its parent (between), the second record's
    TransmitComplete shares its ts with the first's (equal)."""
    k = classes("two_busy_devices")
    assert k["between"] > 20 and k["equal"] > 20 and k["queued"] == 0


def test_queued_packet_behind_it():
    k = classes("queued_behind")
    assert k["queued"] > 100
    assert k["drops"] > 0  # (the queue filled)
    assert k["alone"] > 0  # (and the flows' other hops still meet the fused step)


def test_leaf_pending():
    k = classes("leaf_pending")
    assert k["leaf"] > 20


@pytest.mark.parametrize("name", ["another_between", "equal_ts", "two_busy_devices", "queued_behind", "leaf_pending",
                                  "start_burst"])
def test_every_case_also_has_lone_ones(name):
    assert classes(name)["alone"] > 0


def test_start_burst_is_larger_than_a_window():
    k = classes("start_burst")
    assert k["refits_possible"] > 4096  # (events at t = 0: more than WCAP)
    assert k["alone"] > 0
