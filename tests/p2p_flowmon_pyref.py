"""FlowMonitor added to the Python restatement of the p2p subset (tests/p2p_errmodel_pyref.py and the models under
it, which stay as they are): Model hooks the monitor's probe into ip_send, ip_receive and enqueue, written from the
reference's lines alone.  The hooks only observe: every one runs before the base method it wraps and schedules
nothing, so the base model's events, counters and trace records are untouched (tests/test_flowmon_cpu.py asserts it).

  FlowMonitor   flow-monitor.cc:121-146 (ReportFirstTx), :149-170 (ReportForwarding), :173-234 (ReportLastRx),
                :236-267 (ReportDrop: counted whether or not the packet is tracked), :276-300 (CheckForLostPackets)
  probe         ipv4-flow-probe.cc:192-210 (SendOutgoingLogger: the tag (flowId, packetId, size)), :212-225
                (ForwardLogger), :227-245 (ForwardUpLogger), :247-322 (DropLogger: the reasons), :324-346
                (QueueDropLogger: by the tag, so an untagged packet — an ICMP message — reports nothing)
  classifier    ipv4-flow-classifier.cc:102-155 (UDP and TCP only; a new five-tuple takes the next FlowId; packetId =
                the header's identification)
  trace sources ipv4-l3-protocol.cc:618 (SendOutgoing: after BuildHeader, before SendRealOut; a socket-level no-route
                send never gets there), :838 (UnicastForward: after the TTL check), :861 (LocalDeliver: before the
                protocol's Receive, so before the UDP endpoint lookup), :505 / :835 (Drop: NO_ROUTE at a forwarder,
                TTL_EXPIRED with or without an ICMP error); the devices' TxQueue/Drop (ipv4-flow-probe.cc:181-185)

Not modelled, as in the engine: the monitor's own events (StartRightNow, the check every simulated second: they take
uids and the periodic check only moves losses earlier), histograms, per-probe statistics, Start / Stop times, the
identification's wrap.  check_for_lost does not erase, so it can be asked for several delays.
"""
import numpy as np

import p2p
import p2p_errmodel_pyref
from p2p_pyref import PKT_APP, PKT_ICMP, PKT_REPLY

DROP_NO_ROUTE, DROP_TTL_EXPIRE, DROP_BAD_CHECKSUM, DROP_QUEUE = 0, 1, 2, 3  # Ipv4FlowProbe::DropReason
MAX_PER_HOP_DELAY_NS = 10 * 10**9  # flow-monitor.cc:46-49


class FlowStats:
    """FlowMonitor::FlowStats (flow-monitor.h) without the histograms; times in ns."""

    def __init__(self):
        self.timeFirstTxPacket = self.timeFirstRxPacket = self.timeLastTxPacket = self.timeLastRxPacket = 0
        self.delaySum = self.jitterSum = self.lastDelay = 0
        self.txBytes = self.rxBytes = self.txPackets = self.rxPackets = self.lostPackets = self.timesForwarded = 0
        self.packetsDropped, self.bytesDropped = [], []


class FlowMonitor:
    def __init__(self, now):
        self.now = now  # Simulator::Now
        self.m_flowStats = {}
        self.m_trackedPackets = {}  # (flowId, packetId) -> [firstSeenTime, lastSeenTime, timesForwarded]

    def stats(self, flow_id):  # GetStatsForFlow
        return self.m_flowStats.setdefault(flow_id, FlowStats())

    def report_first_tx(self, flow_id, packet_id, size):  # :121-146
        now = self.now()
        self.m_trackedPackets[(flow_id, packet_id)] = [now, now, 0]
        s = self.stats(flow_id)
        s.txBytes += size
        s.txPackets += 1
        if s.txPackets == 1:
            s.timeFirstTxPacket = now
        s.timeLastTxPacket = now

    def report_forwarding(self, flow_id, packet_id, size):  # :149-170
        t = self.m_trackedPackets.get((flow_id, packet_id))
        if t is None:
            return
        t[2] += 1
        t[1] = self.now()

    def report_last_rx(self, flow_id, packet_id, size):  # :173-234
        t = self.m_trackedPackets.get((flow_id, packet_id))
        if t is None:
            return
        now = self.now()
        delay = now - t[0]
        s = self.stats(flow_id)
        s.delaySum += delay
        if s.rxPackets > 0:
            jitter = s.lastDelay - delay
            if jitter > 0:
                s.jitterSum += jitter
            else:
                s.jitterSum -= jitter
        s.lastDelay = delay
        s.rxBytes += size
        s.rxPackets += 1
        if s.rxPackets == 1:
            s.timeFirstRxPacket = now
        s.timeLastRxPacket = now
        s.timesForwarded += t[2]
        del self.m_trackedPackets[(flow_id, packet_id)]

    def report_drop(self, flow_id, packet_id, size, reason):  # :236-267
        s = self.stats(flow_id)
        s.lostPackets += 1
        if len(s.packetsDropped) < reason + 1:
            s.packetsDropped += [0] * (reason + 1 - len(s.packetsDropped))
            s.bytesDropped += [0] * (reason + 1 - len(s.bytesDropped))
        s.packetsDropped[reason] += 1
        s.bytesDropped[reason] += size
        self.m_trackedPackets.pop((flow_id, packet_id), None)

    def check_for_lost(self, max_delay):  # :276-300, without the erase: {flowId: packets it would count}
        now, lost = self.now(), {}
        for (flow_id, _pid), t in self.m_trackedPackets.items():
            if now - t[1] >= max_delay:
                lost[flow_id] = lost.get(flow_id, 0) + 1
        return lost


class Model(p2p_errmodel_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        assert not sc.frag, "the reference classifies a non-first fragment by its payload bytes: not modelled"
        self.fm = FlowMonitor(lambda: self.now)
        self.m_flowMap = {}     # Ipv4FlowClassifier::m_flowMap: five-tuple -> FlowId (from 1, in first-seen order)
        self.flow_first = {}    # FlowId -> (flow index, ts, uid of the event that classified it first)
        self.tags = {}          # Ipv4FlowProbeTag of a datagram in flight: (app word, ipid) -> (flowId, packetId, size)
        self.fm_diag = dict(queue_drop_at_sender=0, queue_drop_at_forwarder=0, ttl_drop_icmp=0, ttl_drop_no_icmp=0,
                            no_route_drop=0, unreachable_received=0)

    # ---------------- Ipv4FlowClassifier ----------------
    def classify(self, p):
        """(flowId, packetId) of descriptor p, or None (:102-155: neither UDP nor TCP).  One sending application is
        one five-tuple (its socket's ephemeral port); the echo replies to a client are the reverse tuple."""
        if p[0] & PKT_ICMP:
            return None
        a = p[0] & PKT_APP
        A = self.sc.apps[a]
        reply = bool(p[0] & PKT_REPLY)
        src, dst = (A["dst"], A["node"]) if reply else (A["node"], A["dst"])
        tup = (src, dst, 17, ("server" if reply else "client", a), ("client" if reply else "server", a))
        if tup not in self.m_flowMap:
            self.m_flowMap[tup] = len(self.m_flowMap) + 1
            self.flow_first[self.m_flowMap[tup]] = ((len(self.sc.apps) + a) if reply else a, self.now, self.cur_uid)
        return self.m_flowMap[tup], p[1] & 0xFFFF

    # ---------------- Ipv4FlowProbe ----------------
    def send_outgoing_logger(self, p):  # :192-210
        c = self.classify(p)
        if c is not None:
            self.fm.report_first_tx(c[0], c[1], p[2])
            self.tags[(p[0], p[1])] = (c[0], c[1], p[2])

    def forward_logger(self, p):  # :212-225
        c = self.classify(p)
        if c is not None:
            self.fm.report_forwarding(c[0], c[1], p[2])

    def forward_up_logger(self, p):  # :227-245
        c = self.classify(p)
        if c is not None:
            self.tags.pop((p[0], p[1]), None)
            self.fm.report_last_rx(c[0], c[1], p[2])

    def drop_logger(self, p, reason):  # :247-322
        c = self.classify(p)
        if c is not None:
            self.tags.pop((p[0], p[1]), None)
            self.fm.report_drop(c[0], c[1], p[2], reason)

    def queue_drop_logger(self, p):  # :324-346
        tag = self.tags.pop((p[0], p[1]), None)
        if tag is None:
            return False
        self.fm.report_drop(tag[0], tag[1], tag[2], DROP_QUEUE)
        return True

    # ---------------- the hook points ----------------
    def ip_send(self, n, p):  # m_sendOutgoingTrace (:618): the header BuildHeader is about to make, if a route exists
        if self.route(n, p) != p2p.NO_ROUTE:
            self.send_outgoing_logger((p[0], self.node_ipid[n], p[2], p[3]))
        return super().ip_send(n, p)

    def ip_receive(self, n, p, rx_dev):
        if self.pkt_dst_node(p) == n:  # LocalDeliver: m_localDeliverTrace (:861)
            if not p[0] & PKT_ICMP and self.lookup(n, p) is None:
                self.fm_diag["unreachable_received"] += 1
            self.forward_up_logger(p)
        elif self.route(n, p) == p2p.NO_ROUTE:  # m_dropTrace (.., DROP_NO_ROUTE, ..) (:505)
            if not p[0] & PKT_ICMP:
                self.fm_diag["no_route_drop"] += 1
            self.drop_logger(p, DROP_NO_ROUTE)
        elif (p[3] - 1) & 0xFF == 0:  # IpForward: m_dropTrace (.., DROP_TTL_EXPIRED, ..) (:835)
            if not p[0] & PKT_ICMP:
                self.fm_diag["ttl_drop_icmp" if self.sc.icmp else "ttl_drop_no_icmp"] += 1
            self.drop_logger(p, DROP_TTL_EXPIRE)
        else:  # m_unicastForwardTrace (:838)
            self.forward_logger(p)
        return super().ip_receive(n, p, rx_dev)

    def enqueue(self, d, p):  # Queue::Drop -> m_traceDrop -> QueueDropLogger
        ok = super().enqueue(d, p)
        if not ok and self.queue_drop_logger(p):
            a = self.sc.apps[p[0] & PKT_APP]
            origin = a["dst"] if p[0] & PKT_REPLY else a["node"]
            self.fm_diag["queue_drop_at_sender" if self.sc.dev[d][0] == origin else "queue_drop_at_forwarder"] += 1
        return ok

    # ---------------- results ----------------
    def flow_records(self, max_delay=MAX_PER_HOP_DELAY_NS):
        """What Engine.flow_stats returns (p2p.FLOW_STATS_DTYPE), after CheckForLostPackets (max_delay)."""
        lost = self.fm.check_for_lost(max_delay)
        out = np.zeros(len(self.m_flowMap), p2p.FLOW_STATS_DTYPE)
        for i, flow_id in enumerate(sorted(self.m_flowMap.values())):
            s = self.fm.stats(flow_id)
            flow, ts, uid = self.flow_first[flow_id]
            r = out[i]
            r["flow_id"], r["flow"], r["first_tx_ts"], r["first_tx_uid"] = flow_id, flow, ts, uid
            r["tx_packets"], r["tx_bytes"], r["rx_packets"], r["rx_bytes"] = s.txPackets, s.txBytes, s.rxPackets, s.rxBytes
            r["delay_sum_ns"], r["jitter_sum_ns"], r["last_delay_ns"] = s.delaySum, s.jitterSum, s.lastDelay
            r["time_first_tx_ns"], r["time_last_tx_ns"] = s.timeFirstTxPacket, s.timeLastTxPacket
            r["time_first_rx_ns"], r["time_last_rx_ns"] = s.timeFirstRxPacket, s.timeLastRxPacket
            r["times_forwarded"] = s.timesForwarded
            r["lost_packets"] = s.lostPackets + lost.get(flow_id, 0)
            for k, v in enumerate(s.packetsDropped):
                r["packets_dropped"][k] = v
            for k, v in enumerate(s.bytesDropped):
                r["bytes_dropped"][k] = v
        return out


def run(sc, trace_kinds=0x7F, max_delays=(MAX_PER_HOP_DELAY_NS,)):
    """p2p_errmodel_pyref.run's dict for scenario `sc` (the same keys, from the monitored model), and flows =
    {max_delay: the flow records}, fm_diag = what the vacuity checks read, model = the Model itself."""
    m = Model(sc, trace_kinds)
    m.setup()
    m.run()
    devc = np.zeros(len(sc.dev), p2p.DEV_COUNTERS_DTYPE)
    for d, D in enumerate(m.dev):
        for f, v in D["c"].items():
            devc[d][f] = v & 0xFFFFFFFF
    appc = np.zeros(len(sc.apps), p2p.APP_COUNTERS_DTYPE)
    servers = np.zeros(len(sc.apps), p2p.UDP_SERVER_DTYPE)
    for a, S in enumerate(m.app):
        for f, v in S["c"].items():
            appc[a][f] = v
        if S["loss"] is not None:
            servers[a] = (S["received"], S["loss"].m_lost, S["loss"].m_lastMaxSeqNum, 0)
    log = (np.array([e[0] for e in m.log], np.uint64), np.array([e[1] for e in m.log], np.uint32),
           np.array([e[2] for e in m.log], np.uint32))
    stats = dict(dispatched=m.dispatched, cancelled=m.cancelled, digest=m.digest, final_ts=m.now,
                 next_uid=m.m_uid, ttl_drops=m.ttl_drops, no_route_drops=m.no_route_drops,
                 unreach_drops=m.unreach_drops, icmp_sent=m.icmp_sent)
    frag = dict(m.fs)
    frag["cancelled_timers"] = 0
    em = np.zeros(len(sc.dev), p2p.ERROR_MODEL_DTYPE)
    for d, (inv, cor) in m.em_count.items():
        em[d] = (inv & 0xFFFFFFFF, cor & 0xFFFFFFFF)
    # the tracked packets an error model's corrupt frame carried: lost by timeout only
    eaten = {(p[0], p[1]) for _d, p in m.em_dropped if not p[0] & PKT_ICMP}
    fm_diag = dict(m.fm_diag)
    fm_diag["tracked_eaten_by_error_model"] = sum(1 for k in eaten if k in m.tags)
    return dict(stats=stats, devc=devc, appc=appc, servers=servers, log=log, frag=frag, em=em, dropped=m.em_dropped,
                trace=np.array(m.trace, dtype=p2p.TRACE_RECORD_DTYPE), diag=m.diag,
                flows={d: m.flow_records(d) for d in max_delays}, fm_diag=fm_diag, model=m)
