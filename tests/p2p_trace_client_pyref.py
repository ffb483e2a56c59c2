"""UdpTraceClient added to the Python restatement of the p2p subset (tests/p2p_pyref.py and the models above it,
which stay as they are), written from the reference's lines alone:

  entries      udp-trace-client.cc:41-53 (g_defaultEntries), :176-209 (LoadTrace), :211-232 (LoadDefaultTrace)
  application  :234-256 (StartApplication: Schedule (Seconds (0.0), Send)), :258-263 (StopApplication: Cancel),
               :265-309 (SendPacket), :311-335 (Send)

A trace client is a p2p.Scenario application of kind APP_UDP_TRACE_CLIENT: a["size"] is MaxPacketSize, a["entries"]
the (timeToSend ms, packetSize) pairs as a loader left them.  `Model` subclasses p2p_pyref.Model; `MonitoredModel`
puts the same methods over p2p_flowmon_pyref.Model (receive error models and FlowMonitor), whose hooks sit in ip_send,
ip_receive and enqueue and so see every datagram of a burst with its own size.
"""
import numpy as np

import p2p
import p2p_flowmon_pyref
import p2p_pyref

# g_defaultEntries (:41-53): (timeToSend ms as the file would give it, packetSize, frameType)
G_DEFAULT_ENTRIES = ((0, 534, "I"), (40, 1542, "P"), (120, 134, "B"), (80, 390, "B"), (240, 765, "P"),
                     (160, 407, "B"), (200, 504, "B"), (360, 903, "P"), (280, 421, "B"), (320, 587, "B"))
U32 = 0xFFFFFFFF


def load_default_trace():  # :211-232
    entries, prev = [], 0
    for t, size, ft in G_DEFAULT_ENTRIES:
        if ft == "B":
            t = 0
        else:
            t, prev = (t - prev) & U32, t
        entries.append((t, size))
    return entries


def _extract_uint(data, pos, bits):
    """istream >> unsigned: skip whitespace, read digits.  Returns (value or None on failure, pos, hit_eof)."""
    n = len(data)
    while pos < n and data[pos] in " \t\n\r\f\v":
        pos += 1
    if pos >= n:
        return None, pos, True
    start = pos
    if data[pos] in "+-":
        pos += 1
    while pos < n and data[pos].isdigit():
        pos += 1
    if pos == start or not data[start:pos].lstrip("+-"):
        return None, pos, pos >= n
    v = int(data[start:pos])
    if v < 0 or v >= 1 << bits:  # (num_get stores the type's maximum and sets failbit; no golden file goes there)
        return None, pos, pos >= n
    return v, pos, pos >= n


def load_trace(path):
    """LoadTrace (:176-209) over a restatement of ifstream's formatted extraction: `>> index >> frameType >> time >>
    size` inside while (good ()).  An extraction that meets the end of the file sets eofbit; one that finds nothing
    to read sets failbit too, and every later one returns at once — the variables keep their values.  So a file that
    ends in whitespace runs one more round that re-reads nothing and pushes the last entry again (with timeToSend
    time - prevTime = 0 unless it is a B frame, which has 0 anyway); a file that ends in its last digit does not."""
    try:
        with open(path, "r") as f:
            data = f.read()
    except OSError:
        return load_default_trace()  # !ifTraceFile.good () -> LoadDefaultTrace (), and the loop does not run
    entries = []
    pos, eof, fail = 0, False, False
    index = time = size = prev = 0
    ft = "\0"
    while not eof and not fail:  # ifTraceFile.good ()
        for what in ("index", "ft", "time", "size"):
            if eof or fail:  # (the sentry fails: nothing is stored)
                fail = True
                continue
            if what == "ft":  # >> char: skip whitespace, one character
                while pos < len(data) and data[pos] in " \t\n\r\f\v":
                    pos += 1
                if pos >= len(data):
                    eof = fail = True
                else:
                    ft, pos = data[pos], pos + 1
                continue
            v, pos, hit = _extract_uint(data, pos, 16 if what == "size" else 32)
            eof = eof or hit
            if v is None:
                fail = True
            elif what == "index":
                index = v
            elif what == "time":
                time = v
            else:
                size = v
        if ft == "B":
            t = 0
        else:
            t, prev = (time - prev) & U32, time
        entries.append((t, size))
    del index
    return entries


class TraceClientMixin:
    """SendPacket and Send over whatever Model lies below (its ip_send, schedule, cancel)."""

    def _tc_init(self):
        for a, A in enumerate(self.sc.apps):
            if A["kind"] == p2p.APP_UDP_TRACE_CLIENT:
                self.app[a].update(current_entry=0, sends=0)
        self.tc_diag = dict(bursts_over_one=0, zero_remainder=0, header_only=0, wrap_joined=0, noroute_sends=0)

    def tc_send_packet(self, a, size):  # :265-309
        A, S = self.sc.apps[a], self.app[a]
        packet_size = size - 12 if size > 12 else 0  # Create<Packet> (packetSize); AddHeader (seqTs): 12 bytes
        payload = packet_size + 12
        if payload == 12:
            self.tc_diag["header_only"] += 1
        # seqTs.SetSeq (m_sent); m_socket->Send (p) >= 0: ++m_sent
        if self.ip_send(A["node"], (a, 0, payload + 8 + 20, A["ttl"] | (S["sent"] << 8))):
            S["sent"] += 1
            S["c"]["tx_packets"] += 1
            S["c"]["tx_bytes"] += payload
        else:
            self.tc_diag["noroute_sends"] += 1

    def tc_send(self, a):  # :311-335
        A, S = self.sc.apps[a], self.app[a]
        ent, mps = A["entries"], A["size"]
        S["sends"] += 1
        n0 = S["sent"]
        entry = ent[S["current_entry"]]
        while True:  # do { ... } while (entry->timeToSend == 0)
            for _ in range(entry[1] // mps):
                self.tc_send_packet(a, mps)
            sizetosend = entry[1] % mps
            if sizetosend == 0:
                self.tc_diag["zero_remainder"] += 1
            if not (self.nudge == "drop_zero_remainder" and sizetosend == 0):
                self.tc_send_packet(a, sizetosend)
            S["current_entry"] = (S["current_entry"] + 1) % len(ent)
            entry = ent[S["current_entry"]]
            if self.nudge == "no_wrap_join" and S["current_entry"] == 0:
                break  # (the wrong model: a cycle's last burst ends at the wrap)
            if entry[0] != 0:
                break
            if S["current_entry"] == 0:
                self.tc_diag["wrap_joined"] += 1
        if S["sent"] - n0 > 1:
            self.tc_diag["bursts_over_one"] += 1
        # Simulator::Schedule (MilliSeconds (entry->timeToSend), &UdpTraceClient::Send, this)
        S["send_ev"] = self.schedule(entry[0] * 1_000_000, lambda: self.tc_send(a))

    def start_application(self, a):
        if self.sc.apps[a]["kind"] == p2p.APP_UDP_TRACE_CLIENT:  # :234-256: Bind, Connect, null callback, Schedule
            self.app[a]["send_ev"] = self.schedule(0, lambda: self.tc_send(a))
            return
        super().start_application(a)

    def stop_application(self, a):
        if self.sc.apps[a]["kind"] == p2p.APP_UDP_TRACE_CLIENT:  # :258-263: Simulator::Cancel (m_sendEvent)
            self.cancel(self.app[a]["send_ev"])
            return
        super().stop_application(a)


class Model(TraceClientMixin, p2p_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self._tc_init()


class MonitoredModel(TraceClientMixin, p2p_flowmon_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self._tc_init()


def results(m):
    """p2p_pyref.run's dict from a model that has run, plus clients (p2p.UDP_TRACE_CLIENT_DTYPE) and tc_diag."""
    sc = m.sc
    devc = np.zeros(len(sc.dev), p2p.DEV_COUNTERS_DTYPE)
    for d, D in enumerate(m.dev):
        for f, v in D["c"].items():
            devc[d][f] = v & 0xFFFFFFFF
    appc = np.zeros(len(sc.apps), p2p.APP_COUNTERS_DTYPE)
    servers = np.zeros(len(sc.apps), p2p.UDP_SERVER_DTYPE)
    clients = np.zeros(len(sc.apps), p2p.UDP_TRACE_CLIENT_DTYPE)
    for a, S in enumerate(m.app):
        for f, v in S["c"].items():
            appc[a][f] = v
        if S["loss"] is not None:
            servers[a] = (S["received"], S["loss"].m_lost, S["loss"].m_lastMaxSeqNum, 0)
        if sc.apps[a]["kind"] == p2p.APP_UDP_TRACE_CLIENT:
            clients[a] = (S["sent"], S["current_entry"], S["sends"], 0)
    log = (np.array([e[0] for e in m.log], np.uint64), np.array([e[1] for e in m.log], np.uint32),
           np.array([e[2] for e in m.log], np.uint32))
    stats = dict(dispatched=m.dispatched, cancelled=m.cancelled, digest=m.digest, final_ts=m.now,
                 next_uid=m.m_uid, ttl_drops=m.ttl_drops, no_route_drops=m.no_route_drops,
                 unreach_drops=m.unreach_drops, icmp_sent=m.icmp_sent)
    return dict(stats=stats, devc=devc, appc=appc, servers=servers, clients=clients, log=log,
                trace=np.array(m.trace, dtype=p2p.TRACE_RECORD_DTYPE), diag=m.diag, tc_diag=m.tc_diag, model=m)


def run(sc, trace_kinds=0x7F, nudge=None):
    m = Model(sc, trace_kinds, nudge)
    m.setup()
    m.run()
    return results(m)


def run_monitored(sc, trace_kinds=0x7F, max_delays=(p2p_flowmon_pyref.MAX_PER_HOP_DELAY_NS,)):
    """The same with receive error models and FlowMonitor: em = the error models' records, flows = {max_delay: the
    flow records}, fm_diag."""
    m = MonitoredModel(sc, trace_kinds)
    m.setup()
    m.run()
    r = results(m)
    em = np.zeros(len(sc.dev), p2p.ERROR_MODEL_DTYPE)
    for d, (inv, cor) in m.em_count.items():
        em[d] = (inv & 0xFFFFFFFF, cor & 0xFFFFFFFF)
    r.update(em=em, dropped=m.em_dropped, flows={d: m.flow_records(d) for d in max_delays}, fm_diag=dict(m.fm_diag))
    return r
