"""A second restatement of the point-to-point subset, in Python, written from the reference's lines alone (as
tests/wifi_pyref.py is for the Wi-Fi subset).  oracle/nsref_p2p.cc knows neither UDP ports nor UdpClient /
UdpServer; this model does, and where the oracle applies the two must agree event for event
(tests/test_udp_ports_cpu.py), which is what lets the GPU tests of the new ground lean on this one.

It runs a p2p.Scenario (the Python object, not its C struct) for small scenarios only.

  simulator   default-simulator-impl.cc:52-56 (m_uid 4), :117-131 (ProcessOneEvent), :153-165 (Run), :188-233
              (Schedule / ScheduleWithContext / ScheduleNow: key (ts, uid), the context), :292-332 (Cancel /
              IsExpired: a cancelled event is still dispatched)
  setup       node-list.cc:80-90,124-131, node.cc:111-145,183-199, application.cc:87-95, channel-list.cc:80-90
  device      point-to-point-net-device.cc:206-269,304-346,462-518; point-to-point-channel.cc:82-103;
              data-rate.cc:224-227; queue.cc:61-200, drop-tail-queue.cc:83-132
  IPv4        ipv4-l3-protocol.cc:434-537 (Receive), :815-841 (IpForward), Send / BuildHeader (m_identification++),
              :505,:764,:835 (the Drop / Tx / Rx trace sources)
  ICMP        icmpv4-l4-protocol.cc:85-160, icmpv4.cc:306-440
  UDP         udp-l4-protocol.cc:312-407 -> ipv4-end-point-demux.cc:195-307 (Lookup by port) ->
              ipv4-end-point.cc:112-120 (ForwardUp: ScheduleNow DoForwardUp) -> udp-socket-impl.cc:864-905
  OnOff       onoff-application.cc:132-252 (constant on / off times)     PacketSink   packet-sink.cc
  echo pair   udp-echo-client.cc, udp-echo-server.cc
  UdpClient   udp-client.cc:116-187        UdpServer  udp-server.cc:109-190, packet-loss-counter.cc:32-120

Time conversions go through nsref.seconds, as the other models do.

One deviation from the reference is kept on purpose.  The oracle and the engine treat a stopped PacketSink /
UdpEchoServer / UdpEchoClient as unbound: later datagrams are RX_ENDPOINT_UNREACH.  In the reference
UdpSocketImpl::Close only sets the shutdown flags (udp-socket-impl.cc:294-305) and the endpoint lives on, so such a
datagram still costs a DoForwardUp event and no ICMP error.  This model follows the oracle for those three kinds
(`stop_application`, marked there) and the reference for UdpClient / UdpServer; DESIGN.md §6 names the gap.
"""
import heapq

import numpy as np

import nsref
import p2p

M64 = (1 << 64) - 1
PKT_REPLY, PKT_ICMP, PKT_ICMP_UNREACH, PKT_ICMP_OF_REPLY, PKT_APP = (0x80000000, 0x40000000, 0x20000000,
                                                                    0x10000000, 0x0FFFFFFF)
TR_ENQUEUE, TR_DEQUEUE, TR_DROP, TR_RX, TR_IP_TX, TR_IP_RX, TR_IP_DROP = range(7)
NOCTX = 0xFFFFFFFF


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest_term(rank, ts, uid):
    """nsgpu_dispatch_digest_term (include/nsgpu_types.h)."""
    return _mix64(((rank * 0x9E3779B97F4A7C15) & M64) ^ _mix64((ts ^ ((uid << 40) & M64) ^ uid) & M64))


class PacketLossCounter:
    """packet-loss-counter.cc:32-120, literally (the loop runs the gap's length)."""

    def __init__(self, window):
        assert window % 8 == 0  # SetBitMapSize's NS_ASSERT_MSG
        self.m_bitMapSize = window // 8
        self.m_receiveBitMap = [0xFF] * self.m_bitMapSize
        self.m_lost = 0
        self.m_lastMaxSeqNum = 0
        self.wide_gaps = 0  # (diagnostic: NotifyReceived calls whose gap exceeded the window)

    def get_bit(self, seq):
        return (self.m_receiveBitMap[(seq % (self.m_bitMapSize * 8)) // 8] >> (7 - (seq % 8))) & 0x01

    def set_bit(self, seq, val):
        if val:
            self.m_receiveBitMap[(seq % (self.m_bitMapSize * 8)) // 8] |= 0x80 >> (seq % 8)
        else:
            self.m_receiveBitMap[(seq % (self.m_bitMapSize * 8)) // 8] &= ~(0x80 >> (seq % 8)) & 0xFF

    def notify_received(self, seq):
        if seq > self.m_lastMaxSeqNum and seq - self.m_lastMaxSeqNum > self.m_bitMapSize * 8:
            self.wide_gaps += 1
        for i in range(self.m_lastMaxSeqNum + 1, seq + 1):
            if self.get_bit(i) != 1:
                self.m_lost += 1
            self.set_bit(i, 0)
        self.set_bit(seq, 1)
        if seq > self.m_lastMaxSeqNum:
            self.m_lastMaxSeqNum = seq


class _Event:
    __slots__ = ("fn", "cancelled", "ts", "uid")

    def __init__(self, fn, ts, uid):
        self.fn, self.cancelled, self.ts, self.uid = fn, False, ts, uid


class Model:
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        self.sc = sc
        self.nudge = nudge  # a deliberately wrong line (the positive control of the model-against-oracle test)
        self.trace_kinds = trace_kinds
        # ---- DefaultSimulatorImpl ----
        self.heap = []
        self.m_uid = sc.uid_first or 4
        self.now, self.cur_uid, self.cur_ctx = 0, 0, NOCTX
        self.m_stop = False
        self.dispatched = self.cancelled = self.digest = 0
        self.log = []
        # ---- model state ----
        A, D = sc.apps, sc.dev
        self.dev = [dict(busy=False, q=[], c=dict.fromkeys(p2p.DEV_COUNTERS_DTYPE.names, 0)) for _ in D]
        self.app = [dict(started=False, bound=False, receiving=False, send_ev=None, ss_ev=None, last_start=0,
                         residual=0, tot=0, sent=0, c=dict.fromkeys(p2p.APP_COUNTERS_DTYPE.names, 0),
                         received=0, loss=PacketLossCounter(a["window"]) if a["kind"] == p2p.APP_UDP_SERVER else None)
                    for a in A]
        self.node_apps = [[] for _ in range(sc.n_nodes)]
        for i, a in enumerate(A):
            self.node_apps[a["node"]].append(i)
        self.node_ipid = [0] * sc.n_nodes
        self.ttl_drops = self.no_route_drops = self.unreach_drops = self.icmp_sent = 0
        self.trace = []
        self.tr_seq, self.tr_key = 0, None
        self.diag = dict(reordered=0, after_stop=0, noroute_attempts_at_zero=0)

    # ---------------- simulator ----------------
    def _insert(self, ts, ctx, fn):
        ev = _Event(fn, ts, self.m_uid)
        heapq.heappush(self.heap, (ts, self.m_uid, ctx, ev))
        self.m_uid += 1
        return ev

    def schedule(self, delay, fn):
        assert delay >= 0
        return self._insert(self.now + delay, self.cur_ctx, fn)

    def schedule_ctx(self, ctx, delay, fn):
        self._insert(self.now + delay, ctx, fn)

    def is_expired(self, ev):  # :304-332
        return (ev is None or ev.ts < self.now or (ev.ts == self.now and ev.uid <= self.cur_uid) or ev.cancelled)

    def cancel(self, ev):  # :292-302
        if not self.is_expired(ev):
            ev.cancelled = True

    def run(self):
        while self.heap and not self.m_stop:
            ts, uid, ctx, ev = heapq.heappop(self.heap)
            self.now, self.cur_uid, self.cur_ctx = ts, uid, ctx
            self.log.append((ts, uid, ctx))
            self.digest = (self.digest + digest_term(self.dispatched, ts, uid)) & M64
            if ev.cancelled:
                self.cancelled += 1
            self.dispatched += 1
            if not ev.cancelled:
                ev.fn()

    # ---------------- trace sinks ----------------
    def tr(self, kind, d, p):
        if not (self.trace_kinds >> kind) & 1:
            return
        if self.tr_key != (self.now, self.cur_uid):
            self.tr_key, self.tr_seq = (self.now, self.cur_uid), 0
        self.trace.append((self.now, self.cur_uid, self.tr_seq, kind, 0, d, p[0], p[1], p[2], p[3], 0))
        self.tr_seq += 1

    # ---------------- addressing (a packet is (app, ipid, size, ttl), as the device's descriptor) ----------------
    def dst_slot_of(self, a):
        return self.sc.dst_slot.get(self.sc.apps[a]["dst"], 0)

    def src_slot_of(self, a):
        return self.sc.dst_slot.get(self.sc.apps[a]["node"], p2p.NO_ROUTE)

    def pkt_dst_node(self, p):
        A = self.sc.apps
        if p[0] & PKT_ICMP:  # SendMessage (p, header.GetSource (), ...): back to the offending datagram's sender
            fa = p[0] & PKT_APP
            return A[fa]["dst"] if p[0] & PKT_ICMP_OF_REPLY else A[fa]["node"]
        return A[p[0] & ~PKT_REPLY]["node"] if p[0] & PKT_REPLY else A[p[0]]["dst"]

    def pkt_dst_slot(self, p):
        if p[0] & PKT_ICMP:
            fa = p[0] & PKT_APP
            return self.dst_slot_of(fa) if p[0] & PKT_ICMP_OF_REPLY else self.src_slot_of(fa)
        return self.src_slot_of(p[0] & ~PKT_REPLY) if p[0] & PKT_REPLY else self.dst_slot_of(p[0])

    def route(self, n, p):
        k = self.pkt_dst_slot(p)
        return p2p.NO_ROUTE if k == p2p.NO_ROUTE else self.sc.next_hop(n, k)

    # ---------------- Queue / DropTailQueue ----------------
    def enqueue(self, d, p):
        D = self.dev[d]
        if len(D["q"]) >= self.sc.dev[d][5]:  # DoEnqueue: Drop (p)
            self.tr(TR_DROP, d, p)
            D["c"]["drop_packets"] += 1
            D["c"]["drop_bytes"] += p[2]
            return False
        D["q"].append(p)
        self.tr(TR_ENQUEUE, d, p)
        D["c"]["enq_packets"] += 1
        D["c"]["enq_bytes"] += p[2]
        return True

    def dequeue(self, d):
        D = self.dev[d]
        if not D["q"]:
            return None
        p = D["q"].pop(0)
        self.tr(TR_DEQUEUE, d, p)
        D["c"]["deq_packets"] += 1
        return p

    # ---------------- PointToPointNetDevice / PointToPointChannel ----------------
    def transmit_start(self, d, p):  # :206-234
        D, (_node, peer, bps, ifg, delay, _q) = self.dev[d], self.sc.dev[d]
        D["busy"] = True
        D["c"]["tx_packets"] += 1
        tx_time = nsref.seconds(float(p[2]) * 8 / float(bps))  # Seconds (m_bps.CalculateTxTime (p->GetSize ()))
        self.schedule(tx_time + ifg, lambda: self.transmit_complete(d))
        # PointToPointChannel::TransmitStart: ScheduleWithContext (the peer's node, txTime + m_delay, Receive)
        self.schedule_ctx(self.sc.dev[peer][0], tx_time + delay, lambda: self.receive(peer, p))

    def transmit_complete(self, d):  # :236-269
        self.dev[d]["busy"] = False
        p = self.dequeue(d)
        if p is not None:
            self.transmit_start(d, p)

    def device_send(self, d, p):  # :462-518
        p = (p[0], p[1], p[2] + 2, p[3])  # AddHeader (PppHeader)
        if not self.dev[d]["busy"]:
            if self.enqueue(d, p):
                self.transmit_start(d, self.dequeue(d))
        else:
            self.enqueue(d, p)

    def receive(self, d, p):  # :304-346
        self.dev[d]["c"]["rx_packets"] += 1
        p = (p[0], p[1], p[2] - 2, p[3])
        self.tr(TR_RX, d, p)     # m_macRxTrace
        self.tr(TR_IP_RX, d, p)  # Ipv4L3Protocol::Receive: m_rxTrace
        self.ip_receive(self.sc.dev[d][0], p, d)

    # ---------------- IPv4 ----------------
    def ip_out(self, out, p):  # SendRealOut: m_txTrace, then the interface's device
        self.tr(TR_IP_TX, out, p)
        self.device_send(out, p)

    def ip_drop(self, d, p):  # m_dropTrace: the header as received (a UDP datagram's 16-bit identification)
        if not p[0] & PKT_ICMP:
            p = (p[0], p[1] & 0xFFFF, p[2], p[3])
        self.tr(TR_IP_DROP, d, p)

    def icmp_send(self, n, p, unreach):  # Icmpv4L4Protocol::SendMessage; the descriptor's packing: nsgpu_types.h
        of = PKT_ICMP_OF_REPLY if p[0] & PKT_REPLY else 0
        e = (PKT_ICMP | (PKT_ICMP_UNREACH if unreach else 0) | of | (p[0] & PKT_APP), (p[1] & 0xFFFF) << 16, 56,
             64 | ((p[3] & 0xFF) << 8) | (p[2] << 16))
        out = self.route(n, e)
        if out == p2p.NO_ROUTE:  # "drop icmp message"
            self.no_route_drops += 1
            return False
        e = (e[0], e[1] | (self.node_ipid[n] & 0xFFFF), e[2], e[3])
        self.node_ipid[n] += 1
        self.icmp_sent += 1
        self.ip_out(out, e)
        return True

    def lookup(self, n, p):
        """UdpL4Protocol::Receive -> Ipv4EndPointDemux::Lookup: the bound endpoint of node n for datagram p (None:
        RX_ENDPOINT_UNREACH).  An echo reply finds its client's connected socket."""
        A = self.sc.apps
        if p[0] & PKT_REPLY:
            k = p[0] & ~PKT_REPLY
            return k if self.app[k]["bound"] else None
        found = None
        for k in self.node_apps[n]:
            if A[k]["kind"] not in p2p.BOUND:
                continue
            if self.sc.ports:
                if A[k]["port"] == A[p[0]]["remote_port"] and self.app[k]["bound"]:
                    return k
            else:  # no ports: the node's (last) endpoint takes every datagram addressed to the node
                found = k
        return found if found is not None and self.app[found]["bound"] else None

    def ip_receive(self, n, p, rx_dev):  # Ipv4L3Protocol::Receive -> RouteInput
        if self.pkt_dst_node(p) == n:  # LocalDeliver
            if p[0] & PKT_ICMP:  # Icmpv4L4Protocol::Receive -> the endpoint's (null) ICMP callback
                return
            k = self.lookup(n, p)
            if k is None:
                self.unreach_drops += 1
                if self.sc.icmp:
                    self.icmp_send(n, p, True)  # SendDestUnreachPort
                return
            self.schedule(0, lambda: self.do_forward_up(k, p, n))  # Ipv4EndPoint::ForwardUp: ScheduleNow
            return
        out = self.route(n, p)
        if out == p2p.NO_ROUTE:  # DROP_NO_ROUTE
            self.no_route_drops += 1
            self.ip_drop(rx_dev, p)
            return
        received = p
        p = (p[0], p[1], p[2], p[3] - 1)  # IpForward: SetTtl (ttl - 1)
        if p[3] & 0xFF == 0:
            self.ttl_drops += 1
            sent = False
            if self.sc.icmp and not p[0] & PKT_ICMP:
                sent = self.icmp_send(n, p, False)  # SendTimeExceededTtl
            # (the Drop record after an error is rebuilt from the error's descriptor: the TTL byte alone)
            self.ip_drop(out, (received[0], received[1], received[2], 1) if sent else received)
            return
        self.ip_out(out, p)

    def ip_send(self, n, p):  # UdpSocketImpl::DoSendTo (RouteOutput) -> Ipv4L3Protocol::Send; False: no route (-1)
        out = self.route(n, p)
        if out == p2p.NO_ROUTE:
            self.no_route_drops += 1
            return False
        p = (p[0], self.node_ipid[n], p[2], p[3])  # BuildHeader: SetIdentification (m_identification++)
        self.node_ipid[n] += 1
        self.ip_out(out, p)
        return True

    # ---------------- sockets' receive callbacks ----------------
    def do_forward_up(self, k, p, n):  # Ipv4EndPoint::DoForwardUp -> UdpSocketImpl::ForwardUp -> HandleRead
        A, S = self.sc.apps[k], self.app[k]
        if A["kind"] == p2p.APP_UDP_SERVER:
            if not S["receiving"]:  # StopApplication cleared the callback; the socket stays bound
                self.diag["after_stop"] += 1
                return
            seq = p[3] >> 8  # SeqTsHeader::GetSeq (0 from a payload of zeros)
            if seq < S["loss"].m_lastMaxSeqNum:
                self.diag["reordered"] += 1
            S["loss"].notify_received(seq)
            S["received"] += 1
            S["c"]["rx_packets"] += 1
            S["c"]["rx_bytes"] += p[2] - 28
            return
        if not S["bound"]:  # (the oracle's rule for the three old kinds: see the module docstring)
            return
        S["c"]["rx_packets"] += 1
        S["c"]["rx_bytes"] += p[2] - 28
        if A["kind"] == p2p.APP_ECHO_SERVER:  # socket->SendTo (packet, 0, from)
            S["c"]["tx_packets"] += 1
            S["c"]["tx_bytes"] += p[2] - 28
            self.ip_send(n, (p[0] | PKT_REPLY, 0, p[2], A["ttl"]))

    # ---------------- OnOffApplication ----------------
    def cancel_events(self, a):  # :168-181
        S = self.app[a]
        if not self.is_expired(S["send_ev"]):  # m_sendEvent.IsRunning ()
            delta = nsref.I64x64.from_int(self.now - S["last_start"])
            t = delta.mul_by_invert(nsref.I64x64.invert(1000000000))  # delta.To (Time::S)
            bits = t * nsref.I64x64.from_parts(self.sc.apps[a]["rate"], 0)
            S["residual"] = (S["residual"] + bits.high()) & 0xFFFFFFFF
        self.cancel(S["send_ev"])
        self.cancel(S["ss_ev"])

    def schedule_next_tx(self, a):  # :201-219
        A, S = self.sc.apps[a], self.app[a]
        if A["maxb"] == 0 or S["tot"] < A["maxb"]:
            bits = (A["size"] * 8 - S["residual"]) & 0xFFFFFFFF
            S["send_ev"] = self.schedule(nsref.seconds(bits / float(A["rate"])), lambda: self.send_packet(a))
        else:
            self.stop_application(a)

    def start_sending(self, a):  # :184-190
        self.app[a]["last_start"] = self.now
        self.schedule_next_tx(a)
        self.app[a]["ss_ev"] = self.schedule(nsref.seconds(self.sc.apps[a]["on"]), lambda: self.stop_sending(a))

    def stop_sending(self, a):  # :192-198
        self.cancel_events(a)
        self.app[a]["ss_ev"] = self.schedule(nsref.seconds(self.sc.apps[a]["off"]), lambda: self.start_sending(a))

    def send_packet(self, a):  # :240-252
        A, S = self.sc.apps[a], self.app[a]
        S["c"]["tx_packets"] += 1  # (m_txTrace)
        S["c"]["tx_bytes"] += A["size"]
        self.ip_send(A["node"], (a, 0, A["size"] + 8 + 20, A["ttl"]))
        S["tot"] = (S["tot"] + A["size"]) & 0xFFFFFFFF
        S["last_start"] = self.now
        S["residual"] = 0
        self.schedule_next_tx(a)

    # ---------------- UdpEchoClient / UdpClient ----------------
    def echo_send(self, a):  # UdpEchoClient::Send
        A, S = self.sc.apps[a], self.app[a]
        if self.nudge == "send_before_children" and S["sent"] + 1 < A["count"]:  # (the positive control)
            S["send_ev"] = self.schedule(A["interval"], lambda: self.echo_send(a))
        S["c"]["tx_packets"] += 1
        S["c"]["tx_bytes"] += A["size"]
        self.ip_send(A["node"], (a, 0, A["size"] + 8 + 20, A["ttl"]))
        S["sent"] += 1  # ++m_sent, whatever Send returned
        if S["sent"] < A["count"] and self.nudge != "send_before_children":  # ScheduleTransmit (m_interval)
            S["send_ev"] = self.schedule(A["interval"], lambda: self.echo_send(a))

    def udp_client_send(self, a):  # udp-client.cc:148-187
        A, S = self.sc.apps[a], self.app[a]
        # seqTs.SetSeq (m_sent); Create<Packet> (m_size - 12) + the header: m_size bytes of payload
        if self.ip_send(A["node"], (a, 0, A["size"] + 8 + 20, A["ttl"] | (S["sent"] << 8))):
            S["sent"] += 1  # only when Send returned >= 0
            S["c"]["tx_packets"] += 1
            S["c"]["tx_bytes"] += A["size"]
        elif S["sent"] == 0:
            self.diag["noroute_attempts_at_zero"] += 1
        if S["sent"] < A["count"]:
            S["send_ev"] = self.schedule(A["interval"], lambda: self.udp_client_send(a))

    # ---------------- Application start / stop ----------------
    def start_application(self, a):
        A, S = self.sc.apps[a], self.app[a]
        k = A["kind"]
        if k in (p2p.APP_SINK, p2p.APP_ECHO_SERVER):  # Bind (local)
            S["bound"] = True
        elif k == p2p.APP_UDP_SERVER:  # Bind (Any, port); SetRecvCallback (HandleRead)
            S["bound"] = S["receiving"] = True
        elif k == p2p.APP_ECHO_CLIENT:  # Bind, Connect, SetRecvCallback, ScheduleTransmit (Seconds (0.))
            S["bound"] = True
            S["send_ev"] = self.schedule(0, lambda: self.echo_send(a))
        elif k == p2p.APP_UDP_CLIENT:  # Bind, Connect, SetRecvCallback (null), Schedule (Seconds (0.0), Send)
            S["send_ev"] = self.schedule(0, lambda: self.udp_client_send(a))
        else:  # OnOff :132-151
            self.cancel_events(a)
            S["ss_ev"] = self.schedule(nsref.seconds(A["off"]), lambda: self.start_sending(a))

    def stop_application(self, a):
        S, k = self.app[a], self.sc.apps[a]["kind"]
        if k in (p2p.APP_SINK, p2p.APP_ECHO_SERVER):
            S["bound"] = False  # KNOWN DEVIATION (module docstring): the oracle's rule, not Close ()'s
        elif k == p2p.APP_ECHO_CLIENT:
            S["bound"] = False  # (the same deviation)
            self.cancel(S["send_ev"])
        elif k == p2p.APP_UDP_SERVER:  # SetRecvCallback (null): the socket stays bound and open
            S["receiving"] = False
        elif k == p2p.APP_UDP_CLIENT:  # Simulator::Cancel (m_sendEvent)
            self.cancel(S["send_ev"])
        else:
            self.cancel_events(a)

    # ---------------- setup ----------------
    def app_object_start(self, a):  # Object::Start -> Application::DoStart (application.cc:87-95)
        if self.app[a]["started"]:
            return
        self.app[a]["started"] = True
        A = self.sc.apps[a]
        self.schedule(A["start"], lambda: self.start_application(a))
        if A["stop"] != 0:
            self.schedule(A["stop"], lambda: self.stop_application(a))

    def node_start(self, n):  # Node::DoStart: the applications in AddApplication order
        for a in self.node_apps[n]:
            self.app_object_start(a)

    def setup(self):
        sc = self.sc
        for kind, k in sc.setup:
            if kind == p2p.SETUP_NODE:
                self.schedule_ctx(k, 0, lambda k=k: self.node_start(k))
            elif kind == p2p.SETUP_DEVICE:  # NetDevice::Start: already started by Node::Start
                self.schedule_ctx(sc.dev[k][0], 0, lambda: None)
            elif kind == p2p.SETUP_APP:
                self.schedule_ctx(sc.apps[k]["node"], 0, lambda k=k: self.app_object_start(k))
            elif kind == p2p.SETUP_STOP:  # Simulator::Stop (Time)
                self.schedule(sc.stop_ns, lambda: setattr(self, "m_stop", True))
            elif kind == p2p.SETUP_NOOP:
                self.schedule_ctx(k, 0, lambda: None)
            else:  # ScheduleDestroy: a uid, no queued event
                self.m_uid += 1


def run(sc, trace_kinds=0x7F, nudge=None):
    """Runs scenario `sc`; returns a dict: stats (the nsgpu_p2p_stats fields the model has), devc / appc / servers
    (numpy arrays in the device's layouts), log = (ts, uid, ctx) arrays of the whole pop order, trace (records in
    the device's format, in call order) and diag (what the vacuity checks of the GPU scenarios read)."""
    m = Model(sc, trace_kinds, nudge)
    m.setup()
    m.run()
    devc = np.zeros(len(sc.dev), p2p.DEV_COUNTERS_DTYPE)
    for d, D in enumerate(m.dev):
        for f, v in D["c"].items():
            devc[d][f] = v & 0xFFFFFFFF
    appc = np.zeros(len(sc.apps), p2p.APP_COUNTERS_DTYPE)
    servers = np.zeros(len(sc.apps), p2p.UDP_SERVER_DTYPE)
    wide_gaps = 0
    for a, S in enumerate(m.app):
        for f, v in S["c"].items():
            appc[a][f] = v
        if S["loss"] is not None:
            servers[a] = (S["received"], S["loss"].m_lost, S["loss"].m_lastMaxSeqNum, 0)
            wide_gaps += S["loss"].wide_gaps
    log = (np.array([e[0] for e in m.log], np.uint64), np.array([e[1] for e in m.log], np.uint32),
           np.array([e[2] for e in m.log], np.uint32))
    stats = dict(dispatched=m.dispatched, cancelled=m.cancelled, digest=m.digest, final_ts=m.now,
                 next_uid=m.m_uid, ttl_drops=m.ttl_drops, no_route_drops=m.no_route_drops,
                 unreach_drops=m.unreach_drops, icmp_sent=m.icmp_sent)
    m.diag["wide_gaps"] = wide_gaps
    return dict(stats=stats, devc=devc, appc=appc, servers=servers, log=log,
                trace=np.array(m.trace, dtype=p2p.TRACE_RECORD_DTYPE), diag=m.diag)
