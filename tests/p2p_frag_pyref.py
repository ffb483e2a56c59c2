"""IPv4 fragmentation and reassembly added to the Python restatement of the p2p subset (tests/p2p_pyref.py, which
stays as it is): Model overrides the IP send and the local-deliver step and adds the timeout event, written from
the reference's lines alone.

  send        ipv4-l3-protocol.cc:722-731, 751-761 (SendRealOut: above the MTU DoFragmentation, then m_txTrace and the
              interface's Send for each fragment in order), :1116-1206 (DoFragmentation)
  receive     :843-859 (LocalDeliver: a fragment goes through ProcessFragment; `ip`, the header UdpL4Protocol::Receive
              and SendDestUnreachPort get, stays the arrived fragment's), :1208-1257 (ProcessFragment),
              :1259-1389 (Fragments: AddFragment, IsEntire, GetPacket, GetPartialPacket)
  timeout     :1391-1412 (HandleFragmentsTimeout), :61-64 (FragmentExpirationTimeout, Seconds (30))

ProcessFragment builds its map key with `&` where `|` was meant (:1213-1214): `src << 32 & dst` and `id << 16 & proto`
are both 0 for every header, so a node has ONE Fragments buffer and ONE timer for all sources and identifications.
That is restated literally: `key` below is always (0, 0).

A packet is the device's descriptor (app, ipid, size, ttl); a fragment carries offset / 8 << 16 | MF << 29 above its
16-bit identification (include/nsgpu_types.h), and a frag scenario's senders write the 16-bit identification.
Every device has MTU 1500, so a forwarder never fragments and DoFragmentation's alreadyFragmented branch is dead.
"""
import numpy as np

import p2p
import p2p_pyref
from p2p_pyref import PKT_ICMP, PKT_REPLY, TR_IP_TX

MTU = 1500
FRAG_SHIFT, FRAG_OFF_MASK, FRAG_MF = 16, 0x1FFF, 0x20000000
DEFAULT_TIMEOUT_NS = 30_000_000_000  # Seconds (30)


def do_fragmentation(size):
    """DoFragmentation (:1116-1206) for a packet of IPv4 length `size` and MTU 1500: [(offset, part, more)]."""
    payload = size - 20  # p->RemoveHeader (ipv4Header)
    fragment_size = (MTU - 20) & ~0x7  # :1148
    out, offset = [], 0
    while True:
        if payload > offset + fragment_size:  # :1156
            more, part = True, fragment_size
        else:
            more, part = False, payload - offset
        out.append((offset, part, more))
        offset += part
        if not more:
            return out


def fragment_lengths(payload):
    """IPv4 lengths of what SendRealOut puts on the wire for a UDP payload of `payload` bytes."""
    size = payload + 8 + 20
    if size <= MTU:  # :722: packet->GetSize () > outInterface->GetDevice ()->GetMtu ()
        return [size]
    return [20 + part for _o, part, _m in do_fragmentation(size)]


class Fragments:
    """Ipv4L3Protocol::Fragments (:1259-1389).  An entry is (size, offset, tag): size stands for the Ptr<Packet>, tag
    is whatever the caller wants back from the first entry (the fragment's descriptor)."""

    def __init__(self, nudge=None):
        self.m_moreFragment = False  # m_moreFragment (0)
        self.m_fragments = []
        self.nudge = nudge

    def add_fragment(self, size, offset, more, tag=None):  # :1268-1289
        it = 0
        while it < len(self.m_fragments):
            second = self.m_fragments[it][1]
            if second > offset or (self.nudge == "before_equal" and second == offset):
                break
            it += 1
        if it == len(self.m_fragments):
            self.m_moreFragment = more
        self.m_fragments.insert(it, (size, offset, tag))

    def is_entire(self):  # :1291-1319 (uint16_t lastEndOffset, fragmentEnd)
        ret = (not self.m_moreFragment) and len(self.m_fragments) > 0
        if ret:
            last_end = 0
            for size, offset, _t in self.m_fragments:
                if last_end < offset:
                    ret = False
                    break
                fragment_end = (size + offset) & 0xFFFF
                last_end = max(last_end, fragment_end)
        return ret

    def get_packet(self):  # :1321-1356: the size of the packet built
        p, last_end = 0, 0
        for size, offset, _t in self.m_fragments:
            if last_end > offset:
                new_start = last_end - offset
                if size > new_start:
                    p += size - new_start
            else:
                p += size
            last_end = p & 0xFFFF
        return p

    def get_partial_packet(self):  # :1358-1389
        p, last_end = 0, 0
        if self.m_fragments[0][1] > 0:
            return p
        for size, offset, _t in self.m_fragments:
            if last_end > offset:
                new_start = last_end - offset
                assert size >= new_start  # (CreateFragment (newStart, size - newStart) asserts otherwise)
                p += size - new_start
            elif last_end == offset:
                p += size
            last_end = p & 0xFFFF
        return p


def frag_fields(p):
    """(offset in bytes, MF) of descriptor p."""
    return ((p[1] >> FRAG_SHIFT) & FRAG_OFF_MASK) * 8, bool(p[1] & FRAG_MF)


class Model(p2p_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self.frag_timeout = sc.frag_timeout_ns or DEFAULT_TIMEOUT_NS
        self.m_fragments = {}        # key -> Fragments (per node)
        self.m_fragmentsTimers = {}  # key -> EventId
        self.fs = dict.fromkeys(p2p.FRAG_STATS_FIELDS, 0)
        self.timer_events = []       # every timer ever scheduled
        self.diag["mixed"] = 0  # datagrams reassembled from a list longer than their own fragment count

    # ---------------- send ----------------
    def ip_send(self, n, p):  # Ipv4L3Protocol::Send: BuildHeader writes the header's 16-bit identification
        if not self.sc.frag:
            return super().ip_send(n, p)
        out = self.route(n, p)
        if out == p2p.NO_ROUTE:
            self.no_route_drops += 1
            return False
        p = (p[0], self.node_ipid[n] & 0xFFFF, p[2], p[3])
        self.node_ipid[n] += 1
        self.ip_out(out, p)
        return True

    def ip_out(self, out, p):  # SendRealOut (:722-731, 751-761)
        if not (self.sc.frag and p[2] > MTU and self.sc.dev[out][0] == self.origin_of(p)):
            return super().ip_out(out, p)
        frags = do_fragmentation(p[2])
        self.fs["fragmented"] += 1
        self.fs["fragments_sent"] += len(frags)
        for offset, part, more in frags:  # for (it = listFragments...): m_txTrace, outInterface->Send
            f = (p[0], (p[1] & 0xFFFF) | ((offset >> 3) << FRAG_SHIFT) | (FRAG_MF if more else 0), 20 + part, p[3])
            self.tr(TR_IP_TX, out, f)
            self.device_send(out, f)

    def origin_of(self, p):
        """The node that sends datagram p (only it sees a packet above the MTU: a forwarder's are fragments)."""
        A = self.sc.apps
        if p[0] & PKT_ICMP:
            return None
        return A[p[0] & ~PKT_REPLY]["dst"] if p[0] & PKT_REPLY else A[p[0]]["node"]

    # ---------------- receive ----------------
    def ip_receive(self, n, p, rx_dev):
        if not (self.sc.frag and self.pkt_dst_node(p) == n and not p[0] & PKT_ICMP and p[1] >> FRAG_SHIFT):
            return super().ip_receive(n, p, rx_dev)
        # LocalDeliver (:849-859): !IsLastFragment () || GetFragmentOffset () != 0
        ip = p
        whole = self.process_fragment(n, p, rx_dev)
        if whole is None:
            return
        # UdpL4Protocol::Receive (p, ip, ..): the packet is the reassembled one, the header the arrived fragment's
        k = self.lookup(n, whole)
        if k is None:
            self.unreach_drops += 1
            if self.sc.icmp:
                self.icmp_send(n, ip, True)  # SendDestUnreachPort (ip, copy)
            return
        self.schedule(0, lambda: self.do_forward_up(k, whole, n))

    def process_fragment(self, n, p, iif):  # :1208-1257; returns the entire datagram's descriptor or None
        key = (n, 0, 0)  # (addressCombination, idProto) are 0 for every header: one buffer a node
        offset, more = frag_fields(p)
        if key not in self.m_fragments:
            self.m_fragments[key] = Fragments(self.nudge)
            self.m_fragmentsTimers[key] = self.schedule(
                self.frag_timeout, lambda: self.handle_fragments_timeout(key, p, iif))
            self.timer_events.append(self.m_fragmentsTimers[key])
        fragments = self.m_fragments[key]
        if len(fragments.m_fragments) >= p2p.FRAG_CAP:
            raise OverflowError("a reassembly list would pass FRAG_CAP entries")
        fragments.add_fragment(p[2] - 20, offset, more, p)
        self.fs["max_list"] = max(self.fs["max_list"], len(fragments.m_fragments))
        if not fragments.is_entire():
            return None
        size = fragments.get_packet()
        first = fragments.m_fragments[0][2]  # the UDP header (and a SeqTsHeader) are the first entry's bytes
        if len(fragments.m_fragments) > len(do_fragmentation(20 + size)):
            self.diag["mixed"] += 1
        del self.m_fragments[key]
        if self.nudge != "timer_left_running":
            self.cancel(self.m_fragmentsTimers[key])  # IsRunning () -> Cancel ()
        del self.m_fragmentsTimers[key]
        self.fs["reassembled"] += 1
        return (first[0], p[1] & 0xFFFF, 20 + size, (p[3] & 0xFF) | (first[3] & ~0xFF))

    def handle_fragments_timeout(self, key, ip, iif):  # :1391-1412
        n = key[0]
        self.fs["timeouts"] += 1
        if key not in self.m_fragments:  # (only the nudged model gets here: the reference would dereference end ())
            return
        size = self.m_fragments[key].get_partial_packet()
        sent = False
        if size > 8 and self.sc.icmp:  # (icmp == 0: GetIcmp ()'s errors are not generated, only counted)
            sent = self.icmp_send(n, ip, False)  # SendTimeExceededTtl (ipHeader, packet)
        # m_dropTrace (ipHeader, packet, DROP_FRAGMENT_TIMEOUT, .., iif): the captured header's fields — flow,
        # identification, length, TTL; the packet is the partial one, so the record names no sequence number
        del sent
        self.ip_drop(iif, (ip[0], ip[1], ip[2], ip[3] & 0xFF))
        del self.m_fragments[key]
        del self.m_fragmentsTimers[key]



def run(sc, trace_kinds=0x7F, nudge=None):
    """p2p_pyref.run's dict for scenario `sc`, and frag = the nsgpu_frag_stats fields."""
    m = Model(sc, trace_kinds, nudge)
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
    # a cancelled timer is dispatched at its time like any event: those whose key the run reached
    frag["cancelled_timers"] = sum(1 for ev in m.timer_events
                                   if ev.cancelled and (ev.ts, ev.uid) <= (m.now, m.cur_uid))
    return dict(stats=stats, devc=devc, appc=appc, servers=servers, log=log, frag=frag,
                trace=np.array(m.trace, dtype=p2p.TRACE_RECORD_DTYPE), diag=m.diag)
