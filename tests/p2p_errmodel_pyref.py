"""Receive error models added to the Python restatement of the p2p subset (tests/p2p_frag_pyref.py and
tests/p2p_pyref.py, which stay as they are): Model overrides the device's Receive, written from the reference's
lines alone.

  Receive      point-to-point-net-device.cc:304-317 (m_receiveErrorModel->IsCorrupt (packet) first: a corrupt frame
               fires m_phyRxDropTrace, which no ascii / pcap helper hooks, and nothing else)
  IsCorrupt    error-model.cc:60-75 (a disabled model answers false without calling DoCorrupt)
  ReceiveList  error-model.cc:343-360 (m_timesInvoked += 1; m_timesInvoked - 1 in the list)
  Rate         error-model.cc:178-223 (one m_ranvar.GetValue () a frame, against m_rate or 1 - pow (1.0 - m_rate, size
               or 8 * size); size = p->GetSize () with the PppHeader still on)
  RngStream    rng-stream.cc:221-244 (U01), :340-381, 417-444 (the k-th stream of a program: the seed, k jumps of
               2^127 steps, RngRun jumps of 2^76); random-variable.cc:251-258 (UniformVariable (0, 1): U01 itself)

The generator's arithmetic is done in Python integers; the jump matrices come from squaring the one-step matrices.
"""
import math

import numpy as np

import p2p
import p2p_frag_pyref

M1, M2 = 4294967087, 4294944443
A12, A13N, A21, A23N = 1403580, 810728, 527612, 1370589
NORM = 1.0 / (M1 + 1.0)
A1 = ((0, 1, 0), (0, 0, 1), (-A13N % M1, A12, 0))  # the recurrences as matrices on (s0, s1, s2), (s3, s4, s5)
A2 = ((0, 1, 0), (0, 0, 1), (-A23N % M2, 0, A21))


def _matmul(x, y, m):
    return tuple(tuple(sum(x[i][k] * y[k][j] for k in range(3)) % m for j in range(3)) for i in range(3))


def _matvec(x, v, m):
    return [sum(x[i][k] * v[k] for k in range(3)) % m for i in range(3)]


def _pow2(x, e, m):
    for _ in range(e):
        x = _matmul(x, x, m)
    return x


_JUMP = {e: (_pow2(A1, e, M1), _pow2(A2, e, M2)) for e in (127, 76)}


def check_seed(seed):
    """CheckSeed (:268-302) for six equal words."""
    return 0 < seed < M2


class RngStream:
    """The k-th (0-based) RngStream a program with RngSeed `seed` and RngRun `run` constructs."""

    def __init__(self, seed=1, run=1, k=0):
        seed, run = seed or 1, run or 1
        if not check_seed(seed):
            raise ValueError("seed")
        self.cg = [seed] * 6
        for _ in range(k):  # InitializeStream: nextSeed moves on 2^127 steps a stream
            self._jump(127)
        for _ in range(run):  # ResetNthSubstream (run)
            self._jump(76)

    def _jump(self, e):
        b1, b2 = _JUMP[e]
        self.cg = _matvec(b1, self.cg[:3], M1) + _matvec(b2, self.cg[3:], M2)

    def u01(self):  # :221-244
        c = self.cg
        p1 = (A12 * c[1] - A13N * c[0]) % M1
        c[0], c[1], c[2] = c[1], c[2], p1
        p2 = (A21 * c[5] - A23N * c[3]) % M2
        c[3], c[4], c[5] = c[4], c[5], p2
        return float(p1 - p2) * NORM if p1 > p2 else float(p1 - p2 + M1) * NORM


def threshold(unit, rate, size):
    """DoCorruptPkt / DoCorruptByte / DoCorruptBit's right-hand side for a frame of `size` bytes."""
    if unit == "pkt":
        return rate
    return 1 - math.pow(1.0 - rate, size if unit == "byte" else 8 * size)


class ReceiveListModel:
    def __init__(self, packets):
        self.m_packetList = list(packets)
        self.m_timesInvoked = 0

    def do_corrupt(self, _size):
        self.m_timesInvoked = (self.m_timesInvoked + 1) & 0xFFFFFFFF
        return any((self.m_timesInvoked - 1) & 0xFFFFFFFF == i for i in self.m_packetList)


class RateModel:
    def __init__(self, rate, unit, stream):
        self.m_rate, self.m_unit, self.m_ranvar = rate, unit, stream

    def do_corrupt(self, size):
        return self.m_ranvar.u01() < threshold(self.m_unit, self.m_rate, size)


class Model(p2p_frag_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self.em = {}
        self.em_count = {}    # device -> [invoked, corrupted]
        self.em_dropped = []  # (device, frame) of every corrupt frame, in order
        for d, e in getattr(sc, "error_models", {}).items():
            if not e["enabled"]:
                continue
            if e["kind"] == "list":
                self.em[d] = ReceiveListModel(e["packets"])
            else:
                self.em[d] = RateModel(e["rate"], e["unit"], RngStream(sc.rng_seed, sc.rng_run, e["stream"]))
            self.em_count[d] = [0, 0]

    def receive(self, d, p):  # point-to-point-net-device.cc:304-346
        m = self.em.get(d)
        if m is None:
            return super().receive(d, p)
        self.dev[d]["c"]["rx_packets"] += 1
        self.em_count[d][0] += 1
        if m.do_corrupt(p[2]):  # m_phyRxDropTrace (packet)
            self.em_count[d][1] += 1
            self.em_dropped.append((d, p))
            return
        p = (p[0], p[1], p[2] - 2, p[3])     # ProcessHeader
        self.tr(p2p_frag_pyref.p2p_pyref.TR_RX, d, p)     # m_macRxTrace
        self.tr(p2p_frag_pyref.p2p_pyref.TR_IP_RX, d, p)  # Ipv4L3Protocol::Receive: m_rxTrace
        self.ip_receive(self.sc.dev[d][0], p, d)


def run(sc, trace_kinds=0x7F, nudge=None):
    """p2p_frag_pyref.run's dict for scenario `sc`, and em = the nsgpu_error_model_record array, dropped = the corrupt
    frames [(device, descriptor)]."""
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
    frag["cancelled_timers"] = sum(1 for ev in m.timer_events
                                   if ev.cancelled and (ev.ts, ev.uid) <= (m.now, m.cur_uid))
    em = np.zeros(len(sc.dev), p2p.ERROR_MODEL_DTYPE)
    for d, (inv, cor) in m.em_count.items():
        em[d] = (inv & 0xFFFFFFFF, cor & 0xFFFFFFFF)
    return dict(stats=stats, devc=devc, appc=appc, servers=servers, log=log, frag=frag, em=em, dropped=m.em_dropped,
                trace=np.array(m.trace, dtype=p2p.TRACE_RECORD_DTYPE), diag=m.diag)
