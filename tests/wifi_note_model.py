"""An independent reference for the closed-loop PHY's notification stream (nsgpu_wifil_note), in plain Python.

NoteModel restates, per receiver, YansWifiPhy::StartReceivePacket (yans-wifi-phy.cc:399-496) with
InterferenceHelper::AppendEvent / GetEnergyDuration (interference-helper.cc:171-212) and the state fields
GetState reads (wifi-phy-state-helper.cc:159-183).  It is driven by what the oracle already returns: the run's
SendPacket list, the pop log (the Receive events' uids and their order at the receiver) and the end records;
arrival time and rx power of each (send, receiver) pair come from nsref.fanout_yans, the oracle's own arithmetic.

StateHelper restates WifiPhyStateHelper (wifi-phy-state-helper.cc:122-183, 254-423) with its NS_ASSERT
preconditions and a listener-call log; it consumes notes, the phy's own SendPackets and its end records — what
the ns-3 binding feeds the real class with."""
import bisect
import math

import numpy as np

import nsref
import wifi

IDLE, RX, TX, CCA_BUSY = wifi.IDLE, wifi.RX, wifi.TX, wifi.CCA_BUSY


def _dbm_to_w(dbm):  # DbmToW (yans-wifi-phy.cc:727-732)
    return math.pow(10.0, dbm / 10.0) / 1000.0


class _Log:
    """The pop log indexed by uid (uids are unique) and, per context, by ts."""

    def __init__(self, log):
        self.ts, self.uid, self.ctx = (np.asarray(a) for a in log)
        self.by_uid = np.argsort(self.uid, kind="stable")
        self.suid = self.uid[self.by_uid]
        self._ctx = {}

    def find(self, uid):
        """Index of the entry with this uid, or -1."""
        if not 0 <= uid <= 0xffffffff:
            return -1
        i = int(np.searchsorted(self.suid, self.suid.dtype.type(uid)))  # (a Python int would convert the array)
        if i < len(self.suid) and int(self.suid[i]) == uid:
            return int(self.by_uid[i])
        return -1

    def at(self, ts, ctx):
        if ctx not in self._ctx:  # (one scan of the log per probed context)
            m = self.ctx == ctx
            self._ctx[ctx] = (self.ts[m], self.uid[m])
        cts, cuid = self._ctx[ctx]
        return [int(u) for u in cuid[cts == ts]]


def receptions(phys, txs, log, receivers, size, mode, preamble, dbm):
    """For each chosen receiver, its dispatched Receive events (ts, uid, tx, rxPowerW, duration ns), in (ts, uid)
    order.  txs: (ts, closure uid, phy) per SendPacket, the row is the transmission index; size: one value or one
    per SendPacket.  A SendPacket's Receive uids are uid_base + the receiver's place in the channel's loop
    (yans-wifi-channel.cc:77-115): uid_base is the one value for which the log holds the receivers' events at
    their arrival times and contexts."""
    lg = _Log(log)
    chain = nsref.loss_chain(*phys.loss)
    sizes = np.broadcast_to(np.asarray(size), (len(txs),))
    recv = {int(j): [] for j in receivers}
    rarr = np.array(sorted(recv), np.uint32)
    for k, (ts, _cu, s) in enumerate(np.asarray(txs, np.uint64).reshape(-1, 3)):
        ts, s = int(ts), int(s)
        fo = nsref.fanout_yans(phys.x, phys.y, phys.z, phys.channel, phys.node, s, dbm, chain, phys.speed, ts, 0)
        mine = fo[np.isin(fo["phy"], rarr)]
        if not len(mine):
            continue
        base = None
        for probe in mine:
            for c in lg.at(int(probe["ts"]), int(probe["context"])):
                b = c - int(probe["uid"])
                if b < 0:
                    continue
                hits = 0
                for r in mine:
                    i = lg.find(b + int(r["uid"]))
                    if i >= 0 and int(lg.ts[i]) == int(r["ts"]) and int(lg.ctx[i]) == int(r["context"]):
                        hits += 1
                    elif i >= 0:
                        hits = -1
                        break
                if hits > 0 and (base is None or hits > base[1]):
                    base = (b, hits)
            if base is not None:
                break
        if base is None:
            continue  # (sent so late that none of the chosen receivers' Receives was dispatched)
        dur = int(wifi.tx_duration_ns(int(sizes[k]), mode, preamble))
        for r in mine:
            uid = base[0] + int(r["uid"])
            if lg.find(uid) < 0:
                continue
            w = _dbm_to_w(float(r["rx_dbm"]) + phys.rx_gain_db)  # StartReceivePacket: rxPowerDbm += m_rxGainDb
            recv[int(r["phy"])].append((int(r["ts"]), uid, k, w, dur))
    for v in recv.values():
        v.sort()
    return recv


class NoteModel:
    """One receiver's InterferenceHelper list and state fields."""

    def __init__(self, phy, ed_w, cca_w):
        self.phy, self.ed_w, self.cca_w = phy, ed_w, cca_w
        self.ni = []  # NiChanges: [time, delta], sorted by time (AddNiChangeEvent: upper_bound)
        self.first_power = 0.0
        self.rxing = False
        self.end_tx = self.end_rx = self.end_cca = 0
        self.notes = []

    def state(self, now):  # GetState (wifi-phy-state-helper.cc:159-183), no SWITCHING here
        if self.end_tx > now:
            return TX
        if self.rxing:
            return RX
        return CCA_BUSY if self.end_cca > now else IDLE

    def _add(self, t, d):
        self.ni.insert(bisect.bisect_right([e[0] for e in self.ni], t), [t, d])

    def send(self, now, dur):  # SendPacket (yans-wifi-phy.cc:499-522): SwitchToTx, RX cancelled
        assert not self.end_tx > now, "SendPacket while transmitting"
        if self.rxing:
            self.rxing = False
            self.end_rx = now
        self.end_tx = now + dur

    def end_receive(self, cancelled):  # EndReceive (:770-799): NotifyRxEnd, DoSwitchFromRx
        if not cancelled:
            self.rxing = False

    def receive(self, now, uid, tx, w, dur):
        end_new = now + dur
        if not self.rxing:  # AppendEvent (interference-helper.cc:192-212)
            p = bisect.bisect_right([e[0] for e in self.ni], now)
            for e in self.ni[:p]:
                self.first_power += e[1]
            del self.ni[:p]
            self.ni.insert(0, [now, w])
        else:
            self._add(now, w)
        self._add(end_new, -w)
        st = self.state(now)
        maybe, rx_duration = False, 0
        if st in (RX, TX):
            kind = wifi.NOTE_DROP_RX if st == RX else wifi.NOTE_DROP_TX
            until = max((self.end_rx if st == RX else self.end_tx) - now, 0)  # GetDelayUntilIdle
            maybe = end_new > now + until
        elif w > self.ed_w:
            kind, rx_duration = wifi.NOTE_SYNC, dur
            self.rxing = True
            self.end_rx = end_new
        else:
            kind, maybe = wifi.NOTE_DROP_ED, True
        cca = 0
        if maybe:  # GetEnergyDuration (interference-helper.cc:171-190)
            noise, end = self.first_power, now
            for t, d in self.ni:
                noise += d
                end = t
                if end < now:
                    continue
                if noise < self.cca_w:
                    break
            cca = end - now if end > now else 0
            if cca:  # SwitchMaybeToCcaBusy
                self.end_cca = max(self.end_cca, now + cca)
        self.notes.append((now, uid, self.phy, tx, kind, st, 0, rx_duration, cca))


def model_notes(phys, txs, log, ends, receivers, size, mode, preamble, dbm):
    """(notes of the chosen receivers in (ts, uid) order as WIFIL_NOTE_DTYPE, the per-receiver models)."""
    receivers = [int(j) for j in receivers]
    recv = receptions(phys, txs, log, receivers, size, mode, preamble, dbm)
    txs = np.asarray(txs, np.uint64).reshape(-1, 3)
    sizes = np.broadcast_to(np.asarray(size), (len(txs),))
    ed_w, cca_w = _dbm_to_w(phys.ed), _dbm_to_w(phys.cca)
    models, rows = {}, []
    for j in receivers:
        m = NoteModel(j, ed_w, cca_w)
        ev = [(ts, uid, 0, (ts, uid, k, w, dur)) for ts, uid, k, w, dur in recv[j]]
        ev += [(int(t[0]), int(t[1]), 1, int(wifi.tx_duration_ns(int(sizes[k]), mode, preamble)))
               for k, t in enumerate(txs) if int(t[2]) == j]
        ev += [(int(e["ts"]), int(e["uid"]), 2, bool(int(e["flags"]) & wifi.END_CANCELLED))
               for e in ends[ends["phy"] == j]]
        ev.sort(key=lambda v: (v[0], v[1]))
        for ts, _uid, what, arg in ev:
            if what == 0:
                m.receive(*arg)
            elif what == 1:
                m.send(ts, arg)
            else:
                m.end_receive(arg)
        models[j] = m
        rows += m.notes
    rows.sort(key=lambda r: (r[0], r[1]))
    return np.array(rows, dtype=wifi.WIFIL_NOTE_DTYPE), models


class Precondition(AssertionError):
    """An NS_ASSERT / NS_FATAL_ERROR of WifiPhyStateHelper would have fired."""


class StateHelper:
    """WifiPhyStateHelper (wifi-phy-state-helper.cc): its fields, the preconditions of each switch, the State
    trace (m_stateLogger) and the listener calls."""

    def __init__(self):
        self.rxing = False
        self.end_tx = self.end_rx = self.end_cca = self.end_sw = 0
        self.start_tx = self.start_rx = self.start_cca = 0
        self.prev_change = 0
        self.listener, self.state_log = [], []

    def get_state(self, now):  # :159-183
        if self.end_tx > now:
            return TX
        if self.rxing:
            return RX
        if self.end_sw > now:
            raise Precondition("SWITCHING is never entered here")
        return CCA_BUSY if self.end_cca > now else IDLE

    def delay_until_idle(self, now):  # :122-151
        st = self.get_state(now)
        r = {RX: self.end_rx, TX: self.end_tx, CCA_BUSY: self.end_cca, IDLE: now}[st] - now
        return max(r, 0)

    def _need(self, ok, what):
        if not ok:
            raise Precondition(what)

    def _cca_start(self):
        return max(self.end_rx, self.end_tx, self.start_cca, self.end_sw)

    def _log_idle_cca(self, now):  # LogPreviousIdleAndCcaBusyStates (:234-252)
        idle = max(self.end_cca, self.end_rx, self.end_tx, self.end_sw)
        self._need(idle <= now, "idleStart <= now")
        if self.end_cca > self.end_rx and self.end_cca > self.end_sw and self.end_cca > self.end_tx:
            s = self._cca_start()
            self.state_log.append((s, idle - s, CCA_BUSY))
        self.state_log.append((idle, now - idle, IDLE))

    def switch_to_tx(self, now, dur):  # :254-290 (and SendPacket's NS_ASSERT, yans-wifi-phy.cc:508)
        self._need(self.get_state(now) != TX, "SendPacket: !IsStateTx")
        self.listener.append(("NotifyTxStart", now, dur))
        st = self.get_state(now)
        if st == RX:
            self.rxing = False
            self.state_log.append((self.start_rx, now - self.start_rx, RX))
            self.end_rx = now
        elif st == CCA_BUSY:
            s = self._cca_start()
            self.state_log.append((s, now - s, CCA_BUSY))
        else:
            self._log_idle_cca(now)
        self.state_log.append((now, dur, TX))
        self.prev_change = now
        self.end_tx = now + dur
        self.start_tx = now

    def switch_to_rx(self, now, dur):  # :291-321
        self._need(self.get_state(now) in (IDLE, CCA_BUSY), "SwitchToRx: IsStateIdle () || IsStateCcaBusy ()")
        self._need(not self.rxing, "SwitchToRx: !m_rxing")
        self.listener.append(("NotifyRxStart", now, dur))
        if self.get_state(now) == IDLE:
            self._log_idle_cca(now)
        else:
            s = self._cca_start()
            self.state_log.append((s, now - s, CCA_BUSY))
        self.prev_change = now
        self.rxing = True
        self.start_rx = now
        self.end_rx = now + dur
        self._need(self.get_state(now) == RX, "SwitchToRx: IsStateRx ()")

    def switch_from_rx_end(self, now, ok):  # SwitchFromRxEndOk / Error -> DoSwitchFromRx (:367-403)
        self.listener.append(("NotifyRxEndOk" if ok else "NotifyRxEndError", now, 0))
        self._need(self.get_state(now) == RX, "DoSwitchFromRx: IsStateRx ()")
        self._need(self.rxing, "DoSwitchFromRx: m_rxing")
        self.state_log.append((self.start_rx, now - self.start_rx, RX))
        self.prev_change = now
        self.rxing = False
        self._need(self.get_state(now) in (IDLE, CCA_BUSY), "DoSwitchFromRx: IsStateIdle () || IsStateCcaBusy ()")

    def switch_maybe_to_cca_busy(self, now, dur):  # :404-425
        self.listener.append(("NotifyMaybeCcaBusyStart", now, dur))
        if self.get_state(now) == IDLE:
            self._log_idle_cca(now)
        self.start_cca = now
        self.end_cca = max(self.end_cca, now + dur)

    # ---- what the binding does with a note, a SendPacket and a handed-back EndReceive
    def on_note(self, n):
        now = int(n["ts"])
        self._need(self.get_state(now) == int(n["state"]), "the note's state is the helper's GetState ()")
        if int(n["kind"]) == wifi.NOTE_SYNC:
            self.switch_to_rx(now, int(n["rx_duration"]))
        if int(n["cca_duration"]):
            self.switch_maybe_to_cca_busy(now, int(n["cca_duration"]))

    def on_send(self, now, dur):
        self.switch_to_tx(now, dur)

    def on_end(self, e, ok=True):
        if not int(e["flags"]) & wifi.END_CANCELLED:
            self.switch_from_rx_end(int(e["ts"]), ok)


def drive_state_helpers(n_phy, notes, txs, ends, size, mode, preamble, probes=()):
    """One StateHelper per phy fed in (ts, uid) order with its notes, SendPackets (txs rows: ts, closure uid, phy)
    and end records.  probes: (ts, uid, phy, state) of GetState calls made by host closures (e.g. a MAC's
    attempt): each is compared with the helper's state at its place in the order.  Returns the helpers."""
    txs = np.asarray(txs, np.uint64).reshape(-1, 3)
    sizes = np.broadcast_to(np.asarray(size), (len(txs),))
    ev = [(int(n["ts"]), int(n["uid"]), 1, n) for n in notes]
    # a closure's GetState comes before its own SendPacket: the probe first at an equal key
    ev += [(int(p[0]), int(p[1]), 0, p) for p in probes]
    ev += [(int(t[0]), int(t[1]), 2, (int(t[2]), int(wifi.tx_duration_ns(int(sizes[k]), mode, preamble))))
           for k, t in enumerate(txs)]
    ev += [(int(e["ts"]), int(e["uid"]), 3, e) for e in ends]
    ev.sort(key=lambda v: (v[0], v[1], v[2]))
    hs = [StateHelper() for _ in range(n_phy)]
    for ts, _uid, what, arg in ev:
        if what == 1:
            hs[int(arg["phy"])].on_note(arg)
        elif what == 0:
            got = hs[int(arg[2])].get_state(ts)
            if got != int(arg[3]):
                raise Precondition(f"GetState of phy {int(arg[2])} at {ts}: helper {got}, PHY {int(arg[3])}")
        elif what == 2:
            hs[arg[0]].on_send(ts, arg[1])
        else:
            hs[int(arg["phy"])].on_end(arg)
    return hs
