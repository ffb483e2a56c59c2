"""A discrete-event restatement of the whole closed-loop Wi-Fi PHY with channel switching, in plain Python: the
reference of tests/test_wifi_switch_cpu.py and tests/test_gpu_wifi_switch.py (the C++ oracle has no SWITCHING state).

Written from the reference's lines alone:
  src/core/model/default-simulator-impl.cc (the event list keyed (ts, uid), m_uid from 4, Schedule's context),
  src/wifi/model/yans-wifi-phy.cc:327-374 (SetChannelNumber), :399-496 (StartReceivePacket, the SWITCHING case
    :419-436), :499-522 (SendPacket), :770-799 (EndReceive),
  src/wifi/model/yans-wifi-channel.cc:77-115 (Send's receiver loop: the channel test is made at send time),
  src/wifi/model/wifi-phy-state-helper.cc:122-183 (GetDelayUntilIdle, GetState), :323-365
    (SwitchToChannelSwitching), :404-423 (SwitchMaybeToCcaBusy),
  src/wifi/model/interference-helper.cc:171-212 (GetEnergyDuration, AppendEvent), :368-374 (EraseEvents).
Arithmetic it does not restate: arrival time and rx power of every (send, receiver) pair are nsref.fanout_yans's,
called with the channel numbers (and positions) current at the send; durations are wifi.tx_duration_ns's; an
EndReceive's (snr, per) is wifi_per_ref.snr_per's over the phy's StartReceivePacket calls since its last
EraseEvents.  snr_per is given m_rxing as it stood at each of those calls (AppendEvent's branch), kept beside the
window: a lock that a SendPacket or a switch cancelled, and a StartReceive in the nanosecond of a frame's EndReceive (a
reply sent with delay 0 arrives so at a third phy on the line), then fold into m_firstPower as the reference does.

Setup order: the oracle replay's — the closures are scheduled in the order given (the tests list every send, then
every switch, where nsref_wifil_sends puts its moves), then Simulator::Stop.  A closure is (ts, [actions]); actions:
("send", phy, size), ("switch", phy, nch, delay_ns), ("noop",).  Every closure first records GetState of the phys its
actions name (a probe: (ts, uid, phy, state, delay until idle)).

Frames: the model's mode, preamble and tx power are the defaults of send_packet, which takes all three per call; a
reception keeps the (mode, preamble) of its own frame (tx_frames), so frames of different modes may overlap at a phy
(tests/wifi_fuzz_model.py sends them)."""
import bisect
import math

import numpy as np

import mobility_ref
import nsref
import wifi
import wifi_note_model
import wifi_per_ref

IDLE, RX, TX, CCA_BUSY, SWITCHING = wifi.IDLE, wifi.RX, wifi.TX, wifi.CCA_BUSY, 4
NOTE_DROP_SWITCHING = 4
DONE, INIT, POSTPONED, REFUSED = 0, 1, 2, -1  # NSGPU_WIFIL_SWITCH_*; REFUSED: NS_ASSERT (!IsStateSwitching ())
NO_CONTEXT = 0xffffffff
COUNTERS = ("rx", "sync", "drop_rx", "drop_tx", "drop_ed", "cca_switches", "end", "end_cancelled")


class SendError(AssertionError):
    """SendPacket's NS_ASSERT (!IsStateTx () && !IsStateSwitching ()) (yans-wifi-phy.cc:508) would have fired."""


def _dbm_to_w(dbm):  # DbmToW (yans-wifi-phy.cc:727-732)
    return math.pow(10.0, dbm / 10.0) / 1000.0


class _Phy:
    def __init__(self, j, channel):
        self.j, self.channel = j, int(channel)
        self.ni, self.first_power = [], 0.0  # InterferenceHelper: NiChanges [time, delta], m_firstPower
        self.rxing = False                   # (the state helper's m_rxing and the interference helper's agree)
        self.end_tx = self.end_rx = self.end_cca = self.end_sw = self.start_sw = 0
        self.c = dict.fromkeys(COUNTERS, 0)
        self.switches = self.drop_switching = 0
        self.live = None                     # the pending EndReceive of the frame being received
        self.window, self.locked = [], []    # StartReceivePacket calls since the last EraseEvents; the locked ones
        self.window_rxing = []               # m_rxing at each of them (AppendEvent's branch)

    def state(self, now):  # GetState (wifi-phy-state-helper.cc:159-183)
        if self.end_tx > now:
            return TX
        if self.rxing:
            return RX
        if self.end_sw > now:
            return SWITCHING
        return CCA_BUSY if self.end_cca > now else IDLE

    def delay_until_idle(self, now):  # :122-151
        st = self.state(now)
        r = {RX: self.end_rx, TX: self.end_tx, CCA_BUSY: self.end_cca, SWITCHING: self.end_sw, IDLE: now}[st] - now
        return max(r, 0)


class Model:
    def __init__(self, phys, mode, preamble, dbm, notify=(), mob=None, erase=True):
        """phys: wifi.LoopPhys.  mob: {phy: mobility_ref.CvModel} (constant-velocity phys), or None.  erase=False: a
        control that skips m_interference.EraseEvents () at a switch (what the erase tests compare with)."""
        self.erase = erase
        self.end_refs = []   # per end record: None (cancelled) or the reference's (snr, per as mpf, chunks, rx_w)
        self.cfg, self.mode, self.preamble, self.dbm = phys, mode, preamble, dbm
        self.x, self.y, self.z = (np.array(a, np.float64) for a in (phys.x, phys.y, phys.z))
        self.chan = np.array(phys.channel, np.uint32)
        self.node = np.array(phys.node, np.uint32)
        self.phy = [_Phy(j, self.chan[j]) for j in range(phys.n_phy)]
        self.chain = nsref.loss_chain(*phys.loss)
        self.ed_w, self.cca_w = _dbm_to_w(phys.ed), _dbm_to_w(phys.cca)
        self.notify = set(notify)
        self.mob = mob or {}
        self.q = []          # sorted [(ts, uid, ctx, kind, arg)]
        self.uid = 4         # DefaultSimulatorImpl: m_uid (4)
        self.now, self.cur_uid, self.ctx = 0, 0, NO_CONTEXT
        self.log, self.ends, self.notes, self.txs, self.switches, self.probes = [], [], [], [], [], []
        self.log_kinds = []  # per pop-log entry: "closure" | "retry" | "rx" | "end" | "stop"
        self.retries = []    # (ts, uid) of the retry events postponed switches scheduled
        self.tx_sizes = []   # per SendPacket
        self.tx_frames = []  # per SendPacket: (mode, preamble, dbm)

    # ---- Simulator
    def _schedule(self, ts, ctx, kind, arg):
        uid = self.uid
        self.uid += 1
        bisect.insort(self.q, (int(ts), uid, ctx, kind, arg))  # (uids are unique: the order is (ts, uid))
        return uid

    def run(self, closures, stop_ns):
        for ts, actions in closures:
            self._schedule(ts, NO_CONTEXT, "closure", list(actions))
        self._schedule(stop_ns, NO_CONTEXT, "stop", None)
        while self.q:
            ts, uid, ctx, kind, arg = self.q.pop(0)
            self.now, self.cur_uid, self.ctx = ts, uid, ctx
            self.log.append((ts, uid, ctx))
            self.log_kinds.append(kind)
            if kind == "stop":
                break
            if kind == "closure":
                for a in arg:
                    if a[0] not in self.NO_PHY:
                        p = self.phy[a[1]]
                        self.probes.append((ts, uid, a[1], p.state(ts), p.delay_until_idle(ts)))
                for a in arg:
                    self.act(a)
            elif kind == "retry":
                self.set_channel_number(*arg)
            elif kind == "rx":
                self.start_receive(*arg)
            else:
                self.end_receive(arg)
        return self

    NO_PHY = ("noop",)  # the actions that name no phy: a closure probes nothing for them

    def act(self, a):
        """One action of a closure, at its place among the closure's actions (the subclasses add theirs)."""
        if a[0] == "send":
            self.send_packet(a[1], a[2])
        elif a[0] == "switch":
            self.set_channel_number(a[1], a[2], a[3])

    def frame_of(self, mode, preamble, dbm):
        return (self.mode if mode is None else mode, self.preamble if preamble is None else preamble,
                self.dbm if dbm is None else float(dbm))

    # ---- YansWifiPhy::SendPacket (:499-522) and YansWifiChannel::Send (yans-wifi-channel.cc:77-115)
    def send_packet(self, s, size, mode=None, preamble=None, dbm=None):
        """mode, preamble, dbm: this frame's (default: the model's own)."""
        mode, preamble, dbm = self.frame_of(mode, preamble, dbm)
        p, now = self.phy[s], self.now
        st = p.state(now)
        if st in (TX, SWITCHING):
            raise SendError(f"SendPacket of phy {s} at {now} in state {st}")
        dur = int(wifi.tx_duration_ns(int(size), mode, preamble))
        if st == RX:  # m_endRxEvent.Cancel (); NotifyRxEnd (); SwitchToTx's RX case
            p.live["cancelled"] = True
            p.locked.remove(p.live["k"])  # (see the module docstring)
            p.live = None
            p.rxing = False
            p.end_rx = now
        p.end_tx = now + dur
        k = len(self.txs)
        self.txs.append((now, self.cur_uid, s))
        self.tx_sizes.append(int(size))
        self.tx_frames.append((mode, preamble, dbm))
        for j in mobility_ref.send_updates(self.chan, s):  # MobilityModel::GetDistanceFrom's Updates
            if j in self.mob:
                self.mob[j].update(now)
                self.x[j], self.y[j], self.z[j] = self.mob[j].position()
        fo = nsref.fanout_yans(self.x, self.y, self.z, self.chan, self.node, s, dbm, self.chain, self.cfg.speed,
                               now, self.uid)
        for r in fo:  # the receiver loop's ScheduleWithContext calls, in m_phyList order
            w = _dbm_to_w(float(r["rx_dbm"]) + self.cfg.rx_gain_db)  # StartReceivePacket: rxPowerDbm += m_rxGainDb
            uid = self._schedule(int(r["ts"]), int(r["context"]), "rx", (int(r["phy"]), k, w, dur))
            assert uid == int(r["uid"])

    # ---- YansWifiPhy::StartReceivePacket (:399-496)
    def start_receive(self, j, tx, w, dur):
        p, now = self.phy[j], self.now
        end_new = now + dur
        if not p.rxing:  # AppendEvent (interference-helper.cc:192-212)
            n = bisect.bisect_right([e[0] for e in p.ni], now)
            for e in p.ni[:n]:
                p.first_power += e[1]
            del p.ni[:n]
            p.ni.insert(0, [now, w])
        else:
            p.ni.insert(bisect.bisect_right([e[0] for e in p.ni], now), [now, w])
        p.ni.insert(bisect.bisect_right([e[0] for e in p.ni], end_new), [end_new, -w])
        k = len(p.window)
        p.window_rxing.append(p.rxing)
        p.window.append((now, end_new, w) + self.tx_frames[tx][:2])
        st = p.state(now)
        p.c["rx"] += 1
        maybe, rx_duration = False, 0
        if st == SWITCHING:  # :419-436
            kind = NOTE_DROP_SWITCHING
            p.drop_switching += 1
            maybe = end_new > now + p.delay_until_idle(now)
        elif st in (RX, TX):  # :437-457
            kind = wifi.NOTE_DROP_RX if st == RX else wifi.NOTE_DROP_TX
            p.c["drop_rx" if st == RX else "drop_tx"] += 1
            maybe = end_new > now + p.delay_until_idle(now)
        elif w > self.ed_w:  # :461-472: SwitchToRx, Schedule (rxDuration, EndReceive)
            kind, rx_duration = wifi.NOTE_SYNC, dur
            p.c["sync"] += 1
            p.rxing = True
            p.end_rx = end_new
            p.live = dict(phy=j, tx=tx, k=k, w=w, cancelled=False)
            p.locked.append(k)
            self._schedule(end_new, self.ctx, "end", p.live)
        else:  # :475-483
            kind, maybe = wifi.NOTE_DROP_ED, True
            p.c["drop_ed"] += 1
        cca = 0
        if maybe:  # maybeCcaBusy (:485-495): GetEnergyDuration (interference-helper.cc:171-190)
            noise, end = p.first_power, now
            for t, d in p.ni:
                noise += d
                end = t
                if end < now:
                    continue
                if noise < self.cca_w:
                    break
            cca = end - now if end > now else 0
            if cca:  # SwitchMaybeToCcaBusy (wifi-phy-state-helper.cc:404-423), in every state
                p.end_cca = max(p.end_cca, now + cca)
                p.c["cca_switches"] += 1
        if j in self.notify:
            self.notes.append((now, self.cur_uid, j, tx, kind, st, 0, rx_duration, cca))

    # ---- YansWifiPhy::EndReceive (:770-799)
    def end_receive(self, ev):
        p = self.phy[ev["phy"]]
        p.c["end"] += 1
        if ev["cancelled"]:  # EventImpl::Invoke skips a cancelled event; it is still dispatched
            p.c["end_cancelled"] += 1
            self.ends.append((self.now, self.cur_uid, ev["phy"], 0.0, 0.0, ev["tx"], wifi.END_CANCELLED, 0.0))
            self.end_refs.append(None)
            return
        snr, per, chunks = self.snr_per(p, ev["k"])
        self.ends.append((self.now, self.cur_uid, ev["phy"], snr, float(per), ev["tx"], 0, ev["w"]))
        self.end_refs.append((snr, per, chunks, ev["w"]))
        p.rxing = False  # NotifyRxEnd; SwitchFromRxEndOk / Error
        p.live = None

    def snr_per(self, p, k):
        return wifi_per_ref.snr_per(self.cfg.error_model, self.cfg.noise_figure_db, p.window, k, synced=p.locked,
                                    rxing_at=p.window_rxing)

    # ---- YansWifiPhy::SetChannelNumber (:327-374)
    def set_channel_number(self, j, nch, delay):
        p, now = self.phy[j], self.now
        st = p.state(now)
        rec = lambda outcome, retry=0: self.switches.append((now, self.cur_uid, j, outcome, st, retry))
        if now == 0:  # "this is not channel switch, this is initialization"
            self.chan[j] = p.channel = nch
            return rec(INIT)
        if st == SWITCHING:  # NS_ASSERT (!IsStateSwitching ())
            return rec(REFUSED)
        if st == TX:  # Simulator::Schedule (GetDelayUntilIdle (), &YansWifiPhy::SetChannelNumber, this, nch)
            d = p.delay_until_idle(now)
            uid = self._schedule(now + d, self.ctx, "retry", (j, nch, delay))
            self.retries.append((now + d, uid))
            return rec(POSTPONED, d)
        if st == RX:  # m_endRxEvent.Cancel (); SwitchToChannelSwitching's RX case
            p.live["cancelled"] = True
            p.live = None
            p.rxing = False
            p.end_rx = now
        if now < p.end_cca:
            p.end_cca = now
        p.start_sw, p.end_sw = now, now + delay
        if self.erase:
            p.ni, p.first_power = [], 0.0  # m_interference.EraseEvents ()
            p.window, p.locked, p.window_rxing = [], [], []
        p.switches += 1
        self.chan[j] = p.channel = nch
        rec(DONE)

    # ---- outputs, in the device's record layouts
    def log_arrays(self):
        a = np.array(self.log, np.uint64).reshape(-1, 3)
        return a[:, 0].copy(), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32)

    def end_records(self):
        return np.array(self.ends, dtype=wifi.WIFIL_END_DTYPE)

    def note_records(self):
        return np.array(self.notes, dtype=wifi.WIFIL_NOTE_DTYPE)

    def counters(self):
        out = np.zeros(len(self.phy), wifi.PHY_COUNTERS_DTYPE)
        for j, p in enumerate(self.phy):
            for f in COUNTERS:
                out[f][j] = p.c[f]
            out["end_tx"][j], out["end_rx"][j], out["end_cca_busy"][j] = p.end_tx, p.end_rx, p.end_cca
            out["first_power"][j], out["rxing"][j], out["ni_len"][j] = p.first_power, p.rxing, len(p.ni)
        return out

    def channel_records(self):
        return [dict(channel=p.channel, start_switching=p.start_sw, end_switching=p.end_sw, switches=p.switches,
                     drop_switching=p.drop_switching) for p in self.phy]


def run(phys, closures, stop_ns, mode=wifi.DSSS_1M, preamble=wifi.PREAMBLE_LONG, dbm=16.0206, notify=(), mob=None,
        erase=True):
    return Model(phys, mode, preamble, dbm, notify, mob, erase).run(closures, stop_ns)


def closures_of(sends, switches, size=200):
    """The oracle replay's setup order: every send (ts, phy) as its own closure, then every switch
    (ts, phy, nch, delay_ns) as its own closure."""
    return [(int(t), [("send", int(p), size)]) for t, p in sends] + \
           [(int(t), [("switch", int(p), int(c), int(d))]) for t, p, c, d in switches]


class StateHelper(wifi_note_model.StateHelper):
    """wifi_note_model.StateHelper with the SWITCHING state: GetState's rank (wifi-phy-state-helper.cc:159-183) and
    SwitchToChannelSwitching (:323-365) with the reference's NS_FATAL_ERROR / NS_ASSERT preconditions."""

    def __init__(self):
        super().__init__()
        self.start_sw = 0

    def get_state(self, now):
        if self.end_tx > now:
            return TX
        if self.rxing:
            return RX
        if self.end_sw > now:
            return SWITCHING
        return CCA_BUSY if self.end_cca > now else IDLE

    def delay_until_idle(self, now):
        if self.get_state(now) == SWITCHING:
            return max(self.end_sw - now, 0)
        return super().delay_until_idle(now)

    def switch_to_tx(self, now, dur):  # SendPacket's NS_ASSERT (... && !IsStateSwitching ()) (yans-wifi-phy.cc:508)
        self._need(self.get_state(now) != SWITCHING, "SendPacket: !IsStateSwitching")
        super().switch_to_tx(now, dur)

    def switch_to_channel_switching(self, now, dur):
        self.listener.append(("NotifySwitchingStart", now, dur))
        st = self.get_state(now)
        self._need(st not in (TX, SWITCHING), "SwitchToChannelSwitching: Invalid WifiPhy state")
        if st == RX:
            self.rxing = False
            self.state_log.append((self.start_rx, now - self.start_rx, RX))
            self.end_rx = now
        elif st == CCA_BUSY:
            s = self._cca_start()
            self.state_log.append((s, now - s, CCA_BUSY))
        else:
            self._log_idle_cca(now)
        if now < self.end_cca:
            self.end_cca = now
        self.state_log.append((now, dur, SWITCHING))
        self.prev_change = now
        self.start_sw = now
        self.end_sw = now + dur
        self._need(self.get_state(now) == SWITCHING, "SwitchToChannelSwitching: IsStateSwitching ()")

    def on_switch(self, now, dur):
        self.switch_to_channel_switching(now, dur)


def drive_state_helpers(m, delays):
    """One StateHelper per phy fed, in (ts, uid) order, with the model's stream — every phy notifying: its notes,
    its SendPackets, its DONE switches (delays: {(ts, uid): ChannelSwitchDelay}) and its end records — and checked
    against the model's probes.  Raises wifi_note_model.Precondition where the real class would assert."""
    ev = [(int(n[0]), int(n[1]), 1, n) for n in m.note_records()]
    ev += [(p[0], p[1], 0, p) for p in m.probes]
    ev += [(t[0], t[1], 2, (t[2], k)) for k, t in enumerate(m.txs)]
    ev += [(s[0], s[1], 2, s) for s in m.switches if s[3] == DONE]
    ev += [(int(e["ts"]), int(e["uid"]), 3, e) for e in m.end_records()]
    sizes = m.tx_sizes
    hs = [StateHelper() for _ in m.phy]
    # (a closure probes first, then acts, in the order of its actions: equal keys keep this list's order)
    order = sorted(range(len(ev)), key=lambda i: (ev[i][0], ev[i][1], ev[i][2]))
    for i in order:
        ts, _uid, what, arg = ev[i]
        if what == 1:
            hs[int(arg["phy"])].on_note(arg)
        elif what == 0:
            got = hs[arg[2]].get_state(ts)
            if got != arg[3]:
                raise wifi_note_model.Precondition(f"GetState of phy {arg[2]} at {ts}: helper {got}, model {arg[3]}")
        elif what == 2 and len(arg) == 2:
            hs[arg[0]].on_send(ts, int(wifi.tx_duration_ns(int(sizes[arg[1]]), *m.tx_frames[arg[1]][:2])))
        elif what == 2:
            hs[arg[2]].on_switch(ts, delays[(arg[0], arg[1])])
        else:
            hs[int(arg["phy"])].on_end(arg)
    return hs
