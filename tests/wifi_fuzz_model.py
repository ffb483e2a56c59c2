"""tests/lossx_model.py — the plain-Python closed-loop PHY with switching, mobility and the extended loss chain — driven
with everything at once: the reference of tests/test_gpu_wifi_fuzz.py (the scenarios: tests/wifi_fuzz_cases.py), held to
the C++ oracle and checked on its own in tests/test_wifi_fuzz_cpu.py.

What it adds to the model it wraps:

Closure actions (each names a phy, so its closure probes that phy first, as for every such action):
  ("attempt", phy, size, mode, preamble, dbm): SendPacket of that frame unless the phy is TX or SWITCHING (where
    yans-wifi-phy.cc:508 asserts); then the attempt is recorded as held.  A send in RX cancels the reception, as
    SendPacket does; one in CCA_BUSY goes ahead.  Every schedule of attempts is therefore legal.
  ("velocity", phy, vel) ("pause", phy, on) ("position", phy, pos) ("add_waypoint", phy, t, pos)
  ("end_waypoints", phy) ("accel", phy, vel, acc): the call of the phy's mobility_ref.CvModel /
    waypoint_ref.WaypointModel / AccelModel at the closure's time; ("position", ...) of a phy without a model moves it.

The hand-back (YansWifiPhy::EndReceive's host part, yans-wifi-phy.cc:783-797): at every EndReceive of a listened phy that
is not cancelled the model draws the phy's next value of wifi_loop_harness.draws' sequence and, if the draw exceeds the
reference per, calls Simulator::Schedule (delay, attempt of that phy) with the phy's reply frame — one more closure, in
the EndReceive's context (Schedule keeps the current one), with m_uid of that moment.  Every (draw, per) is kept.

Records beyond the wrapped model's: attempts (ts, uid, phy, sent, state, reply), handbacks (ts, uid, phy), draws
(end index, phy, k, draw, per), cancels (ts, uid, phy, "send" | "switch", the cancelled frame's tx), actions (ts, uid,
the action) of every loss and course action, end_mix (what was on the air during each frame received), and the
high-water marks the engine's capacities are checked against."""
import math

import lossx_model
import wifi_per_ref
import wifi_switch_model as wsm

COURSE = ("velocity", "pause", "position", "add_waypoint", "end_waypoints", "accel")
GOLDEN = 0.6180339887498949
_SNR_PER = {}


def draw(j, k):
    """wifi_loop_harness.draws: phy j's k-th draw (k from 0), a fixed value."""
    return ((k + 1) * GOLDEN + j * 0.1) % 1.0


class Model(lossx_model.Model):
    def __init__(self, *a, listen=(), reply=None, flip=(), remode=None, **kw):
        """listen: the phys handed back.  reply: {phy: (delay_ns, size, mode, preamble, dbm)} (a listened phy without
        an entry draws and never replies).  The two mutations tests/test_wifi_fuzz_cpu.py needs — flip: ordinals of
        the draws whose outcome is inverted; remode: {tx index: (mode, preamble)} the frame is taken for at its
        receivers' CalculateSnrPer (its duration stays)."""
        super().__init__(*a, **kw)
        self.listen, self.reply = set(listen), dict(reply or {})
        self.flip, self.remode = set(flip), dict(remode or {})
        self.ndraw = [0] * len(self.phy)
        self.attempts, self.handbacks, self.draws, self.cancels, self.actions = [], [], [], [], []
        self.end_mix = []  # per end record: None, or (interference changes inside the frame, the interferers'
        #                    distinct (mode, preamble) pairs, the same with the frame's own)
        self.end_inputs = []  # per end record: None, or CalculateSnrPer's inputs (the window, m_rxing at each, k)
        self.pending_ends = [0] * len(self.phy)  # EndReceive events scheduled and not yet dispatched (LPE_CAP)
        self.pending_rx = [0] * len(self.phy)    # Receive events likewise (rxq_cap)
        self.max_pending_ends = self.max_pending_rx = self.max_ni = 0

    # ---- the bookkeeping around the wrapped model's events
    def _schedule(self, ts, ctx, kind, arg):
        if kind == "rx":
            self.pending_rx[arg[0]] += 1
            self.max_pending_rx = max(self.max_pending_rx, self.pending_rx[arg[0]])
        elif kind == "end":
            self.pending_ends[arg["phy"]] += 1
            self.max_pending_ends = max(self.max_pending_ends, self.pending_ends[arg["phy"]])
        return super()._schedule(ts, ctx, kind, arg)

    def start_receive(self, j, tx, w, dur):
        self.pending_rx[j] -= 1
        super().start_receive(j, tx, w, dur)
        if tx in self.remode:
            p = self.phy[j]
            p.window[-1] = p.window[-1][:3] + tuple(self.remode[tx])
        self.max_ni = max(self.max_ni, len(self.phy[j].ni))

    def _cancelling(self, j, cause, call):
        p = self.phy[j]
        live = p.live if p.state(self.now) == wsm.RX else None
        call()
        if live is not None and live["cancelled"]:
            self.cancels.append((self.now, self.cur_uid, j, cause, live["tx"]))

    def send_packet(self, s, size, mode=None, preamble=None, dbm=None):
        self._cancelling(s, "send", lambda: super(Model, self).send_packet(s, size, mode, preamble, dbm))

    def set_channel_number(self, j, nch, delay):
        self._cancelling(j, "switch", lambda: super(Model, self).set_channel_number(j, nch, delay))

    # ---- the new actions
    def act(self, a):
        if a[0] == "attempt":
            self.attempt(*a[1:])
        elif a[0] == "reply":  # an attempt the hand-back scheduled: the same rule, marked in the attempts' records
            self.attempt(*a[1:], reply=True)
        elif a[0] in COURSE:
            self.course(a)
        else:
            if a[0] == "loss":
                self.actions.append((self.now, self.cur_uid, a))
            super().act(a)

    def attempt(self, j, size, mode, preamble, dbm, reply=False):
        st = self.phy[j].state(self.now)
        sent = st not in (wsm.TX, wsm.SWITCHING)
        self.attempts.append((self.now, self.cur_uid, j, sent, st, reply))
        if sent:
            self.send_packet(j, size, mode, preamble, dbm)

    def course(self, a):
        kind, j, now = a[0], a[1], self.now
        self.actions.append((now, self.cur_uid, a))
        m = self.mob.get(j)
        if kind == "velocity":
            m.set_velocity(now, a[2])
        elif kind == "pause":
            m.pause(now, a[2])
        elif kind == "position":
            if m is None:  # MobilityModel::SetPosition of a constant-position phy
                self.x[j], self.y[j], self.z[j] = a[2]
                return
            m.set_position(now, a[2])
        elif kind == "add_waypoint":
            m.add_waypoint(a[2], a[3])
        elif kind == "end_waypoints":
            m.end()
        else:
            m.set_velocity_and_acceleration(now, a[2], a[3])
        self.x[j], self.y[j], self.z[j] = m.position()

    def snr_per(self, p, k):
        """The wrapped model's, remembered by its inputs: the runs of one case (the placements of
        tests/wifi_fuzz_cases.py, the controls and pipelines of the tests) repeat most of them."""
        key = (self.cfg.error_model, self.cfg.noise_figure_db, k, tuple(p.window), tuple(p.window_rxing))
        if key not in _SNR_PER:
            _SNR_PER[key] = super().snr_per(p, k)
        return _SNR_PER[key]

    # ---- YansWifiPhy::EndReceive's host part
    def end_receive(self, ev):
        j = ev["phy"]
        self.pending_ends[j] -= 1
        mix = None
        if not ev["cancelled"]:  # the frames on the air during this one: interference changes inside it, their kinds
            w = self.phy[j].window
            start, end = w[ev["k"]][:2]
            others = [e for i, e in enumerate(w) if i != ev["k"] and e[0] < end and e[1] > start]
            changes = sum((start < e[0] < end) + (start < e[1] < end) for e in others)
            mix = (changes, len({e[3:] for e in others}), len({e[3:] for e in others + [w[ev["k"]]]}))
        self.end_mix.append(mix)
        self.end_inputs.append(None if ev["cancelled"] else (tuple(self.phy[j].window), tuple(self.phy[j].window_rxing),
                                                             ev["k"]))
        super().end_receive(ev)
        if ev["cancelled"] or j not in self.listen:
            return
        self.handbacks.append((self.now, self.cur_uid, j))
        per = self.end_refs[-1][1]
        self.mac(j, len(self.ends) - 1, per)

    def mac(self, j, end_index, per):
        """m_random.GetValue () > per (:783), then the MAC's receive callback: the reply rule."""
        u = draw(j, self.ndraw[j])
        self.draws.append((end_index, j, self.ndraw[j], u, per))
        self.ndraw[j] += 1
        ok = u > per
        if len(self.draws) - 1 in self.flip:
            ok = not ok
        if ok and j in self.reply:
            delay, size, mode, preamble, dbm = self.reply[j]
            self.call_later(delay, [("reply", j, size, mode, preamble, dbm)])

    def call_later(self, delay, actions):
        """Simulator::Schedule (delay, ...) from the running event: its context stays."""
        return self._schedule(self.now + int(delay), self.ctx, "closure", list(actions))


def per_under_more_noise(m, i, rel):
    """End record i's reference per with the noise floor raised by `rel` (relative): what a constant added to the
    noise of every chunk — m_firstPower off by that much — does to it."""
    window, rxing, k = m.end_inputs[i]
    nf = m.cfg.noise_figure_db + 10.0 * math.log10(1.0 + rel)
    return wifi_per_ref.snr_per(m.cfg.error_model, nf, list(window), k, rxing_at=rxing)[1]


def run(case, stop=None, **kw):
    """One case of tests/wifi_fuzz_cases.py (or any dict of its form) on the model; stop: an earlier Stop."""
    args = dict(notify=case["notify"], mob=case["mob"]() if case["mob"] else None, lossx=case["lossx"],
                listen=case["listen"], reply=case["reply"])
    args.update(kw)
    return Model(case["phys"], *case["frame"], **args).run(case["closures"], case["stop"] if stop is None else stop)


def final_reads(m, stop):
    """Every mobility model's read at the stop time, as the device's get_mobility / get_waypoints / get_acceleration
    return it (mobility_cases.read_final)."""
    return {j: mm.get(stop) for j, mm in sorted(m.mob.items())}
