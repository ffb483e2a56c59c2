"""tests/wifi_switch_model.py — the plain-Python restatement of the whole closed-loop PHY, with mobility and channel
switching — under an extended loss chain (nsgpu_wifil_set_loss): the reference of tests/test_gpu_lossx.py.

The subclass replaces one thing, the per-receiver power of send_packet: CalcRxPower is tests/loss_ref.py's float
restatement over the chain in force at the send, between the two phys at their positions of that send (after the
send's mobility updates).  Distances, delays, receivers, uids and contexts still come from the model's own path
(nsref.fanout_yans); with no extended chain in force so does the power.  One more closure action, ("loss", spec),
installs a chain at its place among the closure's actions: spec is (links, entries) — loss_ref links and Matrix
(a, b, loss_db) triples — or None for the config's chain again.  It names no phy, so the closure probes nothing for
it.  Every reception's power is kept (rx_powers) for the tests' threshold-margin check.  send_packet takes the frame's
mode, preamble and tx power per call, as wsm.Model.send_packet does (default: the model's own)."""
import numpy as np

import loss_ref
import mobility_ref
import nsref
import wifi
import wifi_switch_model as wsm


class Model(wsm.Model):
    def __init__(self, *a, lossx=None, **kw):
        super().__init__(*a, **kw)
        self.rx_powers = []  # (tx index, receiver, rxPowerW, the new-kind links' branches) of every Receive scheduled
        self.set_loss(lossx)

    def set_loss(self, spec):
        self.lx = None if spec is None else (list(spec[0]), loss_ref.matrix_of(spec[1]))

    NO_PHY = wsm.Model.NO_PHY + ("loss",)  # (("probe", phy) does nothing more than the closure's probe)

    def act(self, a):
        if a[0] == "loss":
            self.set_loss(a[1])
        else:
            super().act(a)

    # wsm.Model.send_packet with the power of the chain in force
    def send_packet(self, s, size, mode=None, preamble=None, dbm=None):
        mode, preamble, dbm = self.frame_of(mode, preamble, dbm)
        p, now = self.phy[s], self.now
        st = p.state(now)
        if st in (wsm.TX, wsm.SWITCHING):
            raise wsm.SendError(f"SendPacket of phy {s} at {now} in state {st}")
        dur = int(wifi.tx_duration_ns(int(size), mode, preamble))
        if st == wsm.RX:
            p.live["cancelled"] = True
            p.locked.remove(p.live["k"])
            p.live = None
            p.rxing = False
            p.end_rx = now
        p.end_tx = now + dur
        k = len(self.txs)
        self.txs.append((now, self.cur_uid, s))
        self.tx_sizes.append(int(size))
        self.tx_frames.append((mode, preamble, dbm))
        for j in mobility_ref.send_updates(self.chan, s):
            if j in self.mob:
                self.mob[j].update(now)
                self.x[j], self.y[j], self.z[j] = self.mob[j].position()
        fo = nsref.fanout_yans(self.x, self.y, self.z, self.chan, self.node, s, dbm, self.chain, self.cfg.speed,
                               now, self.uid)
        pos = lambda i: (float(self.x[i]), float(self.y[i]), float(self.z[i]))
        for r in fo:
            j, taken = int(r["phy"]), []
            if self.lx is None:
                rx_dbm = float(r["rx_dbm"])
            else:  # PropagationLossModel::CalcRxPower (txPowerDbm, senderMobility, receiverMobility)
                rx_dbm = loss_ref.calc(self.lx[0], self.lx[1], s, j, pos(s), pos(j), dbm, taken)
            w = wsm._dbm_to_w(rx_dbm + self.cfg.rx_gain_db)
            self.rx_powers.append((k, j, w, tuple(taken)))
            uid = self._schedule(int(r["ts"]), int(r["context"]), "rx", (j, k, w, dur))
            assert uid == int(r["uid"])


def run(phys, closures, stop_ns, mode=wifi.DSSS_1M, preamble=wifi.PREAMBLE_LONG, dbm=16.0206, notify=(), mob=None,
        lossx=None):
    return Model(phys, mode, preamble, dbm, notify, mob, lossx=lossx).run(closures, stop_ns)


def clear_of_thresholds(m, rel=1e-6):
    """No reception's power within `rel` of the ED or the CCA threshold (the discrete results are then the same
    whichever way the power's last bits round); returns the closest relative distance seen."""
    closest = np.inf
    for k, j, w, _taken in m.rx_powers:
        for thr in (m.ed_w, m.cca_w):
            d = abs(w - thr) / thr
            closest = min(closest, d)
            assert d > rel, (k, j, w, thr)
    return closest
