"""RxStart / CCA-busy notifications of the closed-loop Wi-Fi PHY (nsgpu_wifil_notify, nsgpu_wifil_note): the
device's stream against the plain-Python reference of tests/wifi_note_model.py (pinned to the oracle in
tests/test_wifi_notes_cpu.py).  Every field of a note is an integer, so the comparisons are exact.  The runs go
through the existing harness (wifi_loop_harness.run_gpu) with nsgpu.Sim replaced by a subclass that installs the
note handler, opts phys in and records what the MAC stand-in's closures see."""
import ctypes as C
import functools

import numpy as np
import pytest

import nsgpu
import nsref
import wifi
import wifi_loop_harness as harness
from test_wifi_notes_cpu import burst, burst_oracle, dense_scenario
from wifi_note_model import Precondition, drive_state_helpers, model_notes

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4
PHY_FIELDS = ("rx", "sync", "drop_rx", "drop_tx", "drop_ed", "cca_switches", "end", "end_cancelled", "ni_len",
              "end_tx", "end_rx", "end_cca_busy", "rxing")


class Rec:
    def __init__(self):
        self.notes, self.order, self.probes = [], [], []
        self.ctx_ok = True
        self.off_key = None


def run_with_notes(sc, notify, handler=True, off=None, **kw):
    """run_gpu with every phy of `notify` opted in.  handler: collect the delivered notes (checking Now / uid /
    context at each call) and the order of note and EndReceive handler calls; off = (phy, ts): the first attempt
    closure at or after ts opts phy out."""
    rec = Rec()
    node = sc["phys"].node

    class NoteSim(nsgpu.Sim):
        def attach_wifi(self, lp):
            super().attach_wifi(lp)

            def on_note(n):
                rec.notes.append(n)
                rec.order.append((0, int(n["ts"]), int(n["uid"])))
                rec.ctx_ok &= (self.now(), self.current_uid(), self.context()) == \
                    (int(n["ts"]), int(n["uid"]), int(node[int(n["phy"])]))

            if handler:
                self.wifi_set_note_handler(on_note)
            for p in notify:
                self.wifi_notify(int(p))

        def wifi_state(self, phy):
            st = super().wifi_state(phy)
            rec.probes.append((self.now(), self.current_uid(), phy, st[0]))
            if off is not None and rec.off_key is None and self.now() >= off[1]:
                self.wifi_notify(off[0], False)
                rec.off_key = (self.now(), self.current_uid())
            return st

        def wifi_set_end_handler(self, fn):
            def wrapped(e):
                rec.order.append((1, int(e["ts"]), int(e["uid"])))
                fn(e)
            super().wifi_set_end_handler(wrapped if fn else None)

    real = nsgpu.Sim
    nsgpu.Sim = NoteSim
    try:
        out = harness.run_gpu(sc, **kw)
    finally:
        nsgpu.Sim = real
    return out, rec


def equal_oracle(g, o, n):
    glog, gends, gphys, gtot = g[:4]
    olog, oends, ophys, otot = o
    for f in ("dispatched", "digest", "next_uid", "final_ts", "sends", "busy"):
        assert gtot[f] == otot[f], (f, gtot[f], otot[f])
    for a, b in zip(glog, olog):
        assert np.array_equal(a, b)
    for f in PHY_FIELDS:
        assert np.array_equal(gphys[f], ophys[f]), f
    for f in ("ts", "uid", "phy", "tx", "flags"):
        assert np.array_equal(gends[f], oends[f]), f
    np.testing.assert_allclose(gends["per"], oends["per"], rtol=1e-9, atol=1e-15)
    assert np.array_equal(harness.draws(gends, n), harness.draws(oends, n))


def same_notes(got, want):
    got = np.array(got, dtype=wifi.WIFIL_NOTE_DTYPE) if not isinstance(got, np.ndarray) else got
    assert len(got) == len(want), (len(got), len(want))
    for f in wifi.WIFIL_NOTE_DTYPE.names:
        assert np.array_equal(got[f], want[f]), f
    key = got["ts"].astype(object) * (1 << 32) + got["uid"]
    assert all(key[i] < key[i + 1] for i in range(len(key) - 1)), "(ts, uid) order"
    return got


def want_notes(sc, o, receivers):
    olog, oends, _ophys, otot = o
    return model_notes(sc["phys"], otot["txs"], olog, oends, receivers, sc["size"], sc["mode"], sc["preamble"],
                       sc["dbm"])[0]


def make(name):
    if name == "4x4":
        return harness.scenario()
    if name == "dense":
        return dense_scenario()
    sc = dense_scenario(80_000_000)  # "reply": the hand-back's MAC replies at Schedule (0)
    sc["reply_delay"] = 0
    return sc


@functools.lru_cache(maxsize=None)
def shared(name):
    """One device run, oracle run and model stream per scenario, shared by the tests below (read only)."""
    sc = make(name)
    o = harness.run_oracle(sc)
    g, rec = run_with_notes(sc, range(sc["phys"].n_phy))
    return sc, o, g, rec, want_notes(sc, o, range(sc["phys"].n_phy))


@pytest.mark.parametrize("name", ["4x4", "dense"])
def test_stream_equals_the_model(name):
    sc, o, g, rec, want = shared(name)
    got = same_notes(rec.notes, want)
    assert len(got) > 2000 and set(np.unique(got["kind"])) == {0, 1, 2, 3} and (got["cca_duration"] != 0).any()
    assert rec.ctx_ok, "Now () / uid / context at a handler call are the Receive event's"
    equal_oracle(g, o, sc["phys"].n_phy)
    assert len(g[4][1].read_notes()) == 0  # (delivered notes are consumed)


def test_handback_interleaving():
    sc, o, g, rec, want = shared("reply")
    same_notes(rec.notes, want)
    assert rec.ctx_ok
    equal_oracle(g, o, sc["phys"].n_phy)  # (the oracle's restated MAC, replies included)
    ends = [k for k in rec.order if k[0] == 1]
    assert len(ends) == g[3]["handbacks"] > 20
    # no note delivered after an EndReceive's handler call has a key below that EndReceive's
    later = (1 << 64, 0)
    for what, ts, uid in reversed(rec.order):
        if what == 0:
            later = min(later, (ts, uid))
        else:
            assert later > (ts, uid), (ts, uid, later)


@pytest.mark.parametrize("name", ["dense", "reply"])
def test_notes_drive_the_state_helper(name):
    sc, _o, g, rec, _want = shared(name)
    _glog, gends, gphys, gtot = g[:4]
    notes = np.array(rec.notes, dtype=wifi.WIFIL_NOTE_DTYPE)
    assert len(rec.probes) == gtot["sends"] + gtot["busy"] > 100
    try:
        hs = drive_state_helpers(sc["phys"].n_phy, notes, gtot["txs"], gends, sc["size"], sc["mode"], sc["preamble"],
                                 probes=rec.probes)
    except Precondition as e:
        pytest.fail(f"WifiPhyStateHelper precondition: {e}")
    for j, h in enumerate(hs):
        assert (h.end_tx, h.end_rx, h.end_cca, int(h.rxing)) == \
            (int(gphys["end_tx"][j]), int(gphys["end_rx"][j]), int(gphys["end_cca_busy"][j]), int(gphys["rxing"][j])), j
    calls = [c[0] for h in hs for c in h.listener]
    assert {"NotifyTxStart", "NotifyRxStart", "NotifyRxEndOk", "NotifyMaybeCcaBusyStart"} <= set(calls)


def test_staging_overflow_and_cancellation():
    """The burst replay: each wave emits 79-80 notes in one epoch (more than one staging block, the HBM Receive
    queue), and the 20 syncs are cancelled by the second wave's SendPackets."""
    b = burst()
    ph = b["phys"]
    olog, oends, ophys, otot = burst_oracle(b)
    want = model_notes(ph, otot["txs"], olog, oends, range(ph.n_phy), b["size"], b["mode"], b["preamble"], b["dbm"])[0]
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    got = []
    sim.wifi_set_note_handler(got.append)
    for p in range(ph.n_phy):
        sim.wifi_notify(p)
    for t, p in b["sends"]:
        sim.schedule(t, (lambda p=p: lambda: sim.wifi_send(p, b["size"], b["dbm"], b["mode"], b["preamble"]))())
    sim.stop(b["stop_ns"])
    sim.run()
    assert len(want) == 9900
    same_notes(got, want)
    assert sim.dispatched() == otot["dispatched"] and sim.next_uid() == otot["next_uid"]
    assert sim.host_stats()[2] == otot["digest"]
    gends, gphys = lp.read_ends(), lp.read_phys()
    for f in ("ts", "uid", "phy", "tx", "flags"):
        assert np.array_equal(gends[f], oends[f]), f
    assert len(gends) == 20 and ((gends["flags"] & wifi.END_CANCELLED) != 0).all()
    for f in PHY_FIELDS[:8]:
        assert np.array_equal(gphys[f], ophys[f]), f
    lp.close()


def test_subset_at_scale_100x100():
    """The 100x100 closed loop cut at Stop 0.02 s with 64 phys opted in and no handler: their notes (read back
    from the PHY) equal the model's, no other phy's appears, dispatch count and digest equal the oracle's."""
    x, y, z = wifi.grid(100, 100.0)
    phys = wifi.LoopPhys(x, y, z, tx_cap=1 << 20, rxq_cap=1024, ni_cap=1024)
    rng = np.random.default_rng(11)
    n, period = phys.n_phy, 1_000_000_000
    sc = dict(phys=phys, first=rng.integers(0, period // 2, n).astype(np.uint64),
              backoff=(100_000 + 37_000 * np.arange(n)).astype(np.uint64), period=period, stop_ns=20_000_000,
              size=1000, mode=wifi.DSSS_1M, preamble=wifi.PREAMBLE_LONG, dbm=16.0206 + 1.0)
    fixed = [0, 99, 9900, 9999, 5050]
    rest = np.setdiff1d(np.arange(n), fixed)
    chosen = sorted(fixed + [int(p) for p in np.random.default_rng(64).choice(rest, 59, replace=False)])
    assert len(set(chosen)) == 64
    o = harness.run_oracle(sc, log_cap=1 << 22)
    g, _rec = run_with_notes(sc, chosen, handler=False, log_cap=1 << 22)
    got = g[4][1].read_notes()
    assert set(np.unique(got["phy"])) <= set(chosen)
    want = want_notes(sc, o, chosen)
    assert len(want) > 64 * 250
    same_notes(got, want)
    assert g[3]["dispatched"] == o[3]["dispatched"] > 2_000_000 and g[3]["digest"] == o[3]["digest"]
    assert g[3]["sends"] == o[3]["sends"] == 317


def test_opt_in_only_and_opt_out():
    sc = dense_scenario()
    o = harness.run_oracle(sc)
    g, _rec = run_with_notes(sc, [], handler=False)
    assert len(g[4][1].read_notes()) == 0
    equal_oracle(g, o, sc["phys"].n_phy)
    # phy 14 opted out by the first attempt closure at or after 60 ms: its notes stop with that closure's epoch
    g, rec = run_with_notes(sc, [3, 14], off=(14, 60_000_000))
    equal_oracle(g, o, sc["phys"].n_phy)
    want = want_notes(sc, o, [3, 14])
    assert rec.off_key is not None
    keep = np.array([int(w["phy"]) == 3 or (int(w["ts"]), int(w["uid"])) < rec.off_key for w in want])
    assert 0 < np.count_nonzero(~keep) and np.count_nonzero(keep & (want["phy"] == 14)) > 0
    same_notes(rec.notes, want[keep])


def test_refusals():
    sc = harness.scenario(stop_ns=30_000_000)
    ph = sc["phys"]
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    sim.wifi_set_note_handler(lambda n: sim.schedule(1000, lambda: None))  # a handler must not schedule
    sim.wifi_notify(1)
    sim.schedule(1000, lambda: sim.wifi_send(0, 200, sc["dbm"], sc["mode"], sc["preamble"]))
    sim.stop(sc["stop_ns"])
    for _again in range(2):  # (sticky)
        with pytest.raises(nsgpu.NsgpuError, match=f"nsgpu error {ESTATE}:"):
            sim.run()
    L = nsgpu.lib()
    assert L.nsgpu_wifil_notify(lp.h, 0xffffffff, 1) == EINVAL
    assert L.nsgpu_wifil_notify(lp.h, ph.n_phy, 1) == EINVAL
    lp.close()
    grp = wifi.LoopPhy(ph, bounds=[0, 8, ph.n_phy])
    assert L.nsgpu_wifil_notify(grp.h, 0, 1) == ESTATE
    assert b"single-engine" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_notify(grp.h, 0xffffffff, 1) == EINVAL
    n = C.c_uint64(7)
    assert L.nsgpu_wifil_read_notes(grp.h, None, 0, C.byref(n)) == 0 and n.value == 0
    grp.close()
