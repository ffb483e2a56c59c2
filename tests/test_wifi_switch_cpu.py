"""Channel switching of the closed-loop Wi-Fi PHY (nsgpu_wifil_set_channel): the plain-Python restatement
tests/wifi_switch_model.py held to the unchanged C++ oracle where the oracle can follow (no switch, a switch at ts 0,
a switch on a quiet medium) and to hand-built branch cases where it cannot (it has no SWITCHING state);
tests/test_gpu_wifi_switch.py then holds the device to the model.  The scenarios below are shared with that file.

snr / per against the oracle: the comparison tests/test_wifi_per_cpu.py makes (rx_w ==, snr within 1e-15, per within
wifi_per_ref.psr_bound at K_CPU); everything else is compared exactly."""
import ctypes
import math
import os

import numpy as np
import pytest

import nsref
import wifi
import wifi_note_model
import wifi_per_ref as ref
import wifi_switch_model as wsm
from test_wifi_per_cpu import K_CPU
from wifi_per_ref import mpf

SIZE, DBM, MODE, PREAMBLE = 200, 16.0206, wifi.DSSS_1M, wifi.PREAMBLE_LONG
DUR = int(wifi.tx_duration_ns(SIZE, MODE, PREAMBLE))  # 1 792 000 ns
DELAY = 250_000  # ChannelSwitchDelay's default (yans-wifi-phy.cc: MicroSeconds (250))
IDLE, RX, TX, CCA_BUSY, SWITCHING = wsm.IDLE, wsm.RX, wsm.TX, wsm.CCA_BUSY, wsm.SWITCHING
END_FIELDS = ("ts", "uid", "phy", "tx", "flags")


def phys_of(x, y, z, channel):
    return wifi.LoopPhys(x, y, z, channel=np.asarray(channel, np.uint32), tx_cap=1024)


def run_model(case, **kw):
    return wsm.run(case["phys"], case["closures"], case["stop"], MODE, PREAMBLE, DBM, **kw)


def run_oracle(phys, sends, stop, moves=()):
    ts = np.array([t for t, _p in sends], np.uint64)
    phy = np.array([p for _t, p in sends], np.uint32)
    return nsref.wifil_replay(phys.c_struct(), ts, phy, np.full(len(ts), SIZE, np.uint32), MODE, PREAMBLE, DBM, stop,
                              phys.n_phy, wifi.WIFIL_END_DTYPE, wifi.PHY_COUNTERS_DTYPE, moves=moves)


def noop_move(phys, t, j):
    """MobilityModel::SetPosition of phy j to its own position: holds the closure's uid and log slot."""
    return (int(t), int(j), (float(phys.x[j]), float(phys.y[j]), float(phys.z[j])))


def equal_oracle(m, o, state_fields=()):  # (the oracle reports the counters alone)
    (lts, luid, lctx), oends, ophys, otot = o
    mts, muid, mctx = m.log_arrays()
    assert otot["dispatched"] == len(mts) and otot["next_uid"] == m.uid
    assert np.array_equal(mts, lts) and np.array_equal(muid, luid) and np.array_equal(mctx, lctx)
    mc = m.counters()
    for f in wsm.COUNTERS + tuple(state_fields):
        assert np.array_equal(mc[f], ophys[f]), f
    mends = m.end_records()
    assert len(mends) == len(oends)
    for f in END_FIELDS:
        assert np.array_equal(mends[f], oends[f]), f
    for e, r in zip(oends, m.end_refs):
        if r is None:
            assert int(e["flags"]) & wifi.END_CANCELLED and e["snr"] == 0.0 and e["per"] == 0.0
            continue
        snr, per, chunks, rx_w = r
        assert e["rx_w"] == rx_w and math.isclose(e["snr"], snr, rel_tol=1e-15)
        assert abs(mpf(float(e["per"])) - per) <= ref.psr_bound(chunks, 1 - per, K_CPU), (int(e["phy"]), float(per))


# ---------------------------------------------------------------- the scenarios
def grid_sends(rng, n, n_phy, first=2_000_000, lo=300_000, hi=2_500_000, skip=()):
    """n sends at irregular ns times, senders 5 k mod n_phy (a phy sends again 16 sends later: never while TX)."""
    ts = first + np.cumsum(rng.integers(lo, hi, n))
    out = [(int(ts[k]), 5 * k % n_phy) for k in range(n)]
    return [s for s in out if s[1] not in skip]


def two_channel_case(seed=11):
    x, y, z = wifi.grid(4, 60.0)
    ph = phys_of(x, y, z, [1, 6] * 8)
    sends = grid_sends(np.random.default_rng(seed), 36, 16)
    return dict(phys=ph, sends=sends, switches=[], closures=wsm.closures_of(sends, [], SIZE), stop=sends[-1][0] + 5_000_000)


def quiet_case(seed=12):
    """Phy 7 alone on channel 11 switches to 6 at T; channel 6 is silent until T + DELAY; 7 itself sends later."""
    x, y, z = wifi.grid(4, 60.0)
    chan = np.array([1, 6] * 8, np.uint32)
    chan[7] = 11
    rng = np.random.default_rng(seed)
    T = 30_000_000
    early = [s for s in grid_sends(rng, 24, 16, skip=(7,)) if chan[s[1]] == 1 and s[0] < T + DELAY]
    late = grid_sends(rng, 30, 16, first=T + DELAY + 1_000)
    sends = early + late
    assert any(p == 7 for _t, p in late) and any(chan[p] == 6 for _t, p in late) and len(early) >= 4
    sw = [(T, 7, 6, DELAY)]
    return dict(phys=phys_of(x, y, z, chan), sends=sends, switches=sw, closures=wsm.closures_of(sends, sw, SIZE),
                stop=sends[-1][0] + 5_000_000, T=T)


# The branch cases: a line of phys — 0 (ch 1, x 0), 1 (ch 1, x 60), 2 (ch 6, x 120), 3 (ch 1, x 240: 180 m from 1, whose
# frames reach 1 between the CCA and the ED threshold), 4 (ch 6, 60 m above 1), 5 (ch 11, far away, alone).
LINE_X = (0.0, 60.0, 120.0, 240.0, 60.0, 2000.0)
LINE_Y = (0.0, 0.0, 0.0, 0.0, 60.0, 0.0)
LINE_CH = (1, 1, 6, 1, 6, 11)
T0 = 3_000_000
BRANCHES = {
    # name: (sends [(ts, phy)], switches [(ts, phy, nch, delay)])
    "idle": ([(T0 + 4_000_000, 0)], [(T0, 1, 6, DELAY)]),
    "cca_busy": ([(T0, 3)], [(T0 + 500_000, 1, 6, DELAY)]),
    "rx": ([(T0, 0)], [(T0 + 500_000, 1, 6, DELAY)]),
    "tx": ([(T0, 0), (T0 + 4_000_000, 2)], [(T0 + 300_000, 0, 6, DELAY)]),
    "while_switching": ([], [(T0, 1, 6, DELAY), (T0 + 100_000, 1, 11, DELAY)]),
    "rx_inside_switching": ([(T0 + 1_000_000, 2)], [(T0, 1, 6, 5_000_000)]),
    "rx_outlasts_switching": ([(T0 + 100_000, 2)], [(T0, 1, 6, DELAY)]),
    "in_flight": ([(T0, 0)], [(T0 + 100, 1, 6, DELAY)]),
    "erase": ([(T0, 3), (T0 + 600_000, 4)], [(T0 + 200_000, 1, 6, DELAY)]),
    "send_while_switching": ([(T0 + 100_000, 1)], [(T0, 1, 6, DELAY)]),
}


def branch_case(name):
    sends, sw = BRANCHES[name]
    ph = phys_of(np.array(LINE_X), np.array(LINE_Y), np.zeros(6), LINE_CH)
    last = max([t for t, _p in sends] + [s[0] + s[3] for s in sw])
    return dict(phys=ph, sends=sends, switches=sw, closures=wsm.closures_of(sends, sw, SIZE), stop=last + 10_000_000)


def grid_switch_case():
    """The 4x4 grid (60 m pitch) on channels 1 / 6 / 11, 40 sends 4 ms apart (senders 5 k mod 16) and 11 switch
    calls placed around chosen sends so that every branch of BRANCHES but the SendPacket error is taken; the tests
    assert from the model that they are (branch_coverage)."""
    x, y, z = wifi.grid(4, 60.0)
    chan = np.array([(1, 6, 11)[j % 3] for j in range(16)], np.uint32)
    ph = phys_of(x, y, z, chan)
    chain = nsref.loss_chain(*ph.loss)
    cur = chan.copy()
    ed, cca = ph.ed - ph.rx_gain_db, ph.cca - ph.rx_gain_db
    sends = [(2_000_000 + 4_000_000 * k + 1_237 * k, 5 * k % 16) for k in range(40)]

    def hears(k, lo, hi=1e9, same=True):
        """A phy that would receive send k's frame with rx_dbm in [lo, hi) were it on the sender's channel; same: one
        that is on it."""
        t, s = sends[k]
        one = np.full(16, cur[s], np.uint32)
        fo = nsref.fanout_yans(x, y, z, one, ph.node, s, DBM, chain, ph.speed, t, 0)
        for r in fo:
            j = int(r["phy"])
            busy = {sends[q][1] for q in range(max(k - 1, 0), min(k + 3, 40))}
            if lo <= r["rx_dbm"] < hi and same in (None, cur[j] == cur[s]) and j not in busy and j not in used:
                used.add(j)
                return j
        raise AssertionError(("no phy", k, lo, hi, same))

    used, sw = set(), []
    other = lambda c: {1: 6, 6: 11, 11: 1}[int(c)]

    def switch(t, j, nch, delay=DELAY):
        sw.append((t, j, int(nch), delay))

    def done(j, nch):
        cur[j] = nch

    t, s = sends[2]   # from RX
    j = hears(2, ed)
    switch(t + 500_000, j, other(cur[j])), done(j, other(cur[j]))
    t, s = sends[5]   # from TX: postponed to m_endTx
    switch(t + 300_000, s, other(cur[s])), done(s, other(cur[s]))
    t, s = sends[8]   # from CCA_BUSY
    j = hears(8, cca, ed)
    switch(t + 500_000, j, other(cur[j])), done(j, other(cur[j]))
    t, s = sends[11]  # from IDLE, and a second call while SWITCHING: refused
    j = hears(11, -1e9, same=None)  # (3 ms after the send the medium is quiet again)
    switch(t + 3_000_000, j, other(cur[j])), switch(t + 3_100_000, j, 1)
    done(j, other(cur[j]))
    t, s = sends[14]  # a 5 ms switch onto the sender's channel just before it sends: the frame ends inside it
    j = hears(14, cca, same=False)
    switch(t - 1_000_000, j, cur[s], 5_000_000), done(j, cur[s])
    t, s = sends[17]  # a 250 us switch onto the sender's channel: the frame outlasts it
    j = hears(17, cca, same=False)
    switch(t - 100_000, j, cur[s]), done(j, cur[s])
    t, s = sends[20]  # the receiver leaves between the send and its Receive
    j = hears(20, ed)
    switch(t + 100, j, other(cur[j])), done(j, other(cur[j]))
    t, s = sends[26]  # and back, onto busy channels
    for q in (hears(26, ed), hears(26, cca, same=False)):
        switch(t + 2_200_000, q, cur[s] if cur[q] != cur[s] else other(cur[q]))
    return dict(phys=ph, sends=sends, switches=sw, closures=wsm.closures_of(sends, sw, SIZE),
                stop=sends[-1][0] + 6_000_000)


def big_grid_case():
    """18 x 18 phys (324: two 256-thread blocks of k_wl_rechan / k_wl_rx / k_wl_send, the second partial; six waves),
    60 m pitch, channels 1 / 6 / 11; ten sends and six switch calls: phy 3 (first block), 300 (last block) and 323
    (the last of the list) switch, two of them while receiving, and later sends reach them on their new channels."""
    i = np.arange(324)
    x, y, z = (i % 18) * 60.0, (i // 18) * 60.0, np.zeros(324)
    chan = np.array([(1, 6, 11)[j % 3] for j in range(324)], np.uint32)
    # (2 -> 3, 282 -> 300, 305 -> 323 before the switches; 301 -> 300, 322 -> 323, 4 -> 3 after them: 60 m each)
    senders = (2, 160, 282, 305, 100, 305, 21, 301, 322, 4)
    sends = [(2_000_000 + 4_000_000 * k + 997 * k, s) for k, s in enumerate(senders)]
    sw = [(1_000_000, 3, int(chan[2]), DELAY),            # idle, onto phy 2's channel before phy 2 sends
          (sends[2][0] + 500_000, 300, int(chan[301]), DELAY),  # while receiving phy 282's frame
          (sends[3][0] + 500_000, 323, int(chan[322]), DELAY),  # while receiving phy 305's frame
          (sends[3][0] + 600_000, 323, 1, DELAY),          # refused: still switching
          (sends[5][0] + 300_000, 305, int(chan[4]), DELAY),  # the sender itself: postponed
          (sends[6][0] + 3_000_000, 3, int(chan[4]), DELAY)]
    return dict(phys=phys_of(x, y, z, chan), sends=sends, switches=sw, closures=wsm.closures_of(sends, sw, SIZE),
                stop=sends[-1][0] + 6_000_000)


def burst_case():
    """One closure makes ten SendPackets (more than NSEND = 8: the batch flushes once on its own) from phys 0 .. 9 of a
    one-channel 4 x 4 grid and then switches phy 12 to channel 6: the ten frames are in flight to phy 12, which they
    reach while it is SWITCHING; phy 13's later frame no longer does.  Phy 12 then sends, alone on channel 6."""
    x, y, z = wifi.grid(4, 60.0)
    t0 = 5_000_000
    first = (t0, [("send", p, SIZE) for p in range(10)] + [("switch", 12, 6, DELAY)])
    closures = [first, (t0 + 6_000_000, [("send", 13, SIZE)]), (t0 + 9_000_000, [("send", 12, SIZE)])]
    return dict(phys=phys_of(x, y, z, np.ones(16, np.uint32)), closures=closures, stop=t0 + 15_000_000)


MOBILE = {1: (20.0, -15.0, 0.0), 6: (-25.0, 10.0, 1.0), 12: (12.5, 30.0, 0.0)}  # phy: velocity m/s (grid_switch_case)


def mobile_models(ph):
    import mobility_ref
    return {j: mobility_ref.CvModel((ph.x[j], ph.y[j], ph.z[j]), v, paused=False, last_update=0) for j, v in MOBILE.items()}


def branch_coverage(m):
    """Which branches a model run took."""
    sw, notes, ends = m.switches, m.note_records(), m.end_records()
    got = set()
    for ts, uid, j, outcome, prev, retry in sw:
        if outcome == wsm.DONE:
            got.add(("done", prev))
        elif outcome == wsm.POSTPONED:
            got.add("postponed")
        elif outcome == wsm.REFUSED:
            got.add("refused")
    for n in notes[notes["kind"] == wsm.NOTE_DROP_SWITCHING]:
        got.add("switching_drop_cca" if n["cca_duration"] else "switching_drop_quiet")
    done = [(s[0], s[2]) for s in sw if s[3] == wsm.DONE]
    for e in ends:
        if int(e["flags"]) & wifi.END_CANCELLED and any(t < int(e["ts"]) < t + DUR and j == int(e["phy"]) for t, j in done) \
                and not any(t[2] == int(e["phy"]) and t[0] < int(e["ts"]) < t[0] + DUR for t in m.txs):
            got.add("rx_cancelled_by_switch")
    for (rt, ruid) in m.retries:
        got.add("retry_dispatched" if (rt, ruid, wsm.NO_CONTEXT) in m.log else "retry_pending")
    return got


ALL_BRANCHES = {("done", IDLE), ("done", CCA_BUSY), ("done", RX), "postponed", "refused", "switching_drop_cca",
                "switching_drop_quiet", "rx_cancelled_by_switch", "retry_dispatched"}


# ---------------------------------------------------------------- 1-3: against the oracle
def test_no_switches_equals_the_oracle():
    c = two_channel_case()
    m = run_model(c)
    o = run_oracle(c["phys"], c["sends"], c["stop"])
    equal_oracle(m, o)
    ends = m.end_records()
    assert len(ends) > 60 and np.count_nonzero(ends["flags"]) >= 1 and m.counters()["drop_rx"].sum() > 0


def test_switch_at_ts_0_is_initialisation():
    c = two_channel_case()
    sw = [(0, 5, 1, DELAY), (0, 10, 6, DELAY)]  # (phy 5: 6 -> 1, phy 10: 1 -> 6)
    c["closures"] = wsm.closures_of(c["sends"], sw, SIZE)
    m = run_model(c)
    assert [s[3] for s in m.switches] == [wsm.INIT, wsm.INIT] and all(p.switches == 0 and p.end_sw == 0 for p in m.phy)
    chan = np.array(c["phys"].channel)
    chan[5], chan[10] = 1, 6
    ph = phys_of(c["phys"].x, c["phys"].y, c["phys"].z, chan)
    o = run_oracle(ph, c["sends"], c["stop"], moves=[noop_move(ph, 0, 5), noop_move(ph, 0, 10)])
    equal_oracle(m, o)
    assert [r["channel"] for r in m.channel_records()] == list(chan)


def test_quiet_medium_switch_equals_the_oracle_on_the_new_channel():
    c = quiet_case()
    m = run_model(c)
    assert [s[3:5] for s in m.switches] == [(wsm.DONE, IDLE)]
    chan = np.array(c["phys"].channel)
    chan[7] = 6
    ph = phys_of(c["phys"].x, c["phys"].y, c["phys"].z, chan)
    o = run_oracle(ph, c["sends"], c["stop"], moves=[noop_move(ph, c["T"], 7)])
    equal_oracle(m, o)
    # phy 7 sits mid-list: the channel-6 phys after it take later uids than without it
    ends7 = m.end_records()
    assert np.count_nonzero(ends7["phy"] == 7) >= 3 and m.phy[7].c["sync"] >= 3


# ---------------------------------------------------------------- 4: the branches
def branch(name, **kw):
    c = branch_case(name)
    m = wsm.run(c["phys"], c["closures"], c["stop"], MODE, PREAMBLE, DBM, notify=range(6), **kw)
    return c, m


def log_has(m, ts, uid):
    return any(e[0] == ts and e[1] == uid for e in m.log)


def test_branch_switch_from_idle():
    c, m = branch("idle")
    assert m.switches == [(T0, m.switches[0][1], 1, wsm.DONE, IDLE, 0)]
    p = m.phy[1]
    assert (p.channel, p.start_sw, p.end_sw, p.switches) == (6, T0, T0 + DELAY, 1)
    assert p.state(T0) == SWITCHING and p.delay_until_idle(T0 + 1) == DELAY - 1 and p.state(T0 + DELAY) == IDLE
    assert p.c["rx"] == 0 and m.phy[3].c["rx"] == 1  # phy 0's later frame no longer reaches phy 1; phy 3 takes uid + 0
    rx3 = [e for e in m.log if e[2] == 3]
    assert rx3[0][1] == m.txs[0][1] + 3  # (4 sends + switches + Stop scheduled first: the closure's uid, then m_uid)


def test_branch_switch_from_cca_busy_trims_end_cca_busy():
    c, m = branch("cca_busy")
    n = m.note_records()
    mine = n[n["phy"] == 1]
    assert len(mine) == 1 and mine[0]["kind"] == wifi.NOTE_DROP_ED and mine[0]["cca_duration"] > 500_000
    assert [s[3:5] for s in m.switches] == [(wsm.DONE, CCA_BUSY)]
    assert m.phy[1].end_cca == T0 + 500_000 and m.counters()["end_cca_busy"][1] == T0 + 500_000


def test_branch_switch_from_rx_cancels_the_end_receive():
    c, m = branch("rx")
    assert [s[3:5] for s in m.switches] == [(wsm.DONE, RX)]
    ends = m.end_records()
    e1 = ends[ends["phy"] == 1]
    assert len(e1) == 1 and e1[0]["flags"] == wifi.END_CANCELLED and e1[0]["snr"] == 0.0 and e1[0]["rx_w"] == 0.0
    assert int(e1[0]["ts"]) > T0 + 500_000 and log_has(m, int(e1[0]["ts"]), int(e1[0]["uid"]))  # still dispatched
    p = m.phy[1]
    assert (p.end_rx, p.rxing, p.c["end_cancelled"], p.c["end"]) == (T0 + 500_000, False, 1, 1)
    assert m.end_refs[list(ends["phy"]).index(1)] is None


def test_branch_switch_from_tx_is_postponed_to_end_tx():
    c, m = branch("tx")
    first, retry = m.switches
    assert first[3:] == (wsm.POSTPONED, TX, DUR - 300_000)
    assert (retry[0], retry[3], retry[4]) == (T0 + DUR, wsm.DONE, IDLE)
    # the retry took exactly one uid: 4 setup events (uids 4-7), phy 0's two Receives (phys 1 and 3: 8, 9), phy 1's
    # EndReceive (10), then the retry
    assert m.retries == [(T0 + DUR, retry[1])] and m.txs[0][1] == 4 and retry[1] == 11
    assert log_has(m, T0 + DUR, retry[1])
    # the frame sent before the sender switched still ends at its receivers, on the old channel, with an snr
    ends = m.end_records()
    e1 = ends[ends["phy"] == 1][0]
    assert int(e1["ts"]) > T0 + DUR and e1["flags"] == 0 and e1["snr"] > 1.0 and e1["uid"] == 10
    # phy 0 is on channel 6 afterwards: phy 2's later frame reaches it
    assert m.phy[0].channel == 6 and m.phy[0].c["rx"] == 1 and m.phy[0].c["sync"] == 1


def test_branch_switch_while_switching_is_refused():
    c, m = branch("while_switching")
    assert [s[3:5] for s in m.switches] == [(wsm.DONE, IDLE), (wsm.REFUSED, SWITCHING)]
    assert m.phy[1].channel == 6 and m.phy[1].end_sw == T0 + DELAY and m.phy[1].switches == 1


def test_branch_receive_that_ends_inside_the_switch():
    c, m = branch("rx_inside_switching")
    n = m.note_records()
    mine = n[n["phy"] == 1]
    assert len(mine) == 1 and tuple(mine[0][["kind", "state", "cca_duration"]]) == (wsm.NOTE_DROP_SWITCHING, SWITCHING, 0)
    p = m.phy[1]
    assert (p.drop_switching, p.c["rx"], p.c["cca_switches"], p.end_cca) == (1, 1, 0, 0) and len(p.ni) == 2


def test_branch_receive_that_outlasts_the_switch_raises_cca():
    c, m = branch("rx_outlasts_switching")
    n = m.note_records()
    mine = n[n["phy"] == 1]
    assert len(mine) == 1 and tuple(mine[0][["kind", "state"]]) == (wsm.NOTE_DROP_SWITCHING, SWITCHING)
    p = m.phy[1]
    assert mine[0]["cca_duration"] == DUR and p.end_cca == int(mine[0]["ts"]) + DUR and p.c["cca_switches"] == 1
    assert p.state(T0 + DELAY) == CCA_BUSY and p.drop_switching == 1 and p.c["sync"] == 0


def test_branch_in_flight_receive_reaches_the_phy_that_left():
    c, m = branch("in_flight")
    n = m.note_records()
    mine = n[n["phy"] == 1]
    assert len(mine) == 1 and T0 + 100 < int(mine[0]["ts"]) < T0 + 1_000 and mine[0]["kind"] == wsm.NOTE_DROP_SWITCHING
    assert m.phy[1].channel == 6 != m.phy[0].channel and m.phy[1].c["rx"] == 1


def test_branch_first_sync_on_the_new_channel_sees_only_post_erase_noise():
    c, m = branch("erase")
    ends = m.end_records()
    e = ends[ends["phy"] == 1]
    assert len(e) == 1 and e[0]["flags"] == 0 and m.txs[int(e[0]["tx"])][2] == 4
    # phy 3's frame (below the ED threshold, still on the air at the sync) was erased: the snr is the noise floor's
    floor = wifi_noise_floor(c["phys"])
    assert e[0]["snr"] == e[0]["rx_w"] / floor
    _c2, kept = branch("erase", erase=False)
    k = kept.end_records()
    k = k[k["phy"] == 1]
    assert len(k) == 1 and k[0]["rx_w"] == e[0]["rx_w"] and k[0]["snr"] < 0.9 * e[0]["snr"]


def wifi_noise_floor(ph):
    return math.pow(10.0, ph.noise_figure_db / 10.0) * (1.3803e-23 * 290.0 * MODE[2])


def test_branch_send_packet_while_switching_is_an_error():
    with pytest.raises(wsm.SendError):
        branch("send_while_switching")


def test_grid_scenario_takes_every_branch():
    c = grid_switch_case()
    m = wsm.run(c["phys"], c["closures"], c["stop"], MODE, PREAMBLE, DBM, notify=range(16))
    assert branch_coverage(m) >= ALL_BRANCHES, ALL_BRANCHES - branch_coverage(m)
    assert len(c["sends"]) == 40 and len(c["switches"]) >= 10 and len(set(c["phys"].channel)) == 3


# ---------------------------------------------------------------- 5: the state helper
@pytest.mark.parametrize("name", ["grid"] + [b for b in BRANCHES if b != "send_while_switching"])
def test_state_helper_consumes_the_models_stream(name):
    c = grid_switch_case() if name == "grid" else branch_case(name)
    m = wsm.run(c["phys"], c["closures"], c["stop"], MODE, PREAMBLE, DBM, notify=range(c["phys"].n_phy))
    delays = {}
    for s in m.switches:
        if s[3] == wsm.DONE:
            delays[(s[0], s[1])] = [d for t, j, _n, d in c["switches"] if j == s[2] and t <= s[0]][-1]
    hs = wsm.drive_state_helpers(m, delays)
    for j, h in enumerate(hs):
        p = m.phy[j]
        assert (h.end_tx, h.end_rx, h.end_cca, h.end_sw, h.rxing) == (p.end_tx, p.end_rx, p.end_cca, p.end_sw, p.rxing)
    assert sum(1 for h in hs for call in h.listener if call[0] == "NotifySwitchingStart") == len(delays)


def test_state_helper_refuses_what_the_reference_asserts():
    h = wsm.StateHelper()
    h.switch_to_channel_switching(1000, 250)
    with pytest.raises(wifi_note_model.Precondition):
        h.switch_to_channel_switching(1100, 250)
    with pytest.raises(wifi_note_model.Precondition):
        h.switch_to_tx(1100, 50)
    h.switch_to_tx(1250, 50)
    with pytest.raises(wifi_note_model.Precondition):
        h.switch_to_channel_switching(1260, 250)


# ---------------------------------------------------------------- 6: the exports
def test_exports():
    import nsgpu
    names = ("nsgpu_wifil_set_channel", "nsgpu_wifil_get_channel", "nsgpu_sim_wifi_set_channel", "nsgpu_sim_wifi_get_channel")
    assert set(names) <= set(nsgpu.SIGNATURES)
    assert wifi.SWITCHING == 4 and wifi.NOTE_DROP_SWITCHING == 4
    assert (wifi.SWITCH_DONE, wifi.SWITCH_INIT, wifi.SWITCH_POSTPONED) == (0, 1, 2)
    assert os.path.exists(nsgpu.LIB_PATH), "libnsgpu.so is not built"
    so = ctypes.CDLL(nsgpu.LIB_PATH)
    assert not [n for n in names if not hasattr(so, n)]
    assert ctypes.sizeof(wifi.WifilSwitch) == 16 and ctypes.sizeof(wifi.WifilChannel) == 40


def test_shared_scenarios_run_on_the_model():
    """The other scenarios tests/test_gpu_wifi_switch.py runs, each asserting what it was built for."""
    c = big_grid_case()
    m = run_model(c)
    outcomes = [(s[2], s[3], s[4]) for s in m.switches]
    assert outcomes[:5] == [(3, wsm.DONE, IDLE), (300, wsm.DONE, RX), (323, wsm.DONE, RX), (323, wsm.REFUSED, SWITCHING),
                            (305, wsm.POSTPONED, TX)], outcomes
    assert sorted(o[0] for o in outcomes if o[1] == wsm.DONE) == [3, 3, 300, 305, 323]
    for j in (3, 300, 323):  # they hear their new channels
        assert m.phy[j].c["sync"] >= 1 and m.phy[j].switches >= 1, j
    c = burst_case()
    m = run_model(c)
    p = m.phy[12]
    assert [s[3:5] for s in m.switches] == [(wsm.DONE, IDLE)] and (p.c["rx"], p.drop_switching) == (10, 10)
    assert len(m.txs) == 12 and m.phy[13].c["rx"] == 10 and p.c["end"] == 0 and p.channel == 6
    c = grid_switch_case()
    mob = mobile_models(c["phys"])
    m = run_model(c, mob=mob)
    assert len(m.switches) >= 10 and all(mob[j].last > 100_000_000 for j in mob)
