"""Scenarios of the constant-velocity mobility tests (tests/test_mobility_cpu.py, tests/test_gpu_wifi_mobility.py),
how the unchanged oracle pins the device, and the plan and the device driver every mobility test shares
(tests/waypoint_cases.py holds the scenarios with waypoint and acceleration models).

nsref.wifil_replay (..., moves=...) schedules the sends, then MobilityModel::SetPosition closures, then Stop.
  expected run: for every event of the scenario in dispatch order — a send k: one move at ts[k] - 1 per phy whose
    model updates at it, carrying the restated position (tests/mobility_ref.py) for ts[k]; a course change or a
    read at T: one move at T carrying the restated position at T.
  device run: the same sends with the models installed on the device (LoopPhy.set_mobility), and one host closure
    at the place of every move, in the same schedule order — a no-op for a send's moves, the real call
    (wifi_set_velocity / wifi_pause / wifi_set_position / wifi_get_mobility) for a course change — so the uids,
    the dispatch count and the epochs' cuts are those of the expected run.
The static control is the expected run with every move carrying the phy's position at setup.

A case: dict (phys, specs, sends, course, stop_ns[, burst]).  specs[j]: None (constant position) | cv (vel, paused,
last_update) | ("wp", [(t ns, pos)]) | ("acc", vel, acc) (m_basePosition: the phy's setup position, m_baseTime 0).
course: the events of waypoint_ref.walk other than sends."""
import numpy as np

import nsref
import wifi
from mobility_ref import CvModel, send_updates
from waypoint_ref import AccelModel, WaypointModel, walk

SIZE, DBM, MODE, PREAMBLE = 200, 16.0206, wifi.DSSS_1M, wifi.PREAMBLE_LONG
PHY_FIELDS = ("rx", "sync", "drop_rx", "drop_tx", "drop_ed", "cca_switches", "end", "end_cancelled")


def send_times(rng, n, first=5_000_000):
    """Irregular ns timestamps, gaps of 20-70 ms."""
    return first + np.cumsum(rng.integers(20_000_000, 70_000_000, n))


def velocities(rng, n, vmax=150.0):
    """Up to +-vmax m/s in x and y, a tenth of it in z."""
    return [tuple(float(c) for c in rng.uniform(-vmax, vmax, 3) * (1.0, 1.0, 0.1)) for _ in range(n)]


def cv(vel, paused=False, last_update=0):
    """A constant-velocity spec."""
    return ("cv", tuple(vel), paused, last_update)


def make(x, y, z, channel, specs, sends, course=(), stop_ns=None):
    """sends: [(ts, phy)] in schedule order, ts not decreasing."""
    ph = wifi.LoopPhys(x, y, z, channel=channel, tx_cap=1024)
    sends = [(int(t), int(p)) for t, p in sends]
    stop_ns = int(stop_ns if stop_ns is not None else sends[-1][0] + 30_000_000)
    return dict(phys=ph, specs=list(specs), sends=sends, course=[tuple(e) for e in course], stop_ns=stop_ns)


def grid_case(seed, channel=None, course=(), n_sends=36):
    """The 4x4 grid, 60 m pitch: 16 velocities up to +-150 m/s with one zero (phy 2), one phy left paused (phy 6)
    and one left constant-position (phy 11); n_sends sends, senders 5k mod 16."""
    rng = np.random.default_rng(seed)
    x, y, z = wifi.grid(4, 60.0)
    vel = velocities(rng, 16)
    specs = [cv(v) for v in vel]
    specs[2] = cv((0.0, 0.0, 0.0))
    specs[6] = cv(vel[6], paused=True)
    specs[11] = None
    ts = send_times(rng, n_sends)
    return make(x, y, z, channel, specs, [(ts[k], 5 * k % 16) for k in range(n_sends)], course)


def channels_case(seed):
    """Phys split over channels 1 and 6, and a lone phy on channel 11 (phy 15, which also sends)."""
    ch = np.array([1, 6] * 8, np.uint32)
    ch[15] = 11
    return grid_case(seed, channel=ch)


def block_edge_case(seed):
    """300 phys (20 x 15, 60 m pitch), all mobile, 12 sends: k_wl_move / k_wl_rx run two blocks, the second partial."""
    rng = np.random.default_rng(seed)
    i = np.arange(300)
    x, y, z = (i % 20) * 60.0, (i // 20) * 60.0, np.zeros(300)
    specs = [cv(v) for v in velocities(rng, 300)]
    ts = send_times(rng, 12)
    return make(x, y, z, None, specs, [(ts[k], 83 * k % 300) for k in range(12)])


def course_case(seed, with_get=True):
    """Case 1 with course changes between the sends: SetVelocity twice on phy 3 (the ns2 "square" pattern's turn,
    scaled to the grid), Pause / Unpause on phy 7, SetPosition on the moving phy 9 (its velocity becomes 0), and a
    GetPosition of phy 12 mid-run."""
    c = grid_case(seed)
    ts = [t for t, _p in c["sends"]]
    mid = lambda k: (ts[k] + ts[k + 1]) // 2
    course = [("vel", mid(4), 3, (120.0, 0.0, 0.0)), ("pause", mid(7), 7, True), ("vel", mid(12), 3, (0.0, 120.0, 0.0)),
              ("pos", mid(15), 9, (33.0, 77.0, 0.0)), ("pause", mid(20), 7, False)]
    if with_get:
        course.append(("get", mid(23) + 12_345_677, 12))
    c["course"] = course
    return c


def burst_case(seed):
    """Ten sends at one timestamp (on the device: one closure, more than NSEND = 8, so the batch flushes) from ten
    phys, the first a fast mover; the same closure then moves that sender far away (SetPosition, after the sends in
    the expected run's order too: the sends' receptions keep the positions they were made with); then sends from later
    closures."""
    rng = np.random.default_rng(seed)
    x, y, z = wifi.grid(4, 60.0)
    specs = [cv(v) for v in velocities(rng, 16)]
    specs[0] = cv((150.0, 140.0, 0.0))
    t0 = 40_000_000
    sends = [(t0, p) for p in range(10)] + [(t0 + 55_000_123, 0), (t0 + 101_000_456, 13)]
    c = make(x, y, z, None, specs, sends, course=[("pos", t0, 0, (900.0, 700.0, 0.0))])
    c["burst"] = 10  # the first 10 sends, and the course events at their time, are one device closure
    return c


def events_of(case):
    """The scenario's events in dispatch order (sends keep their schedule order at equal ts; a course event at a
    send's time runs after it: the moves are scheduled after the sends)."""
    ev = [("send", t, p) for t, p in case["sends"]] + list(case["course"])
    times = [e[1] for e in case["course"]]
    send_ts = {t for t, _p in case["sends"]}
    assert len(set(times)) == len(times) and not ({t + 1 for t in times} & send_ts)
    return sorted(ev, key=lambda e: e[1])  # (stable)


def models_of(case):
    ph = case["phys"]
    out = []
    for j, s in enumerate(case["specs"]):
        p = (float(ph.x[j]), float(ph.y[j]), float(ph.z[j]))
        out.append(None if s is None else CvModel(p, *s[1:]) if s[0] == "cv" else WaypointModel(s[1]) if s[0] == "wp"
                   else AccelModel(p, s[1], s[2], base_time=0))
    return out


def plan(case, update_rule=send_updates):
    """Walks the restatements over the scenario.  Returns dict: events, records ((event, {phy: position after it}) per
    event), reads (per record: what a *_get returned, else None), moves (the expected run's), slots (the device run's
    closure per move: None, or (course event, the phy's position after it)), final ({phy: the model's read at the
    final accumulation point stop_ns}), models (as the walk left them)."""
    ph = case["phys"]
    models = models_of(case)
    events = events_of(case)
    start = [(float(ph.x[j]), float(ph.y[j]), float(ph.z[j])) for j in range(ph.n_phy)]
    walked = walk(models, ph.channel, events, update_rule, positions=start)
    moves, slots = [], []
    for ev, touched, _read in walked:
        if ev[0] == "send":
            for j in sorted(touched):
                moves.append((ev[1] - 1, j, touched[j]))
                slots.append(None)
        else:
            moves.append((ev[1], ev[2], touched[ev[2]]))
            slots.append((ev, touched[ev[2]]))
    final = {j: m.get(case["stop_ns"]) for j, m in enumerate(models) if m is not None}
    return dict(events=events, records=[(ev, touched) for ev, touched, _read in walked],
                reads=[read for _ev, _touched, read in walked], moves=moves, slots=slots, final=final, models=models)


def run_oracle(case, moves, log_cap=1 << 16):
    ph = case["phys"]
    ts = np.array([t for t, _p in case["sends"]], np.uint64)
    phy = np.array([p for _t, p in case["sends"]], np.uint32)
    size = np.full(len(ts), SIZE, np.uint32)
    return nsref.wifil_replay(ph.c_struct(), ts, phy, size, MODE, PREAMBLE, DBM, case["stop_ns"], ph.n_phy,
                              wifi.WIFIL_END_DTYPE, wifi.PHY_COUNTERS_DTYPE, log_cap=log_cap, moves=moves)


def static_moves(case, moves):
    ph = case["phys"]
    return [(t, j, (float(ph.x[j]), float(ph.y[j]), float(ph.z[j]))) for t, j, _p in moves]


def reception_margins(case, pl):
    """Smallest relative distance of any reception's power (rxPowerW, with RxGain) from the ED and the CCA
    threshold, over every send at the positions the restatement gives for it."""
    ph = case["phys"]
    pos = np.stack([ph.x, ph.y, ph.z], axis=1).copy()
    chain = nsref.loss_chain(*ph.loss)
    ed_w, cca_w = 10.0 ** (ph.ed / 10.0) / 1000.0, 10.0 ** (ph.cca / 10.0) / 1000.0
    worst = np.inf
    for ev, touched in pl["records"]:
        for j, p in touched.items():
            pos[j] = p
        if ev[0] != "send":
            continue
        rx = nsref.fanout_yans(pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), ph.channel, ph.node, ev[2], DBM,
                               chain, ph.speed, ev[1], 0)
        w = 10.0 ** ((rx["rx_dbm"] + ph.rx_gain_db) / 10.0) / 1000.0
        for thr in (ed_w, cca_w):
            if len(w):
                worst = min(worst, float(np.min(np.abs(w - thr) / thr)))
    return worst


def same_run(a, b):
    """Two oracle runs (log, ends, phys, tot): identical?"""
    return all(np.array_equal(p, q) for p, q in zip(a[0], b[0])) and np.array_equal(a[1], b[1]) and \
        np.array_equal(a[2], b[2]) and a[3]["dispatched"] == b[3]["dispatched"] and a[3]["digest"] == b[3]["digest"]


def bits(final):
    """{phy: position} as exact tuples of float.hex strings."""
    return {j: tuple(float(c).hex() for c in pv[0]) for j, pv in final.items()}


def closed_form(case):
    """x0 + v * GetSeconds (stop): what one update at the end would give (the variant the accumulation guards
    against); only for scenarios without course changes."""
    ph = case["phys"]
    s = nsref.get_seconds(case["stop_ns"])
    out = {}
    for j, sp in enumerate(case["specs"]):
        if sp is None:
            continue
        v = (0.0, 0.0, 0.0) if sp[2] else sp[1]
        out[j] = ((float(ph.x[j]) + v[0] * s, float(ph.y[j]) + v[1] * s, float(ph.z[j]) + v[2] * s), v)
    return out


# ---------------------------------------------------------------- the device run
def install(lp, j, spec, pos):
    if spec[0] == "cv":
        lp.set_mobility(j, pos, spec[1], paused=spec[2], last_update=spec[3])
    elif spec[0] == "wp":
        lp.set_waypoints(j, spec[1])
    else:
        lp.set_acceleration(j, pos, spec[1], spec[2], base_time=0)


def read_final(lp, now, j, kind):
    if kind == "cv":
        return lp.get_mobility(now, j)[:2]
    return lp.get_waypoints(now, j) if kind == "wp" else lp.get_acceleration(now, j)


def run_device(case, pl, log_cap=1 << 16, listen=(), notify=(), prepare=None):
    """The scenario on the device PHY with the models installed.  Returns dict: four (log, ends, phys, tot: for
    equal_oracle), final ({phy: the read of its model's kind at stop_ns}), reads ([(event, result)] of the mid-run
    reads), notes, sim, lp."""
    import nsgpu
    ph = case["phys"]
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    sim.set_log(log_cap)
    if prepare:
        prepare(sim, lp)
    kind = {}
    for j, s in enumerate(case["specs"]):
        if s is not None:
            install(lp, j, s, (ph.x[j], ph.y[j], ph.z[j]))
            kind[j] = s[0]
    handbacks = []
    if listen:
        sim.wifi_set_end_handler(lambda e: handbacks.append((int(e["ts"]), int(e["uid"]))))
        for p in listen:
            sim.wifi_listen(p)
    for p in notify:
        sim.wifi_notify(p)
    reads, failures = [], []

    def course(slot):
        ev, after = slot
        k, _t, phy = ev[0], ev[1], ev[2]
        assert sim.now() == ev[1]
        if k == "pos":
            sim.wifi_set_position(phy, *ev[3])
        elif k == "vel":
            sim.wifi_set_velocity(phy, ev[3])
        elif k == "pause":
            sim.wifi_pause(phy, ev[3])
        elif k == "get":
            reads.append((ev, sim.wifi_get_mobility(phy)))
        elif k == "wp_add":
            sim.wifi_add_waypoint(phy, *ev[3])
        elif k == "wp_end":
            sim.wifi_end_waypoints(phy)
        elif k == "wp_get":
            reads.append((ev, sim.wifi_get_waypoints(phy)))
        elif k == "acc_set":
            sim.wifi_set_velocity_and_acceleration(phy, ev[3], ev[4])
        elif k == "acc_get":
            reads.append((ev, sim.wifi_get_acceleration(phy)))
        elif k == "install_wp":
            sim.wifi_set_waypoints(phy, ev[3])
            kind[phy] = "wp"
        elif k == "install_acc":
            sim.wifi_set_acceleration(phy, ev[3], ev[4], ev[5])
            kind[phy] = "acc"
        elif k == "install_cv":  # (ConstantVelocityHelper takes its position with the install: where the phy is)
            lp.set_mobility(phy, after, ev[3], paused=False, last_update=sim.now())
            kind[phy] = "cv"
        elif k == "remove":
            if kind[phy] == "wp":
                sim.wifi_set_waypoints(phy, [])
            elif kind[phy] == "acc":
                sim.wifi_set_acceleration(phy, None)
            else:
                lp.set_mobility(phy, None, None)
            del kind[phy]
        else:
            raise ValueError(k)

    def guarded(fn):
        def run():
            try:
                fn()
            except BaseException as e:  # (an exception does not cross the C callback: keep it for the test)
                failures.append(e)
        return run

    send = lambda p: sim.wifi_send(p, SIZE, DBM, MODE, PREAMBLE)
    nb = case.get("burst", 0)
    inline = [s for s in pl["slots"] if s is not None and nb and s[0][1] == case["sends"][0][0]]
    for k, (t, p) in enumerate(case["sends"]):
        if k == 0 and nb:  # one closure makes the first nb sends, then the course calls of their time
            sim.schedule(t, guarded(lambda: [send(q) for _t, q in case["sends"][:nb]] + [course(s) for s in inline]))
        elif k < nb:  # (the others' places are held by no-ops)
            sim.schedule(t, lambda: None)
        else:
            sim.schedule(t, guarded((lambda p=p: lambda: send(p))()))
    for (t, _j, _p), slot in zip(pl["moves"], pl["slots"]):
        sim.schedule(t, (lambda: None) if slot is None or slot in inline else guarded((lambda s=slot: lambda: course(s))()))
    sim.stop(case["stop_ns"])
    sim.run()
    assert not failures, failures
    digest = sim.host_stats()[2]
    k = min(sim.dispatched(), log_cap)
    log = (sim.log[0][:k].copy(), sim.log[1][:k].copy(), sim.log[2][:k].copy())
    tot = dict(dispatched=sim.dispatched(), digest=digest, next_uid=sim.next_uid(), handbacks=handbacks)
    final = {j: read_final(lp, case["stop_ns"], j, kd) for j, kd in kind.items()}
    return dict(four=(log, lp.read_ends(), lp.read_phys(), tot), final=final, reads=reads, notes=lp.read_notes(), sim=sim,
                lp=lp)


def equal_oracle(g, o):
    """The device run against the expected run: full pop log, dispatch count, digest, next uid, per-phy counters, end
    records' integer fields exactly; snr / per / rx_w as the closed-loop tests compare them (device libm vs glibc)."""
    glog, gends, gphys, gtot = g
    olog, oends, ophys, otot = o
    for f in ("dispatched", "digest", "next_uid"):
        assert gtot[f] == otot[f], (f, gtot[f], otot[f])
    for a, b in zip(glog, olog):
        assert np.array_equal(a, b)
    for f in PHY_FIELDS:
        assert np.array_equal(gphys[f], ophys[f]), f
    assert len(gends) == len(oends)
    for f in ("ts", "uid", "phy", "tx", "flags"):
        assert np.array_equal(gends[f], oends[f]), f
    np.testing.assert_allclose(gends["snr"], oends["snr"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(gends["per"], oends["per"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(gends["rx_w"], oends["rx_w"], rtol=1e-9, atol=0)


def equal_final(got, want):
    """get_mobility at the end of the run against the restatement: ==, bit for bit (only +, * and integers)."""
    assert set(got) == set(want)
    for j in want:
        assert got[j][0] == want[j][0], (j, "position", [c.hex() for c in got[j][0]], [c.hex() for c in want[j][0]])
        assert got[j][1] == want[j][1], (j, "velocity", got[j][1], want[j][1])
