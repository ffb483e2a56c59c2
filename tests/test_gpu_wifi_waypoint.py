"""Waypoint and ConstantAcceleration mobility of the closed-loop Wi-Fi PHY on the device (nsgpu_wifil_set_waypoints /
nsgpu_wifil_set_acceleration and their neighbours; k_wl_move ahead of every send's k_wl_rx).  Each scenario of
tests/waypoint_cases.py runs on the device with the models installed and on the unchanged oracle with the restated
positions (tests/waypoint_ref.py) written by SetPosition closures: full pop log, dispatch count, digest, next uid,
per-phy counters and the end records' integer fields are equal, snr / per / rx_w within the closed-loop tests' 1e-9
(device libm vs glibc), and every model's read at the end of the run — position, velocity, the waypoint model's
m_current / m_next / m_first / WaypointsLeft, the acceleration model's base fields — equals the restatement with ==, bit
for bit: the device's arithmetic is +, *, the IEEE division and integers.  The scenarios' preconditions are asserted
on the CPU in tests/test_waypoint_cpu.py with the same seeds."""
import ctypes as C

import numpy as np
import pytest

import lossx_cases as lc
import mobility_cases as mc
import nsgpu
import test_wifi_switch_cpu as sc
import waypoint_cases as wc
import wifi
from waypoint_ref import WaypointModel

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4


def check(name, **kw):
    case = wc.CASES[name](wc.SEEDS[name])
    pl = wc.plan(case)
    o = mc.run_oracle(case, pl["moves"], log_cap=kw.get("log_cap", 1 << 16))
    g = wc.run_device(case, pl, **kw)
    mc.equal_oracle(g["four"], o)
    assert set(g["final"]) == set(pl["final"])
    for j, want in pl["final"].items():
        assert g["final"][j] == want, (j, g["final"][j], want)
    want_reads = [(ev, r) for ev, _t, r in pl["records"] if r is not None]
    assert len(g["reads"]) == len(want_reads)
    for (ev, got), (wev, want) in zip(g["reads"], want_reads):
        got = got[:2] if ev[0] == "get" else got  # (get_mobility's paused flag: not part of the restatement's read)
        assert ev == wev and got == want, (ev, got, want)
    g["lp"].close()
    return case, pl, o, g


def test_mixed_grid_4x4():
    """Constant, constant-velocity, waypoint (lists of 1, 2, 3 and 7) and acceleration phys on one channel."""
    _case, pl, o, g = check("grid")
    assert len(o[1]) > 50 and len(pl["final"]) == 14
    assert g["final"][0]["next"][0] is None and g["final"][3]["left"] == 0 and g["final"][3]["next"][0] is not None


def test_channels():
    """Phys on channels 1 and 6 update only at their own channel's sends; the lone waypoint phy on channel 11 sends
    and never updates before the final read."""
    check("channels")


def test_two_blocks_300_waypoint_phys():
    _case, pl, _o, _g = check("blocks", log_cap=1 << 17)
    assert len(pl["final"]) == 300


def test_run_time_calls_from_closures():
    """AddWaypoint past a segment's capacity (it moves) and past the pool's (it is replaced), EndMobility and an
    AddWaypoint after it, SetPosition mid-leg and after the end, mid-run reads, SetVelocityAndAcceleration, one model
    kind replaced by another, models removed."""
    _case, pl, _o, g = check("calls")
    assert len(g["reads"]) == 4 and g["reads"][-1][0][2] == 4 and g["reads"][-1][1]["left"] > 30
    assert sorted(g["final"]) == sorted(j for j, m in enumerate(pl["models"]) if m is not None)


def test_more_than_nsend_sends_then_a_course_call_in_one_closure():
    """Ten SendPackets from one closure (NSEND = 8: the batch flushes), then SetPosition of the first sender in the same
    closure (which flushes the rest): every send keeps the receptions of the positions at its own send."""
    check("burst")


def test_static_control_install_then_remove():
    """Models installed and removed before the first send: the run of a handle that never had one (k_wl_move is not
    launched again once the last model is gone)."""
    case = wc.grid_case(wc.SEEDS["grid"])
    pl = wc.plan(case)
    o = mc.run_oracle(case, mc.static_moves(case, pl["moves"]))
    ph = case["phys"]
    none = dict(case, specs=[None] * 16)

    def install_remove(_sim, lp):
        for j, s in enumerate(case["specs"]):
            if s is not None and s[0] != "wp":  # (a waypoint list moves the phy to its first waypoint at once)
                wc.install(lp, j, s, (ph.x[j], ph.y[j], ph.z[j]))
            elif s is not None:
                lp.set_waypoints(j, [(t, (ph.x[j], ph.y[j], ph.z[j])) for t, _p in s[1]])
        for j, s in enumerate(case["specs"]):
            if s is not None:
                (lp.set_mobility(j, None, None) if s[0] == "cv" else lp.set_waypoints(j, []) if s[0] == "wp"
                 else lp.set_acceleration(j, None))

    a = wc.run_device(none, pl)
    b = wc.run_device(none, pl, prepare=install_remove)
    mc.equal_oracle(a["four"], o)
    mc.equal_oracle(b["four"], o)
    assert a["four"][3]["digest"] == b["four"][3]["digest"] and np.array_equal(a["four"][1], b["four"][1])
    a["lp"].close()
    b["lp"].close()


def test_two_ray_ground_follows_a_climbing_waypoint_phy_and_a_channel_switch():
    """tests/lossx_cases.two_ray_case with phy 6 on a waypoint leg that climbs from z = 0 to 5 m in 50 ms — across the
    pair's crossover distance between phy 0's two sends — and a second waypoint phy (7) that switches to channel 6 at
    24 ms and so keeps its m_current.time from then on.  Against tests/lossx_model.py, driven by the waypoint
    restatement."""
    from test_gpu_lossx import run_device
    from wifi_model_compare import equal_model, finish
    from test_lossx_model_cpu import run_model
    import lossx_model
    base = lc.two_ray_case()
    lists = {6: [(0, (600.0, 0.0, 0.0)), (50_000_000, (600.0, 0.0, 5.0))],
             7: [(1_000_000, (700.0, 0.0, 4.0)), (20_000_000, (690.0, 5.0, 2.0)), (40_000_000, (700.0, 0.0, 9.0))]}
    closures = sorted(base["closures"] + [(24 * lc.MS, [("switch", 7, 6, sc.DELAY)])], key=lambda c: c[0])
    c = dict(base, closures=closures, mob=lambda: {j: WaypointModel(w) for j, w in lists.items()})
    m = run_model(c)
    lossx_model.clear_of_thresholds(m, 1e-6)
    g = run_device(dict(c, mob=None), before=lambda lp: [lp.set_waypoints(j, w) for j, w in lists.items()])
    equal_model(g, m, "two_ray + waypoints")
    for j in lists:
        assert g["lp"].get_waypoints(c["stop"], j) == m.mob[j].get(c["stop"]), j
    assert g["channels"][7]["channel"] == 6 and m.mob[6].hits["advanced"] >= 8
    finish(g)


def test_refusals():
    """Every refusal, with what is installed left in force."""
    case = wc.grid_case(wc.SEEDS["grid"])
    ph = case["phys"]
    L = nsgpu.lib()
    lp = wifi.LoopPhy(ph)
    wp3 = wifi.waypoint_array([(0, (1.0, 2.0, 3.0)), (2_000_000_000, (5.0, 2.0, 3.0)), (4_000_000_000, (5.0, 6.0, 3.0))])
    st, acc, mob = wifi.WaypointState(), wifi.Accel(), wifi.Mobility()
    v = (C.c_double * 3)(1, 1, 1)
    for bad in (ph.n_phy, 0xffffffff):  # (before anything is sized)
        assert L.nsgpu_wifil_set_waypoints(lp.h, bad, wp3, 3) == EINVAL
        assert L.nsgpu_wifil_add_waypoint(lp.h, bad, wp3) == EINVAL
        assert L.nsgpu_wifil_end_waypoints(lp.h, bad) == EINVAL
        assert L.nsgpu_wifil_get_waypoints(lp.h, 0, bad, C.byref(st)) == EINVAL
        assert L.nsgpu_wifil_set_acceleration(lp.h, bad, C.byref(acc)) == EINVAL
        assert L.nsgpu_wifil_set_velocity_and_acceleration(lp.h, 0, bad, v, v) == EINVAL
        assert L.nsgpu_wifil_get_acceleration(lp.h, 0, bad, C.byref(acc)) == EINVAL
    # no model on phy 3
    assert L.nsgpu_wifil_add_waypoint(lp.h, 3, wp3) == ESTATE
    assert L.nsgpu_wifil_end_waypoints(lp.h, 3) == ESTATE
    assert L.nsgpu_wifil_get_waypoints(lp.h, 0, 3, C.byref(st)) == ESTATE
    assert L.nsgpu_wifil_set_velocity_and_acceleration(lp.h, 0, 3, v, v) == ESTATE
    assert L.nsgpu_wifil_get_acceleration(lp.h, 0, 3, C.byref(acc)) == ESTATE
    assert L.nsgpu_wifil_set_waypoints(lp.h, 3, None, 0) == 0 and L.nsgpu_wifil_set_acceleration(lp.h, 3, None) == 0
    # a waypoint model on phy 3, an acceleration model on phy 5
    lp.set_waypoints(3, [(0, (1.0, 2.0, 3.0)), (2_000_000_000, (5.0, 2.0, 3.0)), (4_000_000_000, (5.0, 6.0, 3.0))])
    lp.set_acceleration(5, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0))
    for t in ((0, 1, 1), (0, 2, 2), (5, 4, 6)):  # not strictly ascending: nothing touched
        bad = wifi.waypoint_array([(q * 1_000_000_000, (9.0, 9.0, 9.0)) for q in t])
        assert L.nsgpu_wifil_set_waypoints(lp.h, 3, bad, 3) == EINVAL and b"ascending" in L.nsgpu_last_error()
    for t in (4_000_000_000, 3_000_000_000):     # not above the last one queued
        assert L.nsgpu_wifil_add_waypoint(lp.h, 3, wifi.waypoint_array([(t, (0.0, 0.0, 0.0))])) == EINVAL
    for j in (3, 5):  # no constant-velocity model on them; the untimed SetPosition has no Now
        assert L.nsgpu_wifil_set_velocity(lp.h, 0, j, v) == ESTATE
        assert L.nsgpu_wifil_pause(lp.h, 0, j, 1) == ESTATE
        assert L.nsgpu_wifil_get_mobility(lp.h, 0, j, C.byref(mob)) == ESTATE
        assert L.nsgpu_wifil_set_position(lp.h, j, 0.0, 0.0, 0.0) == ESTATE
        assert b"nsgpu_wifil_set_position_at" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_get_acceleration(lp.h, 0, 3, C.byref(acc)) == ESTATE   # (the other kind's calls)
    assert L.nsgpu_wifil_get_waypoints(lp.h, 0, 5, C.byref(st)) == ESTATE
    assert L.nsgpu_wifil_add_waypoint(lp.h, 5, wp3) == ESTATE
    assert L.nsgpu_wifil_set_position(lp.h, 2, 0.0, 0.0, 0.0) == 0              # (a constant-position phy: as before)
    # what was installed is still in force
    want = WaypointModel([(0, (1.0, 2.0, 3.0)), (2_000_000_000, (5.0, 2.0, 3.0)), (4_000_000_000, (5.0, 6.0, 3.0))])
    assert lp.get_waypoints(3_000_000_000, 3) == want.get(3_000_000_000)
    assert lp.get_waypoints(3_000_000_000, 3)["cur"][1] == (5.0, 4.0, 3.0)
    a = lp.get_acceleration(2_000_000_000, 5)
    assert a["now_pos"] == (6.0, 0.0, 0.0) and a["now_vel"] == (5.0, 0.0, 0.0) and a["base_time"] == 0
    # one model per phy: each install replaces what the phy had
    lp.set_mobility(3, (1.0, 1.0, 1.0), (1.0, 0.0, 0.0))
    assert L.nsgpu_wifil_get_waypoints(lp.h, 0, 3, C.byref(st)) == ESTATE
    assert lp.get_mobility(1_000_000_000, 3)[0] == (2.0, 1.0, 1.0)
    lp.set_acceleration(3, (0.0, 0.0, 0.0))
    assert L.nsgpu_wifil_get_mobility(lp.h, 0, 3, C.byref(mob)) == ESTATE
    lp.set_waypoints(3, [(0, (4.0, 4.0, 4.0))])
    assert L.nsgpu_wifil_get_acceleration(lp.h, 0, 3, C.byref(acc)) == ESTATE
    assert lp.get_waypoints(5, 3)["cur"] == (5, (4.0, 4.0, 4.0))
    lp.close()
    grp = wifi.LoopPhy(ph, bounds=[0, 8, ph.n_phy])  # a partitioned handle refuses the installs
    assert L.nsgpu_wifil_set_waypoints(grp.h, 0, wp3, 3) == EINVAL and b"single-engine" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_set_acceleration(grp.h, 0, C.byref(acc)) == EINVAL and b"single-engine" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_set_waypoints(grp.h, 0xffffffff, wp3, 3) == EINVAL
    assert L.nsgpu_wifil_add_waypoint(grp.h, 0, wp3) == ESTATE
    grp.close()
    sim = nsgpu.Sim()
    assert L.nsgpu_sim_wifi_set_waypoints(sim.h, 0, wp3, 3) == ESTATE  # no PHY attached
    assert L.nsgpu_sim_wifi_get_acceleration(sim.h, 0, C.byref(acc)) == ESTATE
    sim.close()


def test_remove_calls_across_kinds_and_a_reinstall():
    """Each remove call on a phy that holds another kind's model — set_mobility (NULL) removes a constant-velocity model
    only; set_waypoints (n = 0) and set_acceleration (NULL) remove a waypoint or an acceleration model, whichever the
    phy has, and no constant-velocity one — with what is installed afterwards read back; and a phy that goes waypoint ->
    constant velocity -> waypoint with a longer list than its segment held: the segment is reused and grown."""
    ph = wc.grid_case(wc.SEEDS["grid"])["phys"]
    L = nsgpu.lib()
    lp = wifi.LoopPhy(ph)
    st, acc, mob = wifi.WaypointState(), wifi.Accel(), wifi.Mobility()
    S = 1_000_000_000
    way = [(0, (1.0, 2.0, 3.0)), (2 * S, (5.0, 2.0, 3.0)), (4 * S, (5.0, 6.0, 3.0))]
    # a waypoint phy survives set_mobility (NULL); set_acceleration (NULL) removes its model
    lp.set_waypoints(3, way)
    assert L.nsgpu_wifil_set_mobility(lp.h, 3, None) == 0
    assert lp.get_waypoints(3 * S, 3) == WaypointModel(way).get(3 * S)
    assert L.nsgpu_wifil_set_position(lp.h, 3, 0.0, 0.0, 0.0) == ESTATE
    assert L.nsgpu_wifil_set_acceleration(lp.h, 3, None) == 0
    assert L.nsgpu_wifil_get_waypoints(lp.h, 0, 3, C.byref(st)) == ESTATE
    assert L.nsgpu_wifil_set_position(lp.h, 3, 0.0, 0.0, 0.0) == 0
    # a constant-velocity phy survives set_waypoints (n = 0) and set_acceleration (NULL)
    lp.set_mobility(5, (1.0, 1.0, 1.0), (1.0, 0.0, 0.0))
    assert L.nsgpu_wifil_set_waypoints(lp.h, 5, None, 0) == 0
    assert L.nsgpu_wifil_set_acceleration(lp.h, 5, None) == 0
    assert lp.get_mobility(S, 5) == ((2.0, 1.0, 1.0), (1.0, 0.0, 0.0), False)
    assert L.nsgpu_wifil_set_position(lp.h, 5, 0.0, 0.0, 0.0) == ESTATE
    # an acceleration phy survives set_mobility (NULL); set_waypoints (n = 0) removes its model
    lp.set_acceleration(6, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0, 0.0, 0.0))
    assert L.nsgpu_wifil_set_mobility(lp.h, 6, None) == 0
    a = lp.get_acceleration(2 * S, 6)
    assert a["now_pos"] == (6.0, 0.0, 0.0) and a["now_vel"] == (5.0, 0.0, 0.0) and a["base_time"] == 0
    assert L.nsgpu_wifil_set_waypoints(lp.h, 6, None, 0) == 0
    assert L.nsgpu_wifil_get_acceleration(lp.h, 0, 6, C.byref(acc)) == ESTATE
    assert L.nsgpu_wifil_set_position(lp.h, 6, 0.0, 0.0, 0.0) == 0
    # waypoint -> constant velocity -> waypoint, the second list longer than the first one's segment (four slots)
    rng = np.random.default_rng(wc.SEEDS["calls"])
    lp.set_waypoints(9, way[:2])
    lp.set_mobility(9, (7.0, 7.0, 7.0), (1.0, 2.0, 3.0))
    assert L.nsgpu_wifil_get_waypoints(lp.h, 0, 9, C.byref(st)) == ESTATE
    longer = wc.path(rng, (3.0, 4.0, 5.0), [q * S + q * q for q in range(1, 10)])
    lp.set_waypoints(9, longer)
    assert L.nsgpu_wifil_get_mobility(lp.h, 0, 9, C.byref(mob)) == ESTATE
    want = WaypointModel(longer)
    for t in (longer[0][0], 3 * S + S // 3, 7 * S + S // 7, 8 * S + 5):  # (each read is an Update: in time order)
        assert lp.get_waypoints(t, 9) == want.get(t), t
    assert want.get(8 * S + 5)["left"] == 1
    lp.close()
