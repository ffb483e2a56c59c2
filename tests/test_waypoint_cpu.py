"""Waypoint and ConstantAcceleration mobility on the CPU: the restatement (tests/waypoint_ref.py) held to the
reference on three independent grounds — against the already pinned CvModel inside a leg, lazy against non-lazy
driving, and exact values (tests/golden/waypoint_kat.json; an exact rational evaluation within a bound derived by
counting roundings) — the branches each scenario of tests/waypoint_cases.py must reach, and the bindings.  No GPU:
tests/test_gpu_wifi_waypoint.py runs the same scenarios on the device."""
import ctypes
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import nsgpu
import nsref
import waypoint_cases as wc
import wifi
from mobility_ref import CvModel
from waypoint_ref import ENDED, AccelModel, WaypointModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(REPO, "tests", "golden", "waypoint_kat.json")))
NEW_SYMBOLS = tuple(f"nsgpu_{p}_{n}" for p in ("wifil", "sim_wifi") for n in (
    "set_waypoints", "add_waypoint", "end_waypoints", "get_waypoints", "set_acceleration",
    "set_velocity_and_acceleration", "get_acceleration"))
U = 2.0 ** -53


def random_list(rng, n, t0=None):
    """n waypoints at irregular non-dyadic times and positions."""
    t = int(rng.integers(0, 2_000_000_000)) if t0 is None else t0
    out = []
    for _ in range(n):
        out.append((t, tuple(float(c) for c in rng.uniform(-500.0, 500.0, 3))))
        t += int(rng.integers(1, 3_000_000_000))
    return out


def queries(rng, wps, n):
    """Query times around a list: before the first waypoint, inside every leg, exactly at waypoint times, after the
    last — sorted."""
    t0, t1 = wps[0][0], wps[-1][0]
    q = [int(v) for v in rng.integers(max(t0 - 500_000_000, 0), t1 + 2_000_000_000, n)]
    q += [t for t, _p in wps if rng.random() < 0.5] + [max(t0 - 1, 0), t1 + 1, t1 + 3_000_000_000]
    return sorted(q)


# ---------------------------------------------------------------- 1. against the pinned CvModel
@pytest.mark.parametrize("seed", range(20))
def test_inside_a_leg_the_model_is_a_cvmodel_started_at_the_legs_waypoint(seed):
    rng = np.random.default_rng(7000 + seed)
    wps = random_list(rng, int(rng.integers(2, 9)))
    m = WaypointModel(wps)
    qs = [q for q in queries(rng, wps, 40) if wps[0][0] <= q]
    cv, leg = None, -1
    for q in qs:
        m.update(q)
        i = max(k for k, (t, _p) in enumerate(wps) if t <= q)
        if i >= len(wps) - 1:  # at or past the last waypoint: there, at rest
            assert m.position() == wps[-1][1] and m.velocity() == (0.0, 0.0, 0.0) and m.next_t == ENDED
            continue
        if i != leg:  # a waypoint was crossed: the position restarts from its exact coordinates
            leg = i
            cv = CvModel(wps[i][1], m.velocity(), paused=False, last_update=wps[i][0])
            span = nsref.get_seconds(wps[i + 1][0] - wps[i][0])
            assert m.velocity() == tuple((wps[i + 1][1][c] - wps[i][1][c]) / span for c in range(3))
        cv.update(q)
        assert m.position() == cv.position(), (q, i)
        if q == wps[i][0]:
            assert m.position() == wps[i][1]
    assert leg >= 0


# ---------------------------------------------------------------- 2. lazy equals non-lazy
def lazy_and_not(wps, qs):
    """Positions at the queries: the model driven lazily, and with an Update at every waypoint's own time as well (what
    AddWaypoint schedules when LazyNotify is false, :96-99; at equal times the scheduled Update runs first)."""
    a, b = WaypointModel(wps), WaypointModel(wps)
    own = sorted(t for t, _p in wps)
    out_a, out_b = [], []
    for q in qs:
        a.update(q)
        out_a.append(a.position())
        while own and own[0] <= q:
            b.update(own.pop(0))
        b.update(q)
        out_b.append(b.position())
    return out_a, out_b


def test_lazy_equals_non_lazy():
    rng = np.random.default_rng(7100)
    n_lists = at_waypoint = single = before = after = 0
    for k in range(300):
        wps = random_list(rng, 1 if k % 10 == 0 else int(rng.integers(2, 10)))
        qs = queries(rng, wps, int(rng.integers(1, 30)))
        a, b = lazy_and_not(wps, qs)
        assert a == b, k
        times = {t for t, _p in wps}
        n_lists += 1
        at_waypoint += any(q in times for q in qs)
        single += len(wps) == 1
        before += any(q < wps[0][0] for q in qs)
        after += any(q > wps[-1][0] for q in qs)
    assert n_lists == 300 and at_waypoint > 100 and single == 30 and before > 100 and after == 300


# ---------------------------------------------------------------- 3. exact values
def test_get_seconds_of_the_fixture_times_is_exact():
    for t in KAT["times_ns"]:
        assert Fraction(nsref.get_seconds(t)) == Fraction(t, 10 ** 9), t
    used = {op[1] for grp in ("waypoint", "accel") for c in KAT[grp].values() for op in c["ops"]}
    used |= {t for c in KAT["waypoint"].values() for t, _p in c["waypoints"]} - {0}
    assert used <= set(KAT["times_ns"])


@pytest.mark.parametrize("name", sorted(KAT["waypoint"]))
def test_waypoint_fixture(name):
    c = KAT["waypoint"][name]
    m = WaypointModel([(t, p) for t, p in c["waypoints"]])
    for op in c["ops"]:
        if op[0] == "get":
            m.update(op[1])
            assert list(m.position()) == op[2] and list(m.velocity()) == op[3], op
        else:
            m.set_position(op[1], op[2])


@pytest.mark.parametrize("name", sorted(KAT["accel"]))
def test_accel_fixture(name):
    c = KAT["accel"][name]
    m = AccelModel(c["pos"], c["vel"], c["acc"], c["base_time"])
    for op in c["ops"]:
        if op[0] == "get":
            assert list(m.get_position(op[1])) == op[2] and list(m.get_velocity(op[1])) == op[3], op
        elif op[0] == "set_va":
            before = m.get_position(op[1])
            m.set_velocity_and_acceleration(op[1], op[2], op[3])
            assert m.get_position(op[1]) == before  # (continuous)
        else:
            m.set_position(op[1], op[2])
            assert list(m.get_position(op[1])) == op[2]


def gs_err(seconds):
    """|GetSeconds (t) - t / 1e9| at most: the int64x64 product truncates twice and Invert (1e9) once (3 units of 2^-64 s,
    taken as 2^-62), then (double) lo and hi + flo round once each."""
    return 2 * U * seconds + 2.0 ** -62


def waypoint_bound(p0, p1, span, elapsed, k, reach):
    """First-order bound on one coordinate of a position k accumulation points into a leg p0 -> p1 of `span` s, `elapsed`
    s after its start: the velocity carries the subtraction's, the division's and t_span's roundings; every
    accumulation point one GetSeconds, one product and one sum (of magnitude at most `reach`)."""
    v = abs(p1 - p0) / span
    ev = 2 * U + gs_err(span) / span
    return v * (elapsed * (ev + U) + k * 2.0 ** -62 + 2 * U * elapsed) + k * U * reach


def test_against_an_exact_rational_trajectory():
    """Non-dyadic lists: |restatement - exact| <= the bound derived by counting roundings (K = 1, first order).  The
    largest ratio measured is printed (DESIGN 4.3e records it)."""
    rng = np.random.default_rng(7200)
    worst = 0.0
    for _ in range(200):
        wps = random_list(rng, int(rng.integers(2, 8)))
        m = WaypointModel(wps)
        k, leg = 0, -1
        for q in queries(rng, wps, 25):
            m.update(q)
            if q < wps[0][0] or q >= wps[-1][0]:
                assert m.position() == (wps[0][1] if q < wps[0][0] else wps[-1][1])
                continue
            i = max(j for j, (t, _p) in enumerate(wps) if t <= q)
            k = k + 1 if i == leg else 1
            leg = i
            (t0, p0), (t1, p1) = wps[i], wps[i + 1]
            f = Fraction(q - t0, t1 - t0)
            for c in range(3):
                exact = Fraction(p0[c]) + (Fraction(p1[c]) - Fraction(p0[c])) * f
                err = abs(Fraction(m.position()[c]) - exact)
                bound = waypoint_bound(p0[c], p1[c], (t1 - t0) / 1e9, (q - t0) / 1e9, k, max(abs(p0[c]), abs(p1[c])))
                assert err <= bound, (wps, q, c, float(err), bound)
                worst = max(worst, float(err) / bound)
    print(f"waypoint: largest |restatement - exact| / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0
    worst = 0.0
    for _ in range(2000):
        b, v, a = (tuple(float(c) for c in rng.uniform(-s, s, 3)) for s in (500.0, 100.0, 50.0))
        t0 = int(rng.integers(0, 10 ** 9))
        now = t0 + int(rng.integers(1, 20 * 10 ** 9))
        m = AccelModel(b, v, a, t0)
        T = Fraction(now - t0, 10 ** 9)
        got = m.get_position(now)
        for c in range(3):
            exact = Fraction(b[c]) + Fraction(v[c]) * T + Fraction(a[c]) * T * T / 2
            tf = float(T)
            et = gs_err(tf) / tf
            bound = (abs(v[c]) * tf * (et + U) + abs(a[c]) * tf * tf / 2 * (2 * et + 2 * U)
                     + U * abs(b[c] + v[c] * tf) + U * abs(float(exact)))
            err = abs(Fraction(got[c]) - exact)
            assert err <= bound, (b, v, a, t0, now, c, float(err), bound)
            worst = max(worst, float(err) / bound)
    print(f"acceleration: largest |restatement - exact| / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0


# ---------------------------------------------------------------- 4. branches
def test_branches_of_update():
    m = WaypointModel([(1_000_000_000, (1.0, 1.0, 1.0))])
    m.update(500_000_000)
    assert m.hits["early"] == 1
    m.update(1_000_000_000)   # the empty queue's '<=' branch: a path of one waypoint, exactly at its time
    assert m.hits["ended"] == 1 and m.next_t == ENDED and m.state()["next"][0] is None and m.cur_t == 1_000_000_000
    m.update(2_000_000_000)   # later calls: only m_current.time = now
    m.update(3_000_000_000)
    assert m.hits["after_end"] == 2 and m.hits["ended"] == 1 and m.cur_t == 3_000_000_000 and m.position() == (1.0, 1.0, 1.0)
    m = WaypointModel([(k * 1_000_000_000, (float(k), 0.0, 0.0)) for k in range(6)])
    m.update(500_000_000)
    m.update(3_500_000_000)   # one Update crossing three waypoints
    assert m.hits["crossed_1"] == 1 and m.hits["crossed_3"] == 1 and m.left() == 1 and m.position() == (3.5, 0.0, 0.0)


def test_set_position_end_mobility_and_stale_velocity():
    wps = [(0, (0.0, 0.0, 0.0)), (4_000_000_000, (8.0, 0.0, 0.0)), (8_000_000_000, (8.0, 8.0, 0.0))]
    m = WaypointModel(wps)
    m.set_position(1_000_000_000, (50.0, 50.0, 0.0))  # mid-leg: sits still until m_next.time, then jumps to m_next
    assert m.hits["set_position_waits"] == 1 and m.cur_t == 4_000_000_000 and m.velocity() == (0.0, 0.0, 0.0)
    m.update(3_000_000_000)
    assert m.position() == (50.0, 50.0, 0.0)
    m.update(5_000_000_000)
    assert m.position() == (8.0, 2.0, 0.0)
    m.update(9_000_000_000)
    m.set_position(10_000_000_000, (1.0, 2.0, 3.0))   # after the end: at once
    assert m.hits["set_position_now"] == 1 and m.cur_t == 10_000_000_000 and m.position() == (1.0, 2.0, 3.0)
    # the velocity is read stale: the position's Update decides what DoGetVelocity returns
    m = WaypointModel(wps)
    m.update(1_000_000_000)
    assert m.velocity() == (2.0, 0.0, 0.0)            # (now 5 s is in the second leg, but nothing has updated)
    assert m.velocity() == (2.0, 0.0, 0.0)
    m.update(5_000_000_000)
    assert m.velocity() == (0.0, 2.0, 0.0)
    m.end()                                           # EndMobility: times 0, m_first; the next Update jumps to m_next
    assert (m.cur_t, m.next_t, m.first, m.left()) == (0, 0, True, 0)
    m.update(6_000_000_000)
    assert m.position() == (8.0, 8.0, 0.0) and m.next_t == ENDED
    m.add_waypoint(7_000_000_000, (0.0, 0.0, 9.0))    # AddWaypoint after the end starts a new path: there at once
    assert m.position() == (0.0, 0.0, 9.0) and not m.first and m.hits["add_first"] == 2
    m.add_waypoint(9_000_000_000, (4.0, 0.0, 9.0))
    with pytest.raises(ValueError):
        m.add_waypoint(9_000_000_000, (5.0, 0.0, 9.0))
    m.update(8_000_000_000)
    assert m.position() == (2.0, 0.0, 9.0)


def test_acceleration_course_changes_keep_the_position_continuous():
    rng = np.random.default_rng(7300)
    for _ in range(50):
        b, v, a = (tuple(float(c) for c in rng.uniform(-s, s, 3)) for s in (500.0, 100.0, 50.0))
        m = AccelModel(b, v, a, 0)
        t = int(rng.integers(1, 5 * 10 ** 9))
        p, vel = m.get_position(t), m.get_velocity(t)
        m.set_velocity_and_acceleration(t, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
        assert m.get_position(t) == p and m.get_velocity(t) == (1.0, 2.0, 3.0) and m.base_t == t
        m = AccelModel(b, v, a, 0)
        m.set_position(t, (9.0, 8.0, 7.0))
        assert m.get_position(t) == (9.0, 8.0, 7.0) and m.get_velocity(t) == vel and m.acc == a


# ---------------------------------------------------------------- the scenarios' preconditions
@pytest.mark.parametrize("name", sorted(wc.CASES))
def test_scenario_preconditions(name):
    """Each device scenario, walked on the restatement alone: the branches it is about are reached, the oracle sees the
    motion (its run differs from the static control's), and no reception sits within 1e-6 relative of a threshold."""
    case = wc.CASES[name](wc.SEEDS[name])
    pl = wc.plan(case)
    assert wc.margins(case, pl) > 1e-6
    hits = {j: m.hits for j, m in enumerate(pl["models"]) if isinstance(m, (WaypointModel, AccelModel))}
    if name in ("grid", "calls"):
        o = wc.mc.run_oracle(case, pl["moves"])
        assert not wc.mc.same_run(o, wc.mc.run_oracle(case, wc.mc.static_moves(case, pl["moves"])))
    if name == "grid":
        kinds = [wc.kind_of(m) for m in pl["models"]]
        assert (kinds.count(None), kinds.count("cv"), kinds.count("acc"), kinds.count("wp")) == (2, 4, 3, 7)
        assert sorted({len(s[1]) for s in case["specs"] if s and s[0] == "wp"}) == [1, 2, 3, 7]
        assert hits[0]["ended"] == 1 and hits[0]["after_end"] > 10       # one waypoint: '<=' branch, then m_current.time = now
        assert hits[7]["crossed_3"] == 1                                  # three waypoints inside one gap
        assert hits[8]["early"] >= 5 and hits[12]["after_end"] >= 10     # before the first, after the last
        sends = {t for t, _p in case["sends"]}
        assert sum(t in sends for t, _p in case["specs"][15][1]) == 2    # sends exactly at waypoint times
    if name == "channels":
        # the lone phy on channel 11 never updates; phys on the other channel keep their m_current.time at a send
        # (the plan's final read is each model's last Update)
        updates = lambda j: sum(n for k, n in hits[j].items() if k in ("early", "ended", "after_end") or k.startswith("crossed"))
        on = lambda ch: sum(1 for _t, p in case["sends"] if case["phys"].channel[p] == ch)
        assert updates(15) == 1 and on(11) >= 2 and (on(1), on(6)) == (updates(4) - 1, updates(7) - 1)
    if name == "blocks":
        assert len(hits) == 300
    if name == "calls":
        assert hits[7]["set_position_waits"] == 1 and hits[0]["set_position_now"] == 1 and hits[12]["end"] == 1
        assert hits[12]["add_first"] == 2 and hits[4]["add_queued"] == 46 and hits[3]["add_queued"] == 6
        assert [wc.kind_of(pl["models"][j]) for j in (1, 2, 8, 10, 11, 15)] == ["acc", "wp", "cv", None, "wp", None]
        reads = [r for _e, _t, r in pl["records"] if r is not None]
        assert len(reads) == 4
    if name == "burst":
        assert hits[0]["set_position_waits"] == 1


# ---------------------------------------------------------------- bindings
def test_signatures_name_the_new_calls():
    for s in NEW_SYMBOLS:
        assert s in nsgpu.SIGNATURES, s


def test_library_exports_the_new_calls():
    lib = nsgpu.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s


def header_sizeof(name):
    txt = open(os.path.join(REPO, "include", "nsgpu_types.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for ctype, decls in re.findall(r"(uint64_t|int64_t|double|uint32_t)\s+([^;]+);", body):
        for d in decls.split(","):
            n = re.search(r"\[(\d+)\]", d)
            size += (4 if ctype == "uint32_t" else 8) * (int(n.group(1)) if n else 1)
    return size


def test_structs_are_the_c_records():
    assert ctypes.sizeof(wifi.Waypoint) == header_sizeof("nsgpu_waypoint") == 32
    assert ctypes.sizeof(wifi.WaypointState) == header_sizeof("nsgpu_waypoint_state") == 104
    assert ctypes.sizeof(wifi.Accel) == header_sizeof("nsgpu_accel") == 128
    assert (wifi.Waypoint.pos.offset, wifi.WaypointState.next_time.offset, wifi.WaypointState.vel.offset,
            wifi.WaypointState.next_ended.offset, wifi.Accel.base_time.offset, wifi.Accel.now_pos.offset) == (8, 32, 64, 88, 72, 80)
    assert ctypes.sizeof(wifi.Mobility) == 64  # (nsgpu_mobility keeps its layout)


def test_refusals_that_need_no_device():
    L = nsgpu.lib()
    EINVAL = 1
    wp = wifi.waypoint_array([(0, (0.0, 0.0, 0.0))])
    out, acc, v = wifi.WaypointState(), wifi.Accel(), (ctypes.c_double * 3)()
    assert L.nsgpu_wifil_set_waypoints(None, 0, wp, 1) == EINVAL
    assert L.nsgpu_wifil_add_waypoint(None, 0, wp) == EINVAL
    assert L.nsgpu_wifil_end_waypoints(None, 0) == EINVAL
    assert L.nsgpu_wifil_get_waypoints(None, 0, 0, ctypes.byref(out)) == EINVAL
    assert L.nsgpu_wifil_set_acceleration(None, 0, ctypes.byref(acc)) == EINVAL
    assert L.nsgpu_wifil_set_velocity_and_acceleration(None, 0, 0, v, v) == EINVAL
    assert L.nsgpu_wifil_get_acceleration(None, 0, 0, ctypes.byref(acc)) == EINVAL
    assert b"nsgpu_wifil_get_acceleration" in L.nsgpu_last_error()
