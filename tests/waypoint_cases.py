"""Scenarios of the waypoint / acceleration mobility tests (tests/test_waypoint_cpu.py, tests/test_gpu_wifi_waypoint.py),
on the scheme of tests/mobility_cases.py, whose helpers they use: the unchanged oracle replays the sends with the
restated positions (tests/waypoint_ref.py) carried in as SetPosition closures — one a ns before each send per phy that
updates at it, one at the time of every course event — and the device runs the same sends with the models installed,
a no-op closure at the place of every send's move and the real call at the place of every course event.

The case's form, the plan and the device driver (install, run_device) are mobility_cases'."""
import numpy as np

import mobility_cases as mc
import wifi
from mobility_cases import install, run_device  # noqa: F401
from mobility_ref import CvModel, send_updates
from waypoint_ref import WaypointModel

SEEDS = dict(grid=4101, channels=4102, blocks=4103, calls=4104, burst=4105)


def path(rng, start, times, step=35.0):
    """Waypoints at `times` from `start` on: each leg up to +-step m in x and y, a tenth of it in z."""
    p = np.array(start, float)
    out = []
    for k, t in enumerate(times):
        if k:
            p = p + rng.uniform(-step, step, 3) * (1.0, 1.0, 0.1)
        out.append((int(t), tuple(float(c) for c in p)))
    return out


def grid_case(seed, channel=None, course=(), n_sends=36):
    """The 4x4 grid, 60 m pitch, 36 sends (senders 5k mod 16).  Constant: 11, 14.  Constant velocity: 1, 5, 9, 13.
    Acceleration: 2, 6, 10.  Waypoints: 0 (one entry), 3 (two: one long leg), 4 (seven, evenly spread), 7 (seven, three
    of them inside the gap between sends 10 and 11), 8 (two, the first after send 5: sends fall before the first
    waypoint), 12 (seven, the last at send 18's time less a bit: sends fall after the last), 15 (three, the second and
    third exactly at the times of sends 9 and 25)."""
    rng = np.random.default_rng(seed)
    x, y, z = wifi.grid(4, 60.0)
    ts = mc.send_times(rng, n_sends)
    pos = lambda j: (float(x[j]), float(y[j]), float(z[j]))
    specs = [None] * 16
    for j, v in zip((1, 5, 9, 13), mc.velocities(rng, 4, 60.0)):
        specs[j] = mc.cv(v)
    for j in (2, 6, 10):
        specs[j] = ("acc", mc.velocities(rng, 1, 30.0)[0], mc.velocities(rng, 1, 40.0)[0])
    specs[0] = ("wp", path(rng, pos(0), [0]))
    specs[3] = ("wp", path(rng, pos(3), [0, ts[-1] + 1_000_000_000], 90.0))
    specs[4] = ("wp", path(rng, pos(4), np.linspace(ts[2] + 777, ts[30] + 333, 7).astype(np.int64)))
    gap = ts[11] - ts[10]
    specs[7] = ("wp", path(rng, pos(7), [ts[3] + 5, ts[8] + 11, ts[10] + gap // 4, ts[10] + gap // 2, ts[10] + 3 * gap // 4,
                                         ts[20] + 17, ts[33] + 1]))
    specs[8] = ("wp", path(rng, pos(8), [ts[5] + 1_234_567, ts[20] + 99]))
    specs[12] = ("wp", path(rng, pos(12), np.linspace(ts[1] + 3, ts[18] - 1_000, 7).astype(np.int64)))
    specs[15] = ("wp", path(rng, pos(15), [0, ts[9], ts[25]]))
    return mc.make(x, y, z, channel, specs, [(ts[k], 5 * k % 16) for k in range(n_sends)], course)


def channels_case(seed):
    """The grid split over channels 1 and 6, and a lone phy on 11 (phy 15, a waypoint phy that also sends): phys on
    other channels than the sender's keep their m_current.time."""
    ch = np.array([1, 6] * 8, np.uint32)
    ch[15] = 11
    return grid_case(seed, channel=ch)


def blocks_case(seed):
    """300 phys (20 x 15, 60 m pitch), all on four-entry waypoint lists, 12 sends: k_wl_move runs two blocks, the
    second partial."""
    rng = np.random.default_rng(seed)
    i = np.arange(300)
    x, y, z = (i % 20) * 60.0, (i // 20) * 60.0, np.zeros(300)
    ts = mc.send_times(rng, 12)
    specs = []
    for j in range(300):
        t = np.sort(rng.integers(0, ts[-1] + 40_000_000, 4))
        t = t + np.arange(4)  # (strictly ascending)
        specs.append(("wp", path(rng, (x[j], y[j], 0.0), t, 20.0)))
    return mc.make(x, y, z, None, specs, [(ts[k], 83 * k % 300) for k in range(12)])


def calls_case(seed):
    """The grid with run-time calls from closures between the sends: five AddWaypoints on phy 3 (its segment holds four:
    it moves), forty on phy 4 (the segment moves four times and outgrows the pool, which is replaced), EndMobility on
    phy 12 and an AddWaypoint after it, SetPosition mid-leg on phy 4's neighbour 7 (sits still, then jumps) and on the
    ended phy 0, reads of phy 7, SetVelocityAndAcceleration on phy 2, SetPosition on the accelerating phy 6, a read of
    phy 10, and models replaced or removed: 1 constant velocity -> acceleration, 2 acceleration -> waypoints,
    8 waypoints -> constant velocity, 11 none -> waypoints, 15 and 10 removed."""
    c = grid_case(seed)
    ts = [t for t, _p in c["sends"]]
    mid = lambda k, d=0: (ts[k] + ts[k + 1]) // 2 + d
    end = ts[-1] + 1_000_000_000
    rng = np.random.default_rng(seed + 1)
    course = []
    for q in range(5):
        course.append(("wp_add", mid(2, q * 10), 3, (end + (q + 1) * 50_000_000, (100.0 + 10 * q, 50.0 - q, 1.0))))
    t4 = c["specs"][4][1][-1][0]
    for q in range(40):
        course.append(("wp_add", mid(4, q * 7), 4, (t4 + (q + 1) * 1_000_003, (60.0 + q, 120.0 - 2 * q, 0.5))))
    course += [
        ("wp_get", mid(6), 7),
        ("acc_set", mid(7), 2, (10.0, -20.0, 1.0), (-30.0, 5.0, 0.0)),
        ("pos", mid(9), 7, (150.0, 40.0, 2.0)),          # mid-leg: sits still until m_next.time, then jumps
        ("pos", mid(10), 0, (10.0, 20.0, 0.0)),          # after the end of a one-waypoint path
        ("wp_get", mid(12), 7),
        ("pos", mid(13), 6, (77.0, 88.0, 0.0)),          # an acceleration phy: the velocity is kept
        ("wp_end", mid(14), 12),
        ("install_acc", mid(15), 1, (33.0, 44.0, 0.0), (20.0, 10.0, 0.0), (-15.0, 25.0, 1.0)),
        ("wp_add", mid(16), 12, (mid(16) + 30_000_000, (200.0, 10.0, 0.0))),   # after EndMobility: a new path starts
        ("wp_add", mid(17), 12, (mid(17) + 90_000_000, (120.0, 60.0, 3.0))),
        ("acc_get", mid(18), 10),
        ("install_wp", mid(19), 2, path(rng, (70.0, 70.0, 0.0), [mid(19) + 5, mid(24), mid(29)])),
        ("install_cv", mid(21), 8, (25.0, -35.0, 0.5)),
        ("install_wp", mid(22), 11, path(rng, (180.0, 120.0, 0.0), [mid(20), mid(26), mid(31)])),
        ("remove", mid(23), 15),
        ("remove", mid(27), 10),
        ("wp_get", mid(28), 4),
    ]
    c["course"] = sorted(course, key=lambda e: e[1])
    return c


def burst_case(seed):
    """Ten sends at one timestamp from one closure (more than NSEND = 8: the batch flushes), the first sender a waypoint
    phy on a fast leg, followed in the same closure by its SetPosition far away; then sends from later closures."""
    rng = np.random.default_rng(seed)
    x, y, z = wifi.grid(4, 60.0)
    t0 = 40_000_000
    specs = [("wp", path(rng, (x[j], y[j], 0.0), [0, 90_000_000, 200_000_000], 25.0)) for j in range(16)]
    specs[0] = ("wp", [(0, (0.0, 0.0, 0.0)), (100_000_000, (15.0, 14.0, 0.0)), (180_000_000, (0.0, 30.0, 1.0))])
    sends = [(t0, p) for p in range(10)] + [(t0 + 55_000_123, 0), (t0 + 101_000_456, 13), (t0 + 150_000_456, 5)]
    c = mc.make(x, y, z, None, specs, sends, course=[("pos", t0, 0, (900.0, 700.0, 0.0))])
    c["burst"] = 10
    return c


CASES = dict(grid=grid_case, channels=channels_case, blocks=blocks_case, calls=calls_case, burst=burst_case)


def plan(case, update_rule=send_updates):
    """mobility_cases.plan, each record with its read: (event, {phy: position after it}, read)."""
    pl = mc.plan(case, update_rule)
    return dict(pl, records=[(ev, touched, read) for (ev, touched), read in zip(pl["records"], pl["reads"])])


def margins(case, pl):
    return mc.reception_margins(case, dict(records=[(e, t) for e, t, _r in pl["records"]]))


def kind_of(m):
    return None if m is None else "cv" if isinstance(m, CvModel) else "wp" if isinstance(m, WaypointModel) else "acc"
