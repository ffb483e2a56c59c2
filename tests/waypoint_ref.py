"""Plain-Python restatement of the reference's WaypointMobilityModel and ConstantAccelerationMobilityModel, the
tests' reference for the device copies (nsgpu_wifil_set_waypoints / nsgpu_wifil_set_acceleration and their
neighbours).  Written from src/mobility/model/waypoint-mobility-model.cc and constant-acceleration-mobility-model.cc,
statement by statement, in the style of tests/mobility_ref.py: Python floats are IEEE doubles, `a + b * c` rounds the
product and the sum one after the other and `/` is the IEEE division, as the reference's x86-64 build does;
Time::GetSeconds is the oracle's (nsref.get_seconds).  Times are ns; m_next.time is signed (Seconds (-1) ends a path).

Every model here has update (now), position (), set_position (now, pos): what tests/mobility_ref.py's CvModel has,
so the PHY models of tests/wifi_switch_model.py / tests/lossx_model.py drive any of them.  `hits` counts the branches
a model took, so a test can assert that its case reached the branch it is about."""
import collections

import nsref
from mobility_ref import CvModel, send_updates

ENDED = -1_000_000_000  # Seconds (-1.0)


class WaypointModel:
    """WaypointMobilityModel (lazy: no Update events of its own; InitialPositionIsWaypoint false)."""

    def __init__(self, waypoints=()):
        # WaypointMobilityModel::WaypointMobilityModel (:67-72); Waypoint () is (Seconds (0), Vector (0, 0, 0))
        self.first = True
        self.cur_t, self.cur = 0, (0.0, 0.0, 0.0)
        self.next_t, self.next = 0, (0.0, 0.0, 0.0)
        self.vel = (0.0, 0.0, 0.0)
        self.queue = collections.deque()
        self.hits = collections.Counter()
        for t, p in waypoints:
            self.add_waypoint(t, p)

    def add_waypoint(self, t, pos):
        """AddWaypoint (:82-100).  Raises ValueError where the reference aborts (:91)."""
        t, pos = int(t), tuple(float(c) for c in pos)
        if self.first:                                            # :84-88
            self.first = False
            self.cur_t, self.cur = t, pos
            self.next_t, self.next = t, pos
            self.hits["add_first"] += 1
        else:
            if self.queue and self.queue[-1][0] >= t:             # :91
                raise ValueError("Waypoints must be added in ascending time order")
            self.queue.append((t, pos))                           # :93
            self.hits["add_queued"] += 1

    def update(self, now):
        """Update (:114-173)."""
        now = int(now)
        if now < self.cur_t:                                      # :119-122
            self.hits["early"] += 1
            return
        crossed = 0
        while now >= self.next_t:                                 # :124
            if not self.queue:                                    # :126
                if self.cur_t <= self.next_t:                     # :128
                    self.next_t = ENDED                           # :134
                    self.cur = self.next                          # :135
                    self.cur_t = now                              # :136
                    self.vel = (0.0, 0.0, 0.0)                    # :137
                    self.hits["ended"] += 1
                else:
                    self.cur_t = now                              # :142
                    self.hits["after_end"] += 1
                return                                            # :145
            self.cur_t, self.cur = self.next_t, self.next         # :148
            self.next_t, self.next = self.queue.popleft()         # :149-150
            crossed += 1
            t_span = nsref.get_seconds(self.next_t - self.cur_t)  # :153
            assert t_span > 0                                     # :154
            self.vel = ((self.next[0] - self.cur[0]) / t_span,    # :155-157
                        (self.next[1] - self.cur[1]) / t_span,
                        (self.next[2] - self.cur[2]) / t_span)
        self.hits["crossed_%d" % crossed] += 1
        if now > self.cur_t:                                      # :160
            t_diff = nsref.get_seconds(now - self.cur_t)          # :162
            self.cur = (self.cur[0] + self.vel[0] * t_diff,       # :163-165
                        self.cur[1] + self.vel[1] * t_diff,
                        self.cur[2] + self.vel[2] * t_diff)
            self.cur_t = now                                      # :166
            self.hits["advanced"] += 1

    def position(self):
        return self.cur

    def velocity(self):
        """DoGetVelocity (:211-214): no Update."""
        return self.vel

    def set_position(self, now, pos):
        """DoSetPosition (:181-201)."""
        now = int(now)
        self.update(now)                                          # :191
        self.cur_t = max(now, self.next_t)                        # :192
        self.cur = tuple(float(c) for c in pos)                   # :193
        self.vel = (0.0, 0.0, 0.0)                                # :194
        self.hits["set_position_waits" if self.cur_t > now else "set_position_now"] += 1

    def end(self):
        """EndMobility (:203-209); Time (std::numeric_limits<uint64_t>::infinity ()) is Time (0): an integer type has
        no infinity."""
        self.queue.clear()
        self.cur_t = 0
        self.next_t = 0
        self.first = True
        self.hits["end"] += 1

    def left(self):
        return len(self.queue)

    def state(self):
        """The members as wifi.waypoint_record gives the device's."""
        ended = self.next_t == ENDED
        return dict(cur=(self.cur_t, self.cur), next=(None if ended else self.next_t, self.next), vel=self.vel,
                    first=self.first, left=len(self.queue))

    def get(self, now):
        """DoGetPosition (:174-179: Update first), then the members — what nsgpu_wifil_get_waypoints returns."""
        self.update(now)
        return self.state()


class AccelModel:
    """ConstantAccelerationMobilityModel.  The model stores no current position; `seen` is where the phy was last
    seen — the position its last read at a send computed, or the one SetPosition gave it — which is what a receiver
    loop holds for it and where it stays if the model is removed (before the first read: `seen` as given)."""

    def __init__(self, pos, vel=(0.0, 0.0, 0.0), acc=(0.0, 0.0, 0.0), base_time=0, seen=None):
        self.base = tuple(float(c) for c in pos)
        self.vel = tuple(float(c) for c in vel)
        self.acc = tuple(float(c) for c in acc)
        self.base_t = int(base_time)
        self.seen = self.base if seen is None else tuple(float(c) for c in seen)
        self.hits = collections.Counter()

    def get_velocity(self, now):
        """DoGetVelocity (:41-48)."""
        t = nsref.get_seconds(int(now) - self.base_t)
        return tuple(self.vel[c] + self.acc[c] * t for c in range(3))

    def get_position(self, now):
        """DoGetPosition (:50-58): (base + v * t) + a * half_t_square."""
        t = nsref.get_seconds(int(now) - self.base_t)
        half_t_square = t * t * 0.5
        return tuple(self.base[c] + self.vel[c] * t + self.acc[c] * half_t_square for c in range(3))

    def update(self, now):
        self.seen = self.get_position(now)

    def position(self):
        return self.seen

    def set_position(self, now, pos):
        """DoSetPosition (:60-67)."""
        self.vel = self.get_velocity(now)
        self.base_t = int(now)
        self.base = self.seen = tuple(float(c) for c in pos)
        self.hits["set_position"] += 1

    def set_velocity_and_acceleration(self, now, vel, acc):
        """SetVelocityAndAcceleration (:69-78)."""
        self.base = self.get_position(now)
        self.base_t = int(now)
        self.vel = tuple(float(c) for c in vel)
        self.acc = tuple(float(c) for c in acc)
        self.hits["set_va"] += 1

    def get(self, now):
        """What nsgpu_wifil_get_acceleration returns (wifi.accel_record): no state changes."""
        return dict(pos=self.base, vel=self.vel, acc=self.acc, base_time=self.base_t, now_pos=self.get_position(now),
                    now_vel=self.get_velocity(now))


def walk(models, channel, events, update_rule=send_updates, positions=None):
    """tests/mobility_ref.walk over mixed models.  models[j]: CvModel, WaypointModel, AccelModel or None; the list is
    changed in place by the install events.  events, in dispatch order:
      ("send", ts, phy) | ("pos", ts, phy, p) — any model's SetPosition
      CvModel: ("vel", ts, phy, v) | ("pause", ts, phy, flag) | ("get", ts, phy)
      WaypointModel: ("wp_add", ts, phy, (t, p)) | ("wp_end", ts, phy) | ("wp_get", ts, phy)
      AccelModel: ("acc_set", ts, phy, v, a) | ("acc_get", ts, phy)
      ("install_wp", ts, phy, waypoints) | ("install_acc", ts, phy, pos, vel, acc) | ("install_cv", ts, phy, vel) |
      ("remove", ts, phy): one model replaces another; a removed one leaves the phy where its last update did.
    positions: every phy's position at setup (needed when a phy without a model is given one mid-run).
    Returns one record per event: (event, {phy: position after it}, read) — read: what a *_get returned, else None."""
    out = []
    last = dict(enumerate(positions or ()))  # where a phy was last seen (for the phys without a model)
    for ev in events:
        kind, ts, phy = ev[0], int(ev[1]), int(ev[2])
        touched, read = {}, None
        if kind == "send":
            for j in update_rule(channel, phy):
                if models[j] is not None:
                    models[j].update(ts)
                    touched[j] = models[j].position()
        else:
            m = models[phy]
            if kind == "install_wp":
                m = models[phy] = WaypointModel(ev[3])
            elif kind == "install_acc":
                m = models[phy] = AccelModel(ev[3], ev[4], ev[5], base_time=ts, seen=m.position() if m is not None else last[phy])
            elif kind == "install_cv":
                m = models[phy] = CvModel(m.position() if m is not None else last[phy], ev[3], paused=False, last_update=ts)
            elif kind == "remove":
                touched[phy] = m.position()
                m = models[phy] = None
            elif kind == "pos":
                m.set_position(ts, ev[3])
            elif kind == "vel":
                m.set_velocity(ts, ev[3])
            elif kind == "pause":
                m.pause(ts, ev[3])
            elif kind == "get":
                read = m.get(ts)
            elif kind == "wp_add":
                m.add_waypoint(*ev[3])
            elif kind == "wp_end":
                m.end()
            elif kind == "wp_get":
                read = m.get(ts)
            elif kind == "acc_set":
                m.set_velocity_and_acceleration(ts, ev[3], ev[4])
            elif kind == "acc_get":
                read = m.get(ts)
            else:
                raise ValueError(kind)
            if m is not None:
                touched[phy] = m.position()
        last.update(touched)
        out.append((ev, touched, read))
    return out
