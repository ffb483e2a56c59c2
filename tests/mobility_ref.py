"""Plain-Python restatement of the reference's constant-velocity mobility, the tests' reference for the device
copy (nsgpu_wifil_set_mobility and its neighbours).  Written from src/mobility/model/constant-velocity-helper.cc
and constant-velocity-mobility-model.cc; Python floats are IEEE doubles and `a + b * c` rounds the product and
the sum one after the other, as the reference's x86-64 build does.  Time::GetSeconds is the oracle's
(nsref.get_seconds, the int64x64 arithmetic of nstime.h).

Which models update at a SendPacket follows YansWifiChannel::Send (yans-wifi-channel.cc:84-96): for every phy of
m_phyList other than the sender and on the sender's channel number, GetDelay and CalcRxPower call
MobilityModel::GetDistanceFrom (mobility-model.cc:78-84), which reads the receiver's DoGetPosition and then the
sender's — each an Update.  So every such receiver updates, the sender updates if there is at least one of them
(its later Updates of the same send have a zero delta), and phys on other channels keep their m_lastUpdate."""
import nsref


class CvModel:
    """ConstantVelocityMobilityModel over its ConstantVelocityHelper (times in ns)."""

    def __init__(self, pos, vel=(0.0, 0.0, 0.0), paused=True, last_update=0):
        # ConstantVelocityHelper::ConstantVelocityHelper (constant-velocity-helper.cc:27-42): m_paused (true)
        self.x, self.y, self.z = (float(c) for c in pos)
        self.vx, self.vy, self.vz = (float(c) for c in vel)
        self.paused = bool(paused)
        self.last = int(last_update)

    def update(self, now):
        """ConstantVelocityHelper::Update (constant-velocity-helper.cc:69-84)."""
        delta = int(now) - self.last    # :72-74 Time deltaTime = now - m_lastUpdate
        self.last = int(now)            # :75
        if self.paused:                 # :76-79
            return
        delta_s = nsref.get_seconds(delta)  # :80
        self.x += self.vx * delta_s     # :81
        self.y += self.vy * delta_s     # :82
        self.z += self.vz * delta_s     # :83

    def set_velocity(self, now, vel):
        """ConstantVelocityMobilityModel::SetVelocity (constant-velocity-mobility-model.cc:43-50): Update, the
        helper's SetVelocity (constant-velocity-helper.cc:62-67: m_velocity, m_lastUpdate = Now), Unpause."""
        self.update(now)
        self.vx, self.vy, self.vz = (float(c) for c in vel)
        self.last = int(now)
        self.paused = False

    def pause(self, now, paused=True):
        """Update, then ConstantVelocityHelper::Pause / Unpause (constant-velocity-helper.cc:108-118), as
        RandomWaypointMobilityModel does around its legs."""
        self.update(now)
        self.paused = bool(paused)

    def set_position(self, now, pos):
        """ConstantVelocityMobilityModel::DoSetPosition (constant-velocity-mobility-model.cc:59-64) ->
        ConstantVelocityHelper::SetPosition (constant-velocity-helper.cc:43-49): no Update."""
        self.x, self.y, self.z = (float(c) for c in pos)
        self.vx = self.vy = self.vz = 0.0
        self.last = int(now)

    def get(self, now):
        """DoGetPosition (constant-velocity-mobility-model.cc:53-58: Update first) and DoGetVelocity (:65-69 ->
        ConstantVelocityHelper::GetVelocity, constant-velocity-helper.cc:57-61: zero while paused)."""
        self.update(now)
        vel = (0.0, 0.0, 0.0) if self.paused else (self.vx, self.vy, self.vz)
        return (self.x, self.y, self.z), vel

    def position(self):
        return (self.x, self.y, self.z)


def send_updates(channel, sender):
    """The phys whose model updates at one SendPacket of `sender`, in the order of their first Update."""
    rx = [j for j in range(len(channel)) if j != sender and channel[j] == channel[sender]]
    if not rx:
        return []
    return [rx[0], sender] + rx[1:]


def walk(models, channel, events, update_rule=send_updates):
    """Runs `events` (in dispatch order) over the phys' models.  models[j]: a CvModel or None (a constant-position
    phy).  events: ("send", ts, phy) | ("vel", ts, phy, v) | ("pause", ts, phy, flag) |
    ("pos", ts, phy, p) | ("get", ts, phy).  Returns one record per event: (event, {phy: position after it}) with the
    phys the event updated (models only)."""
    out = []
    for ev in events:
        kind, ts, phy = ev[0], int(ev[1]), int(ev[2])
        touched = {}
        if kind == "send":
            for j in update_rule(channel, phy):
                if models[j] is not None:
                    models[j].update(ts)
                    touched[j] = models[j].position()
        elif models[phy] is None:
            raise ValueError(f"{kind} on a constant-position phy {phy}")
        else:
            m = models[phy]
            if kind == "vel":
                m.set_velocity(ts, ev[3])
            elif kind == "pause":
                m.pause(ts, ev[3])
            elif kind == "pos":
                m.set_position(ts, ev[3])
            elif kind == "get":
                m.get(ts)
            else:
                raise ValueError(kind)
            touched[phy] = m.position()
        out.append((ev, touched))
    return out


def everyone_updates(channel, sender):
    """The variant the channel rule guards against: every phy updates at every send."""
    return list(range(len(channel)))
