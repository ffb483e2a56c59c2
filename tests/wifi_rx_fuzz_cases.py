"""Seeded cross-feature scenarios of the open-loop Wi-Fi receive engine (csrc/nsgpu_wifi.hip, wifi.Engine).
tests/test_wifi_rx_fuzz_cpu.py asserts, on the two CPU restatements alone, that every committed case reaches what it
is there for; tests/test_gpu_wifi_rx_fuzz.py runs each case through every pipeline of the device engine.

build (family, seed) rebuilds a case from numpy.random.default_rng ([family's tag, seed]) — nothing else decides it.
A case: dict (family, seed, sc (wifi.Scenario), model (the Python model runs it), expect ("equal", "pending",
"window"), rx_log (the GPU test reads the Receive log), and the figures the family states: see each builder).

Families (CASES lists the committed seeds):
  mixed    20-200 phys, 1-3 channels, 150-400 frames of seven modes (28 us to 18.6 ms), 14-2304 B, a transmit power
           per frame, node ids a permutation with gaps, six loss chains, three Stop variants (after the last event,
           none, inside the schedule — once at the very ts of a frame).
  near     phys 0 m / 0.05 m / 0.14 m apart (0 ns delay), pairs at a loss model's reference / minimum / range
           distance and 2^-20 either side, (3, 4, 5) and (5, 12, 13) lattice rings around one receiver; simultaneous
           sends of symmetric senders, a frame arriving in the nanosecond of an EndReceive, a zero-delay neighbour
           sending in the nanosecond it receives.
  burst    W senders (63, 64, 65, 80) inside one arrival spread, frames before and after.
  pending  a victim syncs to a long frame, cancels it with a short frame of its own, syncs to the next sender's long
           frame ...: 5, PE_CAP, PE_CAP + 1 pending EndReceives; one seed with three victims.
  queues   ni_cap at the edge (the list reaches a power of two exactly, and Receives follow), a hundred
           transmissions on the air at once, a start-queue overflow in the middle of a run.
  blocks   1023 ... 65,600 phys (the phys-per-block values), 20-40 frames, 2 channels: the C++ oracle only."""
import math

import numpy as np

import nsgpu
import nsref
import wifi

US, MS = 1_000, 1_000_000
LONG, SHORT = wifi.PREAMBLE_LONG, wifi.PREAMBLE_SHORT
# the library's capacities the families aim at (csrc/nsgpu_wifi.hip)
PE_CAP, SCAP_LDS, WSORT_MAX = 8, 8, 64
TAGS = dict(mixed=11, near=12, burst=13, pending=14, queues=15, blocks=16)

DSSS1 = ((wifi.DSSS, 1_000_000, 22_000_000), LONG)
DSSS11 = ((wifi.DSSS, 11_000_000, 22_000_000), LONG)
DSSS11S = ((wifi.DSSS, 11_000_000, 22_000_000), SHORT)
OFDM6 = ((wifi.OFDM, 6_000_000, 20_000_000), LONG)
OFDM54 = ((wifi.OFDM, 54_000_000, 20_000_000), LONG)
ERP12 = ((wifi.ERP_OFDM, 12_000_000, 20_000_000), LONG)
OFDM6_10 = ((wifi.OFDM, 6_000_000, 10_000_000), LONG)
OFDM1_5_5 = ((wifi.OFDM, 1_500_000, 5_000_000), LONG)
MODES = (DSSS1, DSSS11, DSSS11S, OFDM6, OFDM54, ERP12, OFDM6_10, OFDM1_5_5)

LOG = (nsgpu.LOSS_LOG_DISTANCE, 3.0, 1.0, 46.6777)  # YansWifiChannelHelper::Default
FRIIS = (nsgpu.LOSS_FRIIS, 0.125, 1.0, 0.5)         # 2.4 GHz, MinDistance 0.5 m
# chain kind -> (links, area (m) in which syncs, drops and below-ED receptions all occur, ED / CCA thresholds dBm, RxGain).
# "fixed": a FixedRss link alone gives every reception one power (all sync, or none): the Range link behind it cuts
# the far ones off (near runs FixedRss alone).  "none": rx = tx + RxGain whatever the distance: RxGain -100 dB puts
# the frames' 0 to 20 dBm at -100 to -80 dBm, and the thresholds move between them.
#
# Received powers stay below about 1e-9 W in every family (phys keep a distance, co-located phys send at -75 dBm):
# m_firstPower keeps, of powers added and taken away again, a residue of their last bits, and the device's pow gives
# some powers one ulp from glibc's — the comparison's atol of 1e-24 W covers that residue only for such powers.
CHAINS = dict(
    log=((LOG,), (600.0, 300.0), -96.0, -99.0, 1.0),
    friis=((FRIIS,), (6000.0, 3000.0), -96.0, -99.0, 1.0),
    log_range=((LOG, (nsgpu.LOSS_RANGE, 150.0, 0.0, 0.0)), (600.0, 300.0), -96.0, -99.0, 1.0),
    fixed=(((nsgpu.LOSS_FIXED_RSS, -80.0, 0.0, 0.0), (nsgpu.LOSS_RANGE, 200.0, 0.0, 0.0)), (600.0, 300.0), -96.0, -99.0,
           1.0),
    none=((), (300.0, 300.0), -89.0, -94.0, -100.0),
    three=((FRIIS, (nsgpu.LOSS_LOG_DISTANCE, 1.0, 50.0, 0.0), (nsgpu.LOSS_RANGE, 2500.0, 0.0, 0.0)), (3000.0, 1500.0),
           -96.0, -99.0, 1.0),
    friis_lossy=(((nsgpu.LOSS_FRIIS, 0.125, 1000.0, 0.5),), None, -96.0, -99.0, 1.0),  # (SystemLoss 30 dB: near)
    fixed_alone=(((nsgpu.LOSS_FIXED_RSS, -80.0, 0.0, 0.0),), None, -96.0, -99.0, 1.0),
)
CHAIN_KINDS = ("log", "friis", "log_range", "fixed", "none", "three")
STOPS = ("after", "none", "inside")


def dur(size, mp):
    return int(wifi.tx_duration_ns(int(size), mp[0], mp[1]))


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


class Sched:
    """The harness's Simulator::Schedule (t, &YansWifiPhy::SendPacket, ...) calls in call order (the setup uids)."""

    def __init__(self):
        self.rows, self.air = [], {}

    def free(self, t, s, d):
        return not any(t <= e and t + d >= b for b, e in self.air.get(s, ()))

    def add(self, t, s, size, mp, dbm):
        """False (and nothing added) when phy s would still be sending: the reference's NS_FATAL_ERROR."""
        t, s, d = int(t), int(s), dur(size, mp)
        if not self.free(t, s, d):
            return False
        self.air.setdefault(s, []).append((t, t + d))
        self.rows.append((t, s, int(size), mp, float(dbm)))
        return True

    def must(self, *a):
        assert self.add(*a), a

    def last_end(self):
        return max(e for v in self.air.values() for _, e in v)

    def tx(self):
        tx = np.zeros(len(self.rows), wifi.TX_DTYPE)
        order = sorted(range(len(self.rows)), key=lambda i: (self.rows[i][0], i))
        for r, i in enumerate(order):
            t, s, size, (m, pre), dbm = self.rows[i]
            tx[r] = (t, 4 + i, s, size, dbm, m[0], m[1], m[2], pre)
        return tx


def scenario(x, y, z, sched, chain="log", channel=None, node=None, stop="after", stop_ts=None, ni_cap=512):
    links, _, ed, cca, gain = CHAINS[chain]
    tx = sched.tx()
    n = len(tx)
    if stop == "after":
        stop_ts = sched.last_end() + 2 * MS
    elif stop == "none":
        stop_ts = wifi.NO_STOP
    return wifi.Scenario(x, y, z, tx, channel=channel, node=node, loss=tuple(links), rx_gain_db=gain,
                         ed_threshold_dbm=ed, cca_threshold_dbm=cca, uid_start=5 + n, stop_ts=stop_ts, stop_uid=4 + n, ni_cap=ni_cap)


def spaced(rng, n, w, h, dmin, fixed=()):
    """n random positions in w x h (z in 0 to 3 m), at least dmin from each other and from `fixed`."""
    pts = [tuple(p) for p in fixed]
    while len(pts) < len(fixed) + n:
        p = (float(rng.random() * w), float(rng.random() * h), float(rng.random() * 3.0))
        if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 >= dmin * dmin for q in pts):
            pts.append(p)
    return tuple(np.array([p[i] for p in pts]) for i in range(3))


def gap_nodes(rng, n):
    """Node ids: a permutation with gaps."""
    return (rng.permutation(n) * 3 + 7).astype(np.uint32)


# ---- the schedule-derived figures nsgpu_wifi_create sizes its queues from (include/nsgpu.h), restated ----
def dispatched(sc):
    """Transmissions with a key below the Stop event's."""
    if sc.stop_ts == wifi.NO_STOP:
        return len(sc.tx)
    return int(sum(1 for t in sc.tx if (int(t["ts"]), int(t["uid"])) < (sc.stop_ts, sc.stop_uid)))


def spread_ns(sc):
    """The arrival spread: the bounding box's diagonal at the propagation speed, rounded up, + 2 ns."""
    d = math.sqrt(sum(float(np.ptp(a)) ** 2 for a in (sc.x, sc.y, sc.z)))
    return int(math.ceil(d / sc.speed * 1e9)) + 2


def durations(sc):
    return [int(wifi.tx_duration_ns(int(t["size"]), (int(t["modclass"]), int(t["rate"]), int(t["bw"])), int(t["preamble"])))
            for t in sc.tx]


def overlap(sc):
    """Most dispatched transmissions whose [ts, ts + spread + duration] holds one instant (closed intervals)."""
    k, dm, du = dispatched(sc), spread_ns(sc), durations(sc)
    ts = [int(t) for t in sc.tx["ts"][:k]]
    ends = sorted(t + dm + d for t, d in zip(ts, du))
    best = gone = 0
    for i, t in enumerate(ts):
        while ends[gone] < t:
            gone += 1
        best = max(best, i + 1 - gone)
    return best


def largest_window(sc):
    """Most dispatched transmissions within one arrival spread of one of them (either side)."""
    k, dm = dispatched(sc), spread_ns(sc)
    ts = np.asarray(sc.tx["ts"][:k], np.int64)
    return int(max((np.searchsorted(ts, t + dm, "right") - np.searchsorted(ts, t - dm, "left") for t in ts), default=0))


def lds_plan(sc, own, n_cu, lds_max):
    """(phys per block, end-queue capacity, most phys a block's LDS holds) of the split-queue store for `own`
    receivers on a device of n_cu CUs and lds_max B of LDS a block (include/nsgpu.h: nsgpu_wifi_set_store)."""
    ecap = max(overlap(sc) + 2, 8) if dispatched(sc) else 8
    per = (SCAP_LDS + ecap) * 16 + ecap * 8 + PE_CAP * 28
    pmax = min(64, lds_max // per)
    return max(1, min(-(-max(own, 1) // (4 * n_cu)), pmax)), ecap, pmax


def ni_pow2(v):
    """The capacity the library rounds ni_cap up to."""
    c = 4
    while c < v:
        c <<= 1
    return c


# ---------------------------------------------------------------- mixed
def random_frames(rng, sched, senders, n_frames, t0, span, modes=MODES, sizes=(14, 2305), dbm=(0.0, 20.0)):
    left = n_frames
    while left:
        size = int(rng.integers(*sizes))
        if sched.add(t0 + int(rng.integers(span)), pick(rng, senders), size, pick(rng, modes), rng.uniform(*dbm)):
            left -= 1


def mixed(seed):
    rng = np.random.default_rng([TAGS["mixed"], seed])
    kind, stop = CHAIN_KINDS[seed % 6], STOPS[seed % 3]
    n = int(rng.integers(20, 201))
    frames = min(int(rng.integers(150, 401)), max(150, 36_000 // n))
    chans = (1, 6, 11)[:int(rng.integers(1, 4))]
    area = CHAINS[kind][1]
    x, y, z = spaced(rng, n, area[0], area[1], area[0] / 40.0)
    channel = np.asarray(chans, np.uint32)[rng.integers(0, len(chans), n)]
    sched = Sched()
    random_frames(rng, sched, range(n), frames, 1000, frames * 300 * US)
    stop_ts = None
    if stop == "inside":  # at the ts of a frame (even seeds: that frame still runs, its Receives never do) or just after
        ts = sorted(r[0] for r in sched.rows)
        stop_ts = ts[int(0.6 * frames)] + (0 if seed % 2 == 0 else 137)
    sc = scenario(x, y, z, sched, kind, channel, gap_nodes(rng, n), stop, stop_ts)
    return dict(sc=sc, chain=kind, stop=stop, model=True)


# ---------------------------------------------------------------- near
RING_A = [(sx * a, sy * b) for a, b in ((3, 4), (4, 3)) for sx in (1, -1) for sy in (1, -1)] + \
         [(5, 0), (-5, 0), (0, 5), (0, -5)]                      # 12 at 5 units
RING_B = [(5, 12), (-5, 12), (12, -5), (-12, -5), (13, 0), (0, -13)]  # 6 at 13 units
NEAR_CHAINS = ("log", "friis_lossy", "log_range", "fixed_alone", "none")
CLUSTER_DBM = -75.0  # co-located phys (and phys a reference distance apart): heard among themselves only


def near(seed):
    rng = np.random.default_rng([TAGS["near"], seed])
    kind = NEAR_CHAINS[seed % 5]
    edge = dict(log=1.0, friis_lossy=0.5, log_range=150.0, fixed_alone=1.0, none=1.0)[kind]  # reference / minimum / range
    pts = [(1000.0, 1000.0, 0.0)]                                       # R, the rings' receiver
    pts += [(1000.0 + 10.0 * a, 1000.0 + 10.0 * b, 0.0) for a, b in RING_A + RING_B]
    ra, rb = list(range(1, 13)), list(range(13, 19))
    c0 = len(pts)                                                       # the zero-delay cluster
    pts += [(1200.0, 1000.0, 1.0), (1200.0, 1000.0, 1.0), (1200.05, 1000.0, 1.0), (1200.0, 1000.14, 1.0)]
    g0 = len(pts)                                                       # the edge-distance group
    pts += [(1000.0, 1300.0, 0.0), (1000.0 + edge, 1300.0, 0.0), (1000.0, 1300.0 + edge * (1 - 2.0 ** -20), 0.0),
            (1000.0 - edge * (1 + 2.0 ** -20), 1300.0, 0.0)]
    nb = int(rng.integers(5, 16))                                       # bystanders
    by = list(range(len(pts), len(pts) + nb))
    x, y, z = spaced(rng, nb, 2000.0, 2000.0, 15.0, fixed=pts)
    pts = list(zip(x.tolist(), y.tolist(), z.tolist()))
    n = len(pts)
    channel = np.ones(n, np.uint32)
    if seed % 2:  # some bystanders on a second channel
        channel[by[::2]] = 6

    def delay(a, b):  # ConstantSpeedPropagationDelayModel::GetDelay between two phys, ns
        return int(nsref.lib().nsref_const_speed_delay(nsref.lib().nsref_distance(*pts[a], *pts[b]), 3e8))
    dA, dB = delay(0, ra[0]), delay(0, rb[0])
    sched = Sched()
    fr = lambda: (int(rng.integers(14, 2305)), pick(rng, MODES))  # noqa: E731
    P = lambda: float(rng.uniform(0.0, 20.0))  # noqa: E731
    PC = P if kind == "none" else (lambda: CLUSTER_DBM)              # the cluster's frames
    PG = P if kind == "none" or edge > 1.0 else (lambda: CLUSTER_DBM)  # the edge-distance group's
    T = 1 * MS
    # 1. symmetric senders at once: 6 of ring A (equal arrivals at R), then 4 of ring B with 2 of ring A timed to meet them
    size, mp = fr()
    for s in ra[:6]:
        sched.must(T, s, size, mp, P())
    T += 25 * MS
    for s in rb[:4]:
        sched.must(T, s, *fr(), P())
    for s in ra[6:8]:
        sched.must(T + dB - dA, s, *fr(), P())
    T += 25 * MS
    # 2. a frame arriving at R in the nanosecond of R's EndReceive (R idle: it syncs to ring A's frame)
    size, mp = fr()
    sched.must(T, ra[8], size, mp, 20.0)
    sched.must(T + dA + dur(size, mp) - dB, rb[4], *fr(), P())
    T += 25 * MS
    # 3. a far sender; a cluster phy sends in the nanosecond the frame arrives (its neighbours 0 ns away sync then)
    size, mp = fr()
    sched.must(T, rb[5], size, mp, 20.0)
    sched.must(T + delay(rb[5], c0 + 1), c0 + 1, *fr(), PC())
    T += 25 * MS
    # 4. two co-located phys send at once; a third starts exactly when the first one's frame ends, 0 ns away
    size, mp = fr()
    sched.must(T, c0, size, mp, PC())
    sched.must(T, c0 + 1, *fr(), PC())
    sched.must(T + dur(size, mp), c0 + 2, *fr(), PC())
    T += 45 * MS
    # 5. a cluster phy and a ring phy at one ts (the cluster's syncs fall on the ring frame's ts, a later uid)
    sched.must(T, c0 + 3, *fr(), PC())
    sched.must(T, ra[9], *fr(), P())
    T += 25 * MS
    # 6. the edge-distance group, each in turn, then two of them at once
    for q in range(4):
        size, mp = fr()
        sched.must(T, g0 + q, size, mp, PG())
        T += dur(size, mp) + 2 * MS
    sched.must(T, g0, *fr(), PG())
    sched.must(T, g0 + 3, *fr(), PG())
    T += 25 * MS
    # 7. everybody, at random, over the episodes
    random_frames(rng, sched, [0] + ra + rb + by, 40, 1000, T)
    sc = scenario(x, y, z, sched, kind, channel, gap_nodes(rng, n), ("after", "none")[seed % 2])
    return dict(sc=sc, chain=kind, model=True)


# ---------------------------------------------------------------- burst
BURST_W = (63, 64, 65, 80)


def burst(seed):
    rng = np.random.default_rng([TAGS["burst"], seed])
    w = BURST_W[seed % 4]
    n = max(100, w + 30) + int(rng.integers(0, 20))
    x, y, z = spaced(rng, n - 2, 2400.0, 1800.0, 120.0, fixed=[(0.0, 0.0, 0.0), (2400.0, 1800.0, 3.0)])  # 3000 m: 10 us
    channel = np.asarray((1, 6), np.uint32)[rng.integers(0, 2, n)]
    dm = int(math.ceil(math.sqrt(2400.0 ** 2 + 1800.0 ** 2 + float(np.ptp(z)) ** 2) / 3e8 * 1e9)) + 2
    sched = Sched()
    short = (OFDM54, ERP12, DSSS11S)
    t = 1000
    for _ in range(20):  # before: one frame every 60 us (more than the spread apart)
        while not sched.add(t, int(rng.integers(n)), int(rng.integers(14, 200)), pick(rng, short), rng.uniform(0, 20)):
            pass
        t += 60 * US
    t += 40 * MS
    senders = rng.permutation(n)[:w]
    offs = np.sort(rng.choice(dm - 1, w, replace=False))
    offs[0], offs[-1] = 0, dm - 2 if w > 1 else 0
    for s, o in zip(senders, offs):
        sched.must(t + int(o), s, int(rng.integers(14, 2305)), pick(rng, MODES), rng.uniform(0, 20))
    t += 40 * MS
    for _ in range(20):
        while not sched.add(t, int(rng.integers(n)), int(rng.integers(14, 200)), pick(rng, short), rng.uniform(0, 20)):
            pass
        t += 60 * US
    sc = scenario(x, y, z, sched, "friis", channel, gap_nodes(rng, n))
    return dict(sc=sc, window=w, model=True, expect="equal" if w <= WSORT_MAX else "window")


# ---------------------------------------------------------------- pending
PENDING = ((5, 1), (PE_CAP, 1), (PE_CAP + 1, 1), (PE_CAP, 3))  # (pending EndReceives, victims)


def pending(seed):
    rng = np.random.default_rng([TAGS["pending"], seed])
    m, nv = PENDING[seed % 4]
    n = m + nv + int(rng.integers(6, 14))
    x, y, z = spaced(rng, n, 100.0, 60.0, 12.0)  # (every long frame above ED everywhere)
    victims = [int(rng.integers(n))] if nv == 1 else [0, n // 2, n - 1]
    others = [j for j in rng.permutation(n) if j not in victims]
    senders = [int(j) for j in others[:m]]
    sched = Sched()
    longf, shortf = (2304, DSSS1), (lambda: (int(rng.integers(14, 100)), OFDM54))

    def cycles(t0, count):
        for i in range(count):
            t = t0 + i * 300 * US + int(rng.integers(20 * US))
            sched.must(t, senders[i], *longf, 16.0)            # every victim idle / CCA-busy: it syncs
            if i + 1 < count:
                for v in victims:                              # ... and cancels with a frame of its own, all at once
                    sched.must(t + 150 * US, v, *shortf(), rng.uniform(0, 14))
    cycles(1 * MS, m)                    # m EndReceives pending at each victim before the first one's 18.6 ms run out
    t = sched.last_end() + 1 * MS
    random_frames(rng, sched, range(n), 6, t, 10 * MS, modes=(OFDM54, ERP12, OFDM6), sizes=(14, 400), dbm=(0.0, 14.0))
    cycles(sched.last_end() + 1 * MS, min(3, m))  # the slots again
    sc = scenario(x, y, z, sched, "log", None, gap_nodes(rng, n), ni_cap=64)
    return dict(sc=sc, victims=victims, pe_max=m, model=True, expect="equal" if m <= PE_CAP else "pending")


# ---------------------------------------------------------------- queues
def queues_ni(seed, rng):
    """One long frame every phy syncs to, m short frames during it (nobody folds: 2 + 2 m entries), then Receives
    after it (the first fold: the list is at its longest just before), then the same with one frame fewer."""
    m = (7, 15)[(seed // 3) % 2]
    n = m + 2 + int(rng.integers(3, 8))
    x, y, z = spaced(rng, n, 100.0, 60.0, 12.0)
    order = [int(j) for j in rng.permutation(n)]
    sched = Sched()

    def wave(t0, count):
        sched.must(t0, order[0], 2304, DSSS1, 16.0)
        for i in range(count):
            sched.must(t0 + 1 * MS + i * 200 * US, order[1 + i], int(rng.integers(14, 100)), OFDM54, rng.uniform(0, 14))
    wave(1 * MS, m)
    t = sched.last_end() + 1 * MS
    for i in range(5):
        sched.must(t + i * MS, order[1 + i % m], int(rng.integers(14, 400)), pick(rng, (OFDM54, ERP12)), rng.uniform(0, 14))
    wave(sched.last_end() + 1 * MS, m - 1)
    sc = scenario(x, y, z, sched, "log", None, gap_nodes(rng, n), ni_cap=2 + 2 * m)
    return dict(sc=sc, variant="ni", ni_max=2 + 2 * m, ni_below=1 + m, model=True)


def queues_deep(seed, rng):
    """Waves of 100-110 senders starting within 200 us, frames of 0.3 to 2.2 ms: about a hundred on the air at once
    (the end queues of 64 phys then pass 160 KB of LDS, those of 23 pass 64 KB)."""
    n = 130 + int(rng.integers(0, 10))
    x, y, z = spaced(rng, n, 300.0, 300.0, 15.0)
    sched = Sched()
    t = 1 * MS
    for _ in range(2):
        for s in rng.permutation(n)[:int(rng.integers(100, 111))]:
            sched.must(t + int(rng.integers(200 * US)), s, int(rng.integers(200, 800)), pick(rng, (OFDM6, ERP12, OFDM6_10)),
                       rng.uniform(0, 20))
        t += 6 * MS
        random_frames(rng, sched, range(n), 10, t, 3 * MS, modes=(OFDM54, ERP12, DSSS11S), sizes=(14, 400))
        t += 6 * MS
    sc = scenario(x, y, z, sched, "log", None, gap_nodes(rng, n))
    return dict(sc=sc, variant="deep", overlap_min=91, model=True)


def queues_overflow(seed, rng):
    """Frames before and after; in the middle ring A's 12 senders at once: 12 starts at R in one nanosecond, 11 of
    them while it receives (SCAP_LDS is 8)."""
    nb = int(rng.integers(6, 14))
    pts = [(500.0, 500.0, 0.0)] + [(500.0 + 8.0 * a, 500.0 + 8.0 * b, 0.0) for a, b in RING_A + RING_B]
    x, y, z = spaced(rng, nb, 1000.0, 1000.0, 15.0, fixed=pts)
    n = len(x)
    sched = Sched()
    random_frames(rng, sched, range(n), 15, 1000, 30 * MS, sizes=(14, 1200))
    t = sched.last_end() + 1 * MS
    for s in range(1, 13):
        sched.must(t, s, int(rng.integers(14, 2305)), pick(rng, MODES), rng.uniform(5, 20))
    t = sched.last_end() + 1 * MS
    for s in range(13, 19):  # (6 at once: within the start queue)
        sched.must(t, s, int(rng.integers(14, 1200)), pick(rng, MODES), rng.uniform(5, 20))
    random_frames(rng, sched, range(n), 15, sched.last_end() + 1 * MS, 30 * MS, sizes=(14, 1200))
    sc = scenario(x, y, z, sched, "log", None, gap_nodes(rng, n))
    return dict(sc=sc, variant="overflow", starts_max=12, model=True)


def queues(seed):
    rng = np.random.default_rng([TAGS["queues"], seed])
    return (queues_ni, queues_deep, queues_overflow)[seed % 3](seed, rng)


# ---------------------------------------------------------------- blocks
BLOCK_PHYS = (1023, 1024, 1025, 2049, 4100, 9217, 65_600)


def blocks(seed):
    rng = np.random.default_rng([TAGS["blocks"], seed])
    n = BLOCK_PHYS[seed % 7]
    # a 40 m grid's cells in random order, each phy 8 to 32 m into its cell (LogDistance: a frame is above ED within 50
    # to 220 m, by its power; no two phys closer than 16 m)
    side = math.isqrt(n - 1) + 1
    cell = rng.permutation(side * side)[:n]
    x, y = (cell % side) * 40.0 + rng.uniform(8.0, 32.0, n), (cell // side) * 40.0 + rng.uniform(8.0, 32.0, n)
    z = rng.random(n) * 3.0
    channel = np.asarray((1, 6), np.uint32)[rng.integers(0, 2, n)]
    sched = Sched()
    frames = int(rng.integers(20, 41))
    random_frames(rng, sched, range(n), frames, 1000, frames * 2 * MS)
    sc = scenario(x, y, z, sched, "log", channel, gap_nodes(rng, n), ni_cap=128)
    return dict(sc=sc, model=False, rx_log=n < 9000)


FAMILIES = dict(mixed=mixed, near=near, burst=burst, pending=pending, queues=queues, blocks=blocks)
CASES = [("mixed", s) for s in range(6)] + [("near", s) for s in range(5)] + [("burst", s) for s in range(4)] + \
        [("pending", s) for s in range(4)] + [("queues", s) for s in range(6)] + [("blocks", s) for s in range(7)]


def build(family, seed):
    c = dict(family=family, seed=seed, expect="equal", rx_log=True)
    c.update(FAMILIES[family](seed))
    return c


def case_id(fs):
    return f"{fs[0]}-{fs[1]}"
