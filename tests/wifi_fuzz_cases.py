"""Seeded cross-feature scenarios of the closed-loop Wi-Fi PHY: notes, the EndReceive hand-back with MAC replies, the
three mobility models, channel switching, mid-run loss chains and frames of many modes in one run.
tests/test_wifi_fuzz_cpu.py asserts on the model alone (tests/wifi_fuzz_model.py) that every committed case is accepted
and that the set reaches the interactions it is there for; tests/test_gpu_wifi_fuzz.py runs each case on the device.

build (family, seed) rebuilds a case from numpy.random.default_rng ([family's tag, seed]) — nothing else decides it.  A
case: dict (family, seed, phys, frame (the default mode, preamble, dbm), lossx (the chain before the first closure, or
None), specs ({phy: mobility_cases spec}), mob (() -> {phy: a fresh model}), closures ((ts, [actions]) in setup order),
listen, reply ({phy: (delay_ns, size, mode, preamble, dbm)}), notify, stop).

Some closures are placed by running the model on the case built so far (deterministic as well): a hand-back's time is
only known from a run, and a switch, an attempt or a neighbour's frame has to land inside a reply's 10 us, or a Receive
in a reply's own nanosecond.  Each is placed after everything it was derived from, so the run up to it stands.

Frames: DsssRate1Mbps (long preamble: the mode table has no short one) and 2 / 5.5 / 11 Mb/s with both preambles,
OfdmRate6 / 24 / 54Mbps, OfdmRate6MbpsBW10MHz and ErpOfdmRate12Mbps; 50 to 1500 B; three tx powers."""
import numpy as np

import loss_ref as lr
import lossx_cases as lc
import nsref
import wifi
import wifi_fuzz_model as fm
import wifi_per_ref as ref
from mobility_ref import CvModel
from waypoint_ref import AccelModel, WaypointModel

MS, US = 1_000_000, 1_000
LONG, SHORT = wifi.PREAMBLE_LONG, wifi.PREAMBLE_SHORT
M = ref.mode_tuple
DSSS = [(M("DsssRate1Mbps"), LONG)] + [(M(n), p) for n in ("DsssRate2Mbps", "DsssRate5_5Mbps", "DsssRate11Mbps")
                                       for p in (LONG, SHORT)]
OFDM = [(M("OfdmRate6Mbps"), LONG), (M("OfdmRate24Mbps"), LONG), (M("OfdmRate54Mbps"), LONG)]
OTHER = [(M("OfdmRate6MbpsBW10MHz"), LONG), (M("ErpOfdmRate12Mbps"), LONG)]
SHORT_FRAMES = [OFDM[1], OFDM[2], (M("DsssRate11Mbps"), SHORT), OTHER[1]]
SIZES = (50, 100, 200, 400, 800, 1500)
POWERS = (16.0206, 12.0, 19.5)
DENSE_POWERS = (15.0, 16.0206, 17.0)  # (dense: heard to the far corner, 212 m, or nearly; a neighbour 25 dB above that)
REPLY_DBM = 5.0  # (a reply reaches the nearest neighbours only: replies to replies die out)
FRAME = (wifi.DSSS_1M, LONG, 16.0206)  # the model's defaults (every attempt names its own)
CHANNELS = (1, 6, 11, 14)
HIDE_DB = 200.0
# Every extended chain starts with a Matrix link of this default loss.  ThreeLogDistance and TwoRayGround alone put a
# neighbour's frame 40 dB and more above the noise floor; m_firstPower then keeps, of such powers added and taken away
# again, a residue of their last bits that is no longer small beside the noise, and a later frame's per follows the
# last bits of earlier powers — which the device's log10 / pow and the host's give differently — beyond the bound
# its own arithmetic is held to (tests/test_wifi_fuzz_cpu.py: the acceptance condition on that residue).
PAD_DB = 25.0
DENSE_PAD_DB = 12.0
TAGS = dict(grid=1, dense=2, blocks=3)


def is_ofdm(mode):
    return mode[0] != wifi.DSSS


def dur(size, mode, preamble):
    return int(wifi.tx_duration_ns(int(size), mode, preamble))


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def frame(rng, sizes=SIZES):
    u = rng.random()
    mode, pre = pick(rng, DSSS) if u < 0.45 else pick(rng, OFDM) if u < 0.85 else pick(rng, OTHER)
    return int(pick(rng, sizes)), mode, pre, float(pick(rng, POWERS))


def attempt(t, j, fr):
    return (int(t), [("attempt", int(j)) + tuple(fr)])


def vec(rng, mag, zmag=None):
    v = rng.uniform(-mag, mag, 3) * (1.0, 1.0, 0.1 if zmag is None else zmag)
    return tuple(float(c) for c in v)


# ---------------------------------------------------------------- the parts of a case
def mobility_specs(rng, x, y, z, movers, span):
    """{phy: spec}: constant velocity (some paused), waypoint lists of 1 to 7 from the phy's position on, or constant
    acceleration; the kinds go round the movers."""
    specs = {}
    for q, j in enumerate(movers):
        kind = ("cv", "wp", "acc")[q % 3]
        if kind == "cv":
            specs[j] = ("cv", vec(rng, 200.0), bool(rng.random() < 0.15), 0)
        elif kind == "wp":
            n = int(rng.integers(1, 8))
            t = np.sort(rng.integers(0, span, n)) + np.arange(n)
            p, pts = np.array([x[j], y[j], z[j]]), []
            for k in range(n):
                if k:
                    p = p + rng.uniform(-12.0, 12.0, 3) * (1.0, 1.0, 0.05)
                pts.append((int(t[k]), (float(p[0]), float(p[1]), float(abs(p[2])))))
            specs[j] = ("wp", pts)
        else:
            specs[j] = ("acc", vec(rng, 150.0), vec(rng, 3000.0))
    return specs


def models_of(case):
    ph, out = case["phys"], {}
    for j, s in case["specs"].items():
        p = (float(ph.x[j]), float(ph.y[j]), float(ph.z[j]))
        out[j] = CvModel(p, *s[1:]) if s[0] == "cv" else WaypointModel(s[1]) if s[0] == "wp" else \
            AccelModel(p, s[1], s[2], base_time=0)
    return out


def course_call(rng, case, j, t, state, queue=True):
    """One course action for phy j at t (state: the last waypoint time queued per waypoint phy, the ended ones).  The
    calls that touch a waypoint queue are drawn in the order of their times (AddWaypoint asks for ascending waypoints
    only while its queue holds one); queue=False: none of those."""
    s = case["specs"].get(j)
    ph = case["phys"]
    near = lambda: tuple(float(c) for c in (ph.x[j] + rng.uniform(-8, 8), ph.y[j] + rng.uniform(-8, 8), float(ph.z[j])))
    if s is None:
        return ("position", j, near())
    u = rng.random()
    if s[0] == "cv":
        return ("velocity", j, vec(rng, 200.0)) if u < 0.5 else ("pause", j, bool(u < 0.7)) if u < 0.8 else \
            ("position", j, near())
    if s[0] == "acc":
        return ("accel", j, vec(rng, 150.0), vec(rng, 3000.0)) if u < 0.7 else ("position", j, near())
    if j in state["ended"] or u > 0.85 or not queue:
        return ("position", j, near())
    if u < 0.65:
        last = max(state["last"].get(j, s[1][-1][0]), t)
        nt = int(last + rng.integers(1 * MS, 8 * MS))
        state["last"][j] = nt
        return ("add_waypoint", j, nt, near())
    state["ended"].add(j)
    return ("end_waypoints", j)


def hidden_chain(rng, ph, chan, link, n_pairs, pad=None):
    """([Matrix (default PAD_DB, or pad), link], entries): pairs (a, b) hidden from each other (HIDE_DB both ways) that share a
    receiver c on their channel; returns the spec and the (a, b, c) triples."""
    n, triples, entries = ph.n_phy, [], []
    for _ in range(20 * n_pairs):
        if len(triples) == n_pairs:
            break
        c = int(rng.integers(n))
        same = [j for j in range(n) if j != c and chan[j] == chan[c]]
        used = {q for t in triples for q in t}
        same = [j for j in same if j not in used]
        if len(same) < 2 or c in used:
            continue
        d = [(float(np.hypot(ph.x[j] - ph.x[c], ph.y[j] - ph.y[c])), j) for j in same]
        a, b = (j for _d, j in sorted(d)[:2])
        triples.append((a, b, c))
        entries += [(a, b, HIDE_DB), (b, a, HIDE_DB)]
    return ([(lr.MATRIX, PAD_DB if pad is None else pad), link], entries), triples


def finish(case):
    case["closures"].sort(key=lambda c: c[0])  # (stable: equal times keep their order)
    case["mob"] = (lambda: models_of(case)) if case["specs"] else None
    return case


def other_channel(rng, chans, cur):
    return int(pick(rng, [c for c in chans if c != cur]))


# ---------------------------------------------------------------- closures placed from a run of the model
def channel_at(case, j, t):
    """Phy j's channel at t as the closures schedule it (a postponed or refused switch aside)."""
    c = int(case["phys"].channel[j])
    for ts, acts in case["closures"]:
        for a in acts:
            if a[0] == "switch" and a[1] == j and ts < t:
                c = a[2]
    return c


def switched(case):
    return {a[1] for _t, acts in case["closures"] for a in acts if a[0] == "switch"}


def place(case, rng, kinds, gap=3 * MS):
    """For each kind in turn: run the model, take the first suitable event later than the last placement + gap, add
    the closure(s).  Returns what was placed, [(kind, time, phy)]."""
    last, placed = 0, []
    for kind in kinds:
        finish(case)
        for horizon in (last + gap + 12 * MS, case["stop"]):  # (a run up to an earlier Stop is the run's beginning)
            got = place_one(case, rng, kind, fm.run(case, stop=min(horizon, case["stop"])), last + gap)
            if got:
                new, last, j = got
                case["closures"] += new
                placed.append((kind, new[0][0], j))
                break
    return placed


def place_one(case, rng, kind, m, after):
    """One placement from the run m: (its closures, the time the next one has to follow, the phy), or None."""
    ph, chans, ends = case["phys"], case["chans"], m.ends
    lim = case["stop"] - 4 * MS
    if kind in ("hold_switching", "hold_tx", "cancel_lock", "same_ns"):
        want = 0 if kind == "same_ns" else 10 * US
        for ei, j, _k, u, per in m.draws:
            T = ends[ei][0]
            if not (u > per and j in case["reply"] and case["reply"][j][0] == want and after < T < lim):
                continue
            if kind == "hold_switching":
                return [(T + 5 * US, [("switch", j, other_channel(rng, chans, channel_at(case, j, T)), 3 * MS)])], T, j
            if kind == "hold_tx":
                return [attempt(T + 5 * US, j, (400, M("DsssRate2Mbps"), LONG, 16.0206))], T, j
            if kind == "cancel_lock":  # the sender of the frame just received sends again, louder
                return [attempt(T + 4 * US, m.txs[ends[ei][5]][2], (200, OFDM[1][0], LONG, 19.5))], T, j
            # a static pair that never switches: its Receive lands in the reply's nanosecond
            fixed = [q for q in range(ph.n_phy) if q not in case["specs"] and q not in switched(case) and q != j]
            pairs = [(s, r) for s in fixed for r in fixed if s != r and ph.channel[s] == ph.channel[r]]
            if pairs:
                s, r = pick(rng, pairs)
                fo = nsref.fanout_yans(ph.x, ph.y, ph.z, np.ones(ph.n_phy, np.uint32), ph.node, s, 16.0206,
                                       nsref.loss_chain(*ph.loss), ph.speed, 0, 0)
                return [attempt(T - int(fo[fo["phy"] == r]["ts"][0]), s, (50, OFDM[2][0], LONG, 16.0206))], T, j
    elif kind == "switch_in_rx":
        for e, r in zip(ends, m.end_refs):
            T, j, tx = e[0], e[2], e[5]
            d = dur(m.tx_sizes[tx], *m.tx_frames[tx][:2])
            if r is not None and j in case["listen"] and d >= 400 * US and after < T - d // 2 < lim:
                return [(T - d // 2, [("switch", j, other_channel(rng, chans, channel_at(case, j, T)), 250 * US)])], T, j
    else:  # a switch while the phy transmits, and a loss action or a course call before its retry
        for t, _uid, j, sent, _st, reply in m.attempts:
            tx = [k for k, x in enumerate(m.txs) if x[0] == t and x[2] == j]
            if not sent or reply or not tx or not after < t < lim or dur(m.tx_sizes[tx[0]], *m.tx_frames[tx[0]][:2]) < MS:
                continue
            between = ("loss", ([(lr.MATRIX, PAD_DB), lc.THREE], ())) if kind == "postponed_loss" else \
                course_call(rng, case, int(pick(rng, [q for q in range(ph.n_phy) if q != j])), t, case["course_state"], False)
            return [(t + 100 * US, [("switch", j, other_channel(rng, chans, channel_at(case, j, t)), 250 * US)]),
                    (t + 300 * US, [between])], t, j
    return None


# ---------------------------------------------------------------- grid
def grid(seed, n_phy=None, n_chan=None):
    """16 to 25 phys at jittered grid positions on two or three channels, 40 to 60 attempts of every frame kind, 4 to 8
    switches, 3 to 6 course calls, an extended chain with Matrix-hidden pairs for part of the run.  n_phy, n_chan:
    other sizes (runs by hand beyond the committed cases; channels 1, 6, 11, 14)."""
    rng = np.random.default_rng([TAGS["grid"], seed])
    n = int(rng.integers(16, 26))
    n = n if n_phy is None else int(n_phy)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    x = (i % side) * 60.0 + rng.uniform(-15.0, 15.0, n)
    y = (i // side) * 60.0 + rng.uniform(-15.0, 15.0, n)
    z = rng.uniform(0.0, 3.0, n)
    chans = CHANNELS[:2 + seed % 2 if n_chan is None else n_chan]
    chan = rng.choice(chans, n).astype(np.uint32)
    ph = wifi.LoopPhys(x, y, z, channel=chan, error_model=wifi.NIST if seed % 2 == 0 else wifi.YANS, tx_cap=1024)
    n_att = int(rng.integers(40, 61))
    ts = 2 * MS + np.cumsum(rng.integers(150 * US, 2200 * US, n_att))
    span = int(ts[-1])
    movers = [int(j) for j in rng.permutation(n)[:max(6, n // 2)]]
    case = dict(family="grid", seed=seed, phys=ph, frame=FRAME, chans=chans, stop=span + 14 * MS,
                specs=mobility_specs(rng, x, y, z, movers, span), course_state=dict(last={}, ended=set()))
    cl = [attempt(ts[k], rng.integers(n), frame(rng)) for k in range(n_att)]
    # switches: one with delay 0, one lasting several frame times, the rest ChannelSwitchDelay's default
    delays = [0, 6 * MS] + [250 * US] * int(rng.integers(0, 3))
    for d in delays:
        j = int(rng.integers(n))
        cl.append((int(rng.integers(3 * MS, span)), [("switch", j, other_channel(rng, chans, chan[j]), d)]))
    # a mover that leaves for a channel of its own, stays, comes back and sends (the kind goes round with the seed)
    j = [q for q in movers if case["specs"][q][0] == ("cv", "wp", "acc")[seed % 3]][0]
    t0 = int(span * rng.uniform(0.2, 0.35))
    cl += [(t0, [("switch", j, 13, 250 * US)]), (t0 + 18 * MS, [("switch", j, int(chans[0]), 250 * US)]),
           attempt(t0 + 20 * MS, j, (400, M("DsssRate2Mbps"), LONG, 19.5))]
    case["loner"] = j
    # the chains: the config's, an extended one from the first loss action on, another (or the config's again) later
    case["lossx"] = ([(lr.MATRIX, PAD_DB), lc.THREE], ()) if seed % 3 == 0 else None
    link = lc.TRG if seed % 2 else lc.THREE
    t1 = int(span * rng.uniform(0.25, 0.4))
    spec, triples = hidden_chain(rng, ph, chan, link, 3)
    cl.append((t1, [("loss", spec)]))
    for q, (a, b, _c) in enumerate(triples):  # the hidden pairs' OFDM frames collide at their common receiver
        t = t1 + (1 + 3 * q) * MS
        cl += [attempt(t, a, (1500, OFDM[0][0], LONG, 19.5)), attempt(t + 300 * US, b, (800, OFDM[1][0], LONG, 19.5))]
    if rng.random() < 0.6:
        spec2 = None if rng.random() < 0.5 else hidden_chain(rng, ph, chan, lc.THREE if seed % 2 else lc.TRG, 2)[0]
        cl.append((int(span * rng.uniform(0.7, 0.85)), [("loss", spec2)]))
    for t in sorted(int(t) for t in rng.integers(3 * MS, span, int(rng.integers(3, 7)))):
        cl.append((t, [course_call(rng, case, int(pick(rng, movers + [int(rng.integers(n))])), t, case["course_state"])]))
    case["closures"] = cl
    listen = sorted(int(j) for j in rng.permutation(n)[:(n + 1) // 2])
    case["listen"] = listen
    case["reply"] = {j: (int(pick(rng, (0, 10 * US))),) + (int(pick(rng, (50, 100, 200))),) + pick(rng, SHORT_FRAMES)
                     + (REPLY_DBM,) for j in listen}
    case["notify"] = sorted(int(j) for j in np.flatnonzero(rng.random(n) < 0.5))
    case["placed"] = place(case, rng, ("switch_in_rx", "hold_switching", "postponed_course" if seed % 2 else
                                       "postponed_loss", "hold_tx", "same_ns", "cancel_lock"))
    return finish(case)


# ---------------------------------------------------------------- dense
def dense(seed):
    """36 phys on one channel at 30 m pitch.  Rounds of: one clean frame, then — inside the 10 us of the replies to it
    — a closure of 9 to 12 attempts and one other call (a switch, a loss action or a course call).  The replies with
    delay 0 go out before that closure, the others after it: held where the phy is among its senders, sent into a
    lock on one of its frames elsewhere.  Even seeds have no mobility model (sends then batch up to NSEND)."""
    rng = np.random.default_rng([TAGS["dense"], seed])
    n = 36
    i = np.arange(n)
    x = (i % 6) * 30.0 + rng.uniform(-3.0, 3.0, n)
    y = (i // 6) * 30.0 + rng.uniform(-3.0, 3.0, n)
    z = rng.uniform(0.0, 2.0, n)
    # (the chain: the config's LogDistance behind DENSE_PAD_DB, with thresholds lowered by as much — everything still
    # hears everything, and a neighbour's frame is 10 dB above the noise floor, not 22: PAD_DB's reason)
    ph = wifi.LoopPhys(x, y, z, channel=np.ones(n, np.uint32), error_model=wifi.NIST if seed % 2 == 0 else wifi.YANS,
                       ed_threshold_dbm=-96.0 - DENSE_PAD_DB, cca_threshold_dbm=-99.0 - DENSE_PAD_DB, tx_cap=1024)
    movers = [int(j) for j in rng.permutation(n)[:6]] if seed % 2 else []
    config = ([(lr.MATRIX, DENSE_PAD_DB)] + [tuple(link) for link in ph.loss], ())
    case = dict(family="dense", seed=seed, phys=ph, frame=FRAME, chans=(1, 6), lossx=config,
                specs=mobility_specs(rng, x, y, z, movers, 6 * MS), course_state=dict(last={}, ended=set()))
    listen = sorted(int(j) for j in rng.permutation(n)[:18])
    short = lambda: (int(pick(rng, (50, 100, 200))),) + pick(rng, SHORT_FRAMES) + (float(pick(rng, DENSE_POWERS)),)
    cl, t, away = [], 1 * MS, set()
    for r in range(int(rng.integers(4, 6))):
        here = [j for j in range(n) if j not in away]
        s = int(pick(rng, here))
        fr = (int(pick(rng, (100, 200, 400))),) + pick(rng, [OFDM[0]] + OTHER) + (DENSE_POWERS[-1],)
        cl.append(attempt(t, s, fr))
        tb = t + dur(*fr[:3]) + 5 * US
        k = int(rng.integers(9, 13))
        senders = [int(j) for j in rng.permutation([j for j in here if j != s])[:k]]
        acts = [("attempt", j) + short() for j in senders]
        rest = [j for j in here if j not in senders]
        what = (r + seed) % 3
        if what == 0:
            j = int(pick(rng, rest))
            other = ("switch", j, 6, int(pick(rng, (0, 250 * US))))
            away.add(j)
        elif what == 1:
            spec = config if rng.random() < 0.3 else hidden_chain(rng, ph, ph.channel, lc.TRG if r % 2 else lc.THREE, 2, PAD_DB + DENSE_PAD_DB)[0]
            other = ("loss", spec)
        else:
            other = course_call(rng, case, int(pick(rng, movers or rest)), tb, case["course_state"])
        acts.insert(int(rng.integers(len(acts) + 1)), other)
        cl.append((tb, acts))
        t = tb + int(rng.integers(600 * US, 1200 * US))
        for _ in range(int(rng.integers(1, 4))):  # single frames into what the burst left
            cl.append(attempt(tb + int(rng.integers(20 * US, 500 * US)), pick(rng, here), short()))
    case.update(closures=cl, stop=t + 2 * MS, listen=listen, notify=sorted(int(j) for j in np.flatnonzero(rng.random(n) < 0.5)),
                reply={j: (int(pick(rng, (0, 10 * US))),) + short() for j in listen}, placed=[])
    return finish(case)


# ---------------------------------------------------------------- blocks
def blocks(seed):
    """270 to 330 phys (18 to a row, 60 m pitch): two 256-phy blocks of k_wl_send / k_wl_rx / k_wl_move.  Phys 255 and
    256 — neighbours in a row, both constant-velocity movers — each lock on a frame, send, take a course call and
    switch to channel 6, where they meet again; Matrix entries name pairs on both sides of the boundary."""
    rng = np.random.default_rng([TAGS["blocks"], seed])
    n = int(rng.integers(270, 331))
    i = np.arange(n)
    x = (i % 18) * 60.0 + rng.uniform(-10.0, 10.0, n)
    y = (i // 18) * 60.0 + rng.uniform(-10.0, 10.0, n)
    z = rng.uniform(0.0, 2.0, n)
    chan = np.where(rng.random(n) < 0.7, 1, 6).astype(np.uint32)
    chan[[237, 238, 254, 255, 256, 257, 273, 274]] = 1
    ph = wifi.LoopPhys(x, y, z, channel=chan, error_model=wifi.NIST if seed % 2 == 0 else wifi.YANS, tx_cap=1024)
    movers = [255, 256] + [int(j) for j in rng.permutation(n)[:40] if j not in (255, 256)]
    case = dict(family="blocks", seed=seed, phys=ph, frame=FRAME, chans=(1, 6), lossx=None, stop=17 * MS,
                course_state=dict(last={}, ended=set()))
    case["specs"] = mobility_specs(rng, x, y, z, movers[2:], 15 * MS)
    for j in (255, 256):
        case["specs"][j] = ("cv", vec(rng, 300.0), False, 0)
    fr = lambda: (int(pick(rng, (100, 200))), M("DsssRate2Mbps"), pick(rng, (LONG, SHORT)), 16.0206)
    entries = [(a, b, float(np.round(rng.uniform(60.0, 110.0), 3))) for a, b in
               ((255, 256), (256, 255), (254, 256), (255, 257), (238, 256), (256, 238), (273, 255), (250, 260), (260, 250))]
    cl = [attempt(2 * MS, 254, fr()), attempt(4 * MS, 255, fr()), attempt(6 * MS, 256, fr()),
          (7 * MS, [("loss", ([(lr.MATRIX, PAD_DB), lc.THREE if seed % 2 else lc.TRG], entries))]),
          (8 * MS, [("velocity", 255, vec(rng, 300.0)), ("position", 256, (float(x[256]) + 5.0, float(y[256]) - 4.0, 1.0))]),
          attempt(8 * MS + 500 * US, 257, fr()),
          (9 * MS, [("switch", 255, 6, 250 * US)]), (9 * MS + 400 * US, [("switch", 256, 6, 0)]),
          attempt(11 * MS, 255, fr()), attempt(13 * MS, 256, fr())]
    for _ in range(int(rng.integers(1, 3))):
        cl.append(attempt(int(rng.integers(3 * MS, 14 * MS)), rng.integers(n), (50, OFDM[2][0], LONG, 19.5)))
    case["closures"] = cl
    listen = sorted({255, 256} | {int(j) for j in rng.permutation(n)[:24]})
    case.update(listen=listen, notify=sorted(int(j) for j in np.flatnonzero(rng.random(n) < 0.2)),
                reply={j: (int(pick(rng, (0, 10 * US))), 50) + pick(rng, SHORT_FRAMES) + (16.0206,) for j in listen})
    case["placed"] = place(case, rng, ("hold_tx",), gap=0)
    return finish(case)


FAMILIES = dict(grid=grid, dense=dense, blocks=blocks)


def build(family, seed):
    return FAMILIES[family](seed)


FUZZ_CASES = [("grid", s) for s in range(12)] + [("dense", s) for s in range(6)] + [("blocks", s) for s in range(3)]


def describe_phy(case, j):
    """What lives on phy j: its channels as scheduled, its mobility, whether it is handed back or notifies, the Matrix
    entries that name it."""
    hist = [int(case["phys"].channel[j])] + [f"{a[2]} at {ts} (+{a[3]})" for ts, acts in case["closures"] for a in acts
                                             if a[0] == "switch" and a[1] == j]
    spec = case["specs"].get(j)
    mob = "static" if spec is None else f"waypoints ({len(spec[1])})" if spec[0] == "wp" else \
        {"cv": "constant velocity", "acc": "constant acceleration"}[spec[0]]
    rows = set()
    for sp in [case["lossx"]] + [a[1] for _t, acts in case["closures"] for a in acts if a[0] == "loss"]:
        if sp is not None:
            rows |= {(a, b, db) for a, b, db in sp[1] if j in (a, b)}
    rep = case["reply"].get(j)
    return (f"phy {j}: channels {hist}; {mob}; " + (f"listened (reply after {rep[0]} ns)" if j in case["listen"] else
                                                    "not listened") +
            ("; notifying" if j in case["notify"] else "") + f"; Matrix entries {sorted(rows)}")
