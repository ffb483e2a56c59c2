"""Random OnOff times added to the Python restatement of the p2p subset (tests/p2p_errmodel_pyref.py and the models
below it, which stay as they are), written from the reference's lines alone.

  OnOff        onoff-application.cc:221-237: ScheduleStartEvent takes Seconds (m_offTime.GetValue ()) (called from
               StartApplication and StopSending), ScheduleStopEvent Seconds (m_onTime.GetValue ()) (from StartSending);
               the draw happens when the event is scheduled; ScheduleNextTx's StopApplication at MaxBytes draws nothing
  Constant     random-variable.cc:316-320: no draw
  Uniform      :251-258: m_min + RandU01 () * (m_max - m_min)
  Exponential  :574-589: r = -m_mean * log (RandU01 ()); with m_bound != 0 redrawn until r <= m_bound

`log` here is math.log: the host's libm, which is what the reference calls.  Beside each Exponential attempt the model
evaluates log (u) with decimal at 60 digits and applies the engine's two-candidate rule (csrc/nsgpu_ranvar.h): hi the
correctly rounded logarithm, its neighbour on the side of the true value; the attempt is ambiguous when Seconds
(-mean * hi) and Seconds (-mean * neighbour) differ, when the two disagree about the bound, or when the true value is
within LOG_ERR ulp of the midpoint.  The model keeps its own list of the ambiguous attempts.
"""
import math
from decimal import Decimal, getcontext

import numpy as np

import nsref
import p2p
import p2p_errmodel_pyref
import p2p_flowmon_pyref

LOG_ERR = 2.0 ** -40  # the engine's stated bound on its log's error, in ulps (NSGPU_RV_LOG_ERR)
M1 = p2p_errmodel_pyref.M1


def exact_log(u):
    """(hi, towards): the correctly rounded log (u) of the double u and its neighbour on the side of the true value;
    and frac = |true - hi| in ulps of hi."""
    getcontext().prec = 60
    t = Decimal(u).ln()
    hi = float(t)
    d = t - Decimal(hi)
    nb = hi if d == 0 else math.nextafter(hi, math.inf if d > 0 else -math.inf)
    return hi, nb, float(abs(d) / Decimal(math.ulp(hi)))


def exponential_attempt(mean, bound, u):
    """One attempt at u: dict (r = the host's value with math.log, ns, accept; dev_ns / dev_other / dev_accept = what the
    engine takes and its other candidate; ambiguous)."""
    r = -mean * math.log(u)
    hi, nb, frac = exact_log(u)
    r1, r2 = -mean * hi, -mean * nb
    ns1, ns2 = nsref.seconds(r1), nsref.seconds(r2)
    acc1, acc2 = bound == 0 or r1 <= bound, bound == 0 or r2 <= bound
    return dict(r=r, ns=nsref.seconds(r), accept=bound == 0 or r <= bound, dev_ns=ns1, dev_other=ns2, dev_accept=acc1,
                ambiguous=ns1 != ns2 or acc1 != acc2 or frac >= 0.5 - LOG_ERR)


class Variable:
    """A RandomVariable with its own RngStream."""

    def __init__(self, var, seed, run):
        self.kind, self.p0, self.p1 = var.kind, var.p0, var.p1
        self.g = p2p_errmodel_pyref.RngStream(seed, run, var.stream) if var.kind != p2p.RV_CONSTANT else None
        self.draws = 0
        self.ambiguous = []  # (ordinal, k, dev_ns, dev_other)
        self.attempts = 0

    def get_value(self):
        if self.kind == p2p.RV_CONSTANT:
            return self.p0
        ordinal = self.draws
        self.draws += 1
        if self.kind == p2p.RV_UNIFORM:
            self.attempts += 1
            return self.p0 + self.g.u01() * (self.p1 - self.p0)
        assert self.kind == p2p.RV_EXPONENTIAL
        while True:
            u = self.g.u01()
            self.attempts += 1
            t = exponential_attempt(self.p0, self.p1, u)
            if t["ambiguous"]:
                self.ambiguous.append((ordinal, int(round(u * (M1 + 1.0))), t["dev_ns"], t["dev_other"]))
            if t["accept"]:
                return t["r"]


class RanvarMixin:
    """The three places of tests/p2p_pyref.py that read the constant on / off times draw from per-application
    variable objects (the helper's attribute copy gives every application its own two)."""

    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self.var = []
        for a in sc.apps:
            on = a.get("on_var") or p2p.Constant(a["on"])
            off = a.get("off_var") or p2p.Constant(a["off"])
            self.var.append((Variable(on, sc.rng_seed, sc.rng_run), Variable(off, sc.rng_seed, sc.rng_run)))
        self.on_at_stop = {}  # application -> whether its m_sendEvent was running when StopApplication came

    def start_sending(self, a):  # :184-190, ScheduleStopEvent :229-237
        self.app[a]["last_start"] = self.now
        self.schedule_next_tx(a)
        self.app[a]["ss_ev"] = self.schedule(nsref.seconds(self.var[a][0].get_value()), lambda: self.stop_sending(a))

    def stop_sending(self, a):  # :192-198, ScheduleStartEvent :221-227
        self.cancel_events(a)
        self.app[a]["ss_ev"] = self.schedule(nsref.seconds(self.var[a][1].get_value()), lambda: self.start_sending(a))

    def start_application(self, a):
        if self.sc.apps[a]["kind"] != p2p.APP_ONOFF:
            return super().start_application(a)
        self.cancel_events(a)  # OnOff :132-151
        self.app[a]["ss_ev"] = self.schedule(nsref.seconds(self.var[a][1].get_value()), lambda: self.start_sending(a))

    def stop_application(self, a):
        if self.sc.apps[a]["kind"] == p2p.APP_ONOFF:
            self.on_at_stop.setdefault(a, not self.is_expired(self.app[a]["send_ev"]))
        return super().stop_application(a)

    def onoff_draws(self):
        out = np.zeros(len(self.sc.apps), p2p.ONOFF_DRAWS_DTYPE)
        for a, (on, off) in enumerate(self.var):
            out[a] = (on.draws, off.draws, len(on.ambiguous) + len(off.ambiguous), 0)
        return out

    def ambiguous_draws(self):
        rec = [(a, w, o, k, ns, other) for a, pair in enumerate(self.var) for w, v in enumerate(pair)
               for o, k, ns, other in v.ambiguous]
        return np.array(rec, p2p.AMBIGUOUS_DRAW_DTYPE)


class Model(RanvarMixin, p2p_errmodel_pyref.Model):
    pass


class MonitoredModel(RanvarMixin, p2p_flowmon_pyref.Model):
    pass


def results(m):
    """p2p_errmodel_pyref.run's dict from a model that has run, with draws / ambiguous / model added."""
    devc = np.zeros(len(m.sc.dev), p2p.DEV_COUNTERS_DTYPE)
    for d, D in enumerate(m.dev):
        for f, v in D["c"].items():
            devc[d][f] = v & 0xFFFFFFFF
    appc = np.zeros(len(m.sc.apps), p2p.APP_COUNTERS_DTYPE)
    servers = np.zeros(len(m.sc.apps), p2p.UDP_SERVER_DTYPE)
    for a, S in enumerate(m.app):
        for f, v in S["c"].items():
            appc[a][f] = v
        if S["loss"] is not None:
            servers[a] = (S["received"], S["loss"].m_lost, S["loss"].m_lastMaxSeqNum, 0)
    log = (np.array([e[0] for e in m.log], np.uint64), np.array([e[1] for e in m.log], np.uint32),
           np.array([e[2] for e in m.log], np.uint32))
    stats = dict(dispatched=m.dispatched, cancelled=m.cancelled, digest=m.digest, final_ts=m.now,
                 next_uid=m.m_uid, ttl_drops=m.ttl_drops, no_route_drops=m.no_route_drops,
                 unreach_drops=m.unreach_drops, icmp_sent=m.icmp_sent)
    frag = dict(m.fs)
    frag["cancelled_timers"] = sum(1 for ev in m.timer_events
                                   if ev.cancelled and (ev.ts, ev.uid) <= (m.now, m.cur_uid))
    em = np.zeros(len(m.sc.dev), p2p.ERROR_MODEL_DTYPE)
    for d, (inv, cor) in m.em_count.items():
        em[d] = (inv & 0xFFFFFFFF, cor & 0xFFFFFFFF)
    return dict(stats=stats, devc=devc, appc=appc, servers=servers, log=log, frag=frag, em=em, dropped=m.em_dropped,
                trace=np.array(m.trace, dtype=p2p.TRACE_RECORD_DTYPE), diag=m.diag, draws=m.onoff_draws(),
                ambiguous=m.ambiguous_draws(), model=m)


def run(sc, trace_kinds=0x7F):
    m = Model(sc, trace_kinds)
    m.setup()
    m.run()
    return results(m)


def run_monitored(sc, trace_kinds=0x7F, max_delays=(p2p_flowmon_pyref.MAX_PER_HOP_DELAY_NS,)):
    """The monitored model's run: results' dict and flows = {max_delay: the flow records}."""
    m = MonitoredModel(sc, trace_kinds)
    m.setup()
    m.run()
    out = results(m)
    out["frag"]["cancelled_timers"] = 0
    out["flows"] = {d: m.flow_records(d) for d in max_delays}
    return out
