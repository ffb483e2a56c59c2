"""Every p2p device feature in one Python model: the random OnOff times (tests/p2p_ranvar_pyref.py) and UdpTraceClient
(tests/p2p_trace_client_pyref.py) mixins over the error-model model (tests/p2p_errmodel_pyref.py: ports, ICMP,
fragmentation, receive error models), or over the monitored one (tests/p2p_flowmon_pyref.py).  Nothing is modelled
here: the two mixins override disjoint application kinds and pass every other call on, so they compose as they are.
tests/test_p2p_sources_fuzz_cpu.py pins the composition: without the features of one layer a run equals that of the
model below it."""
import p2p_errmodel_pyref
import p2p_flowmon_pyref
import p2p_ranvar_pyref
import p2p_trace_client_pyref


class Model(p2p_ranvar_pyref.RanvarMixin, p2p_trace_client_pyref.TraceClientMixin, p2p_errmodel_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self._tc_init()


class MonitoredModel(p2p_ranvar_pyref.RanvarMixin, p2p_trace_client_pyref.TraceClientMixin, p2p_flowmon_pyref.Model):
    def __init__(self, sc, trace_kinds=0x7F, nudge=None):
        super().__init__(sc, trace_kinds, nudge)
        self._tc_init()


def results(m):
    """p2p_ranvar_pyref.results' dict from a model that has run, plus clients (p2p.UDP_TRACE_CLIENT_DTYPE) and tc_diag
    as p2p_trace_client_pyref.results builds them."""
    out = p2p_ranvar_pyref.results(m)
    tc = p2p_trace_client_pyref.results(m)
    out.update(clients=tc["clients"], tc_diag=tc["tc_diag"])
    return out


def run(sc, trace_kinds=0x7F, nudge=None):
    m = Model(sc, trace_kinds, nudge)
    m.setup()
    m.run()
    return results(m)


def run_monitored(sc, trace_kinds=0x7F, max_delays=(p2p_flowmon_pyref.MAX_PER_HOP_DELAY_NS,)):
    """The monitored model's run: results' dict and flows = {max_delay: the flow records}, fm_diag."""
    m = MonitoredModel(sc, trace_kinds)
    m.setup()
    m.run()
    out = results(m)
    out["frag"]["cancelled_timers"] = 0
    out.update(flows={d: m.flow_records(d) for d in max_delays}, fm_diag=dict(m.fm_diag))
    return out
