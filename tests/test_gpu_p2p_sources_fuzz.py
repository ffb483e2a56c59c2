"""The second seeded set (tests/p2p_sources_fuzz_cases.py: UdpTraceClients and random OnOff times added to the
cross-feature scenarios, so that bursts, draws, fragments, ICMP, queue overflow and receive error models meet in one
engine) on the GPU, each case through six pipelines and each run compared bit for bit with the composed Python model
(tests/p2p_full_pyref.py): everything tests/test_gpu_p2p_fuzz.py compares, and trace_clients (), onoff_draws () and an
empty ambiguous_draws ().  tests/test_p2p_sources_fuzz_cpu.py asserts on the model alone that the cases are accepted
and reach the interactions meant.

A failure's message names the family and seed, the first differing pop-log entry and what lives on its node (trace
clients with their entries, sources with their variables): p2p_sources_fuzz_cases.build (family, seed) rebuilds the
scenario on the CPU."""
import numpy as np
import pytest

import flowmon_cases as FMC
import p2p
import p2p_full_pyref as FULL
import p2p_fuzz_cases as FZ
import p2p_sources_fuzz_cases as SF
from p2p_model_compare import assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
DELAYS = (p2p.MAX_PER_HOP_DELAY_NS, FMC.SMALL_DELAY_NS)  # 10 s and 1 ms
_models = {}


def model(family, seed, monitored=False):
    """The model's run of one case (or of its monitored variant; None where there is none), computed once."""
    key = (family, seed, monitored)
    if key not in _models:
        if monitored:
            sc = SF.monitored(family, seed)
            _models[key] = (sc, None if sc is None else FULL.run_monitored(sc, ALL_KINDS, DELAYS))
        else:
            sc = SF.build(family, seed)
            _models[key] = (sc, FULL.run(sc, ALL_KINDS))
        m = _models[key][1]
        assert m is None or len(m["ambiguous"]) == 0
    return _models[key]


def describe(sc, family, seed, pipeline):
    label = "%s seed %d, %s" % (family, seed, pipeline)

    def context(_i, got, want):
        """What lives on the node of the first differing entry (the model's, or the engine's past the model's end)."""
        ctx = (want or got)[2]
        return SF.describe_node(sc, ctx) if ctx < sc.n_nodes else "no node context"
    return dict(label=label, context=context)


def compare(eng, m, res, d, traced=False, note=""):
    """One run of an engine or a group against the model."""
    st, devc, appc, log = res
    log = tuple(x[:int(st.dispatched)] for x in log)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(),
                        eng.trace() if traced else None, label=d["label"] + note, context=d["context"],
                        clients=eng.trace_clients(), draws=eng.onoff_draws())
    rec, over = eng.ambiguous_draws()
    assert len(rec) == 0 and over == 0, "ambiguous draws | " + d["label"] + note


def single_untraced(sc, m, d, want_wide=None):
    """The default engine, run twice: run = reset + launch, so the second run starts from the reset image (rv_init,
    the trace clients' app_tot words, frag_init and the error models' image, all restored together)."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n + 64)
    plan_wide = bool(p2p.dist_plan(sc, None, 0, 1)["wide"])
    assert eng.wide() == (plan_wide if want_wide is None else want_wide), d["label"]
    for again in (False, True):
        compare(eng, m, eng.run(n + 64), d, note=", second run" if again else "")
    return eng


def single_traced(sc, m, d):
    """The scanning pipeline, trace records included."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n + 64)
    eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    compare(eng, m, eng.run(n + 64), d, traced=True)
    return eng


def group(sc, m, d, nranks, owner):
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, nranks, owner=owner, log_cap=n + 64, trace_cap=len(m["trace"]) + 64,
                            trace_kinds=ALL_KINDS)
    compare(grp, m, grp.run(n + 64), d, traced=True)
    # each member drew, and ran Sends, for the applications of its own nodes only
    for r, mem in enumerate(grp.members):
        draws, clients = mem.onoff_draws(), mem.trace_clients()
        for a, A in enumerate(sc.apps):
            if grp.owner[A["node"]] != r:
                where = "rank %d, app %d | %s" % (r, a, d["label"])
                assert draws["on_draws"][a] == draws["off_draws"][a] == 0, "drew for another rank's source: " + where
                assert clients["sends"][a] == 0, "ran another rank's client: " + where


def assert_flows(eng, m, label):
    for delay in DELAYS:
        got, want = eng.flow_stats(delay), m["flows"][delay]
        assert len(got) == len(want) > 0, "flows (max_delay %d) | %s" % (delay, label)
        for f in p2p.FLOW_STATS_DTYPE.names:
            assert np.array_equal(got[f], want[f]), \
                "%s (max_delay %d) | %s: %s != %s" % (f, delay, label, got[f], want[f])


def run_single(family, seed, pipeline, monkeypatch):
    sc, m = model(family, seed)
    d = describe(sc, family, seed, pipeline)
    if pipeline == "single":
        single_untraced(sc, m, d).close()
    elif pipeline == "narrow":
        assert bool(p2p.dist_plan(sc, None, 0, 1)["wide"]), d["label"]
        monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
        single_untraced(sc, m, d, want_wide=False).close()
    elif pipeline == "traced":
        single_traced(sc, m, d).close()
    elif pipeline == "group2_blocks":
        group(sc, m, d, 2, None)
    else:
        group(sc, m, d, 3, FZ.owner_interleaved(sc, 3))


PIPELINES = ("single", "traced", "group2_blocks", "group3_interleaved")


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("family,seed", SF.SRC_FUZZ_CASES)
def test_engine_equals_model(family, seed, pipeline, monkeypatch):
    run_single(family, seed, pipeline, monkeypatch)


@pytest.mark.parametrize("family,seed", SF.WIDE_CASES)
def test_engine_equals_model_narrow(family, seed, monkeypatch):
    """The cases whose plan is wide, through the narrow kernels."""
    run_single(family, seed, "narrow", monkeypatch)


@pytest.mark.parametrize("family,seed", SF.SRC_FUZZ_CASES)
def test_engine_equals_model_monitored(family, seed):
    """The monitored variant (frag off, the monitor on), untraced and traced: the run and, for 10 s and 1 ms, every
    field of the flow records."""
    sc, m = model(family, seed, monitored=True)
    if sc is None:
        pytest.skip("create refuses the monitored variant of this case")
    d = describe(sc, family, seed, "monitored")
    for runner in (single_untraced, single_traced):
        eng = runner(sc, m, d)
        assert_flows(eng, m, d["label"])
        eng.close()


def test_at_least_half_of_the_cases_run_monitored():
    ran = sum(1 for family, seed in SF.SRC_FUZZ_CASES if SF.monitored(family, seed) is not None)
    assert 2 * ran >= len(SF.SRC_FUZZ_CASES), (ran, len(SF.SRC_FUZZ_CASES))


def test_comparison_fails_against_a_wrong_model():
    """The positive control of the comparison itself: with the statistics, or only the clients' records, of the model
    with a deliberately wrong line (a cycle's last burst ends at the wrap), the same engine run is refused; on the
    first case that line matters to."""
    for family, seed in SF.SRC_FUZZ_CASES:
        sc, m = model(family, seed)
        if m["tc_diag"]["wrap_joined"] == 0:
            continue
        wrong = FULL.run(sc, ALL_KINDS, nudge="no_wrap_join")
        assert wrong["stats"]["digest"] != m["stats"]["digest"]
        assert not np.array_equal(wrong["clients"], m["clients"])
        d = describe(sc, family, seed, "traced, wrong model")
        with pytest.raises(AssertionError, match="digest|dispatched"):
            single_traced(sc, dict(m, stats=wrong["stats"]), d)
        with pytest.raises(AssertionError, match="trace clients'"):
            single_traced(sc, dict(m, clients=wrong["clients"]), d)
        return
    raise AssertionError("no case of SRC_FUZZ_CASES joins a burst over the wrap")
