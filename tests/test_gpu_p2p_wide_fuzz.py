"""The third seeded set (tests/p2p_wide_fuzz_cases.py: the band families, every device feature in windows several
holder blocks wide) on the GPU engine.  Every (family, seed) runs through every pipeline, and each run is compared bit
for bit with the Python model (tests/p2p_errmodel_pyref.py; the band_src families: the composed
tests/p2p_full_pyref.py, with trace_clients (), onoff_draws () and an empty ambiguous_draws ()): every statistic, the
full pop log, device and application counters, UdpServer records, fragmentation counters, the error models' records
and the sorted trace records.  The pipelines: the default engine run twice (the second run starts from the reset
image), the traced (scanning) engine, the narrow kernels on a wide plan (NSGPU_P2P_NARROW=1), a LoopbackGroup of two
block ranks and one of three interleaved ranks (owner = node % 3: every hop of every column crosses ranks); the
monitored variants' flow records field by field.  tests/test_p2p_wide_fuzz_cpu.py asserts on the model alone that the
cases are accepted, wide, spread and reach the interactions meant.

The single-engine runs also assert max_window > MIN_WINDOW: a floor that says the engine really cut windows several
holder blocks wide, a condition on the test and not a property under test.  On these bands the floor alone says little:
the setup burst at time 0 (one event a node, device and application: about 3500) already fills a window to its
capacity, and every case reports max_window = 4096.  What was measured beside it (printed by the single runs, not
asserted: window counts are the engine's own business): the band_wide cases dispatch their 46 to 47 thousand events
in 49 windows, about 960 events a window, so the windows after the setup are wide too; the narrow plans take 470 to
540 windows, and a window holds at least every event of its first timestamp, of which
tests/test_p2p_wide_fuzz_cpu.py counts 35 above 512 events; with random sources, whose start and stop events have
lookahead 0, 2700 to 4400 windows.

A failure's message names the family and seed, the pipeline, the first differing pop-log entry and what lives on its
node: p2p_wide_fuzz_cases.build (family, seed) rebuilds the scenario on the CPU."""
import copy

import numpy as np
import pytest

import flowmon_cases as FMC
import p2p
import p2p_errmodel_pyref
import p2p_full_pyref as FULL
import p2p_fuzz_cases as FZ
import p2p_wide_fuzz_cases as WF
from p2p_model_compare import assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
DELAYS = (p2p.MAX_PER_HOP_DELAY_NS, FMC.SMALL_DELAY_NS)  # 10 s and 1 ms
MIN_WINDOW = 256  # four holder blocks of HB events, a whole RKCW tile
_models = {}


def model(family, seed, monitored=False):
    """The scenario and the model's run of one case (or of its monitored variant), computed once."""
    key = (family, seed, monitored)
    if key not in _models:
        if monitored:
            sc = WF.monitored(family, seed)
            m = FULL.run_monitored(sc, ALL_KINDS, DELAYS)
        else:
            sc = WF.build(family, seed)
            m = (FULL.run if family in WF.SRC_FAMILIES else p2p_errmodel_pyref.run)(sc, ALL_KINDS)
        assert len(m.get("ambiguous", ())) == 0
        _models[key] = (sc, m)
    return _models[key]


def describe(sc, family, seed, pipeline):
    label = "%s seed %d, %s" % (family, seed, pipeline)

    def context(_i, got, want):
        """What lives on the node of the first differing entry (the model's, or the engine's past the model's end)."""
        ctx = (want or got)[2]
        return WF.describe_node(sc, ctx) if ctx < sc.n_nodes else "no node context"
    return dict(label=label, context=context)


def compare(eng, m, res, d, traced=False, note=""):
    """One run of an engine or a group against the model."""
    st, devc, appc, log = res
    log = tuple(x[:int(st.dispatched)] for x in log)
    sources = "clients" in m  # (a run of the composed model)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(),
                        eng.trace() if traced else None, label=d["label"] + note, context=d["context"],
                        clients=eng.trace_clients() if sources else None,
                        draws=eng.onoff_draws() if sources else None)
    if sources:
        rec, over = eng.ambiguous_draws()
        assert len(rec) == 0 and over == 0, "ambiguous draws | " + d["label"] + note
    return st


def single_untraced(sc, m, d, want_wide=None):
    """The default engine, run twice: run = reset + launch, so the second run starts from the reset image."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n + 64)
    plan_wide = bool(p2p.dist_plan(sc, None, 0, 1)["wide"])
    assert eng.wide() == (plan_wide if want_wide is None else want_wide), d["label"]
    for again in (False, True):
        st = compare(eng, m, eng.run(n + 64), d, note=", second run" if again else "")
        print(d["label"], "max_window", int(st.max_window), "windows", int(st.windows))
        assert st.max_window > MIN_WINDOW, "max_window %d | %s" % (st.max_window, d["label"])
    return eng


def single_traced(sc, m, d):
    """The scanning pipeline, trace records included."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n + 64)
    eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    assert eng.wide() == bool(p2p.dist_plan(sc, None, 0, 1)["wide"]), d["label"]
    st = compare(eng, m, eng.run(n + 64), d, traced=True)
    assert st.max_window > MIN_WINDOW, "max_window %d | %s" % (st.max_window, d["label"])
    return eng


def group(sc, m, d, nranks, owner):
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, nranks, owner=owner, log_cap=n + 64, trace_cap=len(m["trace"]) + 64,
                            trace_kinds=ALL_KINDS)
    compare(grp, m, grp.run(n + 64), d, traced=True)


def assert_flows(eng, m, label):
    for delay in DELAYS:
        got, want = eng.flow_stats(delay), m["flows"][delay]
        assert len(got) == len(want) > WF.HB, "flows (max_delay %d) | %s" % (delay, label)
        for f in p2p.FLOW_STATS_DTYPE.names:
            assert np.array_equal(got[f], want[f]), \
                "%s (max_delay %d) | %s: first differing flow %d" % (
                    f, delay, label, int(np.argmax(np.any((got[f] != want[f]).reshape(len(got), -1), axis=1))))


PIPELINES = ("single", "traced", "group2_blocks", "group3_interleaved")


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("family,seed", WF.WIDE_FUZZ_CASES)
def test_engine_equals_model(family, seed, pipeline):
    sc, m = model(family, seed)
    d = describe(sc, family, seed, pipeline)
    if pipeline == "single":
        single_untraced(sc, m, d).close()
    elif pipeline == "traced":
        single_traced(sc, m, d).close()
    elif pipeline == "group2_blocks":
        group(sc, m, d, 2, None)
    else:
        group(sc, m, d, 3, FZ.owner_interleaved(sc, 3))


@pytest.mark.parametrize("family,seed", [c for c in WF.WIDE_FUZZ_CASES if c[0] in WF.WIDE_FAMILIES])
def test_engine_equals_model_narrow(family, seed, monkeypatch):
    """The cases whose plan is wide, through the narrow kernels."""
    sc, m = model(family, seed)
    d = describe(sc, family, seed, "narrow")
    assert bool(p2p.dist_plan(sc, None, 0, 1)["wide"]), d["label"]
    monkeypatch.setenv("NSGPU_P2P_NARROW", "1")
    single_untraced(sc, m, d, want_wide=False).close()


@pytest.mark.parametrize("family,seed", [c for c in WF.WIDE_FUZZ_CASES if c[0] in WF.SRC_FAMILIES])
def test_engine_equals_model_monitored(family, seed):
    """The monitored variant (frag off, the monitor on), untraced and traced: the run and, for 10 s and 1 ms, every
    field of the flow records."""
    sc, m = model(family, seed, monitored=True)
    d = describe(sc, family, seed, "monitored")
    for runner in (single_untraced, single_traced):
        eng = runner(sc, m, d)
        assert_flows(eng, m, d["label"])
        eng.close()


@pytest.mark.parametrize("family,seed", [WF.WIDE_FUZZ_CASES[0], WF.WIDE_FUZZ_CASES[6]])
def test_comparison_fails_against_a_changed_model(family, seed):
    """The positive control of the comparison at this size: against the model of the same scenario with two Rate
    models on each other's stream, the same engine run is refused by the statistics, and with the right statistics
    by the error models' records."""
    sc, m = model(family, seed)
    wrong = p2p_errmodel_pyref.run(WF.with_swapped_rate_streams(copy.deepcopy(sc)), ALL_KINDS)
    assert wrong["stats"]["digest"] != m["stats"]["digest"] and not np.array_equal(wrong["em"], m["em"])
    d = describe(sc, family, seed, "traced, changed model")
    with pytest.raises(AssertionError, match="digest|dispatched"):
        single_traced(sc, dict(m, stats=wrong["stats"]), d)
    with pytest.raises(AssertionError, match="error models' records"):
        single_traced(sc, dict(m, em=wrong["em"]), d)
