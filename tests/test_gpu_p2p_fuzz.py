"""The seeded cross-feature scenarios (tests/p2p_fuzz_cases.py: ports, fragmentation, ICMP, queue overflow and receive
error models in one scenario) on the GPU engine, each through four pipelines and each run compared bit for bit with
the Python model (tests/p2p_errmodel_pyref.py): every statistic, the full pop log, device and application counters,
UdpServer records, fragmentation counters, the error models' records and the sorted trace records.
tests/test_p2p_fuzz_cpu.py asserts on the model alone that the cases are accepted and reach the interactions meant.

A failure's message names the family and seed, the first differing pop-log entry and what lives on its node:
p2p_fuzz_cases.build (family, seed) rebuilds the scenario on the CPU."""
import pytest

import p2p
import p2p_errmodel_pyref
import p2p_fuzz_cases as FZ
from p2p_model_compare import assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
_models = {}


def model(family, seed):
    """The model's run of one case, computed once."""
    if (family, seed) not in _models:
        sc = FZ.build(family, seed)
        _models[(family, seed)] = (sc, p2p_errmodel_pyref.run(sc, ALL_KINDS))
    return _models[(family, seed)]


def describe(sc, family, seed, pipeline):
    label = "%s seed %d, %s" % (family, seed, pipeline)

    def context(_i, got, want):
        """What lives on the node of the first differing entry (the model's, or the engine's past the model's end)."""
        ctx = (want or got)[2]
        return FZ.describe_node(sc, ctx) if ctx < sc.n_nodes else "no node context"
    return dict(label=label, context=context)


def single_untraced(sc, m, d):
    """The default engine, run twice: run = reset + launch, so the second run starts from the reset image."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n + 64)
    assert eng.wide() == bool(p2p.dist_plan(sc, None, 0, 1)["wide"]), d["label"]
    for again in (False, True):
        st, devc, appc, log = eng.run(n + 64)
        log = tuple(x[:int(st.dispatched)] for x in log)
        assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(),
                            label=d["label"] + (", second run" if again else ""), context=d["context"])
    eng.close()


def single_traced(sc, m, d):
    """The scanning pipeline, trace records included."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n + 64)
    eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(n + 64)
    log = tuple(x[:int(st.dispatched)] for x in log)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(), eng.trace(),
                        **d)
    eng.close()


def group(sc, m, d, nranks, owner):
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, nranks, owner=owner, log_cap=n + 64, trace_cap=len(m["trace"]) + 64,
                            trace_kinds=ALL_KINDS)
    st, devc, appc, log = grp.run(n + 64)
    log = tuple(x[:int(st.dispatched)] for x in log)
    assert_equals_model(m, st, devc, appc, log, grp.udp_servers(), grp.frag_stats(), grp.error_models(), grp.trace(),
                        **d)


PIPELINES = {
    "single": single_untraced,
    "traced": single_traced,
    "group2_blocks": lambda sc, m, d: group(sc, m, d, 2, None),
    "group3_interleaved": lambda sc, m, d: group(sc, m, d, 3, FZ.owner_interleaved(sc, 3)),
}


@pytest.mark.parametrize("pipeline", list(PIPELINES))
@pytest.mark.parametrize("family,seed", FZ.FUZZ_CASES)
def test_engine_equals_model(family, seed, pipeline):
    sc, m = model(family, seed)
    PIPELINES[pipeline](sc, m, describe(sc, family, seed, pipeline))
