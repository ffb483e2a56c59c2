"""Receive error models (ReceiveListErrorModel, RateErrorModel) on the GPU engine, each run compared with the Python
model (tests/p2p_errmodel_pyref.py, pinned by tests/test_errmodel_cpu.py, which also asserts that the scenarios here
are not vacuous): digest, dispatch count, next uid, the full pop log, device and application counters, UdpServer
records, the fragmentation counters, the error models' records and the sorted trace records."""
import json
import os

import numpy as np
import pytest

import errmodel_cases as EC
import nsgpu
import p2p
import p2p_errmodel_pyref
from p2p_model_compare import assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
_models = {}


def model(name, *args):
    """The model's run of scenario EC.<name> (*args), computed once."""
    if (name, args) not in _models:
        sc = getattr(EC, name)(*args)
        _models[(name, args)] = (sc, p2p_errmodel_pyref.run(sc, ALL_KINDS))
    return _models[(name, args)]


def run_traced(sc, m):
    """A traced single engine (the scanning pipeline) against the model, trace records included."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models(), eng.trace())
    eng.close()
    return st


def run_untraced(sc, m, want_wide=None, again=False):
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    if want_wide is not None:
        assert eng.wide() == want_wide
    for _ in range(2 if again else 1):  # (run = reset + launch: the second run starts from the reset image)
        st, devc, appc, log = eng.run(n)
        assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.error_models())
    eng.close()
    return st


def run_group(sc, m, owner=None):
    n = m["stats"]["dispatched"]
    grp = p2p.LoopbackGroup(sc, 2, owner=owner, log_cap=n, trace_cap=len(m["trace"]) + 64, trace_kinds=ALL_KINDS)
    st, devc, appc, log = grp.run(n)
    assert_equals_model(m, st, devc, appc, log, grp.udp_servers(), grp.frag_stats(), grp.error_models(), grp.trace())
    return grp


def test_rng_stream_on_the_device_equals_the_reference():
    with open(os.path.join(os.path.dirname(__file__), "golden", "rng_stream_kat.json")) as f:
        kat = json.load(f)
    for c in kat["cases"]:
        for k, vals in c["streams"].items():
            got = p2p.rng_stream(c["seed"], c["run"], int(k), kat["n"], on_device=True)
            assert [x.hex() for x in got.tolist()] == vals, (c["seed"], c["run"], k)


def test_receive_list_on_a_udp_server():
    """ReceiveList [0, 3, 3, 19, 25]: sequence numbers 0, 3 and 19 never reach the server; traced and untraced."""
    sc, m = model("udp_list", "list")
    run_traced(sc, m)
    run_untraced(sc, m)
    assert tuple(m["em"][1]) == (20, 3)


def test_chain_with_an_echo_whose_reply_is_dropped():
    sc, m = model("chain_echo")
    st = run_traced(sc, m)
    run_untraced(sc, m)
    assert st.icmp_sent > 0


@pytest.mark.parametrize("icmp", [False, True])
def test_frag_plus_loss(icmp):
    """A dropped middle fragment: a fired timeout (with icmp its error), cancelled timers dispatched, mixed lists.
    The two cases are also the wide (icmp off) and the narrow (icmp on) engine of one scenario."""
    sc, m = model("frag_loss", icmp)
    st = run_traced(sc, m)
    run_untraced(sc, m, want_wide=not icmp)
    assert (st.icmp_sent > 0) == icmp


@pytest.mark.parametrize("rng_run", [1, 3])
def test_rate_models_on_both_ends_of_a_link(rng_run):
    """Streams (0, 1) and (1, 0): each equals the model, and the two differ."""
    res = []
    for streams in ((0, 1), (1, 0)):
        sc, m = model("rate_both_ends", streams, rng_run)
        run_traced(sc, m)
        st = run_untraced(sc, m)
        res.append(st.digest)
    assert res[0] != res[1]


def test_byte_and_bit_units_with_mixed_frame_sizes():
    sc, m = model("mixed_sizes")
    run_traced(sc, m)
    run_untraced(sc, m)


def test_rate_zero_drops_nothing_and_still_draws():
    sc, m = model("udp_list", "rate0")
    run_untraced(sc, m)
    assert tuple(m["em"][1]) == (20, 0)


def test_rate_one_drops_everything():
    sc, m = model("udp_list", "rate1")
    run_untraced(sc, m)
    assert tuple(m["em"][1]) == (20, 20)


def test_disabled_model_equals_no_model():
    sc, m = model("udp_list", "disabled")
    _sc0, m0 = model("udp_list", "none")
    st = run_untraced(sc, m)
    assert tuple(m["em"][1]) == (0, 0)
    assert st.digest == m0["stats"]["digest"] and np.array_equal(m["devc"], m0["devc"])


@pytest.mark.parametrize("n_leaves", [40, 2000])
def test_hub_blocks(n_leaves):
    """A dumbbell router's same-time Receives (tests/test_errmodel_cpu.py asserts more than CH of them in one window:
    a hub block; 2,000 leaves: a sorted run), two of its devices with a ReceiveList, and a Rate model behind the
    bottleneck."""
    sc, m = model("hub_dumbbell", n_leaves)
    run_traced(sc, m)
    run_untraced(sc, m)


def test_wide_windows():
    sc, m = model("grid_wide")
    run_untraced(sc, m, want_wide=True)  # the default engine: deferred, wide windows
    run_traced(sc, m)  # the scanning pipeline


def test_loopback_group_chain():
    """Two ranks, nodes (0, 1) and (2): the forwarder's model and the destination's advance on different ranks."""
    sc, m = model("chain_echo")
    grp = run_group(sc, m)
    assert list(grp.owner) == [0, 0, 1]


@pytest.mark.parametrize("streams", [(0, 1), (1, 0)])
def test_loopback_group_rate_both_ends(streams):
    sc, m = model("rate_both_ends", streams, 3)
    grp = run_group(sc, m)
    assert list(grp.owner) == [0, 1]


def test_reset_and_rerun_reproduces_the_run():
    for name, args in (("rate_both_ends", ((0, 1), 1)), ("chain_echo", ()), ("frag_loss", (True,))):
        sc, m = model(name, *args)
        run_untraced(sc, m, again=True)


def test_error_model_engine_refuses_a_host_closure_runtime():
    eng = p2p.Engine(EC.udp_list("list"))
    sim = nsgpu.Sim()
    with pytest.raises(nsgpu.NsgpuError, match="receive error model cannot be attached to a host-closure runtime"):
        sim.attach_p2p(eng)
    eng.close()
