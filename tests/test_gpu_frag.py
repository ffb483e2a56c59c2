"""IPv4 fragmentation and reassembly on the GPU engine, each run compared with the Python model
(tests/p2p_frag_pyref.py, pinned by tests/test_frag_cpu.py, which also asserts that the scenarios here are not
vacuous): digest, dispatch count, next uid, the full pop log, device and application counters, UdpServer records,
the fragmentation counters and the sorted trace records."""
import numpy as np
import pytest

import frag_cases as F
import nsgpu
import p2p
import p2p_frag_pyref
from p2p_model_compare import assert_equals_frag_model as assert_equals_model

pytestmark = pytest.mark.gpu

ALL_KINDS = p2p.TRACE_DEVICE_KINDS | p2p.TRACE_IPV4_KINDS
_models = {}


def model(name, *args):
    """The model's run of scenario F.<name> (*args), computed once."""
    if (name, args) not in _models:
        sc = getattr(F, name)(*args)
        _models[(name, args)] = (sc, p2p_frag_pyref.run(sc, ALL_KINDS))
    return _models[(name, args)]


def run_traced(sc, m):
    """A traced single engine (the scanning pipeline) against the model, trace records included."""
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    eng.set_trace(len(m["trace"]) + 64, ALL_KINDS)
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats(), eng.trace())
    eng.close()
    return st


def run_untraced(sc, m, want_wide=None):
    n = m["stats"]["dispatched"]
    eng = p2p.Engine(sc, log_cap=n)
    if want_wide is not None:
        assert eng.wide() == want_wide
    st, devc, appc, log = eng.run(n)
    assert_equals_model(m, st, devc, appc, log, eng.udp_servers(), eng.frag_stats())
    eng.close()


def test_echo_2000_bytes():
    """Two fragments each way; traced and untraced."""
    sc, m = model("echo_2000")
    run_traced(sc, m)
    run_untraced(sc, m)
    assert m["frag"]["fragmented"] == 6 and m["frag"]["reassembled"] == 6


def test_forwarder_passes_fragments_on():
    sc, m = model("forwarding_4000")
    run_traced(sc, m)
    run_untraced(sc, m)


def test_largest_datagram():
    """65507 bytes: 45 fragments through one Send, a list of 45."""
    sc, m = model("largest")
    run_traced(sc, m)
    run_untraced(sc, m)
    assert m["frag"]["fragments_sent"] == 45 and m["frag"]["max_list"] == 45


def test_sender_queue_overflow():
    """Five fragments into the sender's own 2-packet queue: enqueue, enqueue, enqueue, drop, drop."""
    sc, m = model("sender_overflow")
    run_traced(sc, m)
    run_untraced(sc, m)


@pytest.mark.parametrize("icmp", [False, True])
def test_loss_at_a_forwarder(icmp):
    """Fired timers, cancelled timers dispatched, lists that mix datagrams, the ICMP error back to the sender."""
    sc, m = model("loss_at_forwarder", icmp)
    st = run_traced(sc, m)
    run_untraced(sc, m)
    assert (st.icmp_sent > 0) == icmp


def test_ttl_expiry_of_fragments():
    sc, m = model("ttl_expiry")
    st = run_traced(sc, m)
    run_untraced(sc, m)
    assert st.ttl_drops == 9 and st.icmp_sent == 9  # one error a fragment


def test_port_unreachable_after_reassembly():
    sc, m = model("port_unreachable")
    st = run_traced(sc, m)
    run_untraced(sc, m)
    assert st.unreach_drops == 3 and st.icmp_sent == 3


def test_udp_client_packet_size_1500():
    """Sequence numbers survive reassembly; received and lost counts match."""
    sc, m = model("udp_client_1500")
    run_traced(sc, m)
    run_untraced(sc, m)


def test_every_pipeline():
    sc, m = model("grid_pipelines")
    n = m["stats"]["dispatched"]
    run_untraced(sc, m, want_wide=True)  # the default engine: deferred, wide windows
    run_traced(sc, m)  # the scanning pipeline
    grp = p2p.LoopbackGroup(sc, 2, log_cap=n, trace_cap=len(m["trace"]) + 64, trace_kinds=ALL_KINDS)
    st, devc, appc, log = grp.run(n)
    assert_equals_model(m, st, devc, appc, log, grp.udp_servers(), grp.frag_stats(), grp.trace())


def test_hub_forwards_fragments():
    sc, m = model("hub_forwards")
    run_traced(sc, m)
    run_untraced(sc, m)


def test_hub_reassembles_and_sends_fragments():
    """Reassembly and a multi-fragment send inside a hub block (the serial device pass)."""
    sc, m = model("hub_echo_server")
    run_traced(sc, m)
    run_untraced(sc, m)


def test_hub_timeout_with_icmp_in_a_single_device_hub_window():
    """A fired timer with icmp inside a hub window whose device steps are all on one device: the Drop record that
    follows the error's Send names the captured input device and TTL (the parallel device scan declines the window)."""
    sc, m = model("hub_timeout")
    st = run_traced(sc, m)
    run_untraced(sc, m)
    assert st.icmp_sent == 1


def test_list_overflow_fails_the_run():
    """Entry 129 of a reassembly list: the run fails with its own error, nothing is truncated silently."""
    eng = p2p.Engine(F.list_overflow())
    with pytest.raises(nsgpu.NsgpuError, match="4096 = a node's IPv4 reassembly list would pass 128 fragments"):
        eng.run()
    eng.close()


def test_frag_engine_refuses_a_host_closure_runtime():
    sc = F.echo_2000()
    eng = p2p.Engine(sc)
    sim = nsgpu.Sim()
    with pytest.raises(nsgpu.NsgpuError, match="cannot be attached to a host-closure runtime"):
        sim.attach_p2p(eng)
    eng.close()


def test_frag_mode_without_large_datagrams_equals_the_default_handlers():
    """A non-ports scenario on the extended handlers behaves exactly as on the default ones."""
    res = []
    for frag in (False, True):
        sc = p2p.grid(8, 8)
        sc.frag = frag
        eng = p2p.Engine(sc, log_cap=1 << 17)
        st, devc, appc, log = eng.run(1 << 17)
        assert 100 < st.dispatched <= 1 << 17
        res.append((p2p.stats_to_dict(st), devc, appc, log, eng.frag_stats()))
        eng.close()
    (s0, d0, a0, l0, f0), (s1, d1, a1, l1, f1) = res
    for k in ("dispatched", "digest", "next_uid", "final_ts", "cancelled", "unreach_drops"):
        assert s0[k] == s1[k], k
    assert np.array_equal(d0, d1) and np.array_equal(a0, a1)
    assert all(np.array_equal(x, y) for x, y in zip(l0, l1))
    assert f0 == f1 == dict.fromkeys(p2p.FRAG_STATS_FIELDS, 0)
