"""The deferred pipeline's per-block partial records (nsgpu_p2p_win.h: Part, publish_part, df_fold):
k2_pa's blocks and k2_handle's holder / hub blocks store their minima and child totals with plain stores, and
k2_rank's bookkeeping block folds them into the run control.  A record that stayed unfolded or stale would move a
window's bound or the uid / dispatch counters, so every case compares the full (ts, uid, context) pop log, the
device and application counters and the digest with the oracle, bit for bit.

The engines here are untraced: a traced engine runs the scanning pipeline, which keeps its atomics (the traced
runs of the same shapes are test_gpu_wide's).  Every case asserts a wide engine."""
import numpy as np
import pytest

import nsgpu
import p2p
from test_gpu_mixed import flows_grid, run_oracle
from test_gpu_trace import oracle_full

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("dispatched", "cancelled", "digest", "final_ts", "next_uid", "ttl_drops", "no_route_drops")


def assert_same_untraced(o, g):
    """assert_same_run (test_gpu_trace) without the trace records."""
    st, devc, appc, olog = o[:4]
    gst, gdevc, gappc, glog = g
    for f in STAT_FIELDS:
        assert getattr(gst, f) == getattr(st, f), (f, getattr(gst, f), getattr(st, f))
    assert np.array_equal(gdevc, devc)
    assert np.array_equal(gappc, appc)
    n = int(min(st.dispatched, len(olog[0])))
    assert n > 0
    for a, b, name in zip(glog, olog, ("ts", "uid", "ctx")):
        assert np.array_equal(a[:n], b[:n]), name


_ORACLE = {}


def check(sc, log_cap, runs=1, key=None):
    """key: the oracle's run is shared by the cases of one scenario (computed once, never modified)."""
    o = _ORACLE.get(key) if key else None
    if o is None:
        o = oracle_full(sc, log_cap)
        if key:
            _ORACLE[key] = o
    assert o[0].dispatched <= log_cap  # (the whole pop log is compared)
    eng = p2p.Engine(sc, log_cap=log_cap)
    assert eng.wide()
    gst = None
    for _ in range(runs):  # (run() resets the engine first)
        g = eng.run(log_n=log_cap)
        assert_same_untraced(o, g)
        gst = g[0]
    eng.close()
    return gst


def config4_shape():
    return p2p.grid(16, 16, stop_ns=600_000_000, sim_stop_ns=650_000_000)


def test_config4_shape():
    """The holders publish the next bound in every window."""
    check(config4_shape(), 400_000, key="config4")


def test_sparse_single_flow_along_a_row():
    """One flow along a row of a 4 x 64 grid: most blocks publish in one window and not in the next, and for whole
    stretches the minimum is held by a pool entry only (the pool blocks' partial alone)."""
    sc = p2p.grid(4, 64, flows=[(0, 63)])
    check(sc, 400_000)


def test_same_engine_twice():
    """reset() restores the partial records: the second run of one engine equals the oracle as the first does."""
    check(config4_shape(), 400_000, runs=2, key="config4")


def test_start_burst_larger_than_a_window():
    """A 32 x 32 grid has ~5,100 events at t = 0, more than a window holds: a sorted run through the scanning
    pipeline, then the handover into the deferred pipeline; an overflowing deferred window takes df_book's
    unranked branch, which reads the folded bound."""
    sc = p2p.grid(32, 32, stop_ns=300_000_000, sim_stop_ns=350_000_000)
    gst = check(sc, 1_000_000)
    assert gst.refits > 0  # (a sorted run happened)


def test_hub_block_in_a_wide_engine():
    """An incast star of degree 15 (a wide engine needs a degree of at most 16) whose sources saturate their links:
    the sink takes ~35 Receives a millisecond, more than a holder thread sorts, so a hub block runs it and
    publishes its partial."""
    sc = p2p.incast(15, rate_bps=10_000_000)
    check(sc, 400_000)


def test_host_closures_cut_windows():
    """test_gpu_mixed's harness on its smallest grid, untraced: every host probe pauses the deferred pipeline
    (MODE_HOST), the pause is flushed, and the run resumes."""
    sc = flows_grid()
    app_send = [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_ONOFF][1]
    app_obs = [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_SINK][0]
    t0, period, count, log_cap = 150_000_000, 5_300_001, 30, 400_000
    st, devc, appc, olog, _otr, osamp = run_oracle(sc, t0, period, count, app_send, app_obs, log_cap)
    eng = p2p.Engine(sc, log_cap=log_cap)
    assert eng.wide()
    eng.reset()
    sim = nsgpu.Sim()
    sim.attach_p2p(eng)
    sim.set_log(log_cap)
    samples = []

    def probe():
        samples.append(eng.counters()[1][app_obs].copy())
        sim.p2p_send(app_send)
        if len(samples) < count:
            sim.schedule(period, probe)

    sim.schedule(t0, probe)
    sim.run()
    gst, gdevc, gappc, (lts, luid, lctx) = eng.results(log_n=log_cap)
    host_n, _host_c, host_d = sim.host_stats()
    assert host_n == count
    m = sim.log[1] != 0  # (the host dispatches' ranks)
    lts, luid, lctx = lts.copy(), luid.copy(), lctx.copy()
    lts[m], luid[m], lctx[m] = sim.log[0][m], sim.log[1][m], sim.log[2][m]
    assert sim.dispatched() == st.dispatched
    assert (int(gst.digest) + host_d) & ((1 << 64) - 1) == st.digest
    assert sim.next_uid() == st.next_uid
    assert np.array_equal(gdevc, devc)
    assert np.array_equal(gappc, appc)
    n = int(min(st.dispatched, len(olog[0])))
    for a, b, name in zip((lts, luid, lctx), olog, ("ts", "uid", "ctx")):
        assert np.array_equal(a[:n], b[:n]), name
    gsamp = np.array(samples)
    assert len(gsamp) == len(osamp)
    for f in ("tx_packets", "rx_packets", "tx_bytes", "rx_bytes"):
        assert np.array_equal(gsamp[f], osamp[f]), f
