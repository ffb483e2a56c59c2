"""The scenarios of tests/test_gpu_p2p_rank_blocks.py hold what they are meant to (the oracle alone, no GPU): a case
that silently exercised nothing would test nothing.  From the oracle's pop log, counters and Dequeue records: the sizes
of the lockstep bursts, the one-hop case's absence of forwarded packets, the start burst, the hub's load and the
saturated rows' chain depth."""
import numpy as np
import pytest

import p2p
import rank_blocks_cases as RC
import trace
from test_gpu_trace import oracle_full

_cache = {}


def run(name, *args, log=200_000):
    key = (name,) + args
    if key not in _cache:
        sc = getattr(RC, name)(*args)
        st, devc, appc, lg, tr = oracle_full(sc, log)
        n = int(st.dispatched)
        assert 0 < n <= log  # (the whole pop log fits)
        _cache[key] = (sc, devc, appc, tuple(np.asarray(a[:n]).astype(np.int64) for a in lg), tr)
    return _cache[key]


@pytest.mark.parametrize("flows", RC.BURSTS)
def test_burst_sizes(flows):
    """After the applications start, every ts of the run carries a whole burst: `flows` Sends, then their `flows`
    TransmitCompletes one transmission time later (the Send window's local records), then the Receives a hop on."""
    sc, _devc, appc, (ts, _uid, _ctx), _tr = run("burst", flows)
    start = min(a["start"] for a in sc.apps if a["kind"] == p2p.APP_ONOFF)
    t, cnt = np.unique(ts[ts > start], return_counts=True)
    assert cnt[-1] == 1  # (Simulator::Stop)
    t, cnt = t[:-1], cnt[:-1]
    assert len(t) >= 10
    assert (cnt % flows == 0).all(), sorted(set(cnt.tolist()))
    assert (cnt == flows).sum() >= 10
    first = t[cnt == flows][0]  # the first burst of Sends; their TransmitCompletes follow within the lookahead
    assert cnt[t == first + RC.TX_NS] == flows
    assert appc["tx_packets"].sum() == 3 * flows  # three packet times


def test_second_round_of_tiles():
    """The Sends of RC.SECOND_ROUND lockstep flows and their TransmitCompletes one transmission time later, inside
    the lookahead of the Sends' window: W = Lt = 3,500, N = 7,000 <= NMAX, and more tiles than the tile blocks' SUBS
    sub-tiles hold at once, so the tile loop goes round a second time."""
    f = RC.SECOND_ROUND
    sc, _devc, _appc, (ts, _uid, _ctx), _tr = run("burst", f, log=400_000)
    start = min(a["start"] for a in sc.apps if a["kind"] == p2p.APP_ONOFF)
    t, cnt = np.unique(ts[ts > start], return_counts=True)
    first = t[cnt == f][0]
    w, lt = int(cnt[t == first][0]), int(cnt[t == first + RC.TX_NS][0])
    assert w == f and lt == f
    assert w <= 4096 and lt <= 4096 and w + lt <= 8192  # (WCAP, LMAX, NMAX)
    assert RC.ntile(w, lt) == 1203
    assert RC.ntile(w, lt) > RC.ROUND == 988
    assert RC.ntile(4096 - 256, 2048) == 496  # (config 4's full window: the arithmetic is the kernel's)
    assert max(RC.ntile(x, x) for x in RC.BURSTS) <= 247  # (the other bursts: sub-tile 0 of a block only)


def test_one_hop_forwards_nothing():
    """Every datagram is transmitted once, by its source's device, and delivered: no node forwards, so no Receive makes
    a local record."""
    _sc, devc, appc, (ts, _uid, _ctx), _tr = run("one_hop")
    sent = int(appc["tx_packets"].sum())
    assert sent >= 5 * RC.ONE_HOP_COLS
    assert int(devc["tx_packets"].sum()) == sent
    assert int(appc["rx_packets"].sum()) > 0
    _t, cnt = np.unique(ts[ts > 100 * RC.MS], return_counts=True)
    assert cnt[-1] == 1  # (Simulator::Stop)
    assert (cnt[:-1] % RC.ONE_HOP_COLS == 0).all()  # (windows of W = 300: Sends, or delivered Receives)


def test_start_burst_is_larger_than_a_window():
    _sc, _devc, _appc, (ts, _uid, _ctx), _tr = run("start_burst", log=1_000_000)
    assert int((ts == 0).sum()) > 4096  # (events at t = 0: more than WCAP)


def test_incast_hub_load():
    """15 saturated 10 Mb/s links deliver 15 / 433.6 us = 34.6 Receives a millisecond to node 0."""
    _sc, _devc, _appc, (ts, _uid, ctx), _tr = run("incast", log=400_000)
    t0, t1 = 1_010 * RC.MS, 1_040 * RC.MS  # (inside the flows' 50 ms, past the first hop's delay)
    at_hub = int(((ctx == 0) & (ts >= t0) & (ts < t1)).sum())
    assert at_hub >= 30 * 30, at_hub


def chain_runs(sc, tr, dev):
    """Lengths of the runs of back-to-back transmissions of device `dev`: each Dequeue exactly one transmission time
    after the one before was started by that one's TransmitComplete (a local record of a local record)."""
    d = np.sort(tr[(tr["kind"] == trace.TR_DEQUEUE) & (tr["dev"] == dev)]["ts"].astype(np.int64))
    assert len(d) > 10
    runs, cur = [], 1
    for gap in np.diff(d):
        if gap == RC.TX_NS:
            cur += 1
        else:
            runs.append(cur)
            cur = 1
    runs.append(cur)
    return d, runs


def source_devices(sc, n):
    """The device each of the first n OnOff applications' nodes transmits on: the one whose peer is the next node of
    its row."""
    nodes = [a["node"] for a in sc.apps if a["kind"] == p2p.APP_ONOFF][:n]
    return [[i for i, d in enumerate(sc.dev) if d[0] == nd and sc.dev[d[1]][0] == nd + 1][0] for nd in nodes]


def test_tie_rows_chain_depth_and_width():
    """The two rows' sources transmit back to back for longer than a window's lookahead holds (3 transmission times),
    at the same instants in both rows; the column flows' bursts are wider than a 256-column tile would be short of."""
    sc, _devc, _appc, (ts, _uid, _ctx), tr = run("tie_rows_wide")
    da, db = source_devices(sc, 2)
    ta, ra = chain_runs(sc, tr, da)
    tb, rb = chain_runs(sc, tr, db)
    assert max(ra) > 3 and max(rb) > 3
    assert np.array_equal(ta, tb)  # (lockstep: the rows' records tie level by level)
    _t, cnt = np.unique(ts[ts > 100 * RC.MS], return_counts=True)
    assert cnt.max() >= RC.TIE_FLOWS + 2


def test_eight_rows_chain_depth():
    sc, _devc, _appc, _log, tr = run("saturated_rows")
    devs = source_devices(sc, 8)
    t0 = None
    for d in devs:
        t, r = chain_runs(sc, tr, d)
        assert max(r) > 3
        t0 = t if t0 is None else t0
        assert np.array_equal(t, t0)
