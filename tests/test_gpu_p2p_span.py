"""The wide windows' span controller (nsgpu_p2p_span.h: span_next, called by df_book and by k2_scan's
bookkeeping) and k2_rank<true>'s wide-column tiles (nsgpu_p2p_win.h: RKCW).

Where a window is cut never changes what is dispatched, so every case compares the counts, the digest, the device and
application counters and the full (ts, uid, context) pop log with the oracle, bit for bit; the window counts, refits and
max_window say what the controller did.  The engines are untraced and wide, so the deferred pipeline runs
(test_gpu_p2p_partials' harness)."""
import pytest

import p2p
from test_gpu_p2p_partials import check

pytestmark = pytest.mark.gpu

NMAX = 8192  # records of one window (nsgpu_p2p_win.h)


def grid64(rate_bps):
    """64 lockstep flows down the columns of a 64 x 64 grid (scripts/span_check.cc models the same shapes)."""
    return p2p.grid(64, 64, rate_bps=rate_bps, stop_ns=300_000_000, sim_stop_ns=320_000_000)


def test_windows_reach_the_lookahead():
    """At 2 Mb/s the steady window at the full lookahead (1.4336 ms) holds ~3,700 gen-0 records: inside WCAP, but above
    the 7/8 mark the replaced rule cut the span at.  With the marks at 15/16 and 13/16 the run takes as many windows as
    the 1 Mb/s run of the same grid, whose windows never come near capacity (model: 153 and 151; the engine also spends
    a few windows on the start burst).
    The replaced rule fails this: 176 windows at 2 Mb/s against 161 at 1 Mb/s (this rule: 163 and 161)."""
    slow = check(grid64(1_000_000), 400_000)
    fast = check(grid64(2_000_000), 800_000)
    print("windows", fast.windows, slow.windows, "refits", fast.refits, slow.refits, "max_window", fast.max_window)
    assert fast.windows <= 1.05 * slow.windows, (fast.windows, slow.windows)
    assert fast.refits == slow.refits, (fast.refits, slow.refits)


@pytest.mark.parametrize("rate_bps,parent_refits", [(3_000_000, 1), (4_000_000, 2)])
def test_held_under_capacity(rate_bps, parent_refits):
    """At 3 and 4 Mb/s the full lookahead would take W to ~5,900 and ~8,200: the controller has to hold the windows
    inside WCAP / NMAX without more sorted runs than the replaced rule needed (parent_refits: measured once on the
    parent commit, which took 257 and 371 windows; this rule 241 and 366)."""
    st = check(grid64(rate_bps), 1_500_000)
    print("windows", st.windows, "refits", st.refits, "max_window", st.max_window)
    assert st.refits <= parent_refits, (st.refits, parent_refits)
    assert st.max_window <= NMAX, st.max_window


def saturated_rows(rows, cols=8):
    """test_gpu_wide's deep-chain construction on `rows` identical rows: each saturated by a flow along it (20 Mb/s
    offered to 10 Mb/s links), so the TransmitComplete chains run 3 deep inside a window, in lockstep across rows."""
    return p2p.grid(rows, cols, flows=[(r * cols, r * cols + cols - 1) for r in range(rows)], rate_bps=20_000_000,
                    qmax=100, stop_ns=160_000_000, sim_stop_ns=180_000_000)


def test_region_guard():
    """Eight saturated rows: at the full lookahead the fullest holder region carries 115 to 118 local records of its
    128 (measured with a diagnostic build that reported the fill; 2 rows: 34, 6 rows: 84 to 88), past the 3/4 mark, so
    the controller shortens the windows (312 or 313 instead of 311 in 21 of 24 runs; all 24 completed with no error).
    The parent commit passes this shape too, with those ~10 records to spare; its fill is not steered.  Which slots
    share a holder block depends on the order of the kernels' allocation atomics, so the fill moves by up to ~30 records
    between runs of one scenario: from 12 rows on a region overflows (error 32) in some runs, under the parent's rule
    and, less often, under this one — the guard steers the trend, it cannot bound one window's jump."""
    st = check(saturated_rows(8), 100_000)
    print("windows", st.windows, "max_window", st.max_window)


@pytest.mark.parametrize("flows", [255, 256, 257])
def test_tile_widths(flows):
    """A burst of `flows` lockstep flows down a 3 x 257 grid: every packet time there is a window of W = Lt = `flows`
    (the Sends, with their devices' TransmitCompletes as local records) and a hop later another — just below, on and
    just above one 256-column tile and one 256-row tile: the last wide tile's padding columns, the row tile that
    straddles W and the local rows' tiles each start or end at the boundary."""
    check(p2p.grid(3, 257, n_flows=flows, stop_ns=150_000_000, sim_stop_ns=160_000_000), 100_000)


def test_tile_widths_with_chain_ties():
    """test_gpu_wide's deep-chain tie case (two identical saturated rows: local records whose two order words tie, so
    k2_rank falls back to the exact chain compare) inside windows wide enough for the 256-column tiles: 250 lockstep
    column flows between rows 2 and 3 of the same grid put W above 256 whenever they send, and the saturated rows'
    records then sit in the straddling row tile and among the wide tiles' columns."""
    cols, n = 257, 250
    flows = [(0, 7), (cols, cols + 7)] + [(2 * cols + x, 3 * cols + x) for x in range(n)]
    sc = p2p.grid(4, cols, flows=flows, stop_ns=150_000_000, sim_stop_ns=160_000_000)
    onoff = [a for a in sc.apps if a["kind"] == p2p.APP_ONOFF]
    assert len(onoff) == n + 2
    for a in onoff[:2]:
        a["rate"] = 20_000_000
    check(sc, 100_000)
