"""Scenarios for the holder's fused TransmitComplete (nsgpu_p2p_win.h, handle_node2): a local
record whose TransmitComplete is the node's next event and finds its device's queue empty is run where it is made,
and every other one goes through the lane's queue as before.  Each scenario aims at one side of one of the fused
step's conditions.  Routing is XY (along the row first, then the column), so a column flow and a row flow meet at one
node.  tests/test_p2p_fused_tc_cpu.py asserts with the oracle alone that each really produces the TransmitCompletes
it is meant to."""
import p2p

MS = 1_000_000
COLS = 6
CROSS = 2 * COLS + 2  # node (2, 2) of the 6 x 6 grid: two hops from (0, 2) down the column and from (2, 0) along the row


def nid(y, x, cols=COLS):
    return y * cols + x


COLUMN = (nid(0, 2), nid(5, 2))  # through CROSS, forwarded down
ROW = (nid(2, 0), nid(2, 5))     # through CROSS, forwarded right


def frame_tx_ns(sc, app, dev):
    """Transmission time of one datagram of OnOff application `app` on device `dev`: payload + UDP, IPv4 and PPP
    headers (30 bytes) at the device's rate, from the scenario's own fields, in the device's own arithmetic."""
    return p2p.seconds_to_ns((sc.apps[app]["size"] + 30) * 8 / float(sc.dev[dev][2]))


def onoffs(sc):
    return [i for i, a in enumerate(sc.apps) if a["kind"] == p2p.APP_ONOFF]


def alone():
    """Case 1: an 8 x 2 grid with its two column flows.  A node sees one datagram every 8.192 ms and its
    TransmitComplete 433.6 us after it: every record meets the fused step."""
    return p2p.grid(8, 2, flows=[(0, 14), (1, 15)], stop_ns=400 * MS, sim_stop_ns=450 * MS)


def _crossing(delta_ns):
    sc = p2p.grid(COLS, COLS, flows=[COLUMN, ROW], stop_ns=400 * MS, sim_stop_ns=450 * MS)
    sc.apps[onoffs(sc)[1]]["start"] += delta_ns
    return sc


def another_between():
    """Case 2: the row flow starts 200 us after the column flow, so at CROSS its Receive falls between the column
    flow's Receive and the TransmitComplete that one started."""
    return _crossing(200_000)


def equal_ts():
    """Case 3: the row flow starts exactly one frame's transmission time later (433,600 ns): its Receive at CROSS
    has the ts of the column flow's TransmitComplete, and the gen-0 Receive goes first."""
    sc = _crossing(0)
    sc.apps[onoffs(sc)[1]]["start"] += frame_tx_ns(sc, onoffs(sc)[0], 0)
    return sc


def two_busy_devices():
    """Case 4: the two flows in lockstep: CROSS has two Receives at one ts towards different devices, so the first
    record has a gen-0 event of its ts behind it, and the second finds the first in the queue."""
    return _crossing(0)


def queued_behind():
    """Case 5: 2 Mb/s links with 10 ms of delay (Lx = 12.168 ms = 5.6 transmission times: wide), and two 1.5 Mb/s
    flows that merge at CROSS onto the link down its column: 3.18 Mb/s offered to 2 Mb/s.  Its queue of 20 fills in
    ~80 ms and drops from then on; a TransmitComplete there starts the next transmission, whose TransmitComplete
    falls in the same window: chains of local records."""
    return p2p.grid(COLS, COLS, bps=2_000_000, delay_ns=10 * MS, qmax=20, rate_bps=1_500_000,
                    flows=[COLUMN, (nid(2, 0), nid(5, 2))], stop_ns=500 * MS, sim_stop_ns=560 * MS)


def leaf_pending():
    """Case 6: a row flow that ends at CROSS in lockstep with the column flow through it (the row flow first: its
    Sends have the older uids): CROSS has a delivered Receive, with its inline leaf, and then a forwarded Receive at
    one ts."""
    return p2p.grid(COLS, COLS, flows=[(nid(2, 0), CROSS), COLUMN], stop_ns=400 * MS, sim_stop_ns=450 * MS)


def start_burst():
    """Case 7: a 32 x 32 grid has ~5,100 events at t = 0, more than a window holds: a sorted run and its handover to
    the window pipeline, then four column flows."""
    return p2p.grid(32, 32, flows=[(x, nid(31, x, 32)) for x in range(4)], stop_ns=300 * MS, sim_stop_ns=340 * MS)


CASES = ("alone", "another_between", "equal_ts", "two_busy_devices", "queued_behind", "leaf_pending", "start_burst")
