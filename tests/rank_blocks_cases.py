"""Scenarios for k2_rank<true>'s list blocks and one-trip tiles (nsgpu_p2p_win.h: df_list, NLIST,
dense_rec2).  The list blocks make the window copy for the next k2_pa and the dense list of the local records; a
list block's thread has one gen-0 slot and one local record, so
a block's share of either is SHARE = 1024 elements.  The tile blocks fetch a tile's column and row in one memory trip.
tests/test_p2p_rank_blocks_cpu.py asserts with the oracle alone that each scenario holds what it is meant to."""
import p2p

MS = 1_000_000
SHARE = 1024   # a list block's threads (RKT_DF): its share of the copy and of the dense list
TILE = 256     # rows and columns of a rel-ts-only tile (RKT, RKCW)
TX_NS = 433_600  # a 512-byte datagram with its 30 bytes of headers on a 10 Mb/s link

BURSTS = (TILE - 1, TILE, TILE + 1, SHARE - 1, SHARE, SHARE + 1)


def burst(flows):
    """`flows` lockstep flows down a 3 x (flows + 1) grid: every packet time the Sends form a window of W = `flows`
    gen-0 records whose devices' TransmitCompletes are its Lt = `flows` local records, and a hop later the forwarded
    Receives form another.  Three packet times."""
    return p2p.grid(3, flows + 1, n_flows=flows, stop_ns=130 * MS, sim_stop_ns=135 * MS)


# k2_rank<true>'s tile space (nsgpu_p2p_win.h): 256 blocks less the bookkeeping, the NSDEF accounting and the NLIST list
# blocks, SUBS = 4 sub-tiles each
ROUND = (256 - 1 - 4 - 4) * 4
SECOND_ROUND = 3500  # lockstep flows whose Send window needs more tiles than one round holds


def ntile(w, lt):
    """Tiles of a window of w gen-0 and lt local records (k2_rank<true>'s arithmetic: RKT = RKCW = 256, RKC = 64)."""
    n = w + lt
    nr, nrg, ncl, nclw = -(-n // TILE), w // TILE, -(-lt // 64), -(-lt // TILE)
    nl, ncg = -(-lt // TILE), -(-w // TILE)
    return nrg * nclw + (nr - nrg) * ncl + nl * ncg


ONE_HOP_COLS = 300


def one_hop():
    """Flows from row 0 to row 1 of a 2 x 300 grid: the Receives are delivered to the sinks and forward nothing, so
    their windows have W = 300 and no local record (Lt = 0): the window copy is made by a kernel that ranks nothing."""
    return p2p.grid(2, ONE_HOP_COLS, stop_ns=150 * MS, sim_stop_ns=160 * MS)


def start_burst():
    """A 32 x 32 grid has ~5,100 events at t = 0, more than a window holds: an unranked window, a sorted run through
    the scanning pipeline, the hand-over into the deferred pipeline and, at the end, its flush."""
    return p2p.grid(32, 32, stop_ns=300 * MS, sim_stop_ns=350 * MS)


INCAST_DEGREE = 15


def incast():
    """An incast star of degree 15 whose sources saturate their links: the sink takes ~35 Receives a millisecond, more
    than a holder thread sorts, so a hub block runs it and its local records lie in a hub region of the dense list."""
    return p2p.incast(INCAST_DEGREE, rate_bps=10_000_000)


TIE_COLS, TIE_FLOWS = 257, 250


def tie_rows_wide():
    """Two identical saturated rows (20 Mb/s offered to 10 Mb/s links: TransmitComplete chains 3 deep inside a window,
    in lockstep, so local records' two order words tie) beside 250 lockstep column flows between rows 2 and 3 of the
    same grid, which put W above 256 whenever they send."""
    cols, n = TIE_COLS, TIE_FLOWS
    flows = [(0, 7), (cols, cols + 7)] + [(2 * cols + x, 3 * cols + x) for x in range(n)]
    sc = p2p.grid(4, cols, flows=flows, stop_ns=150 * MS, sim_stop_ns=160 * MS)
    onoff = [a for a in sc.apps if a["kind"] == p2p.APP_ONOFF]
    assert len(onoff) == n + 2
    for a in onoff[:2]:
        a["rate"] = 20_000_000
    return sc


def saturated_rows(rows=8, cols=8):
    """`rows` identical rows, each saturated by a flow along it: chains 3 deep in every row at once."""
    return p2p.grid(rows, cols, flows=[(r * cols, r * cols + cols - 1) for r in range(rows)], rate_bps=20_000_000,
                    qmax=100, stop_ns=160 * MS, sim_stop_ns=180 * MS)
