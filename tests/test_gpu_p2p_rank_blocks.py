"""k2_rank<true>'s list blocks and one-trip tiles (nsgpu_p2p_win.h: df_list, dense_rec2).

The list blocks make what only the next kernels read — the window copy for the next k2_pa (pwkey / pwctx) and the
dense list of the local records (ldat, ldpd, lrec, their contexts) — and the tile blocks fetch a tile's column and row
in one trip at clamped indices.  A copy or a list entry that was missed or made for the wrong window, or a row fetched
at the wrong index, moves a uid, a rank or a context, so every case
compares the full (ts, uid, context) pop log, the device and application counters, the stats and the digest with the
oracle, bit for bit (test_gpu_p2p_partials' harness: untraced wide engines, the deferred pipeline).  The scenarios are
tests/rank_blocks_cases.py's; tests/test_p2p_rank_blocks_cpu.py checks what each holds."""
import pytest

import rank_blocks_cases as RC
import test_gpu_p2p_partials as partials
from test_gpu_p2p_partials import check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flows", RC.BURSTS)
def test_burst_around_a_share(flows):
    """W = Lt = `flows` in the Send windows: just below, on and just above one tile (256) and one list block's share
    of the copy and of the dense list (1024) — the last thread of a list block, the first of the next."""
    check(RC.burst(flows), 200_000, key=("burst", flows))


def test_second_round_of_tiles():
    """W = Lt = 3,500 in the Send windows: 1,203 tiles against the 988 sub-tiles of a round, so every sub-tile of every
    tile block is used and the tile loop goes round again (tests/test_p2p_rank_blocks_cpu.py has the arithmetic).  The
    Receives a hop on meet the TransmitCompletes of the hop before at one ts, 7,000 gen-0 records: an unranked window
    and a sorted run between the ranked ones."""
    gst = check(RC.burst(RC.SECOND_ROUND), 400_000)
    assert gst.max_window >= 2 * RC.SECOND_ROUND, gst.max_window  # (the Send window was ranked whole)
    assert gst.refits > 0


def test_copy_without_local_records():
    """Windows of delivered Receives: W > 0 and Lt = 0.  The tiles return at once; the copy must still be made, or the
    next k2_pa appends to stale keys."""
    check(RC.one_hop(), 100_000)


def test_start_burst_unranked_window_and_flush():
    """An unranked window (no copy, no list), a sorted run, the hand-over and
    the flush, which reads the list blocks' ldat."""
    gst = check(RC.start_burst(), 1_000_000)
    assert gst.refits > 0  # (a sorted run happened)


def test_hub_regions_in_the_dense_list():
    """The regions' prefix runs over the 64 holder regions and then the hub regions: records past region 64."""
    check(RC.incast(), 400_000)


def test_tied_order_words_in_wide_windows():
    """The exact chain compare after a tile whose row came from the paired search."""
    check(RC.tie_rows_wide(), 100_000)


def test_eight_saturated_rows():
    check(RC.saturated_rows(8), 100_000)


def test_host_closures_cut_windows():
    """Every host probe pauses the deferred pipeline after a window's bookkeeping; the flush reads that window's
    dense list and ranks, and the run resumes with the copy the list blocks made.  The body is test_gpu_p2p_partials'
    own case, run here a second time: it is one of the shapes this file's cases are required to cover, and nothing
    about it is new.  The start burst and the incast star likewise repeat that file's scenarios."""
    partials.test_host_closures_cut_windows()


def test_one_engine_twice():
    """The second run of one engine starts from cleared rank accumulators as the first does."""
    check(RC.burst(RC.SHARE + 1), 200_000, runs=2, key=("burst", RC.SHARE + 1))
