"""Constant-velocity mobility of the closed-loop Wi-Fi PHY on the device (nsgpu_wifil_set_mobility and its
neighbours; k_wl_move ahead of every send's k_wl_rx).  Each scenario of tests/mobility_cases.py runs on the device
with native mobility and on the unchanged oracle with the restated positions (tests/mobility_ref.py) written by
SetPosition closures one ns before each send: full pop log, dispatch count, digest, next uid, per-phy counters and
the end records' integer fields are equal; snr / per / rx_w within the closed-loop tests' 1e-9 (device libm vs
glibc); and get_mobility at the end of the run equals the restatement with ==, bit for bit — the integration is
only +, * and integer arithmetic.  The scenarios' preconditions are asserted on the CPU in
tests/test_mobility_cpu.py with the same seeds."""
import ctypes as C

import numpy as np
import pytest

import mobility_cases as mc
import nsgpu
import wifi
from test_mobility_cpu import SEEDS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4


def check(case, **kw):
    pl = mc.plan(case)
    o = mc.run_oracle(case, pl["moves"])
    g = mc.run_device(case, pl, **kw)
    mc.equal_oracle(g["four"], o)
    mc.equal_final(g["final"], pl["final"])
    g["lp"].close()
    return pl, o, g


def test_grid_4x4_one_channel():
    pl, o, _g = check(mc.grid_case(SEEDS["grid"]))
    assert len(o[1]) > 50 and len(pl["final"]) == 15


def test_channels():
    """Phys on channels 1 and 6 update only at their own channel's sends; the lone sender on channel 11 never
    updates before the final read."""
    check(mc.channels_case(SEEDS["channels"]))


def test_block_edge_300_phys():
    pl, _o, _g = check(mc.block_edge_case(SEEDS["block_edge"]), log_cap=1 << 17)
    assert len(pl["final"]) == 300


def test_course_changes_and_a_mid_run_read():
    case = mc.course_case(SEEDS["course"])
    pl, _o, g = check(case)
    reads = g["reads"]
    assert len(reads) == 1
    (ev, (pos, vel, paused)), = reads
    want = [t for e, t in pl["records"] if e == ev][0][12]
    assert pos == want and not paused and vel == case["specs"][12][1]
    assert g["final"][9][1] == (0.0, 0.0, 0.0) and g["final"][3][1] == (0.0, 120.0, 0.0)


def test_more_than_nsend_sends_in_one_closure():
    """Ten SendPackets from one closure (NSEND = 8: the batch flushes), the first sender a fast mover, then sends from
    later closures made from moved positions: every send keeps the receptions of the positions at its own send."""
    check(mc.burst_case(SEEDS["burst"]))


def test_with_hand_back_and_notes():
    case = mc.grid_case(SEEDS["grid"])
    _pl, o, g = check(case, listen=(1, 14), notify=(4, 9))
    ends, phys, notes = o[1], o[2], g["notes"]
    live = ends[((ends["flags"] & wifi.END_CANCELLED) == 0) & np.isin(ends["phy"], (1, 14))]
    assert g["four"][3]["handbacks"] == [(int(e["ts"]), int(e["uid"])) for e in live] and len(live) > 5
    assert set(np.unique(notes["phy"])) == {4, 9}
    for p in (4, 9):
        mine = notes[notes["phy"] == p]
        for name, kind in (("sync", wifi.NOTE_SYNC), ("drop_rx", wifi.NOTE_DROP_RX), ("drop_tx", wifi.NOTE_DROP_TX),
                           ("drop_ed", wifi.NOTE_DROP_ED)):
            assert int(np.count_nonzero(mine["kind"] == kind)) == int(phys[name][p]), (p, name)
        assert len(mine) == int(phys["rx"][p])
        assert int(np.count_nonzero(mine["cca_duration"])) == int(phys["cca_switches"][p])


def test_refusals():
    """Argument checks, made before any launch."""
    case = mc.grid_case(SEEDS["grid"])
    ph = case["phys"]
    L = nsgpu.lib()
    lp = wifi.LoopPhy(ph)
    m = wifi.Mobility((C.c_double * 3)(1, 2, 3), (C.c_double * 3)(4, 5, 6), 0, 0, 0)
    v = (C.c_double * 3)(1, 1, 1)
    for bad in (ph.n_phy, 0xffffffff):
        assert L.nsgpu_wifil_set_mobility(lp.h, bad, C.byref(m)) == EINVAL
        assert L.nsgpu_wifil_set_velocity(lp.h, 0, bad, v) == EINVAL
        assert L.nsgpu_wifil_pause(lp.h, 0, bad, 1) == EINVAL
        assert L.nsgpu_wifil_set_position_at(lp.h, 0, bad, 0.0, 0.0, 0.0) == EINVAL
        assert L.nsgpu_wifil_get_mobility(lp.h, 0, bad, C.byref(m)) == EINVAL
    assert L.nsgpu_wifil_set_velocity(lp.h, 0, 3, v) == ESTATE  # (no model on phy 3)
    assert L.nsgpu_wifil_get_mobility(lp.h, 0, 3, C.byref(m)) == ESTATE
    lp.set_mobility(3, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    assert L.nsgpu_wifil_set_position(lp.h, 3, 0.0, 0.0, 0.0) == ESTATE
    assert b"nsgpu_wifil_set_position_at" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_set_position(lp.h, 2, 0.0, 0.0, 0.0) == 0  # (a constant-position phy: as before)
    assert lp.get_mobility(2_000_000_000, 3) == ((9.0, 12.0, 15.0), (4.0, 5.0, 6.0), False)
    lp.close()
    grp = wifi.LoopPhy(ph, bounds=[0, 8, ph.n_phy])
    assert L.nsgpu_wifil_set_mobility(grp.h, 0, C.byref(m)) == EINVAL
    assert b"single-engine" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_set_mobility(grp.h, 0xffffffff, C.byref(m)) == EINVAL
    grp.close()


def test_static_control_install_then_remove():
    """A model installed and removed (NULL) before the first send: the log and digest of a run that never had one —
    the oracle's with every move carrying the setup position."""
    case = mc.grid_case(SEEDS["grid"])
    pl = mc.plan(case)
    o = mc.run_oracle(case, mc.static_moves(case, pl["moves"]))
    none = dict(case, specs=[None] * 16)

    def install_remove(_sim, lp):
        for j, s in enumerate(case["specs"]):
            if s is not None:
                lp.set_mobility(j, (case["phys"].x[j], case["phys"].y[j], case["phys"].z[j]), s[1])
        for j in range(16):
            lp.set_mobility(j, None, None)

    ga = mc.run_device(none, pl)
    gb = mc.run_device(none, pl, prepare=install_remove)
    a, b = ga["four"], gb["four"]
    mc.equal_oracle(a, o)
    mc.equal_oracle(b, o)
    for p, q in zip(a[0], b[0]):
        assert np.array_equal(p, q)
    assert a[3]["digest"] == b[3]["digest"]
    assert np.array_equal(a[1], b[1])
    ga["lp"].close()
    gb["lp"].close()
