"""Constant-velocity mobility on the CPU: the restatement (tests/mobility_ref.py) against the reference's own
vectors, the scenarios' preconditions (tests/mobility_cases.py: the oracle sees the motion, no reception sits on a
threshold, the update order shows in the bits), the moves construction's self-consistency, and the C-ABI's exports.
tests/test_gpu_wifi_mobility.py runs the same scenarios on the device."""
import ctypes
import json
import os
import re

import pytest

import mobility_cases as mc
import nsref
import wifi
from mobility_ref import CvModel, everyone_updates

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nsgpu_wifil_set_mobility", "nsgpu_wifil_set_velocity", "nsgpu_wifil_pause", "nsgpu_wifil_set_position_at",
               "nsgpu_wifil_get_mobility", "nsgpu_sim_wifi_set_mobility", "nsgpu_sim_wifi_set_velocity",
               "nsgpu_sim_wifi_pause", "nsgpu_sim_wifi_get_mobility")
# the scenarios' seeds: chosen so that the preconditions below hold (they are asserted, not assumed)
SEEDS = dict(grid=1, channels=2, block_edge=3, course=5, burst=6)


def preconditions(case, pl, margin=1e-6):
    """No reception within 1e-6 relative of the ED / CCA threshold (a last-bit difference of the device's pow could
    not flip a branch), and the oracle's moving run differs from its static control."""
    assert mc.reception_margins(case, pl) > margin
    moving = mc.run_oracle(case, pl["moves"])
    static = mc.run_oracle(case, mc.static_moves(case, pl["moves"]))
    assert not mc.same_run(moving, static)
    return moving, static


# ---------------------------------------------------------------- the reference's own vectors
@pytest.mark.parametrize("name", ["simple setdest", "square setdest"])
def test_restatement_reproduces_the_ns2_helper_reference_points(name):
    """SetVelocity at each reference time; position and velocity there equal the fixture with operator== on the
    doubles, as ns2-mobility-helper-test-suite.cc:57-60,199-202 compares them."""
    pts = json.load(open(os.path.join(REPO, "tests", "golden", "mobility_kat.json")))["cases"][name]
    m = CvModel(pts[0]["pos"])
    assert m.paused
    for p in pts:
        now = p["t"] * 1_000_000_000
        m.set_velocity(now, p["vel"])
        pos, vel = m.get(now)
        assert pos == tuple(float(c) for c in p["pos"]), (p, pos)
        assert vel == tuple(float(c) for c in p["vel"]), (p, vel)


def test_paused_model_keeps_its_place_and_reports_no_velocity():
    m = CvModel((1.0, 2.0, 3.0), (4.0, 5.0, 6.0))  # (a fresh model is paused: constant-velocity-helper.cc:27-42)
    assert m.get(7_000_000_000) == ((1.0, 2.0, 3.0), (0.0, 0.0, 0.0)) and m.last == 7_000_000_000
    m.pause(8_000_000_000, False)
    assert m.get(8_500_000_000) == ((3.0, 4.5, 6.0), (4.0, 5.0, 6.0))
    m.set_position(9_000_000_000, (0.0, 0.0, 0.0))
    assert m.get(10_000_000_000) == ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) and not m.paused


# ---------------------------------------------------------------- the scenarios
def test_grid_case_is_observable_and_order_sensitive():
    case = mc.grid_case(SEEDS["grid"])
    pl = mc.plan(case)
    moving, static = preconditions(case, pl)
    assert moving[3]["dispatched"] > 500 and len(moving[1]) > 50
    assert int(moving[2]["drop_ed"].sum()) != int(static[2]["drop_ed"].sum())
    # accumulated at the sends vs one product at the end: the bits differ for most phys
    acc, one = mc.bits(pl["final"]), mc.bits(mc.closed_form(case))
    assert sum(acc[j] != one[j] for j in acc) >= 8
    assert acc[2] == one[2] and acc[6] == one[6]  # (the zero velocity, the paused phy)
    assert 11 not in acc


def test_channels_case_update_rule_shows_in_the_bits():
    case = mc.channels_case(SEEDS["channels"])
    pl = mc.plan(case)
    preconditions(case, pl)
    # the lone sender never updates before the final read: one product
    assert mc.bits(pl["final"])[15] == mc.bits(mc.closed_form(case))[15]
    every = mc.plan(case, everyone_updates)
    a, b = mc.bits(pl["final"]), mc.bits(every["final"])
    assert a[15] != b[15] and sum(a[j] != b[j] for j in a) >= 6
    # a channel-6 phy is not touched by a channel-1 send
    for ev, touched in pl["records"]:
        ch = case["phys"].channel
        assert all(ch[j] == ch[ev[2]] for j in touched)


def test_block_edge_case():
    case = mc.block_edge_case(SEEDS["block_edge"])
    pl = mc.plan(case)
    preconditions(case, pl)
    assert case["phys"].n_phy == 300 and len(pl["moves"]) == 12 * 300


def test_course_case_read_is_an_accumulation_point():
    case = mc.course_case(SEEDS["course"])
    pl = mc.plan(case)
    preconditions(case, pl)
    without = mc.plan(mc.course_case(SEEDS["course"], with_get=False))
    a, b = mc.bits(pl["final"]), mc.bits(without["final"])
    assert a[12] != b[12] and all(a[j] == b[j] for j in a if j != 12)
    assert pl["final"][9][1] == (0.0, 0.0, 0.0) and pl["final"][3][1] == (0.0, 120.0, 0.0)
    assert pl["final"][7][1] != (0.0, 0.0, 0.0)  # (unpaused again)


def test_burst_case():
    case = mc.burst_case(SEEDS["burst"])
    pl = mc.plan(case)
    moving, _static = preconditions(case, pl)
    # the closure that made the ten sends then moves phy 0 far away: the restated order has the move after them
    p0 = [t[0] for ev, t in pl["records"] if 0 in t]
    assert p0[10] == (900.0, 700.0, 0.0) and p0[9] != p0[10]
    # the variant guarded against (the flush-path hazard): the sends' receptions derived after that move — the
    # oracle with the move one ns before the burst — is a different run
    t0 = case["sends"][0][0]
    early = [(t0 - 1 if t == t0 else t, j, p) for t, j, p in pl["moves"]]
    assert [m for m in early if m[0] != t0 - 1] == [m for m in pl["moves"] if m[0] not in (t0, t0 - 1)]
    assert not mc.same_run(moving, mc.run_oracle(case, early))


def test_moves_construction_is_self_consistent():
    case = mc.grid_case(SEEDS["grid"])
    pl, pl2 = mc.plan(case), mc.plan(mc.grid_case(SEEDS["grid"]))
    assert pl["moves"] == pl2["moves"] and pl["slots"] == pl2["slots"]
    a, b = mc.run_oracle(case, pl["moves"]), mc.run_oracle(case, pl2["moves"])
    assert mc.same_run(a, b)
    assert not mc.same_run(a, mc.run_oracle(case, mc.static_moves(case, pl["moves"])))
    # every move sits one ns before its send, after the previous send
    ts = [t for t, _p in case["sends"]]
    assert {t for t, _j, _p in pl["moves"]} == {t - 1 for t in ts}


# ---------------------------------------------------------------- the C-ABI
def test_library_exports_the_mobility_calls():
    import nsgpu
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "nsgpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsgpu_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW_SYMBOLS) <= declared, set(NEW_SYMBOLS) - declared
    assert set(NEW_SYMBOLS) <= set(nsgpu.SIGNATURES)
    if not os.path.exists(nsgpu.LIB_PATH):
        pytest.skip("libnsgpu.so not built (run __graft_entry__.build())")
    so = ctypes.CDLL(nsgpu.LIB_PATH)
    missing = [s for s in NEW_SYMBOLS if not hasattr(so, s)]
    assert not missing, missing


def test_mobility_struct_is_the_c_record():
    txt = open(os.path.join(REPO, "include", "nsgpu_types.h")).read()
    body = re.search(r"typedef struct nsgpu_mobility \{(.*?)\} nsgpu_mobility;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == \
        ["double pos[3], vel[3]", "int64_t last_update", "uint32_t paused, pad_"]
    assert ctypes.sizeof(wifi.Mobility) == 64
    assert [f for f, _t in wifi.Mobility._fields_] == ["pos", "vel", "last_update", "paused", "pad_"]
    assert (wifi.Mobility.vel.offset, wifi.Mobility.last_update.offset, wifi.Mobility.paused.offset) == (24, 48, 56)
