"""Channel switching of the closed-loop Wi-Fi PHY on the device (nsgpu_wifil_set_channel: k_wl_switch, k_wl_rechan,
the SWITCHING instantiations of k_wl_stepw) against tests/wifi_switch_model.py, the plain-Python restatement that
tests/test_wifi_switch_cpu.py holds to the C++ oracle and to hand-derived branch cases.

Exactly equal: the pop log (ts, uid, context), the dispatch count and next uid, the per-phy counters and state fields,
the end records' integer fields, the notes, every switch call's outcome, get_channel's records, and GetState /
GetDelayUntilIdle at every closure.  snr / per / rx_w: tests/test_gpu_wifi_per.py's compare_record (its bound function,
K_DEVICE) against the model's 60-digit reference values.  The comparison itself is tests/wifi_model_compare.py's
equal_model, which tests/test_gpu_lossx.py and tests/test_gpu_wifi_fuzz.py share."""
import numpy as np
import pytest

import mobility_cases as mc
import nsgpu
import test_wifi_switch_cpu as sc
import wifi
import wifi_switch_model as wsm
from wifi_model_compare import equal_model, error_code, finish

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4


def run_device(case, notify=(), mob=None, log_cap=1 << 16):
    """The scenario's closures on nsgpu.Sim + wifi.LoopPhy, scheduled in the model's setup order, then Stop.  Every
    closure first reads GetState of the phys it acts on (the probes), then acts; a refused switch (ESTATE) is
    recorded as the model records it.  A postponed switch's retry is Sim.wifi_set_channel's own."""
    ph = case["phys"]
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    sim.set_log(log_cap)
    for p in notify:
        sim.wifi_notify(p)
    for j, m in (mob or {}).items():
        lp.set_mobility(j, m.position(), (m.vx, m.vy, m.vz), paused=m.paused, last_update=m.last)
    probes, switches, failures = [], [], []

    def closure(actions):
        try:
            ts, uid = sim.now(), sim.current_uid()
            for a in actions:
                if a[0] != "noop":
                    probes.append((ts, uid, a[1]) + tuple(sim.wifi_state(a[1])))
            for a in actions:
                if a[0] == "send":
                    sim.wifi_send(a[1], a[2], sc.DBM, sc.MODE, sc.PREAMBLE)
                elif a[0] == "switch":
                    try:
                        switches.append((ts, uid, a[1]) + tuple(sim.wifi_set_channel(a[1], a[2], a[3])))
                    except nsgpu.NsgpuError as e:
                        assert error_code(e) == ESTATE and "switching" in str(e), e
                        switches.append((ts, uid, a[1], wsm.REFUSED, wsm.SWITCHING, 0))
        except BaseException as e:  # (an exception does not cross the C callback: keep it for the test)
            failures.append(e)

    for ts, actions in case["closures"]:
        sim.schedule(ts, (lambda a=actions: lambda: closure(a))())
    sim.stop(case["stop"])
    sim.run()
    assert not failures, failures
    n = min(sim.dispatched(), log_cap)
    out = dict(log=tuple(a[:n].copy() for a in sim.log), dispatched=sim.dispatched(), next_uid=sim.next_uid(),
               ends=lp.read_ends(), phys=lp.read_phys(), notes=lp.read_notes(), probes=probes, switches=switches,
               channels=[lp.get_channel(j) for j in range(ph.n_phy)], sim=sim, lp=lp)
    return out


# ---------------------------------------------------------------- device vs model
def test_grid_every_branch():
    c = sc.grid_switch_case()
    m = sc.run_model(c, notify=range(16))
    assert sc.branch_coverage(m) >= sc.ALL_BRANCHES, sc.ALL_BRANCHES - sc.branch_coverage(m)
    g = run_device(c)  # (no phy notifies: k_wl_stepw<false, true> from the first switch on)
    equal_model(g, m, "grid")
    assert len(g["notes"]) == 0 and sum(r["drop_switching"] for r in g["channels"]) >= 2
    # the runtime scheduled the postponed switch's retry: its (ts, uid) in the log, every later uid as the model's
    (rt, ruid), = m.retries
    i = int(np.flatnonzero(g["log"][1] == ruid)[0])
    assert (int(g["log"][0][i]), int(g["log"][2][i])) == (rt, wsm.NO_CONTEXT)
    finish(g)


def test_grid_with_notes_on():
    c = sc.grid_switch_case()
    m = sc.run_model(c, notify=range(16))
    g = run_device(c, notify=range(16))
    equal_model(g, m, "grid + notes")
    notes, want = g["notes"], m.note_records()
    assert len(notes) == len(want)
    for f in wifi.WIFIL_NOTE_DTYPE.names:
        assert np.array_equal(notes[f], want[f]), f
    sw = notes[notes["kind"] == wifi.NOTE_DROP_SWITCHING]
    assert len(sw) >= 2 and (sw["state"] == wifi.SWITCHING).all() and (sw["cca_duration"] != 0).any() \
        and (sw["cca_duration"] == 0).any()
    assert not (notes[notes["kind"] != wifi.NOTE_DROP_SWITCHING]["state"] == wifi.SWITCHING).any()
    finish(g)


def test_324_phys_two_blocks():
    c = sc.big_grid_case()
    m = sc.run_model(c)
    g = run_device(c)
    equal_model(g, m, "18 x 18")
    done = sorted(s[2] for s in g["switches"] if s[3] == wifi.SWITCH_DONE)
    assert done == [3, 3, 300, 323] and g["channels"][305]["switches"] == 1  # (305's: the retry's)
    # the receiver counts behind nsgpu_wifil_receivers follow the channels
    chan = np.array([r["channel"] for r in g["channels"]])
    n = nsgpu.C.c_uint32()
    for j in (0, 3, 4, 300, 301, 305, 323):
        nsgpu.check(nsgpu.lib().nsgpu_wifil_receivers(g["lp"].h, j, nsgpu.C.byref(n)))
        assert n.value == np.count_nonzero(chan == chan[j]) - 1, j
    finish(g)


@pytest.mark.parametrize("name", [b for b in sc.BRANCHES if b != "send_while_switching"])
def test_branch_cases(name):
    c = sc.branch_case(name)
    m = sc.run_model(c, notify=range(6))
    g = run_device(c, notify=range(6))
    equal_model(g, m, name)
    assert np.array_equal(g["notes"], m.note_records())
    finish(g)


def test_postponed_switch_through_the_runtime():
    """Sim.wifi_set_channel while the phy transmits: POSTPONED with GetDelayUntilIdle, and the runtime's own retry
    closure runs at m_endTx with the uid the model's Simulator::Schedule took; the later uids follow."""
    c = sc.branch_case("tx")
    m = sc.run_model(c)
    g = run_device(c)
    equal_model(g, m, "tx")
    assert g["switches"] == [(sc.T0 + 300_000, 6, 0, wifi.SWITCH_POSTPONED, wifi.TX, sc.DUR - 300_000)]
    assert m.retries == [(sc.T0 + sc.DUR, 11)]
    i = list(g["log"][1]).index(11)
    assert int(g["log"][0][i]) == sc.T0 + sc.DUR and list(g["log"][1][i:]) == [e[1] for e in m.log[i:]]
    assert g["channels"][0] == dict(channel=6, start_switching=sc.T0 + sc.DUR, end_switching=sc.T0 + sc.DUR + sc.DELAY,
                                    switches=1, drop_switching=0)
    finish(g)


def test_with_a_constant_velocity_phy():
    c = sc.grid_switch_case()
    mob = sc.mobile_models(c["phys"])
    m = sc.run_model(c, mob=mob)
    g = run_device(c, mob=sc.mobile_models(c["phys"]))
    equal_model(g, m, "grid + mobility")
    got = {j: g["lp"].get_mobility(c["stop"], j)[:2] for j in mob}
    mc.equal_final(got, {j: mob[j].get(c["stop"]) for j in mob})  # k_wl_move follows the switched channels: bit for bit
    finish(g)


def test_more_than_nsend_sends_and_a_switch_in_one_closure():
    c = sc.burst_case()
    m = sc.run_model(c, notify=range(16))
    g = run_device(c, notify=range(16))
    equal_model(g, m, "burst")
    assert np.array_equal(g["notes"], m.note_records())
    assert g["channels"][12]["drop_switching"] == 10 and g["phys"]["rx"][13] == 10
    finish(g)


# ---------------------------------------------------------------- refusals and the error path
def test_refusals():
    c = sc.branch_case("idle")
    ph = c["phys"]
    L, C = nsgpu.lib(), nsgpu.C
    lp = wifi.LoopPhy(ph)
    out, rec = wifi.WifilSwitch(), wifi.WifilChannel()
    for bad in (ph.n_phy, 0xffffffff):
        assert L.nsgpu_wifil_set_channel(lp.h, 1000, bad, 6, sc.DELAY, C.byref(out)) == EINVAL
        assert L.nsgpu_wifil_get_channel(lp.h, bad, C.byref(rec)) == EINVAL
    assert L.nsgpu_wifil_set_channel(lp.h, 1000, 1, 6, -1, C.byref(out)) == EINVAL
    assert b"negative" in L.nsgpu_last_error()
    assert lp.get_channel(1) == dict(channel=1, start_switching=0, end_switching=0, switches=0, drop_switching=0)
    assert lp.set_channel(1000, 1, 6, sc.DELAY) == (wifi.SWITCH_DONE, wifi.IDLE, 0)
    assert L.nsgpu_wifil_set_channel(lp.h, 1100, 1, 11, sc.DELAY, C.byref(out)) == ESTATE  # while SWITCHING
    assert b"yans-wifi-phy.cc:338" in L.nsgpu_last_error()
    st = wifi.WifilPhyState()
    nsgpu.check(L.nsgpu_wifil_get_state(lp.h, 1, 1100, C.byref(st)))
    assert (st.state, st.delay_until_idle) == (wifi.SWITCHING, 1000 + sc.DELAY - 1100)
    assert lp.get_channel(1) == dict(channel=6, start_switching=1000, end_switching=1000 + sc.DELAY, switches=1,
                                     drop_switching=0)
    assert lp.set_channel(1000 + sc.DELAY, 1, 11, 0) == (wifi.SWITCH_DONE, wifi.IDLE, 0)  # (a zero delay is allowed)
    assert lp.get_channel(1)["channel"] == 11 and lp.get_channel(5)["channel"] == 11
    lp.close()
    grp = wifi.LoopPhy(ph, bounds=[0, 3, ph.n_phy])
    assert L.nsgpu_wifil_set_channel(grp.h, 1000, 1, 6, sc.DELAY, C.byref(out)) == ESTATE
    assert b"single-engine" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_get_channel(grp.h, 1, C.byref(rec)) == ESTATE
    assert L.nsgpu_wifil_set_channel(grp.h, 1000, ph.n_phy, 6, sc.DELAY, C.byref(out)) == EINVAL
    grp.close()


def test_send_packet_while_switching_fails_the_next_advance():
    """ns-3's NS_ASSERT (yans-wifi-phy.cc:508): the engine reports it at the next advance, as a SendPacket while TX."""
    c = sc.branch_case("send_while_switching")
    with pytest.raises(wsm.SendError):
        sc.run_model(c)
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(c["phys"])
    sim.attach_wifi(lp)
    for ts, actions in c["closures"]:
        for a in actions:
            if a[0] == "send":
                sim.schedule(ts, (lambda a=a: lambda: sim.wifi_send(a[1], a[2], sc.DBM, sc.MODE, sc.PREAMBLE))())
            else:
                sim.schedule(ts, (lambda a=a: lambda: sim.wifi_set_channel(a[1], a[2], a[3]))())
    sim.stop(c["stop"])
    with pytest.raises(nsgpu.NsgpuError) as ei:
        sim.run()
    assert error_code(ei.value) == ESTATE and "SendPacket while switching channels" in str(ei.value)
    lp.close()
    sim.close()
