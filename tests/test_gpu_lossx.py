"""The extended loss chain of the closed-loop Wi-Fi PHY on the device (nsgpu_wifil_set_loss / nsgpu_sim_wifi_set_loss:
k_wl_rx<true> / k_wl_send<true> over the device-resident chain and Matrix table) against tests/lossx_model.py — the
plain-Python PHY of tests/wifi_switch_model.py with tests/loss_ref.py's CalcRxPower — on the scenarios of
tests/lossx_cases.py, which tests/test_lossx_model_cpu.py checks on the model alone.

Exactly equal (wifi_model_compare.equal_model): the pop log (ts, uid, context), the dispatch count and next uid, the
per-phy counters and state fields, the end records' integer fields, every switch call's outcome, get_channel's records,
and GetState / GetDelayUntilIdle at every probing closure.  rx_w and snr within the project's 1e-9 relative (device and
host log10 / pow differ in the last bits), per within test_gpu_wifi_per.compare_record's bound — the tolerances
tests/test_gpu_wifi_switch.py uses for the same fields.  Each case first asserts on the model that no reception's power is
within 1e-6 relative of the ED or CCA threshold: the exact comparisons cannot hang on those last bits."""
import ctypes as C
import math

import numpy as np
import pytest

import loss_ref as lr
import lossx_cases as lc
import lossx_model
import nsgpu
import test_wifi_switch_cpu as sc
import wifi
import wifi_switch_model as wsm
from wifi_model_compare import equal_model, error_code, finish
from test_lossx_model_cpu import run_model

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4


def lossx_of(spec):
    return None if spec is None else nsgpu.lossx(*spec[0], entries=spec[1])


def run_device(case, log_cap=1 << 16, before=None):
    """The case's closures on nsgpu.Sim + wifi.LoopPhy in the model's setup order, then Stop: the chain of the case
    installed before the first closure (LoopPhy.set_loss), every ("loss", spec) action through Sim.wifi_set_loss at
    its place in its closure.  before (lp): called once the case's chain is installed (the refusal test's calls)."""
    ph = case["phys"]
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    sim.set_log(log_cap)
    if case["lossx"] is not None:
        lp.set_loss(lossx_of(case["lossx"]))
    if before:
        before(lp)
    for j, m in (case["mob"]() if case["mob"] else {}).items():
        lp.set_mobility(j, m.position(), (m.vx, m.vy, m.vz), paused=m.paused, last_update=m.last)
    probes, switches, failures = [], [], []

    def closure(actions):
        try:
            ts, uid = sim.now(), sim.current_uid()
            for a in actions:
                if a[0] not in ("noop", "loss"):
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
                elif a[0] == "loss":
                    sim.wifi_set_loss(lossx_of(a[1]))
        except BaseException as e:  # (an exception does not cross the C callback: keep it for the test)
            failures.append(e)

    for ts, actions in case["closures"]:
        sim.schedule(ts, (lambda a=actions: lambda: closure(a))())
    sim.stop(case["stop"])
    sim.run()
    assert not failures, failures
    n = min(sim.dispatched(), log_cap)
    return dict(log=tuple(a[:n].copy() for a in sim.log), dispatched=sim.dispatched(), next_uid=sim.next_uid(),
                ends=lp.read_ends(), phys=lp.read_phys(), notes=lp.read_notes(), probes=probes, switches=switches,
                channels=[lp.get_channel(j) for j in range(ph.n_phy)], sim=sim, lp=lp)


def check(name, c=None, **kw):
    c = c or lc.CASES[name]()
    m = run_model(c)
    lossx_model.clear_of_thresholds(m, 1e-6)
    g = run_device(c, **kw)
    equal_model(g, m, name)
    return g, m


def test_hidden_terminal():
    g, m = check("hidden")
    ph = g["phys"]
    assert (ph["sync"][lc.B], ph["drop_rx"][lc.B]) == (1, 1)
    for j in (lc.A, lc.C):  # nothing heard: no sync, no CCA, IDLE while the other's frame is on the air
        assert (ph["sync"][j], ph["cca_switches"][j], ph["drop_rx"][j]) == (0, 0, 0)
    assert {p[2]: p[3] for p in g["probes"] if p[0] == 3_900_000} == {lc.A: wifi.IDLE, lc.B: wifi.CCA_BUSY, lc.C: wifi.TX}
    assert ph["first_power"][lc.A] == 0.0 and ph["first_power"][lc.C] == 0.0  # (DBL_MAX: exactly 0 W)
    finish(g)


def test_hidden_terminal_set_loss_mid_run():
    g, m = check("hidden_mid_run")
    ends = g["ends"]
    at_c = ends[ends["phy"] == lc.C]
    assert len(at_c) == 1 and int(at_c["tx"][0]) == 2  # C locks on A's frame once A <-> C is set, not before
    assert math.isclose(at_c["rx_w"][0], lr.dbm_to_w(sc.DBM - 70.0 + 1.0), rel_tol=1e-9)
    # the last closure's send / set_loss / send: B's frame reaches A at B -> A = 60 dB, the entry of its own SendPacket
    at_a = ends[(ends["phy"] == lc.A) & (ends["tx"] == 3)]
    assert len(at_a) == 1 and math.isclose(at_a["rx_w"][0], lr.dbm_to_w(sc.DBM - 60.0 + 1.0), rel_tol=1e-9)
    finish(g)


@pytest.mark.parametrize("name", ["three_log", "two_ray", "big_matrix", "matrix_switch", "revert", "old_kinds"])
def test_case_equals_the_model(name):
    g, m = check(name)
    if name == "two_ray":  # the rising phy's height on the device, bit for bit with the model's
        stop = lc.two_ray_case()["stop"]
        assert g["lp"].get_mobility(stop, 6)[:2] == m.mob[6].get(stop)
    if name == "matrix_switch":
        assert g["channels"][2]["channel"] == 1 and g["channels"][2]["switches"] == 1
    if name == "old_kinds":  # set_loss with the config's own chain: the device without it, record for record
        c = lc.old_kinds_case()
        plain = run_device(dict(c, lossx=None))
        for f in g["ends"].dtype.names:
            assert np.array_equal(g["ends"][f], plain["ends"][f]), f  # (the same device code under both: same bits)
        assert all(np.array_equal(a, b) for a, b in zip(g["log"], plain["log"]))
        finish(plain)
    finish(g)


def test_refusals_leave_the_installed_chain_in_force():
    c = lc.hidden_terminal_case()
    n = c["phys"].n_phy
    L = nsgpu.lib()
    m7 = (lr.MATRIX, 7.0)

    def refused(lp):
        def rc(lx):
            return L.nsgpu_wifil_set_loss(lp.h, C.byref(lx))
        for bad_n in (-1, 5):
            lx = nsgpu.lossx(m7)
            lx.n = bad_n
            assert rc(lx) == EINVAL
        assert rc(nsgpu.lossx((8, 1.0, 1.0, 1.0))) == EINVAL and b"unknown kind" in L.nsgpu_last_error()
        assert rc(nsgpu.lossx(m7, m7)) == EINVAL and b"MATRIX" in L.nsgpu_last_error()
        for e in ((n, 0, 1.0), (0, n, 1.0), (0xffffffff, 1, 1.0)):
            assert rc(nsgpu.lossx(m7, entries=[(0, 1, 2.0), e])) == EINVAL and b"names phy" in L.nsgpu_last_error()
        assert rc(nsgpu.lossx((lr.TWO_RAY_GROUND, 0.125, math.nan, 0.5, 1.5))) == EINVAL
        assert rc(nsgpu.lossx((lr.THREE_LOG, 1.0, 200.0, 500.0, 1.9, 3.8, 3.8, math.inf))) == EINVAL
        assert L.nsgpu_wifil_set_loss(None, None) == EINVAL

    g, m = check("hidden", c, before=refused)  # (the case's own chain still decides every power)
    finish(g)
    grp = wifi.LoopPhy(c["phys"], bounds=[0, 1, n])
    lx = nsgpu.lossx(m7)
    assert L.nsgpu_wifil_set_loss(grp.h, C.byref(lx)) == ESTATE and b"single-engine" in L.nsgpu_last_error()
    assert L.nsgpu_wifil_set_loss(grp.h, None) == ESTATE
    grp.close()
    sim = nsgpu.Sim()
    assert L.nsgpu_sim_wifi_set_loss(sim.h, C.byref(lx)) == ESTATE  # no PHY attached
    sim.close()
