"""The seeded cross-feature scenarios of the closed-loop Wi-Fi PHY (tests/wifi_fuzz_cases.py: notes, the EndReceive
hand-back with MAC replies, three mobility models, channel switches, mid-run loss chains and frames of many modes in one
run) on the device, each through three pipelines and each run compared with the plain-Python model
(tests/wifi_fuzz_model.py), which tests/test_wifi_fuzz_cpu.py holds to the C++ oracle and checks for what the cases
reach.

  plain     no phy notifies, the run is logged: k_wl_stepw<false, *>.  Everything but the notes.
  notes     every phy notifies, a read-only note handler: k_wl_stepw<true, *>.  The notes field by field, everything
            else as in `plain` (a model run with every phy notifying differs from the case's in the notes alone: asserted
            on the CPU).
  unlogged  no log — the benchmark's mode: the epoch order runs behind the PHY on the second stream.  The dispatch count,
            next uid, records, counters, probes, switches; the host digest against the digest of the model's pop log.

Exactly equal (tests/wifi_model_compare.py): the pop log (ts, uid, context), dispatch count, next uid, counters and
state fields, the end records' integer fields, every probe, every attempt with the state it met, every switch outcome
and channel record, every hand-back (seen by the handler at its record's now and uid), every mobility model's read at
the stop time bit for bit.  snr / per / rx_w: test_gpu_wifi_per.compare_record — 1e-9 relative and the K_DEVICE bound.

Measured on an MI355X: the file's 63 tests take 7.3 s, the slowest 0.36 s (grid 0, plain: it builds the first case).
Worst per ratio (|d per| over the K = 1 bound; K_DEVICE is 128) over the committed cases: 0.75 (dense 1), beside the
0.50 of tests/test_gpu_wifi_per.py; 152 further seeds run once by hand through `plain` reached 2.03.  Before the cases'
extended chains were padded (wifi_fuzz_cases.PAD_DB) the ratio reached 161 (grid 11) with every discrete result equal:
per then follows the last bits of earlier, 40 dB stronger powers through m_firstPower's residue, which the bound —
made for the device's arithmetic at equal inputs — does not cover; tests/test_wifi_fuzz_cpu.py now accepts a case only
if that residue cannot move a per by more than 0.9 of its bound.

A failure names the family and seed, the first differing pop-log entry and what lives on its phy;
wifi_fuzz_cases.build (family, seed) rebuilds the case on the CPU."""
import numpy as np
import pytest

import mobility_cases as mc
import nsgpu
import wifi
import wifi_fuzz_cases as FZ
import wifi_fuzz_model as fm
import wifi_switch_model as wsm
from wifi_model_compare import equal_fuzz, error_code, finish

pytestmark = pytest.mark.gpu

ESTATE = 4
_models = {}


def model(family, seed):
    """The model's runs of one case, computed once: the case's own, the one with every phy notifying, the mobility
    models' final reads."""
    if (family, seed) not in _models:
        case = FZ.build(family, seed)
        m = fm.run(case, notify=())
        noted = fm.run(case, notify=range(case["phys"].n_phy))
        _models[(family, seed)] = (case, m, noted.note_records(), fm.final_reads(m, case["stop"]))
    return _models[(family, seed)]


def lossx_of(spec):
    return None if spec is None else nsgpu.lossx(*spec[0], entries=spec[1])


def run_device(case, pipeline):
    """The case on nsgpu.Sim + wifi.LoopPhy: the closures scheduled in the model's setup order, then Stop.  A closure
    first reads GetState of every phy its actions name, then acts; an attempt sends unless the state its phy was read
    in (read again if the closure has acted on that phy since) is TX or SWITCHING.  The end handler is the model's MAC:
    the phy's next draw against the record's per, a reply closure scheduled after the phy's delay."""
    ph, n = case["phys"], case["phys"].n_phy
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    log_cap = 1 << 16
    if pipeline != "unlogged":
        sim.set_log(log_cap)
    if case["lossx"] is not None:
        lp.set_loss(lossx_of(case["lossx"]))
    for j, s in case["specs"].items():
        mc.install(lp, j, s, (ph.x[j], ph.y[j], ph.z[j]))
    probes, switches, attempts, handbacks, seen_notes, failures = [], [], [], [], [], []
    ndraw = [0] * n

    def guarded(fn):
        def run(*a):
            try:
                fn(*a)
            except BaseException as e:  # (an exception does not cross the C callback: keep it for the test)
                failures.append(e)
        return run

    def closure(actions):
        ts, uid = sim.now(), sim.current_uid()
        state, touched = {}, set()
        for a in actions:
            if a[0] not in fm.Model.NO_PHY:
                state[a[1]] = tuple(sim.wifi_state(a[1]))
                probes.append((ts, uid, a[1]) + state[a[1]])
        for a in actions:
            k = a[0]
            if k in ("attempt", "reply"):
                j = a[1]
                st = sim.wifi_state(j)[0] if j in touched else state[j][0]
                sent = st not in (wifi.TX, wifi.SWITCHING)
                attempts.append((ts, uid, j, sent, st, k == "reply"))
                if sent:
                    sim.wifi_send(j, a[2], a[5], a[3], a[4])
            elif k == "switch":
                try:
                    switches.append((ts, uid, a[1]) + tuple(sim.wifi_set_channel(a[1], a[2], a[3])))
                except nsgpu.NsgpuError as e:
                    assert error_code(e) == ESTATE and "switching" in str(e), e
                    switches.append((ts, uid, a[1], wsm.REFUSED, wsm.SWITCHING, 0))
            elif k == "loss":
                sim.wifi_set_loss(lossx_of(a[1]))
            elif k == "velocity":
                sim.wifi_set_velocity(a[1], a[2])
            elif k == "pause":
                sim.wifi_pause(a[1], a[2])
            elif k == "position":
                sim.wifi_set_position(a[1], *a[2])
            elif k == "add_waypoint":
                sim.wifi_add_waypoint(a[1], a[2], a[3])
            elif k == "end_waypoints":
                sim.wifi_end_waypoints(a[1])
            elif k == "accel":
                sim.wifi_set_velocity_and_acceleration(a[1], a[2], a[3])
            else:
                raise ValueError(k)
            if k not in fm.Model.NO_PHY:
                touched.add(a[1])

    def end_receive(e):  # YansWifiPhy::EndReceive's host part: the draw, then the MAC's receive callback
        j = int(e["phy"])
        assert (sim.now(), sim.current_uid()) == (int(e["ts"]), int(e["uid"]))
        handbacks.append((int(e["ts"]), int(e["uid"]), j))
        u = fm.draw(j, ndraw[j])
        ndraw[j] += 1
        if u > e["per"] and j in case["reply"]:
            delay, size, mode, preamble, dbm = case["reply"][j]
            sim.schedule(delay, guarded(lambda: closure([("reply", j, size, mode, preamble, dbm)])))

    def note(r):  # (read-only)
        assert (sim.now(), sim.current_uid()) == (int(r["ts"]), int(r["uid"]))
        seen_notes.append(r.copy())

    sim.wifi_set_end_handler(guarded(end_receive))
    for j in case["listen"]:
        sim.wifi_listen(j)
    if pipeline == "notes":
        sim.wifi_set_note_handler(guarded(note))
        for j in range(n):
            sim.wifi_notify(j)
    for ts, actions in case["closures"]:
        sim.schedule(ts, guarded((lambda a=actions: lambda: closure(a))()))
    sim.stop(case["stop"])
    sim.run()
    assert not failures, failures
    log = None
    if pipeline != "unlogged":
        assert sim.dispatched() <= log_cap
        log = tuple(a[:sim.dispatched()].copy() for a in sim.log)
    kind = {j: s[0] for j, s in case["specs"].items()}
    notes = lp.read_notes()
    if pipeline == "notes":  # (delivered notes are consumed: what the handler saw, in its order, is compared)
        assert len(notes) == 0
        notes = np.array(seen_notes, wifi.WIFIL_NOTE_DTYPE)
    return dict(log=log, dispatched=sim.dispatched(), next_uid=sim.next_uid(), digest=sim.host_stats()[2],
                ends=lp.read_ends(), phys=lp.read_phys(), notes=notes, probes=probes, switches=switches,
                attempts=attempts, handbacks=handbacks, channels=[lp.get_channel(j) for j in range(n)],
                finals={j: mc.read_final(lp, case["stop"], j, kind[j]) for j in sorted(kind)}, sim=sim, lp=lp)


PIPELINES = ("plain", "notes", "unlogged")


@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("family,seed", FZ.FUZZ_CASES)
def test_device_equals_model(family, seed, pipeline):
    case, m, noted, finals = model(family, seed)
    g = run_device(case, pipeline)
    if pipeline != "notes":
        assert len(g["notes"]) == 0
    equal_fuzz(g, m, "%s seed %d, %s" % (family, seed, pipeline), lambda j: FZ.describe_phy(case, j),
               notes=noted if pipeline == "notes" else None, finals=finals)
    finish(g)
