"""tests/lossx_model.py — wifi_switch_model under an extended loss chain, the reference of tests/test_gpu_lossx.py —
checked on its own: with a chain of the old kinds alone it is the unwrapped model exactly, and every scenario of
tests/lossx_cases.py keeps each reception's power clear of the ED and CCA thresholds (so that the device's discrete
results cannot hang on the last bits of a power), takes the branches it is there for, and shows what it claims."""
import numpy as np
import pytest

import loss_ref as lr
import lossx_cases as lc
import lossx_model
import test_wifi_switch_cpu as sc
import wifi
import wifi_switch_model as wsm


def run_model(c, **kw):
    mob = c["mob"]() if c["mob"] else None
    return lossx_model.run(c["phys"], c["closures"], c["stop"], sc.MODE, sc.PREAMBLE, sc.DBM, mob=mob, lossx=c["lossx"], **kw)


def test_old_kinds_alone_reproduce_the_unwrapped_model():
    c = lc.old_kinds_case()
    plain = wsm.run(c["phys"], c["closures"], c["stop"], sc.MODE, sc.PREAMBLE, sc.DBM, notify=range(16))
    same = lossx_model.run(c["phys"], c["closures"], c["stop"], sc.MODE, sc.PREAMBLE, sc.DBM, notify=range(16))
    wrapped = run_model(c, notify=range(16))
    for m in (same, wrapped):
        assert m.log == plain.log and m.uid == plain.uid and m.probes == plain.probes and m.switches == plain.switches
        assert m.ends == plain.ends and m.notes == plain.notes  # (floats and all: the same doubles)
        assert np.array_equal(m.counters(), plain.counters()) and m.channel_records() == plain.channel_records()
    assert len(plain.ends) > 20 and [w for *_k, w, _t in wrapped.rx_powers] == [w for *_k, w, _t in same.rx_powers]


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_no_reception_sits_on_a_threshold(name):
    m = run_model(lc.CASES[name]())
    closest = lossx_model.clear_of_thresholds(m, 1e-6)
    print(f"{name}: {len(m.rx_powers)} receptions, the closest to a threshold {closest:.3g} away (relative)")
    assert len(m.ends) > 0


def branches(m):
    return {b for *_r, taken in m.rx_powers for b in taken}


def test_hidden_terminal_on_the_model():
    m = run_model(lc.hidden_terminal_case())
    c = m.counters()
    # B locks on A's frame and C's is its interferer; A and C get each other's frame at exactly 0 W — A's reaches C
    # before C sends, C's reaches A while A transmits: dropped under the ED threshold / in TX, as the reference counts
    # a Receive of any power — and neither ever syncs or raises CCA
    assert (c["sync"][lc.B], c["drop_rx"][lc.B], c["rx"][lc.B]) == (1, 1, 2)
    for j in (lc.A, lc.C):
        assert (c["sync"][j], c["cca_switches"][j], c["drop_rx"][j], c["rx"][j]) == (0, 0, 0, 1), j
    assert c["drop_tx"][lc.A] == 1 and c["drop_ed"][lc.C] == 1
    assert {(k, j): w for k, j, w, _t in m.rx_powers}[(0, lc.C)] == 0.0
    states = {p[2]: p[3] for p in m.probes if p[0] == 3_900_000}
    assert states == {lc.A: wifi.IDLE, lc.B: wifi.CCA_BUSY, lc.C: wifi.TX}  # (A is IDLE while C's frame is on the air)
    assert [int(e[2]) for e in m.ends] == [lc.B] and branches(m) == {"matrix_hit", "matrix_default"}


def test_hidden_terminal_mid_run_on_the_model():
    m = run_model(lc.hidden_terminal_case(True))
    pw = {(k, j): w for k, j, w, _t in m.rx_powers}
    assert pw[(0, lc.C)] == 0.0 and pw[(2, lc.C)] == lr.dbm_to_w(sc.DBM - 70.0 + 1.0)     # unheard, then heard
    assert {p[2]: p[3] for p in m.probes if p[0] == 12_500_000} == {lc.B: wifi.RX, lc.C: wifi.RX}
    # the last closure: B's frame under the chain of its own SendPacket (B -> A 60 dB), C's under the new one
    assert pw[(3, lc.A)] == lr.dbm_to_w(sc.DBM - 60.0 + 1.0) and pw[(4, lc.A)] == lr.dbm_to_w(sc.DBM - 80.0 + 1.0)
    assert {p[2]: p[3] for p in m.probes if p[0] == 20_900_000}[lc.A] == wifi.RX


def test_three_log_case_takes_all_four_branches():
    m = run_model(lc.three_log_case())
    assert branches(m) == {"three_0", "three_1", "three_2", "three_3"}
    c = m.counters()
    assert c["sync"].sum() > 10 and c["drop_ed"].sum() > 10 and c["drop_rx"].sum() > 0 and c["cca_switches"].sum() > 10


def test_two_ray_case_crosses_the_crossover_distance_as_the_phy_rises():
    m = run_model(lc.two_ray_case())
    assert branches(m) == {"trg_friis", "trg_two_ray"}
    taken = {(k, j): t for k, j, _w, t in m.rx_powers}
    assert taken[(0, 6)] == ("trg_two_ray",) and taken[(7, 6)] == ("trg_friis",)
    assert (m.txs[0][2], m.txs[7][2]) == (0, 0) and 4.1 < m.z[6] < 5.0
    c = m.counters()
    assert c["sync"].sum() > 10 and c["drop_ed"].sum() > 10


def test_big_matrix_case_rows():
    c = lc.big_matrix_case()
    table = lr.matrix_of(c["lossx"][1])
    rows = {a: sorted(b for (s, b) in table if s == a) for a in (7, 100, 255, 256, 323)}
    assert len(rows[100]) == 65 and rows[7] == [] and {255, 256, 323} <= set(rows[100])
    assert table[(100, 255)] == 71.25 and len(c["lossx"][1]) == len(table) + 1  # (the duplicate: the later value)
    m = run_model(c)
    assert {t[2] for t in m.txs} == {100, 7, 255, 256, 323} and branches(m) == {"matrix_hit", "matrix_default"}
    cn = m.counters()
    assert cn["sync"].sum() > 10 and cn["sync"][[255, 256, 323]].sum() > 0 and cn["rx"].min() >= 4


def test_matrix_switch_and_revert_cases():
    m = run_model(lc.matrix_switch_case())
    pw = {(k, j): w for k, j, w, _t in m.rx_powers}
    table = lr.matrix_of(lc.matrix_switch_case()["lossx"][1])
    assert (0, 2) not in pw and pw[(1, 2)] == lr.dbm_to_w(sc.DBM - table[(0, 2)] + 1.0)  # before / after the switch
    assert pw[(2, 0)] == lr.dbm_to_w(sc.DBM - table[(2, 0)] + 1.0) and pw[(4, 2)] == lr.dbm_to_w(sc.DBM - 130.0 + 1.0)
    assert m.channel_records()[2]["switches"] == 1
    r = run_model(lc.revert_case())
    kinds = [set(t) for *_r, t in r.rx_powers]
    n = 15
    assert all(k <= {"matrix_hit", "matrix_default"} and k for k in kinds[:3 * n])
    assert all(k == set() for k in kinds[3 * n:6 * n])                                     # the config's chain
    assert all(len(t) == 2 for *_r, t in r.rx_powers[6 * n:])                              # Matrix, then TwoRayGround
