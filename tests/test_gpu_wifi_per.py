"""The closed-loop Wi-Fi engine's SNR / PER (csrc/nsgpu_wifil_dev.h: the error-rate models, CalculateSnr, the chunk
walk and product) against tests/wifi_per_ref.py, an independent 60-digit evaluation of the reference's formulas at the
reference's own double-precision inputs (tests/wifi_per_cases.py) — not at anything the device reports.

(a) the SNR ladder: one transmitter, 48 receivers at the distances that give tests/test_wifi_per_cpu.py's ladder, one
    SendPacket per mode of the family at 200 B and at 1500 B, under both error-rate models: all 39 (mode, preamble)
    pairs of wifi-phy.cc's CreateWifiMode table, 48 EndReceives each per frame size;
(b) CalculatePer's interval cases, the scenarios of test_wifi_per_cpu.py sent from host closures: V's record and every
    other comparable phy's against the reference, counters and (ts, uid, phy, tx, flags) against the oracle's replay.

Tolerance: |d per| <= K_DEVICE 2^-53 sum_chunks (nbits_i psr + 1) + 1e-15 with K_DEVICE = 128 = 4 x the K_cpu = 29.2
measured on the CPU oracle (test_wifi_per_cpu.py's docstring), rounded up to a power of two; snr and
the received power within the project's 1e-9 of the reference's doubles.
Largest device ratio observed on an MI355X: 0.50 (ladder: DsssRate11Mbps, 1500 B, snr 9.2356, per 0.488; the OFDM
ladders reach 0.49, the CalculatePer cases 0.40).  The device's frames hold no 1-bit chunk, where K_cpu's 29.2 comes from;
on chunks of 24 bits and more the CPU oracle's own worst ratio is 2.23.
"""
import math

import numpy as np
import pytest

import wifi
import wifi_per_cases as cases
import wifi_per_ref as ref
from test_wifi_per_cpu import K_DEVICE, check_signature
from wifi_per_ref import mpf

pytestmark = pytest.mark.gpu

PHY_COUNTERS = ("rx", "sync", "drop_rx", "drop_tx", "drop_ed", "cca_switches", "end", "end_cancelled")


def run_device(phys, sends, stop_ns, tx_dbm=None, log_cap=1 << 16):
    """sends [(ts, phy, size, mode, preamble)] from host closures scheduled in that order, then Stop."""
    import nsgpu
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(phys)
    sim.attach_wifi(lp)
    sim.set_log(log_cap)
    for k, (ts, phy, size, mode, preamble) in enumerate(sends):
        dbm = cases.TX_DBM if tx_dbm is None else tx_dbm[k]
        sim.schedule(ts, (lambda a=(phy, size, dbm, mode, preamble): lambda: sim.wifi_send(*a))())
    sim.stop(stop_ns)
    sim.run()
    n = min(sim.dispatched(), log_cap)
    out = dict(ends=lp.read_ends(), phys=lp.read_phys(), dispatched=sim.dispatched(), next_uid=sim.next_uid(),
               digest=sim.host_stats()[2], log=tuple(a[:n].copy() for a in sim.log))
    lp.close()
    return out


def compare_record(e, snr, per, chunks, rx_w, what):
    """One end record against the reference; returns the ratio of |d per| to the K = 1 bound."""
    assert math.isclose(e["rx_w"], rx_w, rel_tol=1e-9), (what, e["rx_w"], rx_w)
    assert math.isclose(e["snr"], snr, rel_tol=1e-9), (what, e["snr"], snr)
    diff = abs(mpf(float(e["per"])) - per)
    unit = ref.psr_bound(chunks, 1 - per, 1.0)
    assert diff <= ref.psr_bound(chunks, 1 - per, K_DEVICE), (what, float(e["per"]), float(per), float(diff / unit),
                                                              chunks)
    return float(diff / unit)


# ---------------------------------------------------------------- (a) the SNR ladder
D_NEAR = 2.0  # metres: the receiver of the ladder's top rung (LogDistance is flat inside its 1 m reference distance)


def ladder_distances():
    top = cases.LADDER_DB[-1]
    return [D_NEAR * 10.0 ** ((top - db) / (10 * cases.EXPONENT)) for db in cases.LADDER_DB]


def ladder_tx_dbm(model, name):
    """The transmit power that puts the mode's ladder centre (LADDER_DB = 0) on the receiver placed for it."""
    bw = ref.mode_tuple(name)[2]
    d0 = ladder_distances()[cases.LADDER_DB.index(0.0)]
    rx_dbm = 10.0 * math.log10(cases.centre_snr(model, name) * cases.noise_floor_w(bw) * 1000.0)
    return rx_dbm - cases.RX_GAIN_DB + cases.REF_LOSS_DB + 10 * cases.EXPONENT * math.log10(d0)


@pytest.mark.parametrize("model", ["nist", "yans"])
@pytest.mark.parametrize("family", ["ofdm20", "ofdm10", "ofdm5", "erp", "dsss_long", "dsss_short"])
def test_snr_ladder(family, model):
    m = cases.MODELS[model]
    dist = ladder_distances()
    xyz = [(0.0, 0.0, 0.0)] + [(d, 0.0, 0.0) for d in dist]
    x, y, z = (np.array([p[i] for p in xyz]) for i in range(3))
    phys = wifi.LoopPhys(x, y, z, ed_threshold_dbm=-150.0, cca_threshold_dbm=-153.0, error_model=m)
    sends, dbm, names = [], [], []
    for size in (200, 1500):
        for name, preamble in cases.FAMILIES[family]:
            sends.append((1_000_000 + 20_000_000 * len(sends), 0, size, ref.mode_tuple(name), preamble))
            dbm.append(ladder_tx_dbm(m, name))
            names.append(name)
    assert all(ref.tx_duration_ns(s[2], s[3], s[4]) < 19_000_000 for s in sends)
    got = run_device(phys, sends, sends[-1][0] + 20_000_000, tx_dbm=dbm)
    ends = got["ends"]
    assert len(ends) == 48 * len(sends)
    assert not ends["flags"].any()
    seen, worst = {}, (-1.0, None)
    by_key = {(int(e["phy"]), int(e["tx"])): e for e in ends}
    assert len(by_key) == len(ends)
    for phy in range(1, 49):
        arr = cases.arrivals(xyz, sends, phy, tx_dbm=dbm)
        events = [a[:5] for a in arr]
        for k, a in enumerate(arr):
            e = by_key[(phy, a[5])]
            assert int(e["ts"]) == a[1]
            snr, per, chunks = ref.snr_per(m, cases.NOISE_FIGURE_DB, events, k, synced=range(len(arr)))
            assert [c[0] for c in chunks] == [True, False] and chunks[0][2] == chunks[1][2] == 0.0
            name = names[a[5]]
            if name in ("DsssRate5_5Mbps", "DsssRate11Mbps"):
                # an ulp of the device's pow must not be able to flip a CCK cut-off
                assert min(abs(snr - cut) / cut for cut in (0.1, 10.0)) > 1e-6
            r = compare_record(e, snr, per, chunks, a[2], (name, sends[a[5]][2], phy))
            seen.setdefault((name, sends[a[5]][4]), []).append(float(per))
            worst = max(worst, (r, (name, sends[a[5]][2], snr, float(per))), key=lambda w: w[0])
    print(f"ladder {family} {model}: worst ratio {worst[0]:.2f} at (mode, size, snr, per) = {worst[1]}")
    # every (mode, preamble) of the family was compared, across its whole transition
    assert set(seen) == set(cases.FAMILIES[family])
    for key, pers in seen.items():
        assert len(pers) == 96 and sum(1 for p in pers if 1e-6 < p < 1 - 1e-6) >= 8, key
        assert any(p == 0.0 for p in pers) and any(p > 1 - 1e-12 for p in pers), key


# ---------------------------------------------------------------- (b) CalculatePer's cases
@pytest.mark.parametrize("model", ["nist", "yans"])
@pytest.mark.parametrize("row,victim", cases.case_ids())
def test_calculate_per_cases_on_the_device(row, victim, model):
    m = cases.MODELS[model]
    c = cases.build_case(row, victim, m)
    (lts, luid, lctx), oends, ophys, otot = cases.replay_oracle(c, m)
    got = run_device(cases.loop_phys(c, m), c["sends"], c["stop"])
    gends = got["ends"]
    # the state machine, exactly as the oracle's replay
    assert (got["dispatched"], got["next_uid"], got["digest"]) == (otot["dispatched"], otot["next_uid"], otot["digest"])
    for a, b in zip(got["log"], (lts, luid, lctx)):
        assert np.array_equal(a, b)
    for f in PHY_COUNTERS:
        assert np.array_equal(got["phys"][f], ophys[f]), f
    assert len(gends) == len(oends)
    for f in ("ts", "uid", "phy", "tx", "flags"):
        assert np.array_equal(gends[f], oends[f]), f
    # SNR / PER, against the reference
    refs = cases.reference_for_ends(c, m, gends)
    mine = [r for r in refs if int(gends[r[0]]["phy"]) == cases.V]
    assert len(mine) == 1 and int(gends[mine[0][0]]["tx"]) == c["arrivals"][c["k"]][5]
    check_signature(row, victim, c, mine[0][3])
    worst = -1.0
    for i, snr, per, chunks, rx_w in refs:
        worst = max(worst, compare_record(gends[i], snr, per, chunks, rx_w, (row, victim, model, int(gends[i]["phy"]))))
    print(f"case {row} {victim} {model}: {len(refs)} records, worst ratio {worst:.2f}, V's per {float(mine[0][2]):.9g}")
