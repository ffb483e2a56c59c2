"""Shared by tests/test_wifi_per_cpu.py (the C++ oracle) and tests/test_gpu_wifi_per.py (the device): the mode
families, the SNR ladders and the CalculatePer scenarios that both compare with tests/wifi_per_ref.py.

Everything here that feeds the reference is computed in doubles the way the reference computes it
(LogDistancePropagationLossModel::DoCalcRxPower, propagation-loss-model.cc:464-492; ConstantSpeedPropagationDelay
Model::GetDelay; YansWifiPhy::StartReceivePacket's rxPowerDbm += m_rxGainDb and DbmToW, yans-wifi-phy.cc:399-410):
neither the oracle's nor the device's numbers are read back into the reference's inputs.
"""
import functools
import math

import numpy as np

import nsref
import wifi
import wifi_per_ref as ref
from wifi_per_ref import mode_tuple

LONG, SHORT = ref.PREAMBLE_LONG, ref.PREAMBLE_SHORT

# ---- the 39 (mode, preamble) pairs, by family: the CreateWifiMode names of wifi-phy.cc:355-840 ----
FAMILIES = {
    "ofdm20": [(n, LONG) for n in ("OfdmRate6Mbps", "OfdmRate9Mbps", "OfdmRate12Mbps", "OfdmRate18Mbps", "OfdmRate24Mbps",
                                   "OfdmRate36Mbps", "OfdmRate48Mbps", "OfdmRate54Mbps")],
    "ofdm10": [(n, LONG) for n in ("OfdmRate3MbpsBW10MHz", "OfdmRate4_5MbpsBW10MHz", "OfdmRate6MbpsBW10MHz",
                                   "OfdmRate9MbpsBW10MHz", "OfdmRate12MbpsBW10MHz", "OfdmRate18MbpsBW10MHz",
                                   "OfdmRate24MbpsBW10MHz", "OfdmRate27MbpsBW10MHz")],
    "ofdm5": [(n, LONG) for n in ("OfdmRate1_5MbpsBW5MHz", "OfdmRate2_25MbpsBW5MHz", "OfdmRate3MbpsBW5MHz",
                                  "OfdmRate4_5MbpsBW5MHz", "OfdmRate6MbpsBW5MHz", "OfdmRate9MbpsBW5MHz",
                                  "OfdmRate12MbpsBW5MHz", "OfdmRate13_5MbpsBW5MHz")],
    "erp": [(n, LONG) for n in ("ErpOfdmRate6Mbps", "ErpOfdmRate9Mbps", "ErpOfdmRate12Mbps", "ErpOfdmRate18Mbps",
                                "ErpOfdmRate24Mbps", "ErpOfdmRate36Mbps", "ErpOfdmRate48Mbps", "ErpOfdmRate54Mbps")],
    "dsss_long": [(n, LONG) for n in ("DsssRate1Mbps", "DsssRate2Mbps", "DsssRate5_5Mbps", "DsssRate11Mbps")],
    "dsss_short": [(n, SHORT) for n in ("DsssRate2Mbps", "DsssRate5_5Mbps", "DsssRate11Mbps")],
}
MODELS = {"nist": ref.NIST, "yans": ref.YANS}
ALL_MODE_NAMES = sorted({n for fam in FAMILIES.values() for n, _p in fam})
NBITS = (1, 24, 96, 1600, 12000)

# ---- the ladder: 48 SNRs per mode, log-spaced in three stretches around the mode's own transition ----
# dB relative to the SNR at which the reference's success rate over 1600 bits is 1/2: a dense middle (0.4 dB apart,
# the whole 1e-6 .. 1 - 1e-6 transition of every mode lies inside it), a low tail down to where every model clamps
# (pe >= 1; sinr < 0.1 for the CCK rates) and a high tail up to where ber underflows to 0 in doubles (erfc (26.6):
# 24.5 dB above the BPSK 1/2 transition) and the CCK fits are cut off (sinr > 10).  The low tail stops at -20.5 dB:
# DqpskFunction (dsss-error-rate-model.cc:33-39) is no probability at low SNR, it passes 2 at 21 dB below the
# 2 Mb/s transition, and from there |1 - ber| ^ nbits grows until it overflows a double.
LADDER_DB = tuple([-20.5, -19.5, -17.0, -13.0, -10.0, -8.0, -6.5, -5.0] + [round(-4.0 + 0.4 * i, 1) for i in range(26)] +
                  [6.5, 7.0, 8.0, 9.0, 10.0, 12.0, 14.0, 16.0, 18.0, 20.0, 22.0, 25.0, 28.0, 32.0])
assert len(LADDER_DB) == 48 and list(LADDER_DB) == sorted(LADDER_DB)


@functools.lru_cache(maxsize=None)
def centre_snr(model, name):
    """The SNR (a double) at which the reference's chunk success over 1600 bits crosses 1/2: bisection on the
    reference alone, 60 halvings of [0.02, 1e5] in the logarithm."""
    mode = mode_tuple(name)
    lo, hi = math.log(0.02), math.log(1e5)
    assert ref.chunk_success(model, mode, math.exp(lo), 1600) < 0.5 < ref.chunk_success(model, mode, math.exp(hi), 1600)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if ref.chunk_success(model, mode, math.exp(mid), 1600) < 0.5:
            lo = mid
        else:
            hi = mid
    return math.exp(0.5 * (lo + hi))


def ladder(model, name):
    c = centre_snr(model, name)
    return [c * 10.0 ** (db / 10.0) for db in LADDER_DB]


# ---- the reference's doubles for one phy's arrivals ----
REF_LOSS_DB, EXPONENT, SPEED, RX_GAIN_DB, NOISE_FIGURE_DB = 46.6777, 3.0, 300000000.0, 1.0, 7.0
TX_DBM = 16.0206 + 1.0  # TxPowerStart + TxGain (YansWifiPhy::SendPacket, yans-wifi-phy.cc:499-522)


def rx_power_w(tx_dbm, distance):
    """LogDistance (exponent 3, 46.6777 dB at 1 m), + RxGain, DbmToW — in doubles, in the reference's order."""
    if distance <= 1.0:
        rx_dbm = tx_dbm
    else:
        path_loss_db = 10 * EXPONENT * math.log10(distance / 1.0)
        rxc = -REF_LOSS_DB - path_loss_db
        rx_dbm = tx_dbm + rxc
    rx_dbm += RX_GAIN_DB
    return math.pow(10.0, rx_dbm / 10.0) / 1000.0


def delay_ns(distance):
    """ConstantSpeedPropagationDelayModel::GetDelay: Seconds (distance / speed) (nsref.seconds: KAT-pinned)."""
    return int(nsref.seconds(distance / SPEED))


def noise_floor_w(bw):
    return math.pow(10.0, NOISE_FIGURE_DB / 10.0) * (1.3803e-23 * 290.0 * bw)


def distance_for_snr(snr, bw, tx_dbm=TX_DBM):
    """The LogDistance distance at which a lone frame sent at tx_dbm arrives with this SNR (a scenario knob only:
    the SNR the tests use is recomputed from the rounded distance by rx_power_w)."""
    rx_dbm = 10.0 * math.log10(snr * noise_floor_w(bw) * 1000.0)
    return 10.0 ** ((tx_dbm + RX_GAIN_DB - REF_LOSS_DB - rx_dbm) / (10 * EXPONENT))


def arrivals(xyz, sends, at, tx_dbm=None):
    """The StartReceivePacket calls at phy `at`, in dispatch order: [(start_ns, end_ns, rx_w, mode, preamble, tx)].
    sends: [(ts, phy, size, mode, preamble)] in Schedule order; a send's Receive events take their uids when the
    send is dispatched, so equal arrival times keep the sends' (ts, Schedule) order.  tx_dbm: per send, or None."""
    order = sorted(range(len(sends)), key=lambda k: (sends[k][0], k))
    out = []
    for tx, k in enumerate(order):
        ts, phy, size, mode, preamble = sends[k]
        if phy == at:
            continue
        d = math.sqrt(sum((a - b) ** 2 for a, b in zip(xyz[phy], xyz[at])))
        start = ts + delay_ns(d)
        dbm = TX_DBM if tx_dbm is None else tx_dbm[k]
        out.append((start, start + ref.tx_duration_ns(size, mode, preamble), rx_power_w(dbm, d), mode, preamble, tx))
    out.sort(key=lambda e: (e[0], e[5]))
    return out


# ---- the CalculatePer scenarios (interference-helper.cc:280-336) ----
V, T = 0, 1  # the victim phy and its transmitter; the interferers follow
VICTIMS = {
    # name: (mode name, preamble, frame size, interferer power at V relative to T's in dB).  T reaches V 1.5 dB above
    # the SNR at which the model's success over 1600 bits is 1/2 (centre_snr), so that a lone frame mostly survives
    # and every interfered chunk costs a success rate well inside (0, 1): errors in any chunk show in the product.
    "dsss1": ("DsssRate1Mbps", LONG, 200, 4.0),  # 144 + 48 us
    "ofdm6bw10": ("OfdmRate6MbpsBW10MHz", LONG, 200, -10.0),  # QPSK 1/2, header OFDM 3 Mb/s BPSK 1/2, 32 + 8 us
}
ROWS = ("1_in_preamble", "2_preamble_to_header", "3_preamble_to_payload", "4_in_header", "5_header_to_payload",
        "6_in_payload_odd_ns", "7_before_the_frame", "8_ends_on_both_boundaries", "9_equal_twins", "10_walk_31",
        "10_walk_32", "10_walk_33", "11_other_mode")
T0 = 1_000_000  # T's SendPacket


def _j_frame(mode, preamble, want_ns):
    """The frame size whose duration comes closest below want_ns (at least 1 byte), and that duration."""
    size = 1
    while ref.tx_duration_ns(size + 1, mode, preamble) <= want_ns:
        size += 1
    return size, ref.tx_duration_ns(size, mode, preamble)


def build_case(row, victim, model):
    """One scenario: dict (xyz, sends [(ts, phy, size, mode, preamble)] in Schedule order, ed / cca thresholds in dBm,
    stop, arrivals: V's StartReceivePacket calls, k: the index of T's frame among them, pre / hdr / pay / end: V's
    preamble start, header start, payload start and end of that frame, mode, preamble: the victim frame's)."""
    name, preamble, size, j_db = VICTIMS[victim]
    mode = mode_tuple(name)
    bw = mode[2]
    t_snr = centre_snr(model, name) * 10.0 ** 0.15
    if row == "7_before_the_frame":
        j_db = min(j_db, -4.0)  # below the ED threshold set between the two: V does not lock on J, which comes first
    if row.startswith("10_walk"):
        # a long payload; two interferers overlap at a time, so T comes 8 dB above the transition and each J no
        # stronger than T, which keeps every chunk's success rate off the pe clamp
        size, t_snr, j_db = 1500, centre_snr(model, name) * 10.0 ** 0.8, min(j_db, 0.0)
    if row == "6_in_payload_odd_ns":
        size = 1500  # (a payload long enough to hold a 1 ms interferer)
    d_t = round(distance_for_snr(t_snr, bw), 3)
    d_j = round(distance_for_snr(t_snr * 10.0 ** (j_db / 10.0), bw), 3)
    xyz = [(0.0, 0.0, 0.0), (d_t, 0.0, 0.0), (-d_j, 0.0, 0.0), (0.0, d_j, 0.0), (0.0, -d_j, 0.0)]
    t_w, j_w = rx_power_w(TX_DBM, d_t), rx_power_w(TX_DBM, d_j)
    # V must lock on T; in row 7 it must not lock on J, which arrives first and is weaker
    ed_w = math.sqrt(t_w * j_w) if row == "7_before_the_frame" else min(t_w, j_w) / 4.0
    ed = 10.0 * math.log10(ed_w * 1000.0)
    pre = T0 + delay_ns(d_t)
    hdr = pre + ref.preamble_us(mode, preamble) * 1000
    pay = hdr + ref.header_us(mode, preamble) * 1000
    end = pre + ref.tx_duration_ns(size, mode, preamble)
    dj = delay_ns(d_j)
    sends = [(T0, T, size, mode, preamble)]
    n_phy = 3

    def j_between(a, b, phy=2, jmode=mode, jpre=preamble, end_exact=False):
        """An interferer frame that reaches V at or just after a and ends at or before b (exactly at b: end_exact)."""
        jsize, dur = _j_frame(jmode, jpre, b - a)
        start = b - dur if end_exact else a
        assert start >= a and start + dur <= b and start - dj > 0
        sends.append((start - dj, phy, jsize, jmode, jpre))

    short = mode_tuple("OfdmRate54Mbps")  # 16 + 4 us + 4 us per 27 bytes: the shortest frames there are
    us = 1000
    if row == "1_in_preamble":
        j_between(pre + 2 * us, hdr - 1 * us, jmode=short)
    elif row == "2_preamble_to_header":
        j_between(hdr - 21 * us, hdr + 3 * us + 7, jmode=short)
    elif row == "3_preamble_to_payload":
        j_between(hdr - 5 * us, pay + 40 * us + 13, jmode=short)
    elif row == "4_in_header":
        if victim == "dsss1":
            j_between(hdr + 10 * us, pay - 10 * us, jmode=short)
        else:
            # No frame is shorter than 24 us, so none lies inside this victim's 8 us header.  The same branch
            # (previous >= plcpHeaderStart, current < plcpPayloadStart) runs on the gap between one interferer that
            # ends 2 us into the header and another that starts 5 us into it.
            j_between(pre + 1 * us, hdr + 2 * us, phy=2, jmode=short, end_exact=True)
            j_between(hdr + 5 * us, pay + 40 * us, phy=3, jmode=short)
            n_phy = 4
    elif row == "5_header_to_payload":
        j_between(pay - 3 * us - 11, pay + 30 * us, jmode=short)
    elif row == "6_in_payload_odd_ns":
        j_between(pay + 100 * us + 3, pay + 100 * us + 3 + 1_000_003)
    elif row == "7_before_the_frame":
        j_between(pre - 20 * us, pay + 50 * us + 1, jmode=short)
    elif row == "8_ends_on_both_boundaries":
        j_between(pre + 1 * us, hdr, phy=2, jmode=short, end_exact=True)
        # (the second J starts in the header where it is long enough to hold the start, else in the preamble)
        j_between(hdr + 5 * us if victim == "dsss1" else pre + 2 * us, pay, phy=3, jmode=short, end_exact=True)
        n_phy = 4
    elif row == "9_equal_twins":
        xyz[2] = (-d_t, 0.0, 0.0)
        sends.append((T0, 2, size, mode, preamble))
    elif row.startswith("10_walk"):
        n = int(row[-2:])
        for i in range(n):  # 36 us frames 25 us (and i ns) apart on three interferers in turn: two overlap
            sends.append((T0 + 400 * us + i * 25 * us + i, 2 + i % 3, 100, short, LONG))
        n_phy = 5
    elif row == "11_other_mode":
        other = short if victim == "dsss1" else mode_tuple("DsssRate11Mbps")
        j_between(hdr - 30 * us if victim == "dsss1" else pre + 5 * us, pay + 200 * us + 1, jmode=other,
                  jpre=LONG if victim == "dsss1" else SHORT)
    else:
        raise KeyError(row)
    sends_sorted = sorted(sends, key=lambda s: s[0])  # Schedule order = time order (ties keep T first)
    xyz = xyz[:n_phy]
    arr = arrivals(xyz, sends_sorted, V)
    k = [i for i, e in enumerate(arr) if sends_sorted[e[5]][1] == T][0]
    return dict(xyz=xyz, sends=sends_sorted, ed=ed, cca=ed - 3.0, stop=end + 2_000_000, k=k, arrivals=arr,
                pre=pre, hdr=hdr, pay=pay, end=end, mode=mode, preamble=preamble)


def case_ids():
    return [(row, victim) for row in ROWS for victim in VICTIMS]


def loop_phys(case, model):
    x, y, z = (np.array([p[i] for p in case["xyz"]]) for i in range(3))
    return wifi.LoopPhys(x, y, z, ed_threshold_dbm=case["ed"], cca_threshold_dbm=case["cca"], error_model=model)


def replay_oracle(case, model):
    s = case["sends"]
    ph = loop_phys(case, model)
    return nsref.wifil_replay(ph.c_struct(), [e[0] for e in s], [e[1] for e in s], [e[2] for e in s], s[0][3], s[0][4],
                              TX_DBM, case["stop"], ph.n_phy, wifi.WIFIL_END_DTYPE, wifi.PHY_COUNTERS_DTYPE,
                              modes=[e[3] for e in s], preambles=[e[4] for e in s])


def reference_for_ends(case, model, ends):
    """For every end record that is not cancelled and whose phy had no cancelled reception: (record index,
    reference snr, reference per, chunks, reference rx_w).  The frames a phy locked on are read from the records'
    exact (phy, tx) fields; the powers and times are the reference's own doubles (arrivals)."""
    cancelled = {int(e["phy"]) for e in ends if int(e["flags"]) & wifi.END_CANCELLED}
    out = []
    for phy in sorted({int(e["phy"]) for e in ends} - cancelled):
        arr = arrivals(case["xyz"], case["sends"], phy)
        by_tx = {e[5]: i for i, e in enumerate(arr)}
        mine = [i for i, e in enumerate(ends) if int(e["phy"]) == phy]
        synced = [by_tx[int(ends[i]["tx"])] for i in mine]
        for i in mine:
            k = by_tx[int(ends[i]["tx"])]
            assert int(ends[i]["ts"]) == arr[k][1]
            snr, per, chunks = ref.snr_per(model, NOISE_FIGURE_DB, [e[:5] for e in arr], k, synced)
            out.append((i, snr, per, chunks, arr[k][2]))
    return out
