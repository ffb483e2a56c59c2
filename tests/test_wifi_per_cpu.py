"""The closed-loop Wi-Fi oracle's SNR / PER (oracle/nsref_wifi.cc) against tests/wifi_per_ref.py, an independent
60-digit evaluation of the reference's own formulas; tests/test_gpu_wifi_per.py holds the device to the same reference.

(a) every mode of wifi-phy.cc's CreateWifiMode calls (the parameter lists below name them as the reference does) under
    both error-rate models, over a 48-point SNR ladder and five chunk lengths; the ladder's coverage of the ber == 0 /
    sinr > 10 returns, of the pe clamp / sinr < 0.1 region and of the transition is asserted on the reference alone;
(b) CalculatePer's interval cases (interference-helper.cc:280-336) on replayed schedules, each with the branch
    signature its row names asserted on the reference's chunk list;
(c) a positive control: the reference with one coefficient nudged differs from itself by more than the tolerance.

Tolerance (SNR / PER pin): |d psr| <= K 2^-53 sum_chunks (nbits_i psr + 1) + 1e-15, and the same bound
on per = 1 - psr.
K is measured here, on the oracle's IEEE-double evaluation with glibc's libm, never on the device:
    measured K_cpu = 29.2 — NIST BPSK 1/2 (ErpOfdmRate6Mbps / OfdmRate6Mbps / ...3MbpsBW10MHz / ...1_5MbpsBW5MHz),
    snr 1.2115, nbits 1: pe = 0.775 is a sum of D^10 .. D^26 with D = sqrt (4 ber (1 - ber)) near 1, so an ulp of ber
    is some 20 ulps of pe.  By chunk length the worst ratios are 29.2 (1 bit), 2.23 (24), 0.93 (96), 0.50 (1600 and
    12000); over (b)'s multi-chunk products the largest is 0.40.
    K_CPU = 30 is asserted below; the device gets 4 K_cpu rounded up to a power of two, K_DEVICE = 128.
    Largest ratio observed on an MI355X (tests/test_gpu_wifi_per.py): 0.50 — DsssRate11Mbps, 1500 B, snr 9.2356,
    per 0.488 (the device's frames hold no 1-bit chunk).
"""
import math

import pytest

import nsref
import wifi
import wifi_per_cases as cases
import wifi_per_ref as ref
from wifi_per_ref import mpf

K_CPU = 30.0
K_DEVICE = 128.0


def test_the_reference_names_the_projects_constants():
    assert (ref.DSSS, ref.OFDM, ref.ERP_OFDM) == (wifi.DSSS, wifi.OFDM, wifi.ERP_OFDM)
    assert (ref.PREAMBLE_LONG, ref.PREAMBLE_SHORT) == (wifi.PREAMBLE_LONG, wifi.PREAMBLE_SHORT)
    assert (ref.NIST, ref.YANS) == (wifi.NIST, wifi.YANS)
    assert len(ref.WIFI_MODES) == 36 and sum(len(f) for f in cases.FAMILIES.values()) == 39
    assert set(cases.ALL_MODE_NAMES) == set(ref.WIFI_MODES)


def test_mode_ladders_durations_against_the_oracle():
    """make_mode / header_mode / preamble_us / header_us of the oracle through its frame duration, for all 39."""
    for fam in cases.FAMILIES.values():
        for name, preamble in fam:
            mode = ref.mode_tuple(name)
            for size in (1, 27, 200, 1500):
                assert nsref.wifi_tx_duration(size, mode[0], mode[1], mode[2], preamble) == \
                    ref.tx_duration_ns(size, mode, preamble), (name, preamble, size)


# ---------------------------------------------------------------- (a) every mode, both models
@pytest.mark.parametrize("model", ["nist", "yans"])
@pytest.mark.parametrize("name", [
    "DsssRate1Mbps", "DsssRate2Mbps", "DsssRate5_5Mbps", "DsssRate11Mbps",
    "ErpOfdmRate6Mbps", "ErpOfdmRate9Mbps", "ErpOfdmRate12Mbps", "ErpOfdmRate18Mbps", "ErpOfdmRate24Mbps",
    "ErpOfdmRate36Mbps", "ErpOfdmRate48Mbps", "ErpOfdmRate54Mbps",
    "OfdmRate6Mbps", "OfdmRate9Mbps", "OfdmRate12Mbps", "OfdmRate18Mbps", "OfdmRate24Mbps", "OfdmRate36Mbps",
    "OfdmRate48Mbps", "OfdmRate54Mbps",
    "OfdmRate3MbpsBW10MHz", "OfdmRate4_5MbpsBW10MHz", "OfdmRate6MbpsBW10MHz", "OfdmRate9MbpsBW10MHz",
    "OfdmRate12MbpsBW10MHz", "OfdmRate18MbpsBW10MHz", "OfdmRate24MbpsBW10MHz", "OfdmRate27MbpsBW10MHz",
    "OfdmRate1_5MbpsBW5MHz", "OfdmRate2_25MbpsBW5MHz", "OfdmRate3MbpsBW5MHz", "OfdmRate4_5MbpsBW5MHz",
    "OfdmRate6MbpsBW5MHz", "OfdmRate9MbpsBW5MHz", "OfdmRate12MbpsBW5MHz", "OfdmRate13_5MbpsBW5MHz"])
def test_chunk_success_every_mode(model, name):
    m = cases.MODELS[model]
    mode = ref.mode_tuple(name)
    lad = cases.ladder(m, name)
    assert len(lad) >= 48
    # the ladder's coverage, on the reference alone
    at1600 = [ref.chunk_success(m, mode, s, 1600) for s in lad]
    assert sum(1 for r in at1600 if r == 1) >= 3, "ber == 0 / sinr > 10"
    assert sum(1 for r in at1600 if r < 1e-12) >= 3, "pe clamp / sinr < 0.1"
    assert sum(1 for r in at1600 if 1e-6 < r < 1 - 1e-6) >= 8, "the transition"
    if name in ("DsssRate5_5Mbps", "DsssRate11Mbps"):
        for cut in (0.1, 10.0):
            assert any(s < cut for s in lad) and any(s > cut for s in lad)
            assert min(abs(s - cut) / cut for s in lad) > 1e-6, "an ulp of pow must not flip the branch"
    worst = (-1.0, None)
    for s in lad:
        for nbits in cases.NBITS:
            want = at1600[lad.index(s)] if nbits == 1600 else ref.chunk_success(m, mode, s, nbits)
            got = nsref.wifil_chunk_success(m, mode, s, nbits)
            ratio = float(abs(mpf(got) - want)) / (2.0 ** -53 * (nbits * float(want) + 1.0))
            worst = max(worst, (ratio, (s, nbits, got, float(want))), key=lambda w: w[0])
    print(f"{model} {name}: worst ratio {worst[0]:.2f} at (snr, nbits, oracle, reference) = {worst[1]}")
    assert worst[0] <= K_CPU, worst


# ---------------------------------------------------------------- (b) CalculatePer's cases
def check_signature(row, victim, c, chunks):
    """The branch signature of the row, on the reference's chunk list (is_header, duration, noise_before, nbits)."""
    arr, k = c["arrivals"], c["k"]
    pre, hdr, pay, end = c["pre"], c["hdr"], c["pay"], c["end"]
    assert arr[k][0] == pre and arr[k][1] == end
    js = [e for i, e in enumerate(arr) if i != k]
    H = [x for x in chunks if x[0]]
    P = [x for x in chunks if not x[0]]
    assert sum(x[1] for x in H) == pay - hdr and sum(x[1] for x in P) == end - pay  # (the preamble is no chunk)
    assert chunks == H + P
    if row == "1_in_preamble":
        (j,) = js
        assert pre < j[0] and j[1] < hdr
        assert [x[:3] for x in chunks] == [(True, pay - hdr, 0.0), (False, end - pay, 0.0)]
    elif row == "2_preamble_to_header":
        (j,) = js
        assert pre < j[0] < hdr < j[1] < pay
        assert [x[:3] for x in chunks] == [(True, j[1] - hdr, j[2]), (True, pay - j[1], 0.0), (False, end - pay, 0.0)]
    elif row == "3_preamble_to_payload":
        (j,) = js
        assert pre < j[0] < hdr and pay < j[1] < end
        assert [x[:3] for x in chunks] == [(True, pay - hdr, j[2]), (False, j[1] - pay, j[2]), (False, end - j[1], 0.0)]
    elif row == "4_in_header":
        # an interval with both ends inside the header: three header chunks, the middle one is that interval
        assert len(H) == 3 and len({x[2] for x in H}) >= 2
        if victim == "dsss1":
            (j,) = js
            assert hdr < j[0] and j[1] < pay
            assert [x[:3] for x in H] == [(True, j[0] - hdr, 0.0), (True, j[1] - j[0], j[2]), (True, pay - j[1], 0.0)]
        else:
            j1, j2 = js
            assert j1[0] < hdr < j1[1] < j2[0] < pay < j2[1]
            assert H[1][:3] == (True, j2[0] - j1[1], 0.0) and H[0][2] == j1[2] and H[2][2] == j2[2]
    elif row == "5_header_to_payload":
        (j,) = js
        assert hdr < j[0] < pay < j[1] < end
        assert [x[:3] for x in chunks] == [(True, j[0] - hdr, 0.0), (True, pay - j[0], j[2]), (False, j[1] - pay, j[2]),
                                           (False, end - j[1], 0.0)]
    elif row == "6_in_payload_odd_ns":
        (j,) = js
        assert pay < j[0] and j[1] < end
        assert [x[:3] for x in chunks] == [(True, pay - hdr, 0.0), (False, j[0] - pay, 0.0), (False, j[1] - j[0], j[2]),
                                           (False, end - j[1], 0.0)]
        rate = ref.phy_rate(c["mode"])
        trunc = [x for x in P if (rate * x[1]) % 10 ** 9 != 0]
        assert len(trunc) >= 2 and all(x[3] == rate * x[1] // 10 ** 9 for x in P), "rate * seconds truncates"
    elif row == "7_before_the_frame":
        (j,) = js
        assert j[0] < pre and pay < j[1] < end and arr.index(j) < k
        assert [x[:3] for x in chunks] == [(True, pay - hdr, j[2]), (False, j[1] - pay, j[2]), (False, end - j[1], 0.0)]
    elif row == "8_ends_on_both_boundaries":
        j1, j2 = js
        assert j1[0] < hdr == j1[1] and j2[1] == pay  # current == plcpHeaderStart, current == plcpPayloadStart
        n1 = 0.0 + j1[2]
        if victim == "dsss1":  # J2 starts inside the header
            assert hdr < j2[0]
            n2 = (n1 - j1[2]) + j2[2]
            assert chunks == [(True, 0, n1, 0), H[1][:2] + (n1 - j1[2], H[1][3]), H[2][:2] + (n2, H[2][3]),
                              (False, 0, n2, 0), P[1][:2] + (n2 - j2[2], P[1][3])]
            assert (H[1][1], H[2][1], P[1][1]) == (j2[0] - hdr, pay - j2[0], end - pay)
        else:  # the 8 us header holds no start: J2 starts in the preamble as well
            assert j1[0] <= j2[0] < hdr
            n12 = n1 + j2[2]
            assert chunks == [(True, 0, n12, 0), H[1][:2] + (n12 - j1[2], H[1][3]), (False, 0, n12 - j1[2], 0),
                              P[1][:2] + ((n12 - j1[2]) - j2[2], P[1][3])]
            assert (H[1][1], P[1][1]) == (pay - hdr, end - pay)
    elif row == "9_equal_twins":
        (j,) = js
        assert j[:3] == arr[k][:3] and k == 0
        assert [x[:3] for x in chunks] == [(True, pay - hdr, arr[k][2]), (False, end - pay, arr[k][2])]
    elif row.startswith("10_walk"):
        n = int(row[-2:])
        assert len(js) == n and all(pay < j[0] and j[1] < end for j in js)
        assert len(P) == 2 * n + 1 and len(H) == 1  # 2 n NiChanges after the start entry, and the end
    elif row == "11_other_mode":
        (j,) = js
        assert j[3] != c["mode"] and j[0] < pay < j[1]
        hm = ref.header_mode(c["mode"], c["preamble"])
        assert hm != ref.header_mode(j[3], j[4])
        assert all(x[3] == ref.chunk_nbits(x[1], hm) for x in H) and H[-1][2] == j[2]
    else:
        raise KeyError(row)


@pytest.mark.parametrize("model", ["nist", "yans"])
@pytest.mark.parametrize("row,victim", cases.case_ids())
def test_calculate_per_cases(row, victim, model):
    m = cases.MODELS[model]
    c = cases.build_case(row, victim, m)
    _log, ends, _phys, tot = cases.replay_oracle(c, m)
    assert tot["sends"] == len(c["sends"])
    refs = cases.reference_for_ends(c, m, ends)
    mine = [r for r in refs if int(ends[r[0]]["phy"]) == cases.V]
    assert len(mine) == 1 and int(ends[mine[0][0]]["tx"]) == c["arrivals"][c["k"]][5], "V locks on T's frame, only"
    check_signature(row, victim, c, mine[0][3])
    psr_v = 1 - mine[0][2]
    # (equal twins: sinr < 1, which the NIST polynomial clamps to pe = 1)
    assert 0 < psr_v < 1 or (row == "9_equal_twins" and psr_v == 0), psr_v
    for i, snr, per, chunks, rx_w in refs:
        e = ends[i]
        assert e["rx_w"] == rx_w and math.isclose(e["snr"], snr, rel_tol=1e-15)
        bound = ref.psr_bound(chunks, 1 - per, K_CPU)
        ratio = float(abs(mpf(float(e["per"])) - per)) / ref.psr_bound(chunks, 1 - per, 1.0)
        print(f"{row} {victim} {model} phy {int(e['phy'])}: per {float(per):.12g}, {len(chunks)} chunks, "
              f"ratio {ratio:.2f}")
        assert abs(mpf(float(e["per"])) - per) <= bound, (int(e["phy"]), float(per), float(e["per"]), chunks)


# ---------------------------------------------------------------- (c) the positive control
@pytest.mark.parametrize("table,key,nudged,model,name", [
    # NIST b == 2 (64-QAM 2/3 only), leading coefficient 3.0 (nist-error-rate-model.cc:127)
    ("nist_b2", 0, (3.1, 6), "nist", "OfdmRate48Mbps"),
    # the 5.5 Mb/s fit's exponent a4 = 1.0288981434358866e+000 (dsss-error-rate-model.cc:83); see the docstring
    ("cck55", 3, 1.0288981434368866e+000, "nist", "DsssRate5_5Mbps"),
    # YANS adFreePlusOne = 16 for 64-QAM 2/3 (yans-error-rate-model.cc:266)
    ("yans", (64, (2, 3)), (6, 1, 17), "yans", "OfdmRate48Mbps"),
])
def test_positive_control_a_nudged_coefficient_is_caught(table, key, nudged, model, name):
    """The copy error these tests exist for: one coefficient off by one in its last printed digit moves the reference
    by more than the widest tolerance in use (K_DEVICE) at some ladder point.

    The exponent a4 is printed to 17 significant digits: its last digit is 1e-16, half an ulp of a4, and no comparison
    of doubles can see it.  What the conditioning bound can resolve follows from ber = a1 exp (-y), y = x^a4:
    d ber = ber y ln (x) d a4, and ber y ln (x) <= 0.086 over 0.1 <= sinr <= 10 (at y = 3), while the bound allows
    K 2^-53 per bit on ber; so a nudge shows once d a4 > 128 * 1.1e-16 / 0.086 = 1.7e-13.  That row therefore nudges the
    smallest decimal place above it, 1e-12: a4 -> 1.0288981434368866; the last-digit nudge of the other two rows
    (3.0 -> 3.1, 16 -> 17) is kept as the issue states it."""
    m = cases.MODELS[model]
    mode = ref.mode_tuple(name)
    lad = cases.ladder(m, name)
    pts = [(s, n) for s in lad for n in cases.NBITS]
    base = [ref.chunk_success(m, mode, s, n) for s, n in pts]
    with ref.perturbed(table, key, nudged):
        pert = [ref.chunk_success(m, mode, s, n) for s, n in pts]
    assert base == [ref.chunk_success(m, mode, s, n) for s, n in pts], "the nudge is undone"
    over = [float(abs(a - b)) / (K_DEVICE * 2.0 ** -53 * (n * float(a) + 1.0) + 1e-15)
            for a, b, (_s, n) in zip(base, pert, pts)]
    print(f"{table}[{key}] -> {nudged}: largest difference is {max(over):.3g} x the K_DEVICE tolerance")
    assert max(over) > 1.0
