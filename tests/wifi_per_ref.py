"""An independent high-precision evaluation of the reference's SNR / PER formulas (test infrastructure).

Written from the reference's own source lines, cited at each function below, and from nothing of the device
engine or the C++ oracle:
  src/wifi/model/dsss-error-rate-model.cc:29-127 (ENABLE_GSL unset: the CCK rates use the Matlab fits),
  src/wifi/model/nist-error-rate-model.cc:38-270, src/wifi/model/yans-error-rate-model.cc:45-300,
  src/wifi/model/wifi-phy.cc:99-231 (header mode, preamble and header durations), :355-840 (the mode table),
  src/wifi/model/wifi-mode.cc:137-155 (phyRate), src/wifi/model/interference-helper.cc:192-345.

Precision: the *inputs* of the error-rate models keep the reference's IEEE-double semantics (Python floats):
received powers, m_firstPower and the NiChanges running sums in the reference's order of additions, CalculateSnr,
and nbits = (uint64)(double (phyRate) * Time::GetSeconds (duration)) (nsref.get_seconds: KAT-pinned in
tests/test_oracle_kat.py).  Everything from (snir, nbits, mode) onward runs in mpmath at 60 digits, the branch
decisions (sinr > 10.0, ber == 0, pe < 1) included, and so does the product over a frame's chunks.
"""
import bisect
import contextlib
import math

from mpmath import mp, mpf

import nsref

mp.dps = 60

DSSS, OFDM, ERP_OFDM = 0, 1, 2  # (the project's mode tuples: (modulation class, data rate b/s, bandwidth Hz))
PREAMBLE_LONG, PREAMBLE_SHORT = 0, 1
NIST, YANS = 0, 1

# ---- the mode table: WifiModeFactory::CreateWifiMode calls, wifi-phy.cc:355-840 ----
# name: (class, bandwidth, data rate, code rate as (k, n) or None for WIFI_CODE_RATE_UNDEFINED, constellation)
_OFDM_LADDER = ((6, (1, 2), 2), (9, (3, 4), 2), (12, (1, 2), 4), (18, (3, 4), 4), (24, (1, 2), 16), (36, (3, 4), 16),
                (48, (2, 3), 64), (54, (3, 4), 64))


def _rate_name(bps):
    return (f"{bps / 1e6:g}").replace(".", "_")


WIFI_MODES = {
    "DsssRate1Mbps": (DSSS, 22000000, 1000000, None, 2),  # :360-366
    "DsssRate2Mbps": (DSSS, 22000000, 2000000, None, 4),  # :373-379
    "DsssRate5_5Mbps": (DSSS, 22000000, 5500000, None, 4),  # :391-396
    "DsssRate11Mbps": (DSSS, 22000000, 11000000, None, 4),  # :404-409
}
for _r, _c, _m in _OFDM_LADDER:  # :421-517 ErpOfdmRate*, :529-625 OfdmRate*, :634-730 *BW10MHz, :739-835 *BW5MHz
    WIFI_MODES[f"ErpOfdmRate{_r}Mbps"] = (ERP_OFDM, 20000000, _r * 1000000, _c, _m)
    WIFI_MODES[f"OfdmRate{_r}Mbps"] = (OFDM, 20000000, _r * 1000000, _c, _m)
    WIFI_MODES[f"OfdmRate{_rate_name(_r * 500000)}MbpsBW10MHz"] = (OFDM, 10000000, _r * 500000, _c, _m)
    WIFI_MODES[f"OfdmRate{_rate_name(_r * 250000)}MbpsBW5MHz"] = (OFDM, 5000000, _r * 250000, _c, _m)
_BY_TUPLE = {(v[0], v[2], v[1]): v for v in WIFI_MODES.values()}


def mode_tuple(name):
    mc, bw, rate, _code, _cons = WIFI_MODES[name]
    return (mc, rate, bw)


def _lookup(mode):
    return _BY_TUPLE[(int(mode[0]), int(mode[1]), int(mode[2]))]


def phy_rate(mode):
    """WifiModeFactory::CreateWifiMode, wifi-mode.cc:137-155: dataRate * n / k in uint32 arithmetic."""
    _mc, _bw, rate, code, _cons = _lookup(mode)
    return rate if code is None else rate * code[1] // code[0]


def header_mode(mode, preamble):
    """WifiPhy::GetPlcpHeaderMode, wifi-phy.cc:99-139."""
    mc, bw = int(mode[0]), int(mode[2])
    if mc == OFDM:
        if bw == 5000000:
            return mode_tuple("OfdmRate1_5MbpsBW5MHz")
        if bw == 10000000:
            return mode_tuple("OfdmRate3MbpsBW10MHz")
        return mode_tuple("OfdmRate6Mbps")
    if mc == ERP_OFDM:
        return mode_tuple("ErpOfdmRate6Mbps")
    return mode_tuple("DsssRate1Mbps" if preamble == PREAMBLE_LONG else "DsssRate2Mbps")


def header_us(mode, preamble):
    """WifiPhy::GetPlcpHeaderDurationMicroSeconds, wifi-phy.cc:141-187."""
    mc, bw = int(mode[0]), int(mode[2])
    if mc == OFDM:
        return {10000000: 8, 5000000: 16}.get(bw, 4)
    if mc == ERP_OFDM:
        return 16
    return 24 if preamble == PREAMBLE_SHORT else 48


def preamble_us(mode, preamble):
    """WifiPhy::GetPlcpPreambleDurationMicroSeconds, wifi-phy.cc:189-233."""
    mc, bw = int(mode[0]), int(mode[2])
    if mc == OFDM:
        return {10000000: 32, 5000000: 64}.get(bw, 16)
    if mc == ERP_OFDM:
        return 4
    return 72 if preamble == PREAMBLE_SHORT else 144


def payload_us(size, mode):
    """WifiPhy::GetPayloadDurationMicroSeconds, wifi-phy.cc:235-292 (doubles, as the reference)."""
    mc, rate, bw = int(mode[0]), int(mode[1]), int(mode[2])
    if mc in (OFDM, ERP_OFDM):
        sym = {10000000: 8, 5000000: 16}.get(bw, 4)
        ndbps = rate * sym / 1e6
        nsym = int(math.ceil((16 + size * 8.0 + 6.0) / ndbps))
        return nsym * sym + (6 if mc == ERP_OFDM else 0)
    return int(math.ceil((size * 8.0) / (rate / 1.0e6)))


def tx_duration_ns(size, mode, preamble):
    """WifiPhy::CalculateTxDuration, wifi-phy.cc:294-301."""
    return (preamble_us(mode, preamble) + header_us(mode, preamble) + payload_us(size, mode)) * 1000


# ---- the coefficients, as the reference prints them (each C literal is a double: float () first) ----
COEFF = {
    # dsss-error-rate-model.cc:80-83 (5.5 Mb/s) and :113-118 (11 Mb/s)
    "cck55": [5.3681634344056195e-001, 3.3092430025608586e-003, 4.1654372361004000e-001, 1.0288981434358866e+000],
    "cck11": [7.9056742265333456e-003, -1.8397449399176360e-001, 1.0740689468707241e+000, 1.0523316904502553e+000,
              3.0552298746496687e-001, 2.2032715128698435e+000],
    # nist-error-rate-model.cc:112-120 (b = 1), :127-136 (b = 2), :143-152 (b = 3): (coefficient, power of D)
    "nist_b1": [(36.0, 10), (211.0, 12), (1404.0, 14), (11633.0, 16), (77433.0, 18), (502690.0, 20), (3322763.0, 22),
                (21292910.0, 24), (134365911.0, 26)],
    "nist_b2": [(3.0, 6), (70.0, 7), (285.0, 8), (1276.0, 9), (6160.0, 10), (27128.0, 11), (117019.0, 12),
                (498860.0, 13), (2103891.0, 14), (8784123.0, 15)],
    "nist_b3": [(42.0, 5), (201.0, 6), (1492.0, 7), (10469.0, 8), (62935.0, 9), (379644.0, 10), (2253373.0, 11),
                (13073811.0, 12), (75152755.0, 13), (428005675.0, 14)],
    # yans-error-rate-model.cc:182-279: (constellation, code rate) -> (dFree, adFree, adFreePlusOne)
    "yans": {(2, (1, 2)): (10, 11, None), (2, (3, 4)): (5, 8, None), (4, (1, 2)): (10, 11, 0), (4, (3, 4)): (5, 8, 31),
             (16, (1, 2)): (10, 11, 0), (16, (3, 4)): (5, 8, 31), (64, (2, 3)): (6, 1, 16), (64, (3, 4)): (5, 8, 31)},
}


@contextlib.contextmanager
def perturbed(table, key, value):
    """The reference with one coefficient replaced (the positive control of tests/test_wifi_per_cpu.py)."""
    old = COEFF[table][key]
    COEFF[table][key] = value
    try:
        yield
    finally:
        COEFF[table][key] = old


# ---- DsssErrorRateModel, dsss-error-rate-model.cc:29-127 ----
def _dsss_success(rate, sinr, nbits):
    if rate == 1000000:  # GetDsssDbpskSuccessRate :41-47
        ebn0 = sinr * mpf(22000000.0) / mpf(1000000.0)
        ber = mpf(0.5) * mp.exp(-ebn0)
    elif rate == 2000000:  # GetDsssDqpskSuccessRate :49-55, DqpskFunction :33-39
        x = sinr * mpf(22000000.0) / mpf(1000000.0) / mpf(2.0)
        ber = ((mp.sqrt(2) + 1) / mp.sqrt(8 * mpf(3.1415926) * mp.sqrt(2))) * (1 / mp.sqrt(x)) \
            * mp.exp(-(2 - mp.sqrt(2)) * x)
    elif rate == 5500000:  # GetDsssDqpskCck5_5SuccessRate :57-88; WLAN_SIR_PERFECT 10.0, WLAN_SIR_IMPOSSIBLE 0.1 :29-30
        if sinr > mpf(10.0):
            ber = mpf(0)
        elif sinr < mpf(0.1):
            ber = mpf(0.5)
        else:
            a1, a2, a3, a4 = (mpf(float(a)) for a in COEFF["cck55"])
            ber = a1 * mp.exp(-mp.power((sinr - a2) / a3, a4))
    elif rate == 11000000:  # GetDsssDqpskCck11SuccessRate :90-123
        if sinr > mpf(10.0):
            ber = mpf(0)
        elif sinr < mpf(0.1):
            ber = mpf(0.5)
        else:
            a1, a2, a3, a4, a5, a6 = (mpf(float(a)) for a in COEFF["cck11"])
            ber = (a1 * sinr * sinr + a2 * sinr + a3) / (sinr * sinr * sinr + a4 * sinr * sinr + a5 * sinr + a6)
    else:
        raise ValueError(rate)
    return mp.power(1 - ber, nbits)


# ---- NistErrorRateModel, nist-error-rate-model.cc:38-270 ----
def _nist_pe(p, b):  # CalculatePe :104-160
    d = mp.sqrt(4 * p * (1 - p))
    s = sum(mpf(float(c)) * mp.power(d, e) for c, e in COEFF[f"nist_b{b}"])
    return mpf(0.5) * s if b == 1 else 1 / (mpf(2) * b) * s


def _nist_success(mode, snr, nbits):  # GetChunkSuccessRate :190-270
    mc, _bw, rate, code, cons = _lookup(mode)
    if mc == DSSS:
        return _dsss_success(rate, snr, nbits)
    if cons == 2:  # GetBpskBer :44-51
        ber = mpf(0.5) * mp.erfc(mp.sqrt(snr))
    elif cons == 4:  # GetQpskBer :52-59
        ber = mpf(0.5) * mp.erfc(mp.sqrt(snr / 2))
    elif cons == 16:  # Get16QamBer :60-67
        ber = mpf(0.75) * mpf(0.5) * mp.erfc(mp.sqrt(snr / (mpf(5) * 2)))
    else:  # Get64QamBer :68-75
        ber = mpf(7) / 12 * mpf(0.5) * mp.erfc(mp.sqrt(snr / (mpf(21) * 2)))
    if cons == 64:  # :247-262: rate 2/3 -> b = 2, else 3
        b = 2 if code == (2, 3) else 3
    else:  # :196-246: rate 1/2 -> b = 1, else 3
        b = 1 if code == (1, 2) else 3
    if ber == 0:  # GetFec*Ber :76-103, :162-189
        return mpf(1)
    pe = min(_nist_pe(ber, b), mpf(1))
    return mp.power(1 - pe, nbits)


# ---- YansErrorRateModel, yans-error-rate-model.cc:45-300 ----
def _yans_binomial(k, p, n):  # Binomial :80-85 (the factorials and their quotient are uint32: exact for n <= 12)
    f = math.factorial
    return (f(n) // (f(k) * f(n - k))) * mp.power(p, k) * mp.power(1 - p, n - k)


def _yans_pd(ber, d):  # CalculatePd :117-130, CalculatePdOdd :86-99, CalculatePdEven :100-115
    if d % 2 == 0:
        pd = sum((_yans_binomial(i, ber, d) for i in range(d // 2 + 1, d)), mpf(0))
        return pd + mpf(0.5) * _yans_binomial(d // 2, ber, d)
    return sum((_yans_binomial(i, ber, d) for i in range((d + 1) // 2, d)), mpf(0))


def _yans_success(mode, snr, nbits):  # GetChunkSuccessRate :172-298
    mc, bw, rate, code, cons = _lookup(mode)
    if mc == DSSS:
        return _dsss_success(rate, snr, nbits)
    d_free, ad_free, ad_free1 = COEFF["yans"][(cons, code)]
    ebno = snr * bw / phy_rate(mode)
    if cons == 2:  # GetBpskBer :49-57, GetFecBpskBer :132-147
        ber = mpf(0.5) * mp.erfc(mp.sqrt(ebno))
        if ber == 0:
            return mpf(1)
        pmu = min(ad_free * _yans_pd(ber, d_free), mpf(1))
        return mp.power(1 - pmu, nbits)
    log2m = mp.log(cons) / mp.log(2)  # Log2 :44-48; GetQamBer :58-68
    z = mp.sqrt((mpf(1.5) * log2m * ebno) / (cons - mpf(1)))
    z1 = (1 - 1 / mp.sqrt(cons)) * mp.erfc(z)
    z2 = 1 - mp.power(1 - z1, 2)
    ber = z2 / log2m
    if ber == 0:  # GetFecQamBer :149-170
        return mpf(1)
    pmu = ad_free * _yans_pd(ber, d_free)
    pmu += ad_free1 * _yans_pd(ber, d_free + 1)
    pmu = min(pmu, mpf(1))
    return mp.power(1 - pmu, nbits)


def chunk_success(model, mode, snr, nbits):
    """ErrorRateModel::GetChunkSuccessRate (mode, snr, nbits) of the model, in mpmath; snr is taken exactly."""
    snr = mpf(snr)
    nbits = int(nbits)
    return _yans_success(mode, snr, nbits) if model == YANS else _nist_success(mode, snr, nbits)


# ---- InterferenceHelper, interference-helper.cc:192-345 ----
def calculate_snr(signal, noise_interference, noise_figure, mode):
    """CalculateSnr :215-227, in doubles."""
    nt = 1.3803e-23 * 290.0 * int(mode[2])
    noise_floor = noise_figure * nt
    noise = noise_floor + noise_interference
    return signal / noise


def chunk_nbits(duration_ns, mode):
    """CalculateChunkSuccessRate :254-256: (uint64)(rate * duration.GetSeconds ()), then the (uint32_t) cast."""
    return int(float(phy_rate(mode)) * nsref.get_seconds(duration_ns)) & 0xffffffff


def snr_per(model, noise_figure_db, events, k, synced=None, rxing_at=None):
    """CalculateSnrPer (:347-366) of events[k] at one phy.

    events: [(start_ns, end_ns, rx_w, mode, preamble)] in the order their StartReceivePacket calls are dispatched
    (AppendEvent :192-212 runs for every one of them, whatever the PHY does with the frame).  synced: the indices
    the PHY locked on (m_rxing from NotifyRxStart at their start to NotifyRxEnd at their EndReceive); default (k,).
    rxing_at: m_rxing at each event's AppendEvent, where the caller kept it (a PHY model does); it then replaces what
    is derived from `synced` — and holds where a StartReceive shares a nanosecond with a synced frame's end, which
    the derivation refuses.
    Returns (snr, per, chunks): snr a float, per an mpf, chunks the CalculateChunkSuccessRate calls of CalculatePer
    (:260-345) in order as (is_header, duration_ns, noise_before, nbits); a zero duration is listed with nbits 0.
    """
    synced = (k,) if synced is None else tuple(synced)
    noise_figure = math.pow(10.0, noise_figure_db / 10.0)  # DbToRatio, SetRxNoiseFigure (yans-wifi-phy.cc:192-197)
    first_power, ni_t, ni_d = 0.0, [], []  # m_firstPower, m_niChanges (time, delta)
    k_start, k_end, k_w, k_mode, k_preamble = events[k]

    def add(t, d):  # AddNiChangeEvent :381-385: GetPosition = upper_bound on the time
        i = bisect.bisect_right(ni_t, t)
        ni_t.insert(i, t)
        ni_d.insert(i, d)

    last = None
    for i, (start, end, w, _mode, _preamble) in enumerate(events):
        assert last is None or start >= last, "events are in dispatch order"
        last = start
        if i != k and start >= k_end:
            # (a StartReceive in the EndReceive's nanosecond lands behind the frame's own end entry, upper_bound
            # :378, where CalculateNoiseInterferenceW has already stopped: dispatched before or after, no effect)
            break
        rxing = False if rxing_at is None else bool(rxing_at[i])
        for s in synced if rxing_at is None else ():
            if s < i:
                assert events[s][1] != start, "a StartReceive in a synced frame's last nanosecond"
                rxing = rxing or events[s][0] <= start < events[s][1]
        if not rxing:  # AppendEvent :196-205
            pos = bisect.bisect_right(ni_t, start)
            for j in range(pos):
                first_power += ni_d[j]
            del ni_t[:pos], ni_d[:pos]
            ni_t.insert(0, start)
            ni_d.insert(0, w)
        else:
            add(start, w)
        add(end, -w)
        if i == k:
            assert ni_t[0] == start and ni_d[0] == w

    # CalculateNoiseInterferenceW :229-245
    noise_interference = first_power
    t_list, d_list = [k_start], [noise_interference]
    for t, d in zip(ni_t[1:], ni_d[1:]):
        if k_end == t and k_w == -d:
            break
        t_list.append(t)
        d_list.append(d)
    t_list.append(k_end)
    d_list.append(0.0)
    snr = calculate_snr(k_w, noise_interference, noise_figure, k_mode)

    # CalculatePer :260-345
    payload_mode, hdr_mode = k_mode, header_mode(k_mode, k_preamble)
    header_start = t_list[0] + preamble_us(k_mode, k_preamble) * 1000
    payload_start = header_start + header_us(k_mode, k_preamble) * 1000
    psr = mpf(1)
    chunks = []
    noise_w = d_list[0]

    def chunk(is_header, duration):  # CalculateChunkSuccessRate :247-258
        nonlocal psr
        m = hdr_mode if is_header else payload_mode
        if duration == 0:
            chunks.append((is_header, 0, noise_w, 0))
            return
        nbits = chunk_nbits(duration, m)
        chunks.append((is_header, duration, noise_w, nbits))
        psr *= chunk_success(model, m, calculate_snr(k_w, noise_w, noise_figure, m), nbits)

    previous = t_list[0]
    for current, delta in zip(t_list[1:], d_list[1:]):
        assert current >= previous
        if previous >= payload_start:
            chunk(False, current - previous)
        elif previous >= header_start:
            if current >= payload_start:
                chunk(True, payload_start - previous)
                chunk(False, current - payload_start)
            else:
                chunk(True, current - previous)
        else:
            if current >= payload_start:
                chunk(True, payload_start - header_start)
                chunk(False, current - payload_start)
            elif current >= header_start:
                chunk(True, current - header_start)
        noise_w += delta
        previous = current
    return snr, 1 - psr, chunks


def psr_bound(chunks, psr, k):
    """The conditioning bound on the packet success rate: K 2^-53 sum (nbits psr + 1)
    over the chunks, plus the project's atol 1e-15 on per."""
    return k * 2.0 ** -53 * sum(nbits * float(psr) + 1.0 for _h, _d, _n, nbits in chunks) + 1e-15
