"""The extended loss chain (nsgpu_lossx: TwoRayGround, ThreeLogDistance and Matrix links, include/nsgpu_types.h) on
the host: nsgpu_lossx_calc — the __host__ __device__ function the closed-loop kernels call, over the table
nsgpu_wifil_set_loss builds — against

  (a) the reference's own test vectors (tests/golden/loss_kat.json), within the reference's own tolerances;
  (b) tests/loss_ref.py's restatement in Python floats, bit for bit: both are IEEE doubles with the reference's
      operation order and the host libm's log10;
  (c) tests/loss_ref.py's 60-digit evaluation of the same statements at the same double inputs, within a first-order
      rounding bound derived here (link_bound).

The bound.  u = 2^-53.  A link is tx +/- sum of terms c_i log10 (q_i) dB.  A quotient q built with n roundings is off
by n u relatively, which moves 10 c log10 (q) by n u |c| 10 / ln 10 dB whatever q is; the host libm's log10 is within
2 ulp (<= 4 u relative) and each further product rounds once (u relative to the term); each sum rounds once (u
relative to the partial sum).  The counts per formula are in link_bound.  Branches depend on the distance alone, which
both evaluations take as the same double, so no error moves a branch.  K = 1 is the bound itself; the largest ratio
|double - 60-digit| / bound measured over the ladders below is 0.404 (TwoRayGround's Friis branch at 147.69 m;
ThreeLogDistance reaches 0.314, the mixed chains 0.27), so the assertion K_LOSS = 1 stands a factor 2.5 over what is
observed.
"""
import ctypes as C
import json
import math
import os
import struct

import pytest

import loss_ref as lr
import nsgpu

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "loss_kat.json")))
EINVAL = 1
DBL_MAX = 1.7976931348623157e308
U = 2.0 ** -53
K_LOSS = 1.0
NEW_SYMBOLS = ("nsgpu_wifil_set_loss", "nsgpu_sim_wifi_set_loss", "nsgpu_lossx_calc")

TRG = (lr.TWO_RAY_GROUND, 0.125, 1.0, 0.5, 1.5)                          # the reference test case's attributes
THREE = (lr.THREE_LOG, 1.0, 200.0, 500.0, 1.9, 3.8, 3.8, 46.6777)        # the model's default attributes (:495-546)
TX_DBM = 10 * math.log10(KAT["two_ray_ground"]["tx_power_w"]) + 30


def calc(links, entries, a, b, pa, pb, tx):
    return nsgpu.lossx_calc(nsgpu.lossx(*links, entries=entries), a, b, pa, pb, tx)


def bits(v):
    return struct.pack("<d", v)


# ---------------------------------------------------------------- the ladders
def around(v):
    return [math.nextafter(v, 0.0), v, math.nextafter(v, math.inf)]


def d_cross(z):  # (4 PI ht hr) / lambda of two antennas at the same z, as the reference's doubles
    h = z + TRG[4]
    return (4 * lr.PI * h * h) / TRG[1]


def trg_points():
    """(pa, pb): same-z pairs along x — the distance is then x itself, sqrt (x * x) — at, just below and just above
    MinDistance and dCross for three heights, a geometric ladder, and mixed-z pairs on both sides of their dCross."""
    pts = []
    for z in (0.0, 1.0, 4.0):
        for x in around(TRG[3]) + around(d_cross(z)) + [0.7 * 1.37 ** k for k in range(30)]:
            pts.append(((0.0, 0.0, z), (x, 0.0, z)))
    for zs, zj in ((0.0, 1.0), (0.0, 4.0), (10.0, 0.0), (2.5, 7.25)):
        dc = (4 * lr.PI * (zs + 1.5) * (zj + 1.5)) / 0.125
        for f in (0.01, 0.5, 0.999, 1.001, 2.0, 10.0):
            pts.append(((3.0, -4.0, zs), (3.0 + f * dc * 0.6, -4.0 + f * dc * 0.8, zj)))
    return pts


def three_points():
    xs = [0.0] + around(THREE[1]) + around(THREE[2]) + around(THREE[3]) + [0.05 * 1.41 ** k for k in range(36)]
    return [((0.0, 0.0, 0.0), (x, 0.0, 0.0)) for x in xs] + [((1.0, 2.0, 3.0), (1.0 + 0.6 * x, 2.0, 3.0 + 0.8 * x)) for x in xs]


def test_ladders_land_on_and_around_every_boundary_and_take_every_branch():
    for z in (0.0, 1.0, 4.0):
        for bound in (TRG[3], d_cross(z)):
            got = [lr.distance((0.0, 0.0, z), (x, 0.0, z)) for x in around(bound)]
            assert got[0] < got[1] == bound < got[2], (z, bound, got)
    for bound in THREE[1:4]:
        got = [lr.distance((0.0, 0.0, 0.0), (x, 0.0, 0.0)) for x in around(bound)]
        assert got[0] < got[1] == bound < got[2]
    taken = []
    for pa, pb in trg_points():
        lr.calc([TRG], None, 0, 1, pa, pb, TX_DBM, taken)
    for pa, pb in three_points():
        lr.calc([THREE], None, 0, 1, pa, pb, TX_DBM, taken)
    lr.calc([(lr.MATRIX, 7.0)], {(0, 1): 3.0}, 0, 1, (0, 0, 0), (1, 0, 0), TX_DBM, taken)
    lr.calc([(lr.MATRIX, 7.0)], {(0, 1): 3.0}, 1, 0, (0, 0, 0), (1, 0, 0), TX_DBM, taken)
    assert set(taken) == {"trg_min", "trg_friis", "trg_two_ray", "three_0", "three_1", "three_2", "three_3", "matrix_hit",
                          "matrix_default"}
    # the boundary points themselves: <= at MinDistance and dCross, strict < at distance0 / 1 / 2
    t = []
    lr.calc([TRG], None, 0, 1, (0, 0, 0.0), (0.5, 0, 0.0), 0.0, t)
    lr.calc([TRG], None, 0, 1, (0, 0, 0.0), (d_cross(0.0), 0, 0.0), 0.0, t)
    lr.calc([TRG], None, 0, 1, (0, 0, 0.0), (math.nextafter(d_cross(0.0), math.inf), 0, 0.0), 0.0, t)
    for i, bnd in enumerate(THREE[1:4]):
        lr.calc([THREE], None, 0, 1, (0, 0, 0), (bnd, 0, 0), 0.0, t)
    assert t == ["trg_min", "trg_friis", "trg_two_ray", "three_1", "three_2", "three_3"]


# ---------------------------------------------------------------- (a) the reference's vectors
def test_two_ray_ground_known_answers():
    k = KAT["two_ray_ground"]
    link = (nsgpu.LOSSX_TWO_RAY_GROUND, k["lambda"], k["system_loss"], k["min_distance"], k["height_above_z"])
    for v in k["vectors"]:
        dbm = calc([link], (), 0, 1, k["sender"], v["position"], TX_DBM)
        w = math.pow(10.0, dbm / 10.0) / 1000
        assert abs(w - v["pr_w"]) <= v["tolerance"], (v, w)
        assert abs(lr.dbm_to_w(lr.calc([link], None, 0, 1, k["sender"], v["position"], TX_DBM)) - v["pr_w"]) <= v["tolerance"]


def test_matrix_known_answers():
    k = KAT["matrix"]
    entries = []
    for s in k["set_loss"]:
        entries.append((s["a"], s["b"], s["loss"]))
        if s["symmetric"]:
            entries.append((s["b"], s["a"], s["loss"]))
    for e in k["expect"]:
        got = calc([(nsgpu.LOSSX_MATRIX, k["default_loss"])], entries, e["a"], e["b"], (0, 0, 0), (0, 0, 0), k["tx_dbm"])
        assert got == e["rx_dbm"], e
        assert lr.calc([(lr.MATRIX, k["default_loss"])], lr.matrix_of(entries), e["a"], e["b"], (0, 0, 0), (0, 0, 0),
                       k["tx_dbm"]) == e["rx_dbm"]


# ---------------------------------------------------------------- (b), (c): the restatement and its 60-digit evaluation
def link_bound(link, tx, res, pa, pb, d):
    """The first-order rounding bound of one link's result `res` from input `tx` (both floats), in dB."""
    kind, p = link[0], link[1:]
    q = 10.0 / math.log(10.0)
    if kind == lr.TWO_RAY_GROUND:
        if d <= p[2]:
            return 0.0
        # Friis: lambda^2 (1), PI d (1), tmp^2 (1), 16 x (exact), x L (1), the quotient (1): 5.  Two-ray: each height
        # (1), their product (1) — 3 — squared: 2 x 3 + 1 = 7; d^2 (1) squared: 2 + 1 = 3; x L (1); the quotient (1): 12
        n_q = 5 if "trg_friis" in branch_of(link, pa, pb) else 12
        pr = abs(res - tx) + U * (abs(res) + abs(tx))
        return U * (n_q * q + 5 * pr + abs(res))  # (log10 4 u + the product by 10 u; the sum u)
    if kind == lr.THREE_LOG:
        d0, d1, d2, e0, e1, e2, ref_loss = p
        terms = []
        if d >= d0:
            terms.append((e0, math.log10((d if d < d1 else d1) / d0)))
        if d >= d1:
            terms.append((e1, math.log10((d if d < d2 else d2) / d1)))
        if d >= d2:
            terms.append((e2, math.log10(d / d2)))
        if not terms:
            return U * abs(res)  # pathLossDb = 0: the subtraction alone
        err, part = 0.0, abs(ref_loss)
        for e, lg in terms:  # the quotient (1); log10 (4 u), 10 e (u), the product (u); the running sum (u)
            t = abs(10 * e * lg)
            part += t
            err += U * (abs(e) * q + 6 * t + part)
        return err + U * abs(res)
    if kind == lr.MATRIX:
        return U * abs(res)
    if kind == lr.LOG_DISTANCE:  # the quotient (1); log10, 10 n, the product; -L0 - pl; the sum
        return 0.0 if d <= p[1] else U * (abs(p[0]) * q + 7 * abs(res - tx) + 2 * abs(res) + abs(tx))
    if kind == lr.FRIIS:  # lambda^2, PI PI, x d, x d, x L, the quotient: 6
        return 0.0 if d <= p[2] else U * (6 * q + 5 * (abs(res - tx) + U * (abs(res) + abs(tx))) + abs(res))
    return 0.0  # FixedRss, Range: constants and the input itself


def branch_of(link, pa, pb):
    t = []
    lr.calc([link], None, 0, 1, pa, pb, 0.0, t)
    return t


def chain_bound(links, matrix, a, b, pa, pb, tx):
    """The bound of the chain's result: a link passes its input's error on one to one (tx +/- ...), FixedRss and a
    Range cut-off replace it."""
    d = lr.distance(pa, pb)
    err, cur = 0.0, tx
    for link in links:
        res = lr.calc([link], matrix, a, b, pa, pb, cur)
        if link[0] == lr.FIXED_RSS or (link[0] == lr.RANGE and d > link[1]):
            err = 0.0
        else:
            err += link_bound(link, cur, res, pa, pb, d)
        cur = res
    return err


CHAINS = {
    "two_ray_ground": ([TRG], trg_points),
    "three_log": ([THREE], three_points),
    "three_log_then_range": ([THREE, (lr.RANGE, 450.0, 0.0, 0.0)], three_points),
    "three_log_then_two_ray": ([THREE, TRG], trg_points),
    "friis_then_three_log": ([(lr.FRIIS, 0.125, 1.0, 0.5), THREE], three_points),
    "log_distance_then_two_ray": ([(lr.LOG_DISTANCE, 3.0, 1.0, 46.6777), TRG], trg_points),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_bit_for_bit_with_the_float_restatement(name):
    links, points = CHAINS[name]
    for tx in (TX_DBM, 0.0, -3.25):
        for pa, pb in points():
            got = calc(links, (), 0, 1, pa, pb, tx)
            want = lr.calc(links, None, 0, 1, pa, pb, tx)
            assert bits(got) == bits(want), (name, tx, pa, pb, got, want, lr.distance(pa, pb))


@pytest.mark.skipif(not lr.HAVE_MP, reason="mpmath is not installed: the 60-digit half is left out")
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_within_the_rounding_bound_of_the_60_digit_evaluation(name):
    links, points = CHAINS[name]
    worst = (0.0, None)
    for pa, pb in points():
        got = calc(links, (), 0, 1, pa, pb, TX_DBM)
        want = lr.calc_mp(links, None, 0, 1, pa, pb, TX_DBM)
        bound = chain_bound(links, None, 0, 1, pa, pb, TX_DBM)
        diff = float(abs(lr.mpmath.mpf(got) - want))
        if bound == 0.0:
            assert diff == 0.0, (name, pa, pb)
            continue
        if diff / bound > worst[0]:
            worst = (diff / bound, (pa, pb))
        assert diff <= K_LOSS * bound, (name, pa, pb, got, diff, bound)
    print(f"{name}: largest |double - 60 digits| / bound = {worst[0]:.3f} at {worst[1]}")
    assert worst[0] > 0.0  # (the ladder exercises the arithmetic)


# ---------------------------------------------------------------- Matrix
M7 = (nsgpu.LOSSX_MATRIX, 7.0)


def test_matrix_hit_miss_asymmetric_duplicate_and_empty():
    e = [(0, 1, 3.0), (1, 0, 5.5), (2, 0, 9.0), (0, 1, 4.0)]  # (0, 1) twice: the later one stays
    assert calc([M7], e, 0, 1, (0, 0, 0), (9, 9, 9), 10.0) == 6.0
    assert calc([M7], e, 1, 0, (0, 0, 0), (9, 9, 9), 10.0) == 4.5
    assert calc([M7], e, 2, 0, (0, 0, 0), (9, 9, 9), 10.0) == 1.0
    assert calc([M7], e, 0, 2, (0, 0, 0), (9, 9, 9), 10.0) == 3.0   # no (0, 2): the default
    assert calc([M7], e, 5, 6, (0, 0, 0), (9, 9, 9), 10.0) == 3.0   # phys the table never names
    assert calc([M7], e[::-1], 0, 1, (0, 0, 0), (9, 9, 9), 10.0) == 7.0  # the order given decides
    assert calc([M7], (), 0, 1, (0, 0, 0), (9, 9, 9), 10.0) == 3.0  # an empty table
    assert calc([(nsgpu.LOSSX_THREE_LOG,) + THREE[1:]], e, 0, 1, (0, 0, 0), (0.5, 0, 0), 10.0) == 10.0  # entries, no Matrix link
    for (a, b), want in (((0, 1), 6.0), ((0, 2), 3.0)):
        assert lr.calc([(lr.MATRIX, 7.0)], lr.matrix_of(e), a, b, (0, 0, 0), (9, 9, 9), 10.0) == want


def test_matrix_default_dbl_max_is_zero_watts():
    """The reference's DefaultLoss is numeric_limits<double>::max (): tx - DBL_MAX, and DbmToW of it is exactly 0 W."""
    link = (nsgpu.LOSSX_MATRIX, DBL_MAX)
    got = calc([link], [(0, 1, 50.0)], 1, 0, (0, 0, 0), (1, 0, 0), 16.0206)
    assert got == 16.0206 - DBL_MAX == -DBL_MAX and math.isfinite(got)
    assert lr.dbm_to_w(got + 1.0) == 0.0  # (+ RxGain, as StartReceivePacket adds it)
    assert calc([link], [(0, 1, 50.0)], 0, 1, (0, 0, 0), (1, 0, 0), 16.0206) == 16.0206 - 50.0
    assert calc([(nsgpu.LOSSX_MATRIX, math.inf)], (), 0, 1, (0, 0, 0), (1, 0, 0), 16.0206) == -math.inf


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_matrix_row_search(n):
    """A sender's row of n entries, between other senders' rows: every column found with its own loss, and columns
    below, between and above the row's missing."""
    cols = [10 + 3 * i for i in range(n)]
    e = [(2, c, 100.0 + c) for c in cols[::-1]]                    # (given in descending order)
    e += [(1, c, 1.0) for c in range(0, 40)] + [(3, c + 1, 2.0) for c in cols] + [(7, 2, 3.0)]
    lx = nsgpu.lossx(M7, entries=e)
    q = lambda a, b: nsgpu.lossx_calc(lx, a, b, (0, 0, 0), (1, 1, 1), 0.0)
    for c in cols:
        assert q(2, c) == -(100.0 + c), c
        assert q(2, c + 1) == -7.0 and q(2, c + 2) == -7.0, c    # between (and above the last)
    for c in (0, 9, cols[-1] + 1000):
        assert q(2, c) == -7.0, c
    assert q(1, 39) == -1.0 and q(1, 40) == -7.0 and q(3, cols[0] + 1) == -2.0 and q(3, cols[0]) == -7.0
    assert q(0, 10) == -7.0 and q(4, 10) == -7.0 and q(7, 2) == -3.0 and q(8, 2) == -7.0  # rows with no entries


def test_chains_mixing_old_and_new_kinds():
    pa, pb, far = (0, 0, 0), (300.0, 0, 0), (600.0, 0, 0)
    three_range = [THREE, (lr.RANGE, 450.0, 0.0, 0.0)]
    assert calc(three_range, (), 0, 1, pa, pb, TX_DBM) == lr.calc([THREE], None, 0, 1, pa, pb, TX_DBM)
    assert calc(three_range, (), 0, 1, pa, far, TX_DBM) == -1000.0
    e = [(0, 1, 20.0)]
    assert calc([M7, (lr.FIXED_RSS, -55.0, 0.0, 0.0)], e, 0, 1, pa, pb, TX_DBM) == -55.0
    m_friis = [M7, (lr.FRIIS, 0.125, 1.0, 0.5)]
    for a, b in ((0, 1), (1, 0)):
        want = lr.calc([(lr.MATRIX, 7.0), (lr.FRIIS, 0.125, 1.0, 0.5)], lr.matrix_of(e), a, b, pa, pb, TX_DBM)
        assert bits(calc(m_friis, e, a, b, pa, pb, TX_DBM)) == bits(want)
    assert calc([], (), 0, 1, pa, pb, TX_DBM) == TX_DBM  # no links: the power itself
    four = [(lr.LOG_DISTANCE, 3.0, 1.0, 46.6777), TRG, THREE, M7]
    assert bits(calc(four, e, 0, 1, pa, pb, TX_DBM)) == bits(lr.calc(four, lr.matrix_of(e), 0, 1, pa, pb, TX_DBM))


# ---------------------------------------------------------------- the interface
def test_refusals_of_the_host_call():
    L = nsgpu.lib()
    out = C.c_double(123.0)
    pa = (C.c_double * 3)(0, 0, 0)

    def rc(lx):
        return L.nsgpu_lossx_calc(C.byref(lx), 0, 1, pa, pa, 0.0, C.byref(out))

    good = nsgpu.lossx(TRG, THREE, M7, entries=[(0, 1, 3.0)])
    assert rc(good) == 0
    for n in (-1, 5):
        lx = nsgpu.lossx(TRG)
        lx.n = n
        assert rc(lx) == EINVAL
    for kind in (8, -1, 1000):
        assert rc(nsgpu.lossx((kind, 1.0, 1.0, 1.0))) == EINVAL and b"unknown kind" in L.nsgpu_last_error()
    assert rc(nsgpu.lossx(M7, TRG, M7)) == EINVAL and b"MATRIX" in L.nsgpu_last_error()
    for bad in (math.nan, math.inf, -math.inf):
        for q in range(4):
            p = list(TRG)
            p[1 + q] = bad
            assert rc(nsgpu.lossx(tuple(p))) == EINVAL and b"not finite" in L.nsgpu_last_error()
        for q in range(7):
            p = list(THREE)
            p[1 + q] = bad
            assert rc(nsgpu.lossx(tuple(p))) == EINVAL
        assert rc(nsgpu.lossx((lr.LOG_DISTANCE, 3.0, bad, 46.0))) == EINVAL
    assert rc(nsgpu.lossx((lr.FIXED_RSS, -50.0, 0.0, 0.0, math.nan))) == 0  # (a parameter the kind does not read)
    assert rc(nsgpu.lossx((nsgpu.LOSSX_MATRIX, DBL_MAX))) == 0 and rc(nsgpu.lossx((nsgpu.LOSSX_MATRIX, math.inf))) == 0
    lx = nsgpu.lossx(M7)
    lx.n_entry = 3  # entries and no array
    assert rc(lx) == EINVAL
    assert out.value in (-7.0, -math.inf)  # (a refused call leaves the result alone: the last good one's)
    assert L.nsgpu_lossx_calc(None, 0, 1, pa, pa, 0.0, C.byref(out)) == EINVAL
    assert L.nsgpu_lossx_calc(C.byref(good), 0, 1, pa, pa, 0.0, None) == EINVAL


def test_struct_sizes_and_exports():
    assert C.sizeof(nsgpu.LossxModel) == 72 and C.sizeof(nsgpu.LossxEntry) == 16
    assert C.sizeof(nsgpu.Lossx) == 8 + 4 * 72 + 16
    assert (nsgpu.LOSSX_TWO_RAY_GROUND, nsgpu.LOSSX_THREE_LOG, nsgpu.LOSSX_MATRIX) == (5, 6, 7)
    assert (lr.TWO_RAY_GROUND, lr.THREE_LOG, lr.MATRIX) == (5, 6, 7)
    L = nsgpu.lib()
    for name in NEW_SYMBOLS:
        assert name in nsgpu.SIGNATURES and hasattr(L, name), name
    hdr = open(os.path.join(HERE, "..", "include", "nsgpu.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in hdr, name
    import wifi
    assert hasattr(wifi.LoopPhy, "set_loss") and hasattr(nsgpu.Sim, "wifi_set_loss")
