"""An independent restatement of the three PropagationLossModels the extended loss chain adds (nsgpu_lossx), the
reference of tests/test_lossx_cpu.py and tests/lossx_model.py.  Written from the reference's lines alone:

  src/propagation/model/propagation-loss-model.cc
    :64-74    PropagationLossModel::CalcRxPower (the chain: each link's DoCalcRxPower feeds the next),
    :197-239  FriisPropagationLossModel::DoCalcRxPower,          :464-491 LogDistancePropagationLossModel,
    :718-723  FixedRssLossModel,                                 :822-834 RangePropagationLossModel,
    :247      TwoRayGroundPropagationLossModel::PI,
    :339-409  TwoRayGroundPropagationLossModel::DoCalcRxPower,
    :548-587  ThreeLogDistancePropagationLossModel::DoCalcRxPower,
    :752-772  MatrixPropagationLossModel::SetLoss,               :781-796 its DoCalcRxPower,
  src/core/model/vector.cc:63-70 (CalculateDistance).

Two evaluations of the same statements:
  * calc (...): Python floats — IEEE doubles, one rounding per operation, math.log10 the host libm's: the statement
    order is the reference's, so the library's host build gives the same bits;
  * calc_mp (...): mpmath at 60 digits, from the same double inputs (the distance too: the double the float path
    computes, so that the branch taken is the same and what is compared is the formula).  It is there when mpmath imports
    (HAVE_MP).

A link is (kind, p0, p1, ...) with the parameters in nsgpu_lossx_kind's order; the Matrix link's entries are a dict
{(a, b): loss_db} built by matrix_of (entries) the way SetLoss builds m_loss.  Each call can report the branch taken."""
import math

try:
    import mpmath
    HAVE_MP = True
except ImportError:  # the float half alone
    mpmath = None
    HAVE_MP = False

LOG_DISTANCE, FRIIS, FIXED_RSS, RANGE, TWO_RAY_GROUND, THREE_LOG, MATRIX = 1, 2, 3, 4, 5, 6, 7
PI = 3.14159265358979323846  # (:116, :247)
MP_DIGITS = 60


def distance(pa, pb):  # CalculateDistance (vector.cc:63-70)
    dx = pb[0] - pa[0]
    dy = pb[1] - pa[1]
    dz = pb[2] - pa[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def matrix_of(entries):
    """m_loss after SetLoss (a, b, loss, false) for each (a, b, loss_db) in order (:752-772): a later one overwrites."""
    m = {}
    for a, b, loss_db in entries:
        m[(int(a), int(b))] = float(loss_db)
    return m


class _Float:
    log10 = staticmethod(math.log10)
    num = staticmethod(float)


class _Mp:
    @staticmethod
    def log10(v):
        return mpmath.log10(v)

    @staticmethod
    def num(v):
        return mpmath.mpf(v)


def _link(A, link, matrix, tx, a, b, pa, pb, d, taken):
    kind, p = link[0], [A.num(v) for v in link[1:]]
    if kind == TWO_RAY_GROUND:  # :339-409
        lam, system_loss, min_distance, height_above_z = p[:4]
        if d <= min_distance:
            taken.append("trg_min")
            return tx
        tx_ant_height = A.num(pa[2]) + height_above_z
        rx_ant_height = A.num(pb[2]) + height_above_z
        # dCross = (4 * PI * txAntHeight * rxAntHeight) / GetLambda (), in doubles in both evaluations: the 60-digit
        # one follows the branch the doubles take (everything else it compares is an exact double already)
        d_cross = (4 * PI * (float(pa[2]) + float(link[4])) * (float(pb[2]) + float(link[4]))) / float(link[1])
        if float(d) <= d_cross:
            taken.append("trg_friis")
            numerator = lam * lam
            tmp = A.num(PI) * d
            denominator = 16 * tmp * tmp * system_loss
            pr = 10 * A.log10(numerator / denominator)
            return tx + pr
        taken.append("trg_two_ray")
        tmp = tx_ant_height * rx_ant_height
        ray_numerator = tmp * tmp
        tmp = d * d
        ray_denominator = tmp * tmp * system_loss
        ray_pr = 10 * A.log10(ray_numerator / ray_denominator)
        return tx + ray_pr
    if kind == THREE_LOG:  # :548-587
        d0, d1, d2, e0, e1, e2, ref_loss = p[:7]
        if d < d0:
            taken.append("three_0")
            loss = A.num(0)
        elif d < d1:
            taken.append("three_1")
            loss = ref_loss + 10 * e0 * A.log10(d / d0)
        elif d < d2:
            taken.append("three_2")
            loss = ref_loss + 10 * e0 * A.log10(d1 / d0) + 10 * e1 * A.log10(d / d1)
        else:
            taken.append("three_3")
            loss = ref_loss + 10 * e0 * A.log10(d1 / d0) + 10 * e1 * A.log10(d2 / d1) + 10 * e2 * A.log10(d / d2)
        return tx - loss
    if kind == MATRIX:  # :781-796
        hit = (int(a), int(b)) in matrix
        taken.append("matrix_hit" if hit else "matrix_default")
        return tx - (A.num(matrix[(int(a), int(b))]) if hit else p[0])
    if kind == LOG_DISTANCE:  # :464-491
        if d <= p[1]:
            return tx
        path_loss_db = 10 * p[0] * A.log10(d / p[1])
        rxc = -p[2] - path_loss_db
        return tx + rxc
    if kind == FRIIS:  # :197-239
        if d <= p[2]:
            return tx
        numerator = p[0] * p[0]
        denominator = 16 * A.num(PI) * A.num(PI) * d * d * p[1]
        return tx + 10 * A.log10(numerator / denominator)
    if kind == FIXED_RSS:  # :718-723
        return p[0]
    if kind == RANGE:  # :822-834
        return tx if d <= p[0] else A.num(-1000.0)
    return tx


def _calc(A, links, matrix, a, b, pa, pb, tx_dbm, taken):
    d = A.num(distance(pa, pb))  # (the double both evaluations branch on)
    self_ = A.num(tx_dbm)
    for link in links:  # CalcRxPower (:64-74)
        self_ = _link(A, link, matrix, self_, a, b, pa, pb, d, taken)
    return self_


def calc(links, matrix, a, b, pa, pb, tx_dbm, taken=None):
    """CalcRxPower (tx_dbm, a, b) in doubles; taken: a list that receives the branch each new-kind link took."""
    return _calc(_Float, links, matrix or {}, a, b, pa, pb, tx_dbm, [] if taken is None else taken)


def calc_mp(links, matrix, a, b, pa, pb, tx_dbm):
    """The same at 60 digits (mpmath.mpf); -inf where a float default (DBL_MAX) swamps everything is still exact."""
    with mpmath.workdps(MP_DIGITS):
        return +_calc(_Mp, links, matrix or {}, a, b, pa, pb, tx_dbm, [])


def dbm_to_w(dbm):  # DbmToW (yans-wifi-phy.cc:727-732)
    return math.pow(10.0, dbm / 10.0) / 1000.0
