// nsgpu_ranvar.h — RandomVariable::GetValue (random-variable.cc) for the kinds OnOffApplication's OnTime / OffTime take
// on the device, restated as functions the host and the device share (the style of nsgpu_rng_stream.h): one body, both
// compile it, and with -ffp-contract=off both execute the same IEEE operations.
//
//   ConstantVariable      (:316-320)  m_const; no draw
//   UniformVariable       (:251-258)  m_min + RandU01 () * (m_max - m_min): one U01 a value, product and sum rounded
//                                     separately
//   ExponentialVariable   (:574-589)  r = -m_mean * log (RandU01 ()); with m_bound != 0 redrawn until r <= m_bound:
//                                     one U01 an attempt
//
// The reference's log is the host's libm, which no device function reproduces bit for bit.  nsgpu_rv_log evaluates
// log (u) in double-double with + - * / only (no libm, no fma) and returns hi + lo, hi the nearest double to the
// true logarithm and |hi + lo - log u| < NSGPU_RV_LOG_ERR ulp (hi) (tests/test_ranvar_cpu.py checks it against
// decimal).  A libm whose log errs by less than 1 ulp returns hi or hi's neighbour on the side of the true value
// (the side lo points to), so a draw is evaluated for both: r = -mean * hi, which the device takes, and
// r' = -mean * neighbour.  The draw is AMBIGUOUS when Seconds (r) != Seconds (r'), when r <= bound and r' <= bound
// disagree, or when |lo| is within the log's own error of half an ulp (hi itself is then not certain).  Every other
// draw has the reference's timestamp on any host whose libm stays below 1 ulp.
//
// The log.  u = m 2^e, m in [0.75, 1.5) (u < 1: e <= 0); T = j / 128 the table point nearest m (j = 96 .. 191);
//   log u = e ln 2 + log T + 2 atanh (s),   s = (m - T) / (m + T),   |s| < 1 / 381,
//   atanh s = s (1 + s^2 / 3 + s^4 / 5 + s^6 / 7 + s^8 / 9 + s^10 / 11) + O (s^13): the first omitted term is below
//   2^-106 of the result.
// m - T is exact (Sterbenz), m + T a two-sum, s their double-double quotient; the series' two leading corrections in
// double-double, the rest in double (they are below 2^-51 of s).  For u in [127.5 / 128, 1) the table term and e are
// exactly 0: the result keeps its relative accuracy where log u is tiny.  ln 2, 1/3, 1/5 and the table are
// double-double constants from decimal at 80 digits (scripts/gen_ranvar_log_table.py).  Error: each double-double
// operation errs by at most a few 2^-104 of its result, the sum of three terms cancels by less than a factor 4
// (|log u| >= |log T| / 2 wherever T != 1): below 2^-96 relative, which is 2^-43 ulp (hi) at most.  NSGPU_RV_LOG_ERR
// states 2^-40 ulp (the test measures about 2^-52 over 100,000 arguments; what the scheme needs is 2^-20).
#pragma once
#include "nsgpu_device.h"
#include "nsgpu_ranvar_log_table.h"
#include "nsgpu_rng_stream.h"
#include <string.h>

#define NSGPU_RV_LOG_ERR 9.094947017729282e-13 /* 2^-40: the bound on the error of hi + lo, in ulps of hi */
#define NSGPU_RV_MAX_ATTEMPTS 1024u          /* a bounded Exponential's redraws (create refuses bound < mean / 8) */

struct nsgpu_dd {
  double hi, lo;
};
NSGPU_HD static inline nsgpu_dd nsgpu_dd_quick(double a, double b) {  // |a| >= |b|
  const double s = a + b;
  return nsgpu_dd{s, b - (s - a)};
}
NSGPU_HD static inline nsgpu_dd nsgpu_dd_two_sum(double a, double b) {
  const double s = a + b;
  const double bb = s - a;
  return nsgpu_dd{s, (a - (s - bb)) + (b - bb)};
}
NSGPU_HD static inline nsgpu_dd nsgpu_dd_two_prod(double a, double b) {  // Dekker: no fma
  const double p = a * b;
  const double ta = 134217729.0 * a, tb = 134217729.0 * b;
  const double ah = ta - (ta - a), bh = tb - (tb - b);
  const double al = a - ah, bl = b - bh;
  return nsgpu_dd{p, ((ah * bh - p) + ah * bl + al * bh) + al * bl};
}
NSGPU_HD static inline nsgpu_dd nsgpu_dd_add(nsgpu_dd a, nsgpu_dd b) {
  nsgpu_dd s = nsgpu_dd_two_sum(a.hi, b.hi);
  const nsgpu_dd t = nsgpu_dd_two_sum(a.lo, b.lo);
  s.lo += t.hi;
  s = nsgpu_dd_quick(s.hi, s.lo);
  s.lo += t.lo;
  return nsgpu_dd_quick(s.hi, s.lo);
}
NSGPU_HD static inline nsgpu_dd nsgpu_dd_neg(nsgpu_dd a) { return nsgpu_dd{-a.hi, -a.lo}; }
NSGPU_HD static inline nsgpu_dd nsgpu_dd_mul_d(nsgpu_dd a, double b) {
  nsgpu_dd p = nsgpu_dd_two_prod(a.hi, b);
  p.lo += a.lo * b;
  return nsgpu_dd_quick(p.hi, p.lo);
}
NSGPU_HD static inline nsgpu_dd nsgpu_dd_mul(nsgpu_dd a, nsgpu_dd b) {
  nsgpu_dd p = nsgpu_dd_two_prod(a.hi, b.hi);
  p.lo += a.hi * b.lo + a.lo * b.hi;
  return nsgpu_dd_quick(p.hi, p.lo);
}
NSGPU_HD static inline nsgpu_dd nsgpu_dd_div(nsgpu_dd a, nsgpu_dd b) {  // three quotient digits
  const double q1 = a.hi / b.hi;
  nsgpu_dd r = nsgpu_dd_add(a, nsgpu_dd_neg(nsgpu_dd_mul_d(b, q1)));
  const double q2 = r.hi / b.hi;
  r = nsgpu_dd_add(r, nsgpu_dd_neg(nsgpu_dd_mul_d(b, q2)));
  const double q3 = r.hi / b.hi;
  const nsgpu_dd q = nsgpu_dd_quick(q1, q2);
  return nsgpu_dd_add(q, nsgpu_dd{q3, 0.0});
}

NSGPU_HD static inline nsgpu_dd nsgpu_rv_log_table(int j) {
#define NSGPU_RV_X(h, l) {h, l},
  static constexpr double tab[NSGPU_RV_LOG_J1 - NSGPU_RV_LOG_J0 + 1][2] = {NSGPU_RV_LOG_TABLE(NSGPU_RV_X)};
#undef NSGPU_RV_X
  return nsgpu_dd{tab[j - NSGPU_RV_LOG_J0][0], tab[j - NSGPU_RV_LOG_J0][1]};
}

// log (u) for a double u in [2^-33, 1): hi + lo as described above.
NSGPU_HD static inline nsgpu_dd nsgpu_rv_log(double u) {
  double m = u;
  int e = 0;
  while (m < 0.75 && e > -64) {  // (exact doublings; at most 33 for a U01 value)
    m *= 2.0;
    e--;
  }
  int j = (int)(m * 128.0 + 0.5);
  j = j < NSGPU_RV_LOG_J0 ? NSGPU_RV_LOG_J0 : j > NSGPU_RV_LOG_J1 ? NSGPU_RV_LOG_J1 : j;
  const double T = (double)j / 128.0;
  const nsgpu_dd s = nsgpu_dd_div(nsgpu_dd{m - T, 0.0}, nsgpu_dd_two_sum(m, T));
  const nsgpu_dd s2 = nsgpu_dd_mul(s, s);
  const double q = 1.0 / 7.0 + s2.hi * (1.0 / 9.0 + s2.hi * (1.0 / 11.0));
  nsgpu_dd t = nsgpu_dd_add(nsgpu_dd{NSGPU_RV_FIFTH_HI, NSGPU_RV_FIFTH_LO}, nsgpu_dd_mul_d(s2, q));
  t = nsgpu_dd_add(nsgpu_dd{NSGPU_RV_THIRD_HI, NSGPU_RV_THIRD_LO}, nsgpu_dd_mul(s2, t));
  t = nsgpu_dd_mul(s2, t);
  nsgpu_dd a = nsgpu_dd_add(s, nsgpu_dd_mul(s, t));  // atanh s
  a.hi *= 2.0;
  a.lo *= 2.0;
  const nsgpu_dd c = nsgpu_dd_add(nsgpu_dd_mul_d(nsgpu_dd{NSGPU_RV_LN2_HI, NSGPU_RV_LN2_LO}, (double)e),
                                  nsgpu_rv_log_table(j));
  return nsgpu_dd_add(c, a);
}

NSGPU_HD static inline double nsgpu_rv_from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
NSGPU_HD static inline uint64_t nsgpu_rv_bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}
// ulp of a normal double (the spacing above |x|); the neighbour of a negative x on the side of lo (towards 0: lo > 0).
NSGPU_HD static inline double nsgpu_rv_ulp(double x) {
  return nsgpu_rv_from_bits(((nsgpu_rv_bits(x) >> 52 & 0x7ffull) - 52ull) << 52);
}
NSGPU_HD static inline double nsgpu_rv_neighbour(nsgpu_dd l) {
  if (l.lo == 0.0) return l.hi;
  const uint64_t b = nsgpu_rv_bits(l.hi);  // (log u < 0: the magnitude goes down towards 0, up away from it)
  return nsgpu_rv_from_bits(l.lo > 0.0 ? b - 1 : b + 1);
}

// One attempt of ExponentialVariable::GetValue from the integer k behind u.
struct nsgpu_rv_attempt {
  double r;          // -mean * hi: what the device takes
  int64_t ns, ns2;   // Seconds (r), Seconds (-mean * neighbour)
  bool accept;       // no bound, or r <= bound
  bool ambiguous;
};
NSGPU_HD static inline nsgpu_rv_attempt nsgpu_rv_exponential(double mean, double bound, uint32_t k) {
  const double u = (double)k * (1.0 / 4294967088.0);  // (U01's last step: nsgpu_rng_u01)
  const nsgpu_dd l = nsgpu_rv_log(u);
  const double r = -mean * l.hi, r2 = -mean * nsgpu_rv_neighbour(l);
  nsgpu_rv_attempt o;
  o.r = r;
  o.ns = nsgpu::seconds_to_ts(r);
  o.ns2 = nsgpu::seconds_to_ts(r2);
  o.accept = bound == 0.0 || r <= bound;
  const bool accept2 = bound == 0.0 || r2 <= bound;
  const double alo = l.lo < 0.0 ? -l.lo : l.lo;
  o.ambiguous = o.ns != o.ns2 || o.accept != accept2 || alo >= (0.5 - NSGPU_RV_LOG_ERR) * nsgpu_rv_ulp(l.hi);
  return o;
}

// RandomVariable::GetValue on variable v with its stream g.  `amb (k, ns, ns2)` is called for every ambiguous attempt.
// False: a bounded Exponential was rejected NSGPU_RV_MAX_ATTEMPTS times (the value is then the last attempt's).
template <class Amb>
NSGPU_HD static inline bool nsgpu_ranvar_value(const nsgpu_ranvar &v, nsgpu_rng_stream *g, double *seconds, Amb &&amb) {
  if (v.kind == NSGPU_RV_UNIFORM) {
    *seconds = v.p0 + nsgpu_rng_u01(g) * (v.p1 - v.p0);
    return true;
  }
  if (v.kind != NSGPU_RV_EXPONENTIAL) {
    *seconds = v.p0;
    return true;
  }
  for (uint32_t i = 0; i < NSGPU_RV_MAX_ATTEMPTS; i++) {
    const uint32_t k = nsgpu_rng_next(g);
    const nsgpu_rv_attempt t = nsgpu_rv_exponential(v.p0, v.p1, k);
    if (t.ambiguous) amb(k, t.ns, t.ns2);
    *seconds = t.r;
    if (t.accept) return true;
  }
  return false;
}
