// The span controller of the single p2p engine's wide windows (nsgpu_p2p_win.h): from one window's span and load,
// the span target (span_t) of the next.  Plain C++ that compiles for the host and the device, so the rule is stated
// once — df_book and k2_scan's bookkeeping both call it, and they hand over to each other in mid-run — and runs
// under the host sanitizers against a model of the grid scenarios (scripts/span_check.cc).
//
// A window's span is span_t clamped between the narrow and the wide lookahead (window_bound).  The rule keeps a
// window inside the capacities with a hysteresis on each load figure: past its upper mark the next target is the
// span just run less a quarter, and only under every lower mark the target grows by an eighth.  Between the marks
// the target stays.
//
// The marks of the gen-0 records (W) are 15/16 and 13/16 of their capacity: lockstep traffic moves W in steps of
// 64 to 128 records, so 1/16 (256 of 4,096) is the headroom a window needs over the last one, and the band between
// the marks is wider than the eighth a widening adds to a window at the lower mark (13/16 x 9/8 = 0.914 < 15/16).
// With 7/8 and 3/4 (the marks N, and until now W, are held to) config 4's steady window — W ~3,700 to 3,840 at the
// full lookahead of 1.4336 ms — sat above the upper mark: the span was cut to 3/4, widened once or twice and then
// parked in the dead band, ~1.12 ms wide, for the rest of the run.
//
// A local region (one holder or hub block's local records) is the one capacity whose overflow ends the run
// (error 32), so the fullest region is a load figure as well: cut past 3/4 of a region, widen under 5/8 (5/8 x 9/8
// = 0.70 < 3/4).  A holder's 64 slots make one local record each on unsaturated links (64 of 128: under both
// marks); only TransmitComplete chains inside a window fill a region further.
#ifndef NSGPU_P2P_SPAN_H
#define NSGPU_P2P_SPAN_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NSGPU_SPAN_HD __host__ __device__
#else
#define NSGPU_SPAN_HD
#endif

namespace nsgpu {

struct SpanCaps {   // the capacities of one window
  uint32_t nmax;    // records, gen-0 + local
  uint32_t wcap;    // gen-0 records
  uint32_t lmax;    // local records
  uint32_t lr;      // local records of one holder block's region
  uint32_t lrh;     // ... of one hub block's
};

struct SpanLoad {   // what one window held
  uint32_t N, W, Lt;
  uint32_t reg;     // the fullest holder region
  uint32_t hreg;    // the fullest hub region
};

constexpr uint64_t SPAN_T_MAX = 1ull << 40;  // a target at or above it is not widened further

// span: the window's span (ns); span_t: the target it was formed with.  Returns the next window's target.
NSGPU_SPAN_HD inline uint64_t span_next(const SpanCaps &c, uint64_t span, uint64_t span_t, const SpanLoad &l) {
  const bool cut = l.N > c.nmax / 8 * 7 || l.W > c.wcap / 16 * 15 || l.Lt > c.lmax / 8 * 7 || l.reg > c.lr / 4 * 3 ||
                   l.hreg > c.lrh / 4 * 3;
  if (cut) return span - span / 4;
  const bool widen = l.N < c.nmax / 4 * 3 && l.W < c.wcap / 16 * 13 && l.Lt < c.lmax / 4 * 3 && l.reg < c.lr / 8 * 5 &&
                     l.hreg < c.lrh / 8 * 5 && span_t < SPAN_T_MAX;
  return widen ? span_t + span_t / 8 + 1 : span_t;
}

}  // namespace nsgpu
#endif
