// Stand-alone check of the wide windows' span controller (ns-3-dev-dnemu_amd/csrc/nsgpu_p2p_span.h) against a model
// of the grid scenarios, under the host sanitizers; no device.
//   g++ -std=c++17 -g -fsanitize=address,undefined -Ins-3-dev-dnemu_amd/csrc scripts/span_check.cc -o span_check && ./span_check
//
// The model: lockstep CBR flows down the columns of a rows x flows grid with uncongested 10 Mb/s, 1 ms links and
// 512-B datagrams (542-B frames).  A flow's Send comes every 4096 bit / rate; each Send and each forwarding Receive
// makes a TransmitComplete at +433,600 ns and the next hop's Receive at +1,433,600 ns.  The flows are identical, so
// one flow's (ts, parent ts) list is built and every count is multiplied by the flow count.  A window is
// [tmin, tmin + clamp(span_t, 433,600, 1,433,600)) with tmin the first pending ts; of its records those whose parent's
// ts is below tmin are gen-0 (W), the others local (Lt); N = W + Lt.  A window over a capacity is counted and run as
// it is (the engine would sort it).
//
// Three controllers drive the same list: the committed rule (span_next), the rule it replaced, written out below as
// the reference, and a span pinned at the wide lookahead.  Conditions:
//   - where the lookahead fits (128 x 128 at 500 kb/s, 64 x 64 at 2 Mb/s) the committed rule takes exactly as many
//     windows as the pinned span;
//   - on every shape the committed rule has no more windows over a capacity than the reference rule (which has none);
//   - on the overloaded shapes (2.5 Mb/s and up) the committed rule takes no more windows than the reference rule.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nsgpu_p2p_span.h"

using namespace nsgpu;

namespace {

constexpr uint64_t TX_NS = 433600, HOP_NS = 1433600;  // a 542-B frame at 10 Mb/s; + the 1 ms delay
constexpr uint64_t START_NS = 100000000;
constexpr SpanCaps CAPS{8192, 4096, 4096, 128, 512};  // the engine's NMAX, WCAP, LMAX, LR, LRH (nsgpu_p2p_win.h)

struct Rec {
  uint64_t ts, parent;
};

struct Shape {
  const char *name;
  uint32_t rows, flows;
  uint64_t rate_bps, onoff_stop_ns, stop_ns;
  bool fits;  // the full lookahead fits the capacities
};

// one flow's records up to the Stop, by ts
std::vector<Rec> flow_records(const Shape &s) {
  std::vector<Rec> v;
  const uint64_t gap = 4096ull * 1000000000ull / s.rate_bps;
  uint64_t prev = START_NS;  // (StartApplication schedules the first Send)
  for (uint64_t t = START_NS + gap; t < s.onoff_stop_ns; t += gap) {
    v.push_back({t, prev});  // Send
    prev = t;
    for (uint32_t h = 0; h + 1 < s.rows; h++) {  // hop h: the device's TransmitComplete, the next node's Receive
      const uint64_t at = t + h * HOP_NS;
      v.push_back({at + TX_NS, at});
      v.push_back({at + HOP_NS, at});
    }
  }
  v.erase(std::remove_if(v.begin(), v.end(), [&](const Rec &r) { return r.ts >= s.stop_ns; }), v.end());
  std::stable_sort(v.begin(), v.end(), [](const Rec &a, const Rec &b) { return a.ts < b.ts; });
  return v;
}

// the rule span_next replaced (7/8 and 3/4 of both capacities)
uint64_t reference_next(uint64_t span, uint64_t span_t, uint32_t N, uint32_t W) {
  if (N > 7 * CAPS.nmax / 8 || W > 7 * CAPS.wcap / 8) return span - span / 4;
  if (N < 3 * CAPS.nmax / 4 && W < 3 * CAPS.wcap / 4 && span_t < (1ull << 40)) return span_t + span_t / 8 + 1;
  return span_t;
}

enum Rule { COMMITTED, REFERENCE, PINNED };

struct Result {
  uint64_t windows = 0, over = 0, span_sum = 0;
  uint32_t maxW = 0, maxN = 0, maxLt = 0;
};

Result drive(const std::vector<Rec> &v, uint32_t flows, Rule rule) {
  Result r;
  uint64_t span_t = ~0ull >> 2;  // (the engine starts at its widest)
  size_t i = 0;
  while (i < v.size()) {
    const uint64_t tmin = v[i].ts;
    const uint64_t span = rule == PINNED ? HOP_NS : std::min(std::max(span_t, TX_NS), HOP_NS);
    uint32_t w = 0, l = 0;
    size_t j = i;
    for (; j < v.size() && v[j].ts < tmin + span; j++) (v[j].parent < tmin ? w : l)++;
    const uint32_t W = w * flows, Lt = l * flows, N = W + Lt;
    r.windows++;
    r.span_sum += span;
    r.maxW = std::max(r.maxW, W), r.maxN = std::max(r.maxN, N), r.maxLt = std::max(r.maxLt, Lt);
    if (W > CAPS.wcap || N > CAPS.nmax || Lt > CAPS.lmax) r.over++;
    if (rule == COMMITTED) span_t = span_next(CAPS, span, span_t, SpanLoad{N, W, Lt, 0, 0});
    if (rule == REFERENCE) span_t = reference_next(span, span_t, N, W);
    i = j;
  }
  return r;
}

}  // namespace

int main() {
  const Shape shapes[] = {
      {"128x128 500k", 128, 128, 500000, 2000000000, 2100000000, true},
      {"64x64 2M", 64, 64, 2000000, 300000000, 320000000, true},
      {"64x64 2.5M", 64, 64, 2500000, 300000000, 320000000, false},
      {"64x64 3M", 64, 64, 3000000, 300000000, 320000000, false},
      {"64x64 4M", 64, 64, 4000000, 300000000, 320000000, false},
      {"32x128 4M", 32, 128, 4000000, 250000000, 260000000, false},
  };
  int bad = 0;
  for (const Shape &s : shapes) {
    const std::vector<Rec> v = flow_records(s);
    const Result c = drive(v, s.flows, COMMITTED), p = drive(v, s.flows, REFERENCE), f = drive(v, s.flows, PINNED);
    const Result *rs[3] = {&c, &p, &f};
    const char *names[3] = {"committed", "reference", "pinned"};
    for (int k = 0; k < 3; k++)
      std::printf("%-13s %-9s windows %5llu  mean span %7llu ns  max W %5u N %5u Lt %5u  over capacity %llu\n", s.name,
                  names[k], (unsigned long long)rs[k]->windows, (unsigned long long)(rs[k]->span_sum / rs[k]->windows),
                  rs[k]->maxW, rs[k]->maxN, rs[k]->maxLt, (unsigned long long)rs[k]->over);
    auto fail = [&](const char *what) {
      std::fprintf(stderr, "span_check: %s: %s\n", s.name, what);
      bad = 1;
    };
    if (c.over > p.over) fail("the committed rule has more windows over capacity than the reference rule");
    if (s.fits) {
      if (f.over != 0) fail("the pinned span overflows: the shape does not fit");
      if (c.windows != f.windows) fail("the committed rule does not reach the pinned span's window count");
    } else if (c.windows > p.windows) {
      fail("the committed rule takes more windows than the reference rule");
    }
  }
  if (!bad) std::printf("span_check ok\n");
  return bad;
}
