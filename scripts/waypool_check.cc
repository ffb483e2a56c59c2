// Stand-alone check of the waypoint pool's host bookkeeping (ns-3-dev-dnemu_amd/csrc/nsgpu_waypool.h) under the host
// sanitizers; no device.  The pool is mirrored by a plain array that is grown and copied exactly as the plans say,
// so an offset or a count that is off reads or writes out of bounds and the sanitizer reports it.
//   g++ -std=c++17 -g -fsanitize=address,undefined -Iinclude -Ins-3-dev-dnemu_amd/csrc scripts/waypool_check.cc -o waypool_check && ./waypool_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "nsgpu_waypool.h"

using namespace nsgpu;

#define CHECK(c) \
  do { \
    if (!(c)) { \
      std::fprintf(stderr, "waypool_check: %s failed at line %d\n", #c, __LINE__); \
      return 1; \
    } \
  } while (0)

int main() {
  WayPool pool;
  std::unique_ptr<nsgpu_waypoint[]> dev;  // (exactly pool.cap entries: the sanitizer guards both ends)
  const int n_phy = 40;
  std::vector<WaySeg> seg(n_phy);
  std::mt19937_64 rng(12345);
  uint64_t grows = 0, moves = 0;
  auto perform = [&](const WayPlan &p, const WaySeg &s, uint64_t old_end) {
    if (p.grow) {
      std::unique_ptr<nsgpu_waypoint[]> np(new nsgpu_waypoint[p.pool_cap]);
      for (uint64_t i = 0; i < old_end; i++) np[i] = dev[i];
      dev = std::move(np);
      grows++;
    }
    if (p.move) {
      for (uint32_t i = 0; i < s.cnt; i++) dev[p.off + i] = dev[p.old_off + i];
      moves++;
    }
  };
  for (int step = 0; step < 20000; step++) {
    const int j = (int)(rng() % n_phy);
    WaySeg &s = seg[j];
    if (rng() % 16 == 0) {  // set_waypoints: a fresh list of n, the first not queued
      const uint64_t n = 1 + rng() % 12;
      s.cnt = 0;
      s.list.clear();
      const uint64_t old_end = pool.end;
      perform(pool.reserve(s, n - 1), s, old_end);
      for (uint64_t i = 0; i < n; i++) {
        const nsgpu_waypoint w{(uint64_t)step * 100 + i, {(double)j, (double)i, 0.0}};
        s.list.push_back(w);
        if (i) dev[s.off + i - 1] = w;
      }
      s.cnt = (uint32_t)(n - 1);
    } else if (!s.list.empty()) {  // add_waypoint
      const nsgpu_waypoint w{s.list.back().time + 1, {(double)j, -1.0, (double)step}};
      const uint64_t old_end = pool.end;
      perform(pool.reserve(s, (uint64_t)s.cnt + 1), s, old_end);
      dev[s.off + s.cnt] = w;
      s.cnt++;
      s.list.push_back(w);
    }
    CHECK(s.off + s.cap <= pool.end && pool.end <= pool.cap && s.cnt <= s.cap);
  }
  for (int j = 0; j < n_phy; j++) {  // every segment holds its list (less the first waypoint), none overlaps another
    const WaySeg &s = seg[j];
    CHECK(s.list.empty() ? s.cnt == 0 : s.cnt + 1 == s.list.size());
    for (uint32_t i = 0; i < s.cnt; i++) {
      const nsgpu_waypoint &a = dev[s.off + i], &b = s.list[i + 1];
      CHECK(a.time == b.time && a.pos[0] == b.pos[0] && a.pos[1] == b.pos[1] && a.pos[2] == b.pos[2]);
    }
    for (int k = 0; k < j; k++)
      CHECK(!seg[k].cap || !s.cap || seg[k].off + seg[k].cap <= s.off || s.off + s.cap <= seg[k].off);
  }
  const nsgpu_waypoint up[3] = {{1, {}}, {2, {}}, {3, {}}}, flat[3] = {{1, {}}, {2, {}}, {2, {}}};
  CHECK(ascending(up, 3) && !ascending(flat, 3) && ascending(up, 1) && ascending(nullptr, 0));
  CHECK(grows > 3 && moves > 20);
  std::printf("waypool_check ok: %llu entries handed out of %llu, %llu pool replacements, %llu segment moves\n",
              (unsigned long long)pool.end, (unsigned long long)pool.cap, (unsigned long long)grows, (unsigned long long)moves);
  return 0;
}
