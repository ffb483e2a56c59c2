// Host bookkeeping of the closed-loop PHY's waypoint pool (nsgpu_wifil.hip): every phy's waypoint list is one
// segment [off, off + cap) of a single device array of nsgpu_waypoint.  Plain C++ — no device call in here — so it
// builds and runs under the host sanitizers with a stand-alone main (scripts/waypool_check.cc).
//
// A segment that is full moves to the pool's end with twice the room (its old slots are not reused: a path grows a
// few times in a run, and a moved segment's old copy may still be read by kernels in flight).  A pool that cannot
// hold the new segment is replaced by one 1.5 times as large, or as large as the request needs.
#ifndef NSGPU_WAYPOOL_H
#define NSGPU_WAYPOOL_H
#include <algorithm>
#include <cstdint>
#include <vector>

#include "nsgpu_types.h"

namespace nsgpu {

struct WaySeg {
  uint64_t off = 0;
  uint32_t cap = 0, cnt = 0;  // slots owned, slots written (the device's head runs through [0, cnt))
  bool first = true;          // m_first: the next AddWaypoint starts a path and is not queued
  bool any = false;           // a waypoint was added since the install / EndMobility: `last` is its time
  uint64_t last = 0;
  std::vector<nsgpu_waypoint> list;  // every waypoint given since the install, the first one included
};

struct WayPlan {           // what the caller does on the device for `need` slots in a segment
  bool grow = false;       // replace the pool by one of pool_cap entries first (copy [0, old end))
  uint64_t pool_cap = 0;
  bool move = false;       // the segment's written slots go from old_off to off
  uint64_t old_off = 0, off = 0;
};

struct WayPool {
  uint64_t cap = 0, end = 0;  // entries allocated; entries handed out

  // Room for `need` slots in `s` (need >= s.cnt).  Updates s.off / s.cap and this pool's cap / end; the caller
  // performs the plan in that order (grow, then move).
  WayPlan reserve(WaySeg &s, uint64_t need) {
    WayPlan p;
    p.off = p.old_off = s.off;
    if (need <= s.cap) return p;
    const uint64_t ncap = std::max<uint64_t>({need, (uint64_t)s.cap * 2, 4});
    if (end + ncap > cap) {
      p.grow = true;
      p.pool_cap = cap = std::max(cap + cap / 2, end + ncap);
    }
    p.move = s.cnt != 0;
    p.off = s.off = end;
    s.cap = (uint32_t)ncap;
    end += ncap;
    return p;
  }
};

// AddWaypoint's order rule over a list given at once: strictly ascending times.
inline bool ascending(const nsgpu_waypoint *wp, uint64_t n) {
  for (uint64_t i = 1; i < n; i++)
    if (wp[i].time <= wp[i - 1].time) return false;
  return true;
}

}  // namespace nsgpu
#endif
