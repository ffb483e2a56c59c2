// nsgpu_p2p_ranvar.hip — the extended handler kernels once more, for scenarios with a random OnOff time
// (nsgpu_p2p_scenario_ext.app_on_var / app_off_var): nsgpu_p2p_ports.hip's k2_handle<.., PORTS = true> with
// NSGPU_P2P_RANVAR, which compiles the OnTime / OffTime draw (rv_draw, nsgpu_p2p_dev.h "random OnOff times") into
// schedule_start_event / schedule_stop_event.  A translation unit and so a code object of its own, for the reason
// nsgpu_p2p_ports.hip is one: the draw's registers shape the allocation of every handler that can reach it, so the
// engines of scenarios without a random variable keep the code they had.  The kernels live in namespace nsgpu::rv:
// their template arguments equal the ports unit's, their symbols must not.
#define NSGPU_P2P_HANDLERS_ONLY
#define NSGPU_P2P_RANVAR
#include "nsgpu_p2p_dev.h"
namespace nsgpu {
namespace rv {
#include "nsgpu_p2p_win.h"
}  // namespace rv

void launch_handle_ranvar(const P2PDev &M, bool wide, bool xl, bool df, int grid, hipStream_t s, hipEvent_t ev0,
                          hipEvent_t ev1) {
  const dim3 g(grid), b(HB);
  if (df) hipExtLaunchKernelGGL((rv::k2_handle<true, false, true, true>), g, b, 0, s, ev0, ev1, 0, M);
  else if (wide && xl) hipExtLaunchKernelGGL((rv::k2_handle<true, true, false, true>), g, b, 0, s, ev0, ev1, 0, M);
  else if (wide) hipExtLaunchKernelGGL((rv::k2_handle<true, false, false, true>), g, b, 0, s, ev0, ev1, 0, M);
  else hipExtLaunchKernelGGL((rv::k2_handle<false, false, false, true>), g, b, 0, s, ev0, ev1, 0, M);
}
}  // namespace nsgpu
