// nsgpu_p2p_ports.hip — the p2p subset's extended handler kernels, for scenarios with UDP ports, IPv4 fragmentation
// or receive error models (k2_handle<.., PORTS = true>: the per-flow endpoint lookup, UdpClient, UdpServer; fragments
// sent by the device step, reassembly and its timeout; ReceiveListErrorModel and RateErrorModel; nsgpu_p2p_dev.h "UDP
// ports", "IPv4 fragmentation", "receive error models"), and PacketLossCounter, RngStream and the random variables
// (nsgpu_ranvar.h) on their own.  A scenario with a random OnOff time runs nsgpu_p2p_ranvar.hip's copy of them.
// A translation unit of its own, and so a code object of its own: nsgpu_p2p.hip's holds exactly the kernels it held
// before ports existed, so the engines of scenarios without ports run the same code at the same layout.  The window
// header is compiled here for k2_handle alone (NSGPU_P2P_HANDLERS_ONLY): its other kernels stay nsgpu_p2p.hip's.
#define NSGPU_P2P_HANDLERS_ONLY
#include "nsgpu_p2p_dev.h"
namespace nsgpu {
#include "nsgpu_p2p_win.h"

// (nsgpu_p2p_ranvar.hip: the same handlers with the random OnOff times' draw compiled in)
void launch_handle_ranvar(const P2PDev &M, bool wide, bool xl, bool df, int grid, hipStream_t s, hipEvent_t ev0,
                          hipEvent_t ev1);
void launch_handle_ports(const P2PDev &M, bool wide, bool xl, bool df, int grid, hipStream_t s, hipEvent_t ev0,
                         hipEvent_t ev1) {
  if (M.ranvar) return launch_handle_ranvar(M, wide, xl, df, grid, s, ev0, ev1);
  const dim3 g(grid), b(HB);
  if (df) hipExtLaunchKernelGGL((k2_handle<true, false, true, true>), g, b, 0, s, ev0, ev1, 0, M);
  else if (wide && xl) hipExtLaunchKernelGGL((k2_handle<true, true, false, true>), g, b, 0, s, ev0, ev1, 0, M);
  else if (wide) hipExtLaunchKernelGGL((k2_handle<true, false, false, true>), g, b, 0, s, ev0, ev1, 0, M);
  else hipExtLaunchKernelGGL((k2_handle<false, false, false, true>), g, b, 0, s, ev0, ev1, 0, M);
}

// FlowMonitor::CheckForLostPackets (maxDelay) (flow-monitor.cc:276-300) at `now`, without the erase: lost[f] += the
// entries of flow f still tracked with now - lastSeenTime >= max_delay.  A grid-stride pass over every node's table
// (the tables are contiguous); the tables are only read, so the answer for another delay is another launch.  A
// wave's hits are summed per flow before the atomic: a table's neighbours are one node's datagrams, a few flows.
__global__ __launch_bounds__(TB) void k_flow_sweep(const FmEnt *ents, uint64_t n_entries, int64_t now, int64_t max_delay,
                                                   unsigned long long *lost) {
  const uint64_t stride = (uint64_t)gridDim.x * TB;
  const int lane = threadIdx.x & 63;
  for (uint64_t i0 = (uint64_t)blockIdx.x * TB; i0 < n_entries; i0 += stride) {  // (block-uniform bound)
    const uint64_t i = i0 + threadIdx.x;
    uint32_t flow1 = 0;
    if (i < n_entries) {
      const FmEnt e = ents[i];
      if (e.flow1 != 0 && now - e.last >= max_delay) flow1 = e.flow1;
    }
    uint64_t pend = __ballot(flow1 != 0);
    while (pend) {  // (wave-uniform: one round per distinct flow among the wave's hits)
      const int lead = __ffsll((unsigned long long)pend) - 1;
      const uint32_t f1 = rl32(flow1, lead);
      const bool same = flow1 == f1;
      const uint32_t cnt = wave_sum32(same ? 1u : 0u);
      if (lane == lead) atomicAdd(&lost[f1 - 1], (unsigned long long)cnt);
      pend &= ~__ballot(same);
    }
  }
}
void launch_flow_sweep(const P2PDev &M, int64_t now, int64_t max_delay, uint64_t n_entries, unsigned long long *lost,
                       hipStream_t s) {
  if (!n_entries) return;
  // (the pool sweeps' sizing: GRID_POOL blocks, GRID_POOL_BIG above 2^20 entries)
  const int grid = n_entries > (1ull << 20) ? GRID_POOL_BIG : GRID_POOL;
  hipLaunchKernelGGL(k_flow_sweep, dim3(grid), dim3(TB), 0, s, fm_ents(M.node_ipid, M.n_nodes, 2 * M.n_apps), n_entries,
                     now, max_delay, lost);
}
}  // namespace nsgpu

using namespace nsgpu;

// PacketLossCounter::NotifyReceived over seq[0 .. n): lost[k] = GetLost () after seq[k]; on_device = 0 runs
// nsgpu_loss_counter_notify on the host, 1 in a one-thread kernel (the function the handlers call).
__global__ void k_loss_counter(nsgpu_loss_counter c, const uint32_t *seq, uint64_t n, uint32_t *lost) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (uint64_t k = 0; k < n; k++) {
    nsgpu_loss_counter_notify(&c, seq[k]);
    lost[k] = c.lost;
  }
}
extern "C" int nsgpu_loss_counter_run(uint32_t window, const uint32_t *seq, uint64_t n, uint32_t *lost, int on_device,
                                      void *stream) {
  if (n && (!seq || !lost)) return set_error(NSGPU_EINVAL, "nsgpu_loss_counter_run: null");
  if (window % 8 != 0 || window < 8 || window > NSGPU_LOSS_WINDOW_MAX)
    return set_error(NSGPU_EINVAL, "nsgpu_loss_counter_run: window must be a multiple of 8 in [8, 256]");
  nsgpu_loss_counter c;
  nsgpu_loss_counter_init(&c, window);
  if (!on_device) {
    for (uint64_t k = 0; k < n; k++) {
      nsgpu_loss_counter_notify(&c, seq[k]);
      lost[k] = c.lost;
    }
    return NSGPU_OK;
  }
  if (!n) return NSGPU_OK;
  hipStream_t s = (hipStream_t)stream;
  uint32_t *d = nullptr;
  NSGPU_HIP(hipMalloc((void **)&d, 2 * n * sizeof(uint32_t)));
  hipError_t e = hipMemcpyAsync(d, seq, n * sizeof(uint32_t), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_loss_counter, dim3(1), dim3(64), 0, s, c, d, n, d + n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(lost, d + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  if (e != hipSuccess) return set_error(NSGPU_EHIP, "nsgpu_loss_counter_run: %s", hipGetErrorString(e));
  return NSGPU_OK;
}

// RngStream::U01 of the stream_index-th stream: out[0 .. n).  on_device = 0 runs nsgpu_rng_u01 on the host, 1 in a
// one-thread kernel (the function the handlers call); the initial state is the host's either way (nsgpu_rng_stream_init).
__global__ void k_rng_stream(nsgpu_rng_stream g, uint64_t n, double *out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (uint64_t k = 0; k < n; k++) out[k] = nsgpu_rng_u01(&g);
}
extern "C" int nsgpu_rng_stream_run(uint32_t seed, uint32_t run, uint32_t stream_index, uint64_t n, double *out,
                                    int on_device, void *stream) {
  if (n && !out) return set_error(NSGPU_EINVAL, "nsgpu_rng_stream_run: null");
  nsgpu_rng_stream g;
  if (!nsgpu_rng_stream_init(&g, seed, run, stream_index))
    return set_error(NSGPU_EINVAL, "nsgpu_rng_stream_run: seed %u is not a seed RngStream::CheckSeed accepts (below "
                     "4294944443)", seed);
  if (!on_device) {
    for (uint64_t k = 0; k < n; k++) out[k] = nsgpu_rng_u01(&g);
    return NSGPU_OK;
  }
  if (!n) return NSGPU_OK;
  hipStream_t s = (hipStream_t)stream;
  double *d = nullptr;
  NSGPU_HIP(hipMalloc((void **)&d, n * sizeof(double)));
  hipLaunchKernelGGL(k_rng_stream, dim3(1), dim3(64), 0, s, g, n, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, n * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  if (e != hipSuccess) return set_error(NSGPU_EHIP, "nsgpu_rng_stream_run: %s", hipGetErrorString(e));
  return NSGPU_OK;
}

// RandomVariable::GetValue over n draws of variable v, whose stream is the v->stream-th of a program with RngSeed
// `seed` and RngRun `run`: seconds[i] the value, ns[i] = Seconds (value), ns_other[i] the other candidate's timestamp
// (the last ambiguous attempt's; ns[i] for an unambiguous draw), ambiguous[i] whether any attempt of the draw was
// ambiguous (nsgpu_ranvar.h).  on_device = 0 runs nsgpu_ranvar_value on the host, 1 in a one-thread kernel (the
// function the handlers call).  Any output may be NULL.
struct RvRunOut {
  double *seconds;
  int64_t *ns, *ns_other;
  uint8_t *ambiguous;
};
NSGPU_HD static inline bool rv_run(nsgpu_ranvar v, nsgpu_rng_stream g, uint64_t n, const RvRunOut &o) {
  bool ok = true;
  for (uint64_t i = 0; i < n; i++) {
    double sec;
    bool amb = false;
    int64_t other = 0;
    ok = nsgpu_ranvar_value(v, &g, &sec, [&](uint32_t, int64_t, int64_t ns2) {
           amb = true;
           other = ns2;
         }) && ok;
    const int64_t ts = seconds_to_ts(sec);
    if (o.seconds) o.seconds[i] = sec;
    if (o.ns) o.ns[i] = ts;
    if (o.ns_other) o.ns_other[i] = amb ? other : ts;
    if (o.ambiguous) o.ambiguous[i] = amb ? 1 : 0;
  }
  return ok;
}
__global__ void k_ranvar(nsgpu_ranvar v, nsgpu_rng_stream g, uint64_t n, RvRunOut o, uint32_t *bad) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  *bad = rv_run(v, g, n, o) ? 0u : 1u;
}
extern "C" int nsgpu_ranvar_run(const nsgpu_ranvar *v, uint32_t seed, uint32_t run, uint64_t n, double *seconds,
                                int64_t *ns, int64_t *ns_other, uint8_t *ambiguous, int on_device, void *stream) {
  if (!v) return set_error(NSGPU_EINVAL, "nsgpu_ranvar_run: null");
  if (v->kind > NSGPU_RV_EXPONENTIAL)
    return set_error(NSGPU_EINVAL, "nsgpu_ranvar_run: only Constant, Uniform and Exponential variables are modelled");
  nsgpu_rng_stream g;
  if (!nsgpu_rng_stream_init(&g, seed, run, v->stream))
    return set_error(NSGPU_EINVAL, "nsgpu_ranvar_run: seed %u is not a seed RngStream::CheckSeed accepts (below "
                     "4294944443)", seed);
  const char *const erange = "nsgpu_ranvar_run: a bounded ExponentialVariable was rejected %u times in one GetValue";
  if (!on_device) {
    if (!rv_run(*v, g, n, RvRunOut{seconds, ns, ns_other, ambiguous})) return set_error(NSGPU_ERANGE, erange, NSGPU_RV_MAX_ATTEMPTS);
    return NSGPU_OK;
  }
  if (!n) return NSGPU_OK;
  hipStream_t s = (hipStream_t)stream;
  uint8_t *d = nullptr;  // [n] seconds, [n] ns, [n] ns_other, the flag word, [n] ambiguous
  NSGPU_HIP(hipMalloc((void **)&d, 25 * n + 8));
  const RvRunOut o{reinterpret_cast<double *>(d), reinterpret_cast<int64_t *>(d + 8 * n),
                   reinterpret_cast<int64_t *>(d + 16 * n), d + 24 * n + 8};
  uint32_t *dbad = reinterpret_cast<uint32_t *>(d + 24 * n);
  uint32_t bad = 0;
  hipLaunchKernelGGL(k_ranvar, dim3(1), dim3(64), 0, s, *v, g, n, o, dbad);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && seconds) e = hipMemcpyAsync(seconds, o.seconds, 8 * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && ns) e = hipMemcpyAsync(ns, o.ns, 8 * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && ns_other) e = hipMemcpyAsync(ns_other, o.ns_other, 8 * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && ambiguous) e = hipMemcpyAsync(ambiguous, o.ambiguous, n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  if (e != hipSuccess) return set_error(NSGPU_EHIP, "nsgpu_ranvar_run: %s", hipGetErrorString(e));
  if (bad) return set_error(NSGPU_ERANGE, erange, NSGPU_RV_MAX_ATTEMPTS);
  return NSGPU_OK;
}
// log (u) by nsgpu_rv_log on the host, for the accuracy tests: hi[i] + lo[i] for u[i] in [2^-33, 1).
extern "C" int nsgpu_ranvar_log(const double *u, uint64_t n, double *hi, double *lo) {
  if (n && (!u || !hi || !lo)) return set_error(NSGPU_EINVAL, "nsgpu_ranvar_log: null");
  for (uint64_t i = 0; i < n; i++) {
    if (!(u[i] >= 1.0 / 8589934592.0 && u[i] < 1.0)) return set_error(NSGPU_EINVAL, "nsgpu_ranvar_log: u[%llu] outside [2^-33, 1)", (unsigned long long)i);
    const nsgpu_dd l = nsgpu_rv_log(u[i]);
    hi[i] = l.hi;
    lo[i] = l.lo;
  }
  return NSGPU_OK;
}
// One ExponentialVariable attempt from k by nsgpu_rv_exponential on the host, for the constructed-ambiguity tests:
// r, Seconds (r), Seconds (r'), accepted, ambiguous.
extern "C" int nsgpu_ranvar_exponential(double mean, double bound, uint32_t k, double *r, int64_t *ns, int64_t *ns_other,
                                        int *accept, int *ambiguous) {
  if (!r || !ns || !ns_other || !accept || !ambiguous) return set_error(NSGPU_EINVAL, "nsgpu_ranvar_exponential: null");
  if (k == 0 || k > NSGPU_RNG_M1) return set_error(NSGPU_EINVAL, "nsgpu_ranvar_exponential: k outside [1, 4294967087]");
  const nsgpu_rv_attempt t = nsgpu_rv_exponential(mean, bound, k);
  *r = t.r, *ns = t.ns, *ns_other = t.ns2, *accept = t.accept, *ambiguous = t.ambiguous;
  return NSGPU_OK;
}
