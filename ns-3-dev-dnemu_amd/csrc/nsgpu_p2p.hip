// nsgpu_p2p.hip — the host side of the GPU-resident point-to-point subset (configs 2, 4, 5): scenario planning and
// upload, the run drivers, the C ABI (include/nsgpu.h) and the loopback group.  The device code is included below, in
// one translation unit and in this order: the shared structs and model code (nsgpu_p2p_dev.h), the single-GPU window
// pipeline (nsgpu_p2p_win.h) and the partitioned run's kernels (nsgpu_p2p_dist.h).
#include "nsgpu_p2p_dev.h"
namespace nsgpu {
#include "nsgpu_p2p_win.h"
}  // namespace nsgpu
#include "nsgpu_p2p_dist.h"

#include <vector>
#include <fstream>
#include <algorithm>
#include <string.h>
#include <stdlib.h>
#include <math.h>
#include <rccl/rccl.h>

using namespace nsgpu;

namespace nsgpu {
// k2_handle<WIDE, XL, DF, PORTS = true> (nsgpu_p2p_ports.hip: the ports-mode handlers are a translation unit, and
// so a code object, of their own — this one holds the kernels it held before ports existed, laid out as they were)
void launch_handle_ports(const P2PDev &M, bool wide, bool xl, bool df, int grid, hipStream_t s, hipEvent_t ev0,
                         hipEvent_t ev1);
// k_flow_sweep (the same translation unit: the per-flow statistics are the extended handlers')
void launch_flow_sweep(const P2PDev &M, int64_t now, int64_t max_delay, uint64_t n_entries, unsigned long long *lost,
                       hipStream_t s);
}  // namespace nsgpu
static_assert(sizeof(nsgpu_flow_record) == 184 && offsetof(nsgpu_flow_record, packets_dropped) == 104 &&
              offsetof(nsgpu_flow_record, first_tx_ts) == 168, "nsgpu_flow_record");
static_assert(offsetof(nsgpu_p2p_scenario, flowmon) == offsetof(nsgpu_p2p_scenario, frag) + 4 &&
              offsetof(nsgpu_p2p_scenario, frag_timeout_ns) == offsetof(nsgpu_p2p_scenario, frag) + 8 &&
              sizeof(nsgpu_p2p_scenario) == offsetof(nsgpu_p2p_scenario, rng_run) + 4,
              "flowmon takes the padding word behind frag: no field moves, the struct keeps its size");

// (nsgpu_comm, NCCL_TRY: nsgpu_internal.h)

extern "C" int nsgpu_comm_unique_id(uint8_t *id) {
  if (!id) return set_error(NSGPU_EINVAL, "nsgpu_comm_unique_id: null");
  ncclUniqueId u;
  NCCL_TRY(ncclGetUniqueId(&u));
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return NSGPU_OK;
}

extern "C" int nsgpu_comm_init(const uint8_t *id, int nranks, int rank, nsgpu_comm **out) {
  if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks)
    return set_error(NSGPU_EINVAL, "nsgpu_comm_init: bad arguments");
  ncclUniqueId u;
  memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  nsgpu_comm *c = new nsgpu_comm();
  const ncclResult_t r = ncclCommInitRank(&c->comm, nranks, u, rank);
  if (r != ncclSuccess) {
    delete c;
    return set_error(NSGPU_EHIP, "ncclCommInitRank: %s", ncclGetErrorString(r));
  }
  c->nranks = nranks;
  c->rank = rank;
  *out = c;
  return NSGPU_OK;
}

extern "C" int nsgpu_comm_destroy(nsgpu_comm *c) {
  if (!c) return NSGPU_OK;
  if (c->comm) (void)ncclCommDestroy(c->comm);
  delete c;
  return NSGPU_OK;
}

// NSGPU_P2P_EAGER (set to anything): the replays' kernels launched one by one instead of as graph replays
// (rocprofv3's kernel tracer does not follow graphs).  An engine reads it at create (nsgpu_p2p_set_eager
// overrides it), a loopback group once a process.
static bool env_eager() { return getenv("NSGPU_P2P_EAGER") != nullptr; }

struct nsgpu_p2p {
  P2PDev M;
  nsgpu_p2p_scenario sc;  // (its host pointers are the caller's: not used after nsgpu_p2p_create)
  std::vector<uint32_t> app_kind;
  std::vector<void *> allocs;
  Ctl C0{};               // run control after reset
  uint32_t uid_hint = 4;  // the run control's uid as last seen by the host (the deferred pipeline starts below UID_DF_SOFT)
  uint64_t max_windows = ~0ull;
  hipStream_t s = nullptr;  // engine stream (graph capture and replay)
  hipGraphExec_t gexec = nullptr;
  hipGraphExec_t gexec_df = nullptr;  // the deferred pipeline's replay (single wide engine, untraced)
  hipGraphExec_t gtail[2] = {nullptr, nullptr};  // NWIN_TAIL-window replays (plain, deferred): a run's last windows
  hipEvent_t ev[2] = {nullptr, nullptr}, t0 = nullptr, t1 = nullptr;
  Ctl *snap = nullptr;  // pinned, 2 run-control snapshots
  float last_ms = 0.f;
  bool eager = env_eager();  // kernels one by one instead of graph replays
  // NSGPU_P2P_POISON=1: every device array is filled with 0xa5 bytes when allocated, before create initialises
  // it (a deterministic stand-in for device memory a previous engine dirtied: create must zero what it reads)
  bool poison = [] {
    const char *e = getenv("NSGPU_P2P_POISON");
    return e && e[0] == '1';
  }();
  // pristine initial pool (device) for resets
  uint64_t *init_ts = nullptr;
  uint32_t *init_uid = nullptr, *init_ctx = nullptr, *init_kind = nullptr, *init_a = nullptr;
  const DevRec *dev_init = nullptr;  // device records after reset (tx state idle), and behind them the receive error
  size_t dev_bytes = 0;              // models' reset image (nsgpu_p2p_dev.h "receive error models"); its bytes
  uint32_t em_models = 0;            // enabled receive error models
  // an engine with a random OnOff time: the reset image of app_last_start's allocation (the times, and behind them the
  // variables' records and the empty ambiguous log), its bytes
  const uint64_t *rv_init = nullptr;
  size_t rv_bytes = 0;
  const nsgpu_loss_counter *loss_init = nullptr;  // ports mode: the UdpServers' loss counters after reset
  uint32_t n_apps = 0;
  // an engine with a UdpTraceClient: app_tot holds 3 * n_apps words (m_sent, m_currentEntry, the Send events run)
  bool has_trace_client = false;
  // frag mode: the reset image of what lies behind node_ipid up to the FragNodes (device), its words, the whole
  // allocation's bytes, the FragNodes
  const uint32_t *frag_init = nullptr;
  size_t frag_words = 0, frag_bytes = 0;
  uint32_t frag_nf = 0;
  // a monitored engine (scenario flowmon) keeps its reset image in frag_init / frag_words / frag_bytes too (the two
  // share the place behind node_ipid and exclude each other): the tracked-packet tables' entries, the sweep's counts
  uint64_t fm_entries = 0;
  unsigned long long *fm_lost = nullptr;
  // partitioned run
  nsgpu_comm *comm = nullptr;  // RCCL transport (null: a loopback group member)
  X1Hdr x1h0{};                // empty X1 summary (reset template)
};

namespace {
template <class T>
int dalloc(nsgpu_p2p *h, T **p, size_t n) {
  void *q = nullptr;
  hipError_t e = hipMalloc(&q, (n ? n : 1) * sizeof(T));
  if (e != hipSuccess) return set_error(NSGPU_ENOMEM, "nsgpu_p2p: hipMalloc(%zu): %s", n * sizeof(T),
                                        hipGetErrorString(e));
  h->allocs.push_back(q);
  if (h->poison) NSGPU_HIP(hipMemset(q, 0xa5, (n ? n : 1) * sizeof(T)));
  *p = (T *)q;
  return NSGPU_OK;
}
template <class T>
int dupload(nsgpu_p2p *h, const T **dst, const T *src, size_t n) {
  T *p;
  int rc = dalloc(h, &p, n);
  if (rc) return rc;
  if (n) NSGPU_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  *dst = p;
  return NSGPU_OK;
}
// The device-resident copy of the engine descriptor the handlers' out-of-line code reads (nsgpu_p2p_dev.h "cold
// paths"): written when create has filled h->M, and again by every call that changes a field of it afterwards
// (nsgpu_p2p_set_trace, nsgpu_p2p_set_trace_kinds).  The copy is done when this returns; no run is in flight then.
int mdev_sync(nsgpu_p2p *h) {
  NSGPU_HIP(hipMemcpy(reinterpret_cast<char *>(h->M.C) + CTL_MDEV_OFF, &h->M, sizeof(P2PDev), hipMemcpyHostToDevice));
  return NSGPU_OK;
}
}  // namespace

#define TRY(x)            \
  do {                    \
    int rc_ = (x);        \
    if (rc_) {            \
      nsgpu_p2p_destroy(h); \
      return rc_;         \
    }                     \
  } while (0)

extern "C" int nsgpu_p2p_destroy(nsgpu_p2p *h) {
  if (!h) return NSGPU_OK;
  if (h->s) (void)hipStreamSynchronize(h->s);
  if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
  if (h->gexec_df) (void)hipGraphExecDestroy(h->gexec_df);
  for (hipGraphExec_t g : h->gtail)
    if (g) (void)hipGraphExecDestroy(g);
  for (hipEvent_t e : {h->ev[0], h->ev[1], h->t0, h->t1})
    if (e) (void)hipEventDestroy(e);
  if (h->snap) (void)hipHostFree(h->snap);
  if (h->s) (void)hipStreamDestroy(h->s);
  for (void *p : h->allocs) (void)hipFree(p);
  delete h;
  return NSGPU_OK;
}

// What a rank's engine is built from, computed on the host before any device allocation (create_engine) and
// exposed as nsgpu_p2p_dist_plan: every rank of a partitioned run must get the same lookaheads, window capacities
// and exchange sizes — a mismatch would be a collective of different sizes (an RCCL hang), which the multi-process
// CPU tests check (tests/test_dist_cpu.py).
struct EnginePlan {
  uint32_t qcap = 1, maxapps = 0, maxc = 3, wide = 0;
  bool has_echo = false;
  std::vector<uint32_t> napps, node_list;
  std::vector<int32_t> sink;
  bool ports = false;               // ports mode (nsgpu_p2p_scenario.app_port given)
  std::vector<int32_t> ep_of_flow;  // ports mode: the application a sender's datagrams are delivered to (-1: none)
  // UdpTraceClients (nsgpu_p2p_scenario_ext): what lies behind app_pkt_size on the device — n_apps + 1 offsets, the
  // entries as (timeToSend ms, packetSize) pairs (nsgpu_p2p_dev.h "UdpTraceClient") — and per application the walk of
  // its cycle (plan_trace_client): the datagrams it sends before the run can end, for flowmon's table bound
  bool has_trace_client = false;
  std::vector<uint32_t> tc_img;
  std::vector<uint64_t> tc_bound;
  int64_t tx_min = 0, lx = 0, send_ivl = 0;
  int64_t lookahead[K_NKINDS], lookw[K_NKINDS];
  bool frag = false;                 // frag mode (nsgpu_p2p_scenario.frag)
  std::vector<uint32_t> frag_flows;  // frag mode: the fragmenting flows that deliver fragments to each node
  int64_t frag_timeout = 0;          // FragmentExpirationTimeout
  // receive error models: each device's enabled model + 1 (0: none), the models' reset records, the EU_BYTE / EU_BIT
  // threshold tables and the ReceiveList models' sorted lists
  std::vector<uint32_t> dev_em;
  std::vector<EmRec> em_recs;
  std::vector<double> em_tabs;
  std::vector<uint32_t> em_list;
  std::vector<uint32_t> em_streams;  // the RngStreams the enabled Rate models name
  // random OnOff times (nsgpu_p2p_scenario_ext.app_on_var / app_off_var): two reset records an application (OnTime,
  // OffTime; nsgpu_p2p_dev.h "random OnOff times"), empty without a random variable
  std::vector<RvRec> rv_recs;
  // per-flow statistics (scenario flowmon): each node's tracked-packet table size (plan_flowmon)
  bool flowmon = false;
  std::vector<uint32_t> fm_cap;
  // the setup-time events (this rank's, partitioned) and the bound of window 0 (the whole setup: every rank)
  std::vector<uint64_t> its;
  std::vector<uint32_t> iuid, ictx, ikind, ia;
  Red red0{};
  uint32_t n_init = 0, uid_init = 0;
  uint64_t pool_cap = 0;
  uint32_t capx = 0;  // partitioned: X2 records per peer per window
  uint64_t x2b = 0;   // partitioned: X2 bytes per peer
};

// RateErrorModel::DoCorruptByte / DoCorruptBit (error-model.cc:207-223): out[n] = the threshold for a frame of n bytes,
// n = 0 .. 1502, in the reference's expression and operation order, with the host's pow (the device looks it up).
static void em_thresholds(uint32_t unit, double rate, double *out) {
  for (uint32_t n = 0; n < NSGPU_EM_TABLE_SIZE; n++)
    out[n] = 1 - pow(1.0 - rate, (double)(unit == NSGPU_EU_BIT ? 8 * n : n));
}
extern "C" int nsgpu_error_model_thresholds(uint32_t unit, double rate, double *out) {
  if (!out || (unit != NSGPU_EU_BYTE && unit != NSGPU_EU_BIT))
    return set_error(NSGPU_EINVAL, "nsgpu_error_model_thresholds: unit must be EU_BYTE or EU_BIT");
  em_thresholds(unit, rate, out);
  return NSGPU_OK;
}

// The receive error models of a scenario (nsgpu_p2p_scenario.dev_em_kind), validated; the models' reset records.
static int plan_error_models(const nsgpu_p2p_scenario *sc, EnginePlan &P) {
  const uint32_t D = sc->n_devices;
  P.dev_em.assign(D, 0);
  if (!sc->dev_em_kind) return NSGPU_OK;
  if (!nsgpu_rng_check_seed(sc->rng_seed ? sc->rng_seed : 1u))
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: rng_seed %u is not a seed RngStream::CheckSeed accepts (below "
                     "4294944443)", sc->rng_seed);
  std::vector<std::pair<uint32_t, uint64_t>> tabs;  // (unit, the rate's bits) of each table
  std::vector<std::pair<uint32_t, uint32_t>> streams;  // (stream, device) of the enabled Rate models
  for (uint32_t d = 0; d < D; d++) {
    const uint32_t kind = sc->dev_em_kind[d];
    if (kind == NSGPU_EM_NONE) continue;
    if (kind == NSGPU_EM_LIST)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: ListErrorModel is not modelled (it selects by "
                       "Packet::GetUid, and the engine carries no packet uids)", d);
    if (kind != NSGPU_EM_RECEIVE_LIST && kind != NSGPU_EM_RATE)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: unknown error model kind %u", d, kind);
    EmRec r{};
    r.kind = kind;
    r.tab = EM_NOTAB;
    r.dev = d;
    if (kind == NSGPU_EM_RATE) {
      if (!sc->dev_em_rate || !sc->dev_em_stream)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: a Rate error model without dev_em_rate / dev_em_stream", d);
      const uint32_t unit = sc->dev_em_unit ? sc->dev_em_unit[d] : (uint32_t)NSGPU_EU_BYTE;
      if (unit > NSGPU_EU_BIT)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: unknown error unit %u", d, unit);
      r.rate = sc->dev_em_rate[d];
      if (r.rate != r.rate)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: the Rate error model's ErrorRate is NaN", d);
      if (sc->dev_em_enabled && !sc->dev_em_enabled[d]) continue;  // (disabled: it draws nothing, no stream is used)
      for (const auto &st : streams)
        if (st.first == sc->dev_em_stream[d])
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: devices %u and %u name the same RngStream %u (one Rate error "
                           "model object shared by two devices is not modelled)", st.second, d, st.first);
      streams.emplace_back(sc->dev_em_stream[d], d);
      P.em_streams.push_back(sc->dev_em_stream[d]);
      nsgpu_rng_stream_init(&r.g, sc->rng_seed, sc->rng_run, sc->dev_em_stream[d]);
      if (unit != NSGPU_EU_PKT) {
        uint64_t bits;
        memcpy(&bits, &r.rate, 8);
        uint32_t t = 0;
        while (t < tabs.size() && !(tabs[t].first == unit && tabs[t].second == bits)) t++;
        if (t == tabs.size()) {
          if (t == NSGPU_EM_MAX_TABLES)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: more than %u distinct (unit, rate) pairs of "
                             "EU_BYTE / EU_BIT error models", d, NSGPU_EM_MAX_TABLES);
          tabs.emplace_back(unit, bits);
          P.em_tabs.resize((size_t)(t + 1) * NSGPU_EM_TABLE_SIZE);
          em_thresholds(unit, r.rate, P.em_tabs.data() + (size_t)t * NSGPU_EM_TABLE_SIZE);
        }
        r.tab = t;
      }
    } else {
      const uint64_t lo = sc->em_list_off ? sc->em_list_off[d] : 0, hi = sc->em_list_off ? sc->em_list_off[d + 1] : 0;
      if (hi < lo || (hi > lo && !sc->em_list))
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: bad ReceiveList error model list", d);
      if (sc->dev_em_enabled && !sc->dev_em_enabled[d]) continue;
      // the std::list acts as a set: sorted, duplicates dropped
      std::vector<uint32_t> l(sc->em_list + lo, sc->em_list + hi);
      std::sort(l.begin(), l.end());
      l.erase(std::unique(l.begin(), l.end()), l.end());
      if (P.em_list.size() + l.size() > 0xffffffffull)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: the ReceiveList error models' lists hold 2^32 entries or more");
      r.cur = (uint32_t)P.em_list.size();
      P.em_list.insert(P.em_list.end(), l.begin(), l.end());
      r.end = (uint32_t)P.em_list.size();
    }
    P.em_recs.push_back(r);
    P.dev_em[d] = (uint32_t)P.em_recs.size();
  }
  return NSGPU_OK;
}

// The OnOff applications' OnTime / OffTime variables (nsgpu_p2p_scenario_ext.app_on_var / app_off_var), validated; the
// reset records.  A caller compiled against the shorter record, a NULL array and a Constant entry all mean app_on_s /
// app_off_s; without a random variable P.rv_recs stays empty and the engine is today's.
static bool rv_finite(double x) { return x - x == 0.0; }
static int plan_ranvars(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext, EnginePlan &P) {
  const uint32_t A = sc->n_apps;
  if (!ext || ext->size < offsetof(nsgpu_p2p_scenario_ext, app_off_var) + sizeof(void *)) return NSGPU_OK;
  const nsgpu_ranvar *var[2] = {ext->app_on_var, ext->app_off_var};
  if (!var[0] && !var[1]) return NSGPU_OK;
  static const char *const name[2] = {"OnTime", "OffTime"};
  std::vector<RvRec> recs(2 * (size_t)A);
  std::vector<std::pair<uint32_t, uint32_t>> streams;  // (stream, 2 a + which)
  bool any = false;
  for (uint32_t a = 0; a < A; a++)
    for (int w = 0; w < 2; w++) {
      RvRec r{};
      r.v.kind = NSGPU_RV_CONSTANT;
      const double *cs = w == 0 ? sc->app_on_s : sc->app_off_s;
      r.v.p0 = cs ? cs[a] : 0.0;
      const nsgpu_ranvar *v = var[w] ? var[w] + a : nullptr;
      if (v && v->kind != NSGPU_RV_CONSTANT) {
        if (v->kind == NSGPU_RV_OTHER)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: only Constant, Uniform and Exponential variables "
                           "are modelled (pow, sqrt and exp would each need what log got)", a, name[w]);
        if (v->kind != NSGPU_RV_UNIFORM && v->kind != NSGPU_RV_EXPONENTIAL)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: unknown random variable kind %u", a, name[w], v->kind);
        if (sc->app_kind[a] != NSGPU_APP_ONOFF)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: a random variable on an application that is not "
                           "an OnOff", a, name[w]);
        if (v->kind == NSGPU_RV_UNIFORM) {
          if (!rv_finite(v->p0) || !rv_finite(v->p1))
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Uniform with a non-finite parameter", a, name[w]);
          if (v->p0 < 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Uniform with min < 0", a, name[w]);
          if (v->p1 < v->p0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Uniform with max < min", a, name[w]);
          if (v->p1 >= 9.2e9)  // (2^63 ns)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Uniform whose max overflows the timestamp", a, name[w]);
        } else {
          if (!rv_finite(v->p0))
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Exponential with a non-finite mean", a, name[w]);
          if (!(v->p0 > 0)) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Exponential with mean <= 0", a, name[w]);
          // -log (U01) is at most 32 ln 2 = 22.2
          if (23.0 * v->p0 >= 9.2e9)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Exponential whose mean overflows the timestamp "
                             "(23 * mean seconds)", a, name[w]);
          if (!(v->p1 >= 0))  // (a NaN too)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Exponential with bound < 0", a, name[w]);
          if (v->p1 > 0 && v->p1 < v->p0 / 8)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s: Exponential with a bound below mean / 8 (the "
                             "device redraws at most %u times)", a, name[w], NSGPU_RV_MAX_ATTEMPTS);
        }
        for (const auto &st : streams)
          if (st.first == v->stream)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u %s and app %u %s name the same RngStream %u (a "
                             "variable owns its stream)", st.second / 2, name[st.second & 1], a, name[w], v->stream);
        for (const uint32_t es : P.em_streams)
          if (es == v->stream)
            return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %s names RngStream %u, which a Rate error model "
                             "names too", a, name[w], v->stream);
        streams.emplace_back(v->stream, 2 * a + (uint32_t)w);
        r.v = *v;
        if (!nsgpu_rng_stream_init(&r.g, sc->rng_seed, sc->rng_run, v->stream))
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: rng_seed %u is not a seed RngStream::CheckSeed accepts (below "
                           "4294944443)", sc->rng_seed);
        any = true;
      }
      recs[2 * (size_t)a + w] = r;
    }
  if (any) P.rv_recs.swap(recs);
  return NSGPU_OK;
}

// One UdpTraceClient's entries, validated, and the walk of its cycle (udp-trace-client.cc:311-335) from entry 0 until
// m_currentEntry repeats at a Send's start: the smallest and largest UDP payload it puts on a wire, the largest burst,
// the shortest delay between two Sends, and per cycle the datagrams and the time.
struct TraceWalk {
  uint32_t min_payload = 0xffffffffu, max_payload = 0, max_burst = 0;
  int64_t min_delay = (int64_t)1 << 61;
  uint64_t head_dgrams = 0, cycle_dgrams = 0;  // before the cycle is entered; one round of it
  int64_t cycle_ns = 0;
};
static int plan_trace_client(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext, uint32_t a, bool ports,
                             TraceWalk &W) {
  if (!ports)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: UdpTraceClient needs UDP ports (app_port)", a);
  if (!ext || ext->size < offsetof(nsgpu_p2p_scenario_ext, trace_entries) + sizeof(void *) || !ext->trace_off)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: no trace entries (an nsgpu_p2p_scenario_ext "
                     "through the _ex entry points carries them)", a);
  const uint64_t lo = ext->trace_off[a], hi = ext->trace_off[a + 1];
  if (hi <= lo || !ext->trace_entries)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: no trace entries", a);
  if (hi - lo > 0x7fffffffull)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: 2^31 trace entries or more", a);
  const uint32_t N = sc->n_nodes;
  if (sc->app_dst_node[a] >= N || sc->app_dst_slot[a] >= sc->n_dst || sc->app_ttl[a] == 0 || sc->app_ttl[a] > 255 ||
      sc->app_dst_node[a] == sc->app_node[a] ||
      (sc->app_src_slot && sc->app_src_slot[a] != 0xffffffffu && sc->app_src_slot[a] >= sc->n_dst))
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: bad destination/ttl/source slot", a);
  // (also in a frag scenario: a trace client sends no fragments — MaxPacketSize is a uint16 the example sets to 1472)
  const uint32_t mps = sc->app_pkt_size[a];
  if (mps == 0 || mps > 1472)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: MaxPacketSize %u outside [1, 1472]", a, mps);
  const nsgpu_udp_trace_entry *T = ext->trace_entries + lo;
  const uint32_t cnt = (uint32_t)(hi - lo);
  bool any = false;
  for (uint32_t e = 0; e < cnt; e++) {
    if (T[e].packet_size > 65535)  // (TraceEntry::packetSize is a uint16)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: entry %u: packet_size %u above 65535", a, e,
                       T[e].packet_size);
    any = any || T[e].time_to_send_ms != 0;
  }
  if (!any)  // (the do-while of Send would never end)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: every entry's timeToSend is 0 (the "
                     "reference's Send loop would not end)", a);
  // the walk: Send k starts at entry start[k]; the state of the client between Sends is that entry alone
  std::vector<int64_t> seen_t(cnt, -1);
  std::vector<uint64_t> seen_d(cnt, 0);
  uint32_t e = 0;
  int64_t t = 0;
  uint64_t dg = 0;
  while (seen_t[e] < 0) {
    seen_t[e] = t;
    seen_d[e] = dg;
    uint64_t burst = 0;
    do {
      const uint32_t ps = T[e].packet_size, nfull = ps / mps;
      for (uint32_t i = 0; i <= nfull; i++) {
        const uint32_t sz = i < nfull ? mps : ps % mps, pay = sz > 12 ? sz : 12;
        W.min_payload = std::min(W.min_payload, pay);
        W.max_payload = std::max(W.max_payload, pay);
      }
      burst += (uint64_t)nfull + 1;
      e = e + 1 == cnt ? 0 : e + 1;
    } while (T[e].time_to_send_ms == 0);
    if (burst > NSGPU_UDP_TRACE_MAX_BURST)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: a Send of %llu datagrams (at most %u: "
                       "NSGPU_UDP_TRACE_MAX_BURST)", a, (unsigned long long)burst, NSGPU_UDP_TRACE_MAX_BURST);
    W.max_burst = std::max<uint32_t>(W.max_burst, (uint32_t)burst);
    dg += burst;
    const int64_t d = (int64_t)T[e].time_to_send_ms * 1000000ll;
    W.min_delay = std::min(W.min_delay, d);
    t += d;
  }
  W.head_dgrams = seen_d[e];
  W.cycle_dgrams = dg - seen_d[e];
  W.cycle_ns = t - seen_t[e];
  return NSGPU_OK;
}

// Per-flow statistics (nsgpu_p2p_scenario.flowmon): the refusals, and each node's tracked-packet table size — a bound
// on the identifications the node hands out before the run ends (nsgpu_p2p_dev.h "per-flow statistics"), at most
// FM_NODE_CAP.  A node originates its senders' datagrams, the echo replies to the clients that address it, and with
// icmp its ICMP errors, which take identifications too: at most one error a datagram of the scenario.  Called once
// the applications are validated.
static int plan_flowmon(const nsgpu_p2p_scenario *sc, const uint32_t *owner, EnginePlan &P) {
  // (the word was padding before: a value other than 0 or 1 is a caller that never set it, not a request)
  if (sc->flowmon > 1)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: flowmon is %u (0 or 1: the word behind frag, padding in earlier "
                     "versions of the struct, must be zeroed)", sc->flowmon);
  P.flowmon = sc->flowmon == 1;
  if (!P.flowmon) return NSGPU_OK;
  if (sc->frag)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: flowmon with frag is not modelled (the reference classifies a "
                     "non-first fragment by reading payload bytes as a UDP header, and so invents flows)");
  if (owner)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create_dist: flowmon on a partitioned engine is not modelled (a tracked "
                     "packet's entry belongs to the rank of its originating node)");
  const uint32_t N = sc->n_nodes, A = sc->n_apps;
  bool has_stop = false;
  for (uint32_t i = 0; i < sc->n_setup; i++) has_stop = has_stop || sc->setup_kind[i] == NSGPU_SETUP_STOP;
  const uint64_t CAP = FM_NODE_CAP;
  auto sender = [&](uint32_t k) {
    return k == NSGPU_APP_ONOFF || k == NSGPU_APP_ECHO_CLIENT || k == NSGPU_APP_UDP_CLIENT || k == NSGPU_APP_UDP_TRACE_CLIENT;
  };
  // the datagrams application a can send before the run (or the application) stops, CAP when nothing bounds them
  auto bound = [&](uint32_t a) -> uint64_t {
    int64_t t1 = has_stop ? sc->stop_ns : -1;
    if (sc->app_stop_ns[a] != 0 && (t1 < 0 || sc->app_stop_ns[a] < t1)) t1 = sc->app_stop_ns[a];
    const int64_t dur = t1 < 0 ? -1 : std::max<int64_t>(0, t1 - sc->app_start_ns[a]);
    if (sc->app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT) {  // (the walk of its cycle: plan_trace_client)
      if (dur < 0) return CAP;
      const u128 b = (u128)P.tc_bound[3 * a] + ((u128)(dur / P.tc_bound[3 * a + 2]) + 2) * P.tc_bound[3 * a + 1];
      return b < CAP ? (uint64_t)b : CAP;
    }
    if (sc->app_kind[a] != NSGPU_APP_ONOFF) {  // MaxPackets, one an Interval
      uint64_t b = sc->app_count[a];
      if (dur >= 0 && sc->app_interval_ns[a] > 0) b = std::min<uint64_t>(b, (uint64_t)(dur / sc->app_interval_ns[a]) + 1);
      return std::min(b, CAP);
    }
    // OnOff: MaxBytes (a packet while m_totBytes < m_maxBytes); the rate paces size * 8 bits a packet over the on
    // time, the residual bits included; each interval is rounded to a ns, so an eighth more and a few for the ends
    const uint64_t size = sc->app_pkt_size[a];
    uint64_t b = CAP;
    if (sc->app_max_bytes[a]) b = std::min<uint64_t>(b, (sc->app_max_bytes[a] + size - 1) / size);
    if (dur >= 0 && (u128)size * 8 * 1000000000ull >= (u128)sc->app_rate_bps[a] * 8) {  // (intervals of 8 ns or more)
      const u128 est = (u128)sc->app_rate_bps[a] * (uint64_t)dur / ((u128)size * 8 * 1000000000ull);
      if (est < CAP) b = std::min<uint64_t>(b, (uint64_t)est + (uint64_t)est / 8 + 16);
    }
    return b;
  };
  std::vector<uint64_t> cap(N, 0);
  uint64_t total = 0;
  for (uint32_t a = 0; a < A; a++) {
    if (!sender(sc->app_kind[a])) continue;
    const uint64_t b = bound(a);
    cap[sc->app_node[a]] += b;
    total += b;
    if (sc->app_kind[a] == NSGPU_APP_ECHO_CLIENT) {  // (a reply at most a request)
      cap[sc->app_dst_node[a]] += b;
      total += b;
    }
  }
  P.fm_cap.assign(N, 0);
  for (uint32_t n = 0; n < N; n++)
    if (cap[n]) P.fm_cap[n] = (uint32_t)std::min(cap[n] + (sc->icmp ? total : 0), CAP);
  return NSGPU_OK;
}

static int plan_engine(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext, const uint32_t *owner, int rank,
                       int nranks, uint64_t pool_cap, EnginePlan &P) {
  if (!sc) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: null");
  const uint32_t N = sc->n_nodes, D = sc->n_devices, A = sc->n_apps;
  if (N == 0 || !sc->setup_kind || !sc->setup_index) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: empty");
  // ---- validation (host arrays) ----
  uint32_t &qcap = P.qcap;
  qcap = 1;
  for (uint32_t d = 0; d < D; d++) {
    if (sc->dev_node[d] >= N || sc->dev_peer[d] >= D || sc->dev_peer[sc->dev_peer[d]] != d)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: bad node/peer", d);
    if (sc->dev_bps[d] == 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: zero DataRate", d);
    if (sc->dev_delay_ns[d] < 0 || sc->dev_ifg_ns[d] < 0)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: device %u: negative delay", d);
    qcap = std::max(qcap, sc->dev_qmax[d]);
  }
  if (int rce = plan_error_models(sc, P)) return rce;
  if (int rcv = plan_ranvars(sc, ext, P)) return rcv;
  if (owner) {
    if (nranks < 1 || nranks > MAXR || rank < 0 || rank >= nranks ||
        (uint64_t)nranks * CAPX_MAX + TB + 2 * WCAP >= (uint64_t)GRID_POOL_DIST * TB)  // (k2_pa: slot, remote, chunk blocks)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create_dist: rank %d of %d (at most %d ranks)", rank, nranks,
                       (int)(((uint64_t)GRID_POOL_DIST * TB - TB - 2 * WCAP - 1) / CAPX_MAX));
    for (uint32_t n = 0; n < N; n++)
      if (owner[n] >= (uint32_t)nranks) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create_dist: node %u: owner %u", n, owner[n]);
  }
  if (!sc->route) {  // compressed next-hop table
    if (!sc->route_default || !sc->route_exc_off || !sc->route_exc_slot || !sc->route_exc_dev ||
        sc->route_exc_off[0] != 0)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: no route table");
    for (uint32_t n = 0; n < N; n++) {
      if (sc->route_exc_off[n + 1] < sc->route_exc_off[n])
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: route_exc_off not ascending at node %u", n);
      if (sc->route_default[n] != 0xffffffffu && sc->route_default[n] >= D)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: node %u: bad default route", n);
      for (uint64_t j = sc->route_exc_off[n]; j < sc->route_exc_off[n + 1]; j++)
        if ((j > sc->route_exc_off[n] && sc->route_exc_slot[j] <= sc->route_exc_slot[j - 1]) ||
            sc->route_exc_slot[j] >= sc->n_dst || (sc->route_exc_dev[j] != 0xffffffffu && sc->route_exc_dev[j] >= D))
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: node %u: bad route exception %llu", n,
                           (unsigned long long)j);
    }
  }
  std::vector<uint32_t> &napps = P.napps;
  std::vector<int32_t> &sink = P.sink;
  napps.assign(N + 1, 0);
  sink.assign(N, -1);
  uint32_t min_pkt = 0xffffffffu;
  uint32_t min_frag_wire = 0xffffffffu;  // frag: the smallest last fragment's frame (PPP included)
  const bool frag = sc->frag != 0;
  P.frag = frag;
  if (frag && sc->frag_timeout_ns < 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: negative frag_timeout_ns");
  P.frag_flows.assign(N, 0);
  bool &has_echo = P.has_echo;
  has_echo = false;
  int64_t echo_ivl = (int64_t)1 << 61;
  std::vector<uint32_t> tc_min_payload(A, 0);  // (a trace client's smallest UDP payload)
  const bool ports = sc->app_port != nullptr;
  P.ports = ports;
  if (ports && !sc->app_remote_port) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app_port without app_remote_port");
  for (uint32_t a = 0; a < A; a++) {
    if (sc->app_node[a] >= N) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: bad node", a);
    napps[sc->app_node[a] + 1]++;
    const uint32_t ak = sc->app_kind[a];
    if (ak == NSGPU_APP_UDP_TRACE_CLIENT && !ports)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: UdpTraceClient needs UDP ports (app_port)", a);
    if ((ak == NSGPU_APP_UDP_CLIENT || ak == NSGPU_APP_UDP_SERVER) && !ports)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: UdpClient / UdpServer need UDP ports (app_port)", a);
    if (ak == NSGPU_APP_UDP_SERVER) {  // (bound like a sink: the endpoints are resolved below)
      if (!sc->app_loss_window || sc->app_loss_window[a] % 8 != 0 || sc->app_loss_window[a] < 8 ||
          sc->app_loss_window[a] > NSGPU_LOSS_WINDOW_MAX)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpServer %u: PacketWindowSize must be a multiple of 8 in [8, 256]", a);
    } else if (ak == NSGPU_APP_UDP_TRACE_CLIENT) {
      TraceWalk W;
      if (int rct = plan_trace_client(sc, ext, a, ports, W)) return rct;
      if (!P.has_trace_client) {
        P.has_trace_client = true;
        P.tc_bound.assign(3 * (size_t)A, 0);
      }
      P.tc_bound[3 * a] = W.head_dgrams + W.max_burst, P.tc_bound[3 * a + 1] = W.cycle_dgrams;
      P.tc_bound[3 * a + 2] = (uint64_t)W.cycle_ns;
      tc_min_payload[a] = W.min_payload;
      // the smallest frame the flow can put on a wire bounds the lookaheads; the largest is at most MaxPacketSize + 30
      // (1502: the error models' table and a frame's MTU hold it)
      min_pkt = std::min(min_pkt, W.min_payload);
      echo_ivl = std::min(echo_ivl, W.min_delay);  // (the next Send's delay: at least 1 ms)
    } else if (ak == NSGPU_APP_UDP_CLIENT) {
      if (!sc->app_count || !sc->app_interval_ns || sc->app_dst_node[a] >= N || sc->app_dst_slot[a] >= sc->n_dst ||
          sc->app_ttl[a] == 0 || sc->app_ttl[a] > 255 || sc->app_dst_node[a] == sc->app_node[a] ||
          sc->app_interval_ns[a] < 0 ||
          (sc->app_src_slot && sc->app_src_slot[a] != 0xffffffffu && sc->app_src_slot[a] >= sc->n_dst))
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpClient %u: bad destination/ttl/interval/source slot", a);
      if (sc->app_pkt_size[a] < 12 || sc->app_pkt_size[a] > 1472) {
        if (!frag)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpClient %u: PacketSize %u outside [12, 1472]", a,
                           sc->app_pkt_size[a]);
        if (sc->app_pkt_size[a] < 12 || sc->app_pkt_size[a] > 1500)  // (udp-client.cc:70: the attribute's checker)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpClient %u: PacketSize %u outside [12, 1500]", a,
                           sc->app_pkt_size[a]);
      }
      if (sc->app_count[a] > (1u << 24))  // (the descriptor carries the sequence number in 24 bits)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpClient %u: MaxPackets %u above 2^24", a, sc->app_count[a]);
      min_pkt = std::min(min_pkt, sc->app_pkt_size[a]);
      echo_ivl = std::min(echo_ivl, sc->app_interval_ns[a]);
    } else if (ak == NSGPU_APP_SINK || ak == NSGPU_APP_ECHO_SERVER) {  // the node's bound UDP endpoint
      if (!ports) {
        if (sink[sc->app_node[a]] >= 0)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: node %u has two bound endpoints", sc->app_node[a]);
        sink[sc->app_node[a]] = (int32_t)a;
      }
      if (ak == NSGPU_APP_ECHO_SERVER) {
        if (sc->app_ttl[a] == 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpEchoServer %u: ttl", a);
        has_echo = true;
      }
    } else if (ak == NSGPU_APP_ECHO_CLIENT) {
      if (!sc->app_count || !sc->app_interval_ns || !sc->app_src_slot || sc->app_dst_node[a] >= N ||
          sc->app_dst_slot[a] >= sc->n_dst || sc->app_src_slot[a] >= sc->n_dst || sc->app_pkt_size[a] == 0 ||
          sc->app_ttl[a] == 0 || sc->app_dst_node[a] == sc->app_node[a] || sc->app_interval_ns[a] < 0)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpEchoClient %u: bad destination/size/ttl/interval", a);
      has_echo = true;
      min_pkt = std::min(min_pkt, sc->app_pkt_size[a]);
      echo_ivl = std::min(echo_ivl, sc->app_interval_ns[a]);
    } else if (ak != NSGPU_APP_ONOFF) {
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: unknown kind %u", a, ak);
    } else {
      if (sc->app_dst_node[a] >= N || sc->app_dst_slot[a] >= sc->n_dst || sc->app_rate_bps[a] == 0 ||
          sc->app_pkt_size[a] == 0 || sc->app_ttl[a] == 0 || sc->app_dst_node[a] == sc->app_node[a] ||
          (sc->app_src_slot && sc->app_src_slot[a] != 0xffffffffu && sc->app_src_slot[a] >= sc->n_dst))
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: OnOff %u: bad destination/rate/size/ttl/source slot", a);
      min_pkt = std::min(min_pkt, sc->app_pkt_size[a]);
    }
    // SendRealOut fragments a datagram above the device MTU (ipv4-l3-protocol.cc:722-731; PointToPointNetDevice
    // Mtu 1500): not modelled, so payloads are bounded by 1500 - 20 (IPv4) - 8 (UDP)
    if (ak == NSGPU_APP_ECHO_CLIENT || ak == NSGPU_APP_ONOFF) {
      if (sc->app_pkt_size[a] > 1472 && !frag)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %u-byte payload needs IPv4 fragmentation", a,
                         sc->app_pkt_size[a]);
      // frag: up to MAX_IPV4_UDP_DATAGRAM_SIZE (udp-socket-impl.cc:45); above it DoSendTo fails with EMSGSIZE
      if (sc->app_pkt_size[a] > 65507)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %u-byte payload is above the largest UDP datagram "
                         "(65507 bytes: EMSGSIZE)", a, sc->app_pkt_size[a]);
    }
    if (frag && (ak == NSGPU_APP_ECHO_CLIENT || ak == NSGPU_APP_ONOFF || ak == NSGPU_APP_UDP_CLIENT)) {
      const uint32_t sz = sc->app_pkt_size[a];
      if (sz > 1472) {  // a fragmenting flow: its fragments reach its destination, an echo's reply its client's node
        P.frag_flows[sc->app_dst_node[a]]++;
        if (ak == NSGPU_APP_ECHO_CLIENT) P.frag_flows[sc->app_node[a]]++;
        // the smallest frame on a wire: the last fragment (IPv4 length 20 + what 1480-byte parts leave) + PPP
        // (down to 21 + 2 bytes; the lookaheads below take it)
        const uint32_t L = sz + 8, tail = L - (L - 1) / FRAG_PART * FRAG_PART;
        min_frag_wire = std::min(min_frag_wire, 20 + tail + 2);
      }
    }
    if (A > NSGPU_PKT_APP) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: more than 2^28 applications");
  }
  if (ports) {
    // Ipv4EndPointDemux for sockets bound to (Any, port): the binding (node, port) -> application is static
    auto bound = [&](uint32_t k) { return k == NSGPU_APP_SINK || k == NSGPU_APP_ECHO_SERVER || k == NSGPU_APP_UDP_SERVER; };
    auto sender = [&](uint32_t k) {
      return k == NSGPU_APP_ONOFF || k == NSGPU_APP_ECHO_CLIENT || k == NSGPU_APP_UDP_CLIENT || k == NSGPU_APP_UDP_TRACE_CLIENT;
    };
    std::vector<std::vector<uint32_t>> eps(N);
    std::vector<uint8_t> sends(N, 0);
    for (uint32_t a = 0; a < A; a++)
      if (sender(sc->app_kind[a])) sends[sc->app_node[a]] = 1;
    for (uint32_t a = 0; a < A; a++) {
      if (!bound(sc->app_kind[a])) continue;
      const uint32_t n = sc->app_node[a], port = sc->app_port[a];
      if (port == 0 || port > 65535) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: bound port %u", a, port);
      for (uint32_t b : eps[n])  // the second Bind fails (ipv4-end-point-demux.cc:60-76)
        if (sc->app_port[b] == port)
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: node %u has two applications bound to port %u", n, port);
      // a sending application's sockets take ephemeral ports from 49152 up (ipv4-end-point-demux.cc:351-372)
      if (port >= 49152 && sends[n])
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: port %u is in the ephemeral range of node %u's senders",
                         a, port, n);
      eps[n].push_back(a);
    }
    P.ep_of_flow.assign(A, -1);
    std::vector<uint8_t> other(N, 0);  // a flow addressed to the node targets another port than its first endpoint's
    for (uint32_t a = 0; a < A; a++) {
      if (!sender(sc->app_kind[a])) continue;
      const uint32_t n = sc->app_dst_node[a];
      for (uint32_t b : eps[n])
        if (sc->app_port[b] == sc->app_remote_port[a]) P.ep_of_flow[a] = (int32_t)b;
      const int32_t e = P.ep_of_flow[a];
      if (eps[n].empty() || e != (int32_t)eps[n][0]) other[n] = 1;
      // a UdpServer reads a SeqTsHeader from every datagram (udp-server.cc:159-160)
      if (sc->app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT) {
        // (its payloads always hold the header; a datagram that is the header alone is for a UdpServer only)
        if (tc_min_payload[a] == 12 && !(e >= 0 && sc->app_kind[e] == NSGPU_APP_UDP_SERVER))
          return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: UdpTraceClient %u: a 12-byte payload (the SeqTsHeader alone) "
                           "to port %u, which is no UdpServer's", a, sc->app_remote_port[a]);
        continue;
      }
      if (e >= 0 && sc->app_kind[e] == NSGPU_APP_UDP_SERVER && sc->app_pkt_size[a] < 12)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: app %u: %u-byte payload to UdpServer %d holds no SeqTsHeader", a,
                         sc->app_pkt_size[a], e);
    }
    // sink[n]: the node's single endpoint when every flow addressed to n targets it; EP_BY_FLOW: per flow
    for (uint32_t n = 0; n < N; n++)
      sink[n] = eps[n].empty() ? -1 : (eps[n].size() == 1 && !other[n]) ? (int32_t)eps[n][0] : EP_BY_FLOW;
  }
  if (frag) {
    // ProcessFragment's key is always (0, 0) (nsgpu_p2p_dev.h "IPv4 fragmentation"): a node has one reassembly
    // buffer for all sources.  With one fragmenting flow a node that shows only when loss mixes the flow's own
    // datagrams, which is modelled; several flows into one node are refused
    for (uint32_t n = 0; n < N; n++)
      if (P.frag_flows[n] > 1)
        return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: node %u receives fragments of %u fragmenting flows (at most "
                         "one: the reference's nodes have one reassembly buffer for all sources)", n, P.frag_flows[n]);
    P.frag_timeout = sc->frag_timeout_ns ? sc->frag_timeout_ns : 30000000000ll;  // Seconds (30) (:61-64)
  }
  if (P.has_trace_client) {  // the offsets and entries as the device reads them (tc_offsets, tc_entries)
    uint64_t tot = 0;
    for (uint32_t a = 0; a < A; a++)
      if (sc->app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT) tot += ext->trace_off[a + 1] - ext->trace_off[a];
    if (tot > 0x3fffffffull)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: the UdpTraceClients' traces hold 2^30 entries or more");
    P.tc_img.reserve((size_t)A + 1 + 2 * tot);
    P.tc_img.assign((size_t)A + 1, 0);
    for (uint32_t a = 0; a < A; a++) {
      if (sc->app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT)
        for (uint64_t j = ext->trace_off[a]; j < ext->trace_off[a + 1]; j++) {
          P.tc_img.push_back(ext->trace_entries[j].time_to_send_ms);
          P.tc_img.push_back(ext->trace_entries[j].packet_size);
        }
      P.tc_img[a + 1] = (uint32_t)((P.tc_img.size() - A - 1) / 2);
    }
  }
  if (int rcf = plan_flowmon(sc, owner, P)) return rcf;
  uint32_t &maxapps = P.maxapps;
  maxapps = 0;
  for (uint32_t n = 0; n < N; n++) maxapps = std::max(maxapps, napps[n + 1]);
  for (uint32_t n = 0; n < N; n++) napps[n + 1] += napps[n];
  std::vector<uint32_t> &node_list = P.node_list, fill(napps.begin(), napps.end() - 1);
  node_list.assign(A, 0);
  for (uint32_t a = 0; a < A; a++) node_list[fill[sc->app_node[a]]++] = a;
  // ---- lookahead per event kind: the smallest delay a child of that kind can get ----
  const int64_t INFL = (int64_t)1 << 61;
  int64_t tx_min = INFL;
  // the smallest frame a sender puts on a wire: payload + UDP, IPv4, PPP headers, or a frag flow's last fragment
  const uint32_t min_wire = std::min(min_pkt == 0xffffffffu ? min_pkt : min_pkt + 30, min_frag_wire);
  if (min_pkt != 0xffffffffu)
    for (uint32_t d = 0; d < D; d++) {
      tx_min = std::min(tx_min, seconds_to_ts(static_cast<double>(min_wire) * 8 / (double)sc->dev_bps[d]));
      // an ICMP error is a 56-byte IPv4 packet (+2 PPP)
      if (sc->icmp) tx_min = std::min(tx_min, seconds_to_ts(static_cast<double>(56 + 2) * 8 / (double)sc->dev_bps[d]));
    }
  int64_t send_ivl = INFL;
  for (uint32_t a = 0; a < A; a++)
    if (sc->app_kind[a] == NSGPU_APP_ONOFF)
      send_ivl = std::min(send_ivl, seconds_to_ts((sc->app_pkt_size[a] * 8) / static_cast<double>(sc->app_rate_bps[a])));
  P.tx_min = tx_min;
  P.send_ivl = send_ivl;
  P.maxc = std::max(3u, 2 * maxapps);
  for (int k = 0; k < K_NKINDS; k++) P.lookahead[k] = INFL;
  P.lookahead[K_NODE_START] = 0;     // children at app start/stop times (may be 0)
  P.lookahead[K_APPOBJ_START] = 0;
  P.lookahead[K_APP_START] = 0;      // StartSending after OffTime (may be 0)
  P.lookahead[K_START_SENDING] = 0;  // first send after residual-shortened interval
  P.lookahead[K_STOP_SENDING] = 0;   // StartSending after OffTime
  P.lookahead[K_SEND] = std::min(std::min(tx_min, send_ivl), echo_ivl);
  P.lookahead[K_TX_COMPLETE] = tx_min;
  P.lookahead[K_RECEIVE] = tx_min;
  P.lookahead[K_FWD_UP_Q] = tx_min;  // UdpEchoServer reply: device children
  // A datagram for a UDP echo endpoint is delivered by a queued zero-delay DoForwardUp (its handler
  // schedules): the window must then end at the delivering Receive's time, so that the DoForwardUp is
  // the next window's first event at that time.
  if (has_echo) P.lookahead[K_RECEIVE] = 0;
  // frag: a Receive that opens a reassembly buffer schedules the timeout, and a timeout that fires may send an
  // ICMP error from its node (the class of K_FWD_UP_Q)
  constexpr int KFT = K_FRAG_TIMEOUT;
  if (frag) {
    P.lookahead[K_RECEIVE] = std::min(P.lookahead[K_RECEIVE], P.frag_timeout);
    P.lookahead[KFT] = tx_min;
  }
  // Wide windows (nsgpu_p2p_win.h): an event on another node is at least one transmission
  // plus its channel delay away — Lx = min over devices of (smallest frame's tx time + delay) — and a
  // same-node TransmitComplete before the window's end runs inside the window (a local record), so only
  // the children that are neither bound the window: lookw = lookahead with tx_min replaced by Lx.
  int64_t lx = INFL;
  if (min_pkt != 0xffffffffu)
    for (uint32_t d = 0; d < D; d++) {
      int64_t t = seconds_to_ts(static_cast<double>(min_wire) * 8 / (double)sc->dev_bps[d]);
      if (sc->icmp) t = std::min(t, seconds_to_ts(static_cast<double>(56 + 2) * 8 / (double)sc->dev_bps[d]));
      lx = std::min(lx, t + sc->dev_delay_ns[d]);
    }
  for (int k = 0; k < K_NKINDS; k++) P.lookw[k] = P.lookahead[k];
  P.lookw[K_SEND] = std::min(std::min(lx, send_ivl), echo_ivl);
  P.lookw[K_TX_COMPLETE] = lx;
  P.lookw[K_RECEIVE] = has_echo ? 0 : lx;
  P.lookw[K_FWD_UP_Q] = lx;
  if (frag) {
    P.lookw[K_RECEIVE] = std::min(P.lookw[K_RECEIVE], P.frag_timeout);
    P.lookw[KFT] = lx;
  }
  {  // a node's pending local records are its busy devices' TransmitCompletes: at most its degree
    std::vector<uint32_t> deg(N, 0);
    uint32_t dmax = 0;
    for (uint32_t d = 0; d < D; d++) dmax = std::max(dmax, ++deg[sc->dev_node[d]]);
    const char *nw = getenv("NSGPU_P2P_NARROW");
    // (a chain of same-node TransmitCompletes inside a window is shorter than Lx / tx_min: LKD levels)
    P.wide = (dmax <= (uint32_t)LQ && lx > tx_min && lx <= (int64_t)LKD * tx_min && lx < INFL &&
              !(nw && nw[0] == '1')) ? 1u : 0u;
    // partitioned: the ranks order each other's local records by their two order words (k_gtile), which are
    // exact for chains of at most 2 levels below a gen-0 event (the ancestor uid in X1Loc): the wide span is
    // kept below 3 tx_min, so a third level (3 transmissions after its gen-0 event) never falls in a window
    if (owner && P.wide)
      for (int k = 0; k < K_NKINDS; k++) P.lookw[k] = std::min<int64_t>(P.lookw[k], 3 * tx_min - 1);
  }
  P.lx = lx;
  // ---- setup-time events (node-list.cc:124-131, node.cc:111-145, default-simulator-impl.cc:179-183) ----
  std::vector<uint64_t> &its = P.its;
  std::vector<uint32_t> &iuid = P.iuid, &ictx = P.ictx, &ikind = P.ikind, &ia = P.ia;
  uint32_t uid = sc->uid_first ? sc->uid_first : 4u;  // (DefaultSimulatorImpl: m_uid (4), :52-56)
  if ((uint64_t)uid + sc->n_setup > UID_MAX_NEXT) {
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: the setup calls' uids would pass 0xfffffffe");
  }
  for (uint32_t i = 0; i < sc->n_setup; i++) {
    const uint32_t k = sc->setup_index[i];
    switch (sc->setup_kind[i]) {
      case NSGPU_SETUP_NODE:
        if (k >= N) { return set_error(NSGPU_EINVAL, "setup: node %u", k); }
        its.push_back(0); iuid.push_back(uid); ictx.push_back(k); ikind.push_back(K_NODE_START); ia.push_back(k);
        break;
      case NSGPU_SETUP_DEVICE:
        if (k >= D) { return set_error(NSGPU_EINVAL, "setup: device %u", k); }
        its.push_back(0); iuid.push_back(uid); ictx.push_back(sc->dev_node[k]); ikind.push_back(K_DEV_START); ia.push_back(k);
        break;
      case NSGPU_SETUP_APP:
        if (k >= A) { return set_error(NSGPU_EINVAL, "setup: app %u", k); }
        its.push_back(0); iuid.push_back(uid); ictx.push_back(sc->app_node[k]); ikind.push_back(K_APPOBJ_START); ia.push_back(k);
        break;
      case NSGPU_SETUP_NOOP:
        if (k >= N) { return set_error(NSGPU_EINVAL, "setup: noop node %u", k); }
        its.push_back(0); iuid.push_back(uid); ictx.push_back(k); ikind.push_back(K_DEV_START); ia.push_back(k);
        break;
      case NSGPU_SETUP_STOP:
        if (sc->stop_ns < 0) { return set_error(NSGPU_EINVAL, "setup: negative stop"); }
        its.push_back((uint64_t)sc->stop_ns); iuid.push_back(uid); ictx.push_back(NOCTX); ikind.push_back(K_STOP); ia.push_back(0);
        break;
      default:
        break;  // consumes a uid, no event
    }
    uid++;
  }
  // reduction of the whole initial pending set: window 0 is bounded by red[1] on every rank
  Red &red0 = P.red0;
  red0 = Red{~0ull, ~0ull, ~0ull, 0, 0, ~0ull};
  for (size_t i = 0; i < its.size(); i++) {
    red0.tmin = std::min<uint64_t>(red0.tmin, its[i]);
    red0.wend = std::min<uint64_t>(red0.wend, its[i] + (uint64_t)P.lookahead[ikind[i] & 0xffu]);
    red0.wendw = std::min<uint64_t>(red0.wendw, its[i] + (uint64_t)P.lookw[ikind[i] & 0xffu]);
    if ((ikind[i] & 0xffu) == K_STOP) {
      red0.stopts = its[i];
      red0.stopuid = iuid[i];
    }
  }
  if (owner) {  // this rank's initial events (Simulator::Stop: rank 0)
    size_t k = 0;
    for (size_t i = 0; i < its.size(); i++) {
      const bool mine = ictx[i] == NOCTX ? rank == 0 : owner[ictx[i]] == (uint32_t)rank;
      if (!mine) continue;
      its[k] = its[i], iuid[k] = iuid[i], ictx[k] = ictx[i], ikind[k] = ikind[i], ia[k] = ia[i];
      k++;
    }
    its.resize(k), iuid.resize(k), ictx.resize(k), ikind.resize(k), ia.resize(k);
  }
  P.n_init = (uint32_t)its.size();
  P.uid_init = uid;
  P.pool_cap = pool_cap ? pool_cap : std::max<uint64_t>(4ull * P.n_init + 65536, 1ull << 20);
  if (P.n_init > P.pool_cap) { return set_error(NSGPU_EINVAL, "pool_cap < setup events"); }
  if (owner) {
    {  // X2 capacity: the largest number of devices of one rank whose peer another rank owns
      std::vector<uint32_t> cut((size_t)nranks * nranks, 0);
      for (uint32_t d = 0; d < D; d++) {
        const uint32_t p = owner[sc->dev_node[d]], q = owner[sc->dev_node[sc->dev_peer[d]]];
        if (p != q) cut[(size_t)p * nranks + q]++;
      }
      uint32_t mx = 1;
      for (uint32_t c : cut) mx = std::max(mx, c);
      if (P.wide) mx *= 3;  // (wide: a device's gen-0 TransmitStart and up to two local ones, chain depth <= 2)
      P.capx = std::min<uint32_t>((mx + 15) / 16 * 16, CAPX_MAX);
      P.x2b = sizeof(X2Hdr) + sizeof(Ev) * (uint64_t)P.capx;
    }
  }
  return NSGPU_OK;
}

// owner == null: the whole scenario on this device; otherwise the partition `rank` of `nranks`
// (node n belongs to rank owner[n]).
static int create_engine(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext, const uint32_t *owner, int rank,
                         int nranks, nsgpu_comm *comm, uint64_t pool_cap, uint64_t log_cap, nsgpu_p2p **out) {
  if (!out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: null");
  *out = nullptr;
  EnginePlan P;
  if (int rcp = plan_engine(sc, ext, owner, rank, nranks, pool_cap, P)) return rcp;
  const uint32_t N = sc->n_nodes, D = sc->n_devices, A = sc->n_apps;
  const uint32_t qcap = P.qcap;
  const std::vector<uint32_t> &napps = P.napps, &node_list = P.node_list;
  const std::vector<int32_t> &sink = P.sink;
  nsgpu_p2p *h = new nsgpu_p2p();
  h->sc = *sc;
  h->app_kind.assign(sc->app_kind, sc->app_kind + A);
  h->n_apps = A;
  P2PDev &M = h->M;
  memset(&M, 0, sizeof(M));
  M.n_nodes = N;
  M.n_devices = D;
  M.n_apps = A;
  M.n_dst = sc->n_dst;
  M.qcap = qcap;
  M.maxc = P.maxc;
  for (int k = 0; k < K_NKINDS; k++) M.lookahead[k] = P.lookahead[k], M.lookw[k] = P.lookw[k];
  M.wide = P.wide;
  // ---- scenario upload ----
  TRY(dupload(h, &M.dev_node, sc->dev_node, D));
  if (sc->route) {
    TRY(dupload(h, &M.route, sc->route, (size_t)N * sc->n_dst));
  } else {
    const uint64_t ne = sc->route_exc_off[N];
    TRY(dupload(h, &M.route_def, sc->route_default, N));
    TRY(dupload(h, &M.route_exc_off, sc->route_exc_off, N + 1));
    TRY(dupload(h, &M.route_exc_slot, sc->route_exc_slot, ne));
    TRY(dupload(h, &M.route_exc_dev, sc->route_exc_dev, ne));
  }
  TRY(dupload(h, &M.app_kind, sc->app_kind, A));
  TRY(dupload(h, &M.app_node, sc->app_node, A));
  TRY(dupload(h, &M.app_dst_node, sc->app_dst_node, A));
  if (P.ports) {  // (the per-flow endpoint table lies behind the slots: ep_of_flow)
    std::vector<uint32_t> ds(sc->app_dst_slot, sc->app_dst_slot + A);
    for (uint32_t a = 0; a < A; a++) ds.push_back((uint32_t)P.ep_of_flow[a]);
    TRY(dupload(h, &M.app_dst_slot, ds.data(), 2 * (size_t)A));
  } else {
    TRY(dupload(h, &M.app_dst_slot, sc->app_dst_slot, A));
  }
  if (P.has_trace_client) {  // (the trace clients' offsets and entries lie behind the sizes: tc_entries)
    std::vector<uint32_t> ps(sc->app_pkt_size, sc->app_pkt_size + A);
    ps.insert(ps.end(), P.tc_img.begin(), P.tc_img.end());
    TRY(dupload(h, &M.app_pkt_size, ps.data(), ps.size()));
    h->has_trace_client = true;
  } else {
    TRY(dupload(h, &M.app_pkt_size, sc->app_pkt_size, A));
  }
  TRY(dupload(h, &M.app_max_bytes, sc->app_max_bytes, A));
  TRY(dupload(h, &M.app_ttl, sc->app_ttl, A));
  TRY(dupload(h, &M.app_start, sc->app_start_ns, A));
  TRY(dupload(h, &M.app_stop, sc->app_stop_ns, A));
  TRY(dupload(h, &M.app_rate, sc->app_rate_bps, A));
  TRY(dupload(h, &M.app_on_s, sc->app_on_s, A));
  TRY(dupload(h, &M.app_off_s, sc->app_off_s, A));
  {
    std::vector<uint32_t> cnt(A, 0), src(A, 0);
    std::vector<int64_t> ivl(A, 0);
    for (uint32_t a = 0; a < A; a++) {
      src[a] = sc->app_src_slot ? sc->app_src_slot[a] : 0xffffffffu;
      if (sc->app_kind[a] == NSGPU_APP_ECHO_CLIENT || sc->app_kind[a] == NSGPU_APP_UDP_CLIENT) {
        cnt[a] = sc->app_count[a];
        ivl[a] = sc->app_interval_ns[a];
      }
    }
    TRY(dupload(h, &M.app_count, cnt.data(), A));
    TRY(dupload(h, &M.app_interval, ivl.data(), A));
    TRY(dupload(h, &M.app_src_slot, src.data(), A));
  }
  TRY(dupload(h, &M.node_app_off, napps.data(), N + 1));
  TRY(dupload(h, &M.node_app_list, node_list.data(), A));
  const int32_t *sinkp;
  TRY(dupload(h, &sinkp, sink.data(), N));
  M.sink_of_node = sinkp;
  M.icmp = sc->icmp ? 1u : 0u;
  M.trace_kinds = 0xfu;
  // ---- state ----
  {  // the device records' reset image: tx state idle, the static parameters
    std::vector<DevRec> dr(D);
    for (uint32_t d = 0; d < D; d++) {
      DevRec r{};
      r.qmax = sc->dev_qmax[d];
      r.peer = sc->dev_peer[d];
      r.peer_node = sc->dev_node[sc->dev_peer[d]];
      r.rkind = K_RECEIVE | ((owner && owner[r.peer_node] != (uint32_t)rank) ? REMOTEBIT : 0u);
      r.bps = sc->dev_bps[d];
      r.ifg = sc->dev_ifg_ns[d];
      r.delay = sc->dev_delay_ns[d];
      r.em = P.dev_em[d];
      dr[d] = r;
    }
    // ... and behind them the receive error models: header, records, threshold tables, lists (em_is_corrupt)
    const uint32_t nm = (uint32_t)P.em_recs.size(), nt = (uint32_t)(P.em_tabs.size() / NSGPU_EM_TABLE_SIZE);
    h->dev_bytes = (size_t)D * sizeof(DevRec) + (nm ? em_bytes(nm, nt, P.em_list.size()) : 0);
    std::vector<uint8_t> img(h->dev_bytes ? h->dev_bytes : 1, 0);
    if (D) memcpy(img.data(), dr.data(), (size_t)D * sizeof(DevRec));
    if (nm) {
      uint8_t *q = img.data() + (size_t)D * sizeof(DevRec);
      const EmHdr eh{nm, nt, P.em_list.size()};
      memcpy(q, &eh, sizeof(eh));
      q += sizeof(eh);
      memcpy(q, P.em_recs.data(), (size_t)nm * sizeof(EmRec));
      q += (size_t)nm * sizeof(EmRec);
      if (nt) memcpy(q, P.em_tabs.data(), P.em_tabs.size() * sizeof(double));
      q += P.em_tabs.size() * sizeof(double);
      if (!P.em_list.empty()) memcpy(q, P.em_list.data(), P.em_list.size() * sizeof(uint32_t));
      M.errm = 1;
      h->em_models = nm;
    }
    const uint8_t *init;
    TRY(dupload(h, &init, img.data(), h->dev_bytes));
    h->dev_init = reinterpret_cast<const DevRec *>(init);
    uint8_t *devp;
    TRY(dalloc(h, &devp, h->dev_bytes));
    M.dev = reinterpret_cast<DevRec *>(devp);
  }
  TRY(dalloc(h, &M.q_buf, (size_t)D * qcap));
  TRY(dalloc(h, &M.app_flags, A));
  TRY(dalloc(h, &M.app_send_gen, A));
  TRY(dalloc(h, &M.app_ss_gen, A));
  TRY(dalloc(h, &M.app_residual, A));
  TRY(dalloc(h, &M.app_tot, (P.has_trace_client ? 3 : 1) * (size_t)A));  // (+ m_currentEntry, the Sends run)
  if (P.frag) {
    // behind the identifications: each node's FragNode index, the FragHdr, a FragNode for every node that is the
    // destination of a fragmenting flow (nsgpu_p2p_dev.h "IPv4 fragmentation"); kept as the reset image too
    std::vector<uint32_t> img((frag_hdr_off(N) + sizeof(FragHdr)) / 4, 0);
    uint32_t nf = 0;
    for (uint32_t n = 0; n < N; n++) img[N + n] = P.frag_flows[n] ? nf++ : NOFRAG;
    FragHdr fh{P.frag_timeout, nf, 0};
    memcpy(img.data() + frag_hdr_off(N) / 4, &fh, sizeof(fh));
    h->frag_words = img.size();
    h->frag_bytes = img.size() * 4 + (size_t)nf * sizeof(FragNode);
    h->frag_nf = nf;
    TRY(dupload(h, &h->frag_init, img.data(), img.size()));
    TRY(dalloc(h, &M.node_ipid, h->frag_bytes / 4));
    M.frag = 1;
  } else if (P.flowmon) {
    // behind the identifications: the FmHdr, the nodes' table bases and sizes, the flows' records and the tracked-
    // packet tables (nsgpu_p2p_dev.h "per-flow statistics"); header, bases and sizes are the reset image, the rest
    // starts as zeros
    std::vector<uint32_t> img(fm_rec_off(N) / 4, 0);
    uint64_t ne = 0;
    uint64_t *base = fm_node_base(img.data(), N);
    uint32_t *cap = fm_node_cap(img.data(), N);
    for (uint32_t n = 0; n < N; n++) {
      base[n] = ne;
      cap[n] = P.fm_cap[n];
      ne += P.fm_cap[n];
    }
    const FmHdr fh{2 * A, N, ne, {}};
    memcpy(reinterpret_cast<char *>(img.data()) + fm_hdr_off(N), &fh, sizeof(fh));
    h->frag_words = img.size();
    h->frag_bytes = fm_bytes(N, 2 * A, ne);
    h->fm_entries = ne;
    TRY(dupload(h, &h->frag_init, img.data(), img.size()));
    TRY(dalloc(h, &M.node_ipid, h->frag_bytes / 4));
    TRY(dalloc(h, &h->fm_lost, 2 * (size_t)A));
    M.flowmon = 1;
  } else {
    TRY(dalloc(h, &M.node_ipid, N));
  }
  if (!P.rv_recs.empty()) {
    // behind the last-start times: the RvHdr, the variables' records, the ambiguous log (nsgpu_p2p_dev.h "random OnOff
    // times"); kept as the reset image too
    h->rv_bytes = rv_bytes(A);
    std::vector<uint64_t> img(h->rv_bytes / 8, 0);
    memcpy(rv_recs(img.data(), A), P.rv_recs.data(), P.rv_recs.size() * sizeof(RvRec));
    TRY(dupload(h, &h->rv_init, img.data(), img.size()));
    TRY(dalloc(h, &M.app_last_start, img.size()));
    M.ranvar = 1;
  } else {
    TRY(dalloc(h, &M.app_last_start, A));
  }
  if (P.ports) {  // (the UdpServers' loss counters lie behind the counters: loss_counters)
    static_assert(sizeof(nsgpu_loss_counter) == 2 * sizeof(nsgpu_app_counters), "loss_counters");
    TRY(dalloc(h, &M.appc, 3 * (size_t)A));
    std::vector<nsgpu_loss_counter> lc(A);
    for (uint32_t a = 0; a < A; a++)
      nsgpu_loss_counter_init(&lc[a], sc->app_kind[a] == NSGPU_APP_UDP_SERVER ? sc->app_loss_window[a] : 8u);
    TRY(dupload(h, &h->loss_init, lc.data(), A));
  } else {
    TRY(dalloc(h, &M.appc, A));
  }
  TRY(dalloc(h, &M.node_tab, (size_t)N * NTAB));
  const std::vector<uint64_t> &its = P.its;
  const std::vector<uint32_t> &iuid = P.iuid, &ictx = P.ictx, &ikind = P.ikind, &ia = P.ia;
  const uint32_t uid = P.uid_init;
  const Red red0 = P.red0;
  M.n_init = P.n_init;
  M.uid_init = P.uid_init;
  M.pool_cap = P.pool_cap;
  for (int b = 0; b < 2; b++) {
    TRY(dalloc(h, &M.ev_ts[b], M.pool_cap));
    TRY(dalloc(h, &M.ev_uid[b], M.pool_cap));
    TRY(dalloc(h, &M.ev_ctx[b], M.pool_cap));
    TRY(dalloc(h, &M.ev_kind[b], M.pool_cap));
    TRY(dalloc(h, &M.ev_a[b], M.pool_cap));
    TRY(dalloc(h, &M.ev_pkt[b], M.pool_cap));
  }
  const size_t chn = (size_t)WTOT * M.maxc;  // children of gen-0 and local records
  TRY(dalloc(h, &M.ch_ts, chn));
  TRY(dalloc(h, &M.ch_ctx, chn));
  TRY(dalloc(h, &M.ch_kind, chn));
  TRY(dalloc(h, &M.ch_a, chn));
  TRY(dalloc(h, &M.ch_pkt, chn));
  // window records: a whole sorted run (single engine), a whole window before its cut (partitioned)
  M.fcap = (size_t)NMAX * M.maxc;  // children parked in one window: at most every record's
  M.runcap = M.pool_cap + M.fcap;
  if (M.runcap >= 0xffffffffull) {  // (so a window's slots and fcap each fit a half of the allocation word, Ctl::wnf)
    nsgpu_p2p_destroy(h);
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create: pool_cap too large for 32-bit slots");
  }
  TRY(dalloc(h, &M.wkey, M.runcap));
  TRY(dalloc(h, &M.wpkt, M.runcap));
  for (uint32_t **p : {&M.wctx, &M.wkind, &M.wa}) TRY(dalloc(h, p, M.runcap));
  TRY(dalloc(h, &M.pwkey, WTOT));
  TRY(dalloc(h, &M.sinfo, WTOT));
  TRY(dalloc(h, &M.widx, WCAP));
  for (uint32_t **p : {&M.nchild, &M.ninl, &M.pwctx, &M.wpar}) TRY(dalloc(h, p, WTOT));
  TRY(dalloc(h, &M.wrank, 2 * (size_t)WTOT));  // (by window parity)
  TRY(dalloc(h, &M.lcnt, NLR));
  TRY(dalloc(h, &M.lrec, NMAX));  // (k2_pa loads lrec[k] speculatively: zeroed, every entry stays < WTOT)
  TRY(dalloc(h, &M.lkey, LCAP));
  TRY(dalloc(h, &M.lkw, LCAP));
  TRY(dalloc(h, &M.ldat, LMAX));
  TRY(dalloc(h, &M.lrank, 2 * (size_t)LMAX));
  // deferred windows (single wide engine): staged records, their leaves, child prefixes, dense map
  if (M.wide) {
    TRY(dalloc(h, &M.stage, NMAX));
    TRY(dalloc(h, &M.sleaf, (size_t)NMAX * M.maxc));
    TRY(dalloc(h, &M.stx, NMAX));
    TRY(dalloc(h, &M.cpt, 2 * (size_t)NMAX));
    TRY(dalloc(h, &M.ldpd, LMAX));
  }
  // (k2_pa loads lrec / ldat entries speculatively and follows their record index: zeroed, every entry
  // stays < WTOT; the deferred pipeline's arrays start zeroed too, so a stale entry is always in range)
  bool zok = hipMemset(M.lrec, 0, NMAX * sizeof(uint32_t)) == hipSuccess &&
             hipMemset(M.lcnt, 0, NLR * sizeof(uint32_t)) == hipSuccess &&
             hipMemset(M.ldat, 0, LMAX * sizeof(uint4)) == hipSuccess;
  if (zok && M.wide)
    zok = hipMemset(M.stage, 0, (size_t)NMAX * sizeof(Stg)) == hipSuccess &&
          hipMemset(M.sleaf, 0, (size_t)NMAX * M.maxc * sizeof(uint2)) == hipSuccess &&
          hipMemset(M.stx, 0, (size_t)NMAX * sizeof(uint32_t)) == hipSuccess &&
          hipMemset(M.cpt, 0, 2 * (size_t)NMAX * sizeof(uint32_t)) == hipSuccess &&
          hipMemset(M.ldpd, 0, (size_t)LMAX * sizeof(uint32_t)) == hipSuccess;
  if (!zok) {
    nsgpu_p2p_destroy(h);
    return set_error(NSGPU_EHIP, "nsgpu_p2p_create: hipMemset failed");
  }
  // in-place pool, fresh buffer, free stack, hub blocks, compaction; radix sort scratch (single engine)
  TRY(dalloc(h, &M.wsrc, M.runcap));
  TRY(dalloc(h, &M.f_ts, M.fcap));
  for (uint32_t **p : {&M.f_uid, &M.f_ctx, &M.f_kind, &M.f_a}) TRY(dalloc(h, p, M.fcap));
  TRY(dalloc(h, &M.f_pkt, M.fcap));
  TRY(dalloc(h, &M.fstack, M.pool_cap));
  TRY(dalloc(h, &M.hub_list, MAXHUB));
  TRY(dalloc(h, &M.hx, WCAP));
  TRY(dalloc(h, &M.hub_key, (size_t)NHUB * WCAP));
  TRY(dalloc(h, &M.hub_slot, (size_t)(NHUB + 1) * WCAP));  // (+ hub_mark's WCAP)
  TRY(dalloc(h, &M.cmp_cnt, 1));
  {  // radix sort scratch: the single engine's sorted runs, a partitioned rank's run (sorted once per run)
    TRY(dalloc(h, &M.s_key2, M.runcap));
    for (uint32_t **p : {&M.s_val, &M.s_val2}) TRY(dalloc(h, p, M.runcap));
    TRY(dalloc(h, &M.s_hist, 256 * ((M.runcap + RS_TILE - 1) / RS_TILE)));
    if (!owner) {  // (the single engine gathers in place through these; a partitioned rank into rn_*)
      TRY(dalloc(h, &M.g_u32, M.runcap));
      TRY(dalloc(h, &M.g_pkt, M.runcap));
    }
  }
  if (owner) {
    TRY(dalloc(h, &M.rn_key, M.runcap));
    for (uint32_t **p : {&M.rn_ctx, &M.rn_kind, &M.rn_a, &M.rn_src}) TRY(dalloc(h, p, M.runcap));
    TRY(dalloc(h, &M.rn_pkt, M.runcap));
    M.dist = 1;
    M.rank = (uint32_t)rank;
    M.nranks = (uint32_t)nranks;
    TRY(dupload(h, &M.owner, owner, N));
    TRY(dalloc(h, &M.x0_recv, 2 * (size_t)nranks));
    TRY(dalloc(h, &M.xk_send, 2));
    TRY(dalloc(h, &M.xk_recv, 2 * (size_t)nranks));
    TRY(dalloc(h, &M.x1_recv, X1B * nranks));
    TRY(dalloc(h, &M.x1_own, X1OWN));
    M.x1_send = M.x1_recv + (size_t)rank * X1B;  // (in place: NCCL moves only the other ranks' slots)
    if ((uint64_t)nranks * WCAP * M.maxc >= (1ull << 32))  // (k_gtile's packed child prefix)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_create_dist: %d ranks x %u children per event", nranks, M.maxc);
    M.capx = P.capx;
    M.x2b = P.x2b;
    TRY(dalloc(h, &M.x2_send, M.x2b * nranks));
    TRY(dalloc(h, &M.x2_recv, M.x2b * nranks));
    TRY(dalloc(h, &M.gacc, 4 * (size_t)NACC));
    h->comm = comm;
    memset(&h->x1h0, 0, sizeof(X1Hdr));
    h->x1h0.red.tmin = h->x1h0.red.wend = h->x1h0.red.stopts = h->x1h0.red.wendw = ~0ull;
    h->x1h0.rkey = ~0ull;
  }
  {  // the run control, and behind it the deferred pipeline's partial records (Part), empty
    uint8_t *cb;
    TRY(dalloc(h, &cb, CTL_MDEV_OFF + sizeof(P2PDev)));  // (... and behind those the descriptor's copy: mdev_sync)
    M.C = reinterpret_cast<Ctl *>(cb);
    hipLaunchKernelGGL(k_part_clear, dim3((NPARTS + 255) / 256), dim3(256), 0, nullptr, M.C);
    NSGPU_HIP(hipGetLastError());
    NSGPU_HIP(hipDeviceSynchronize());
  }
  if (owner) M.x0_send = reinterpret_cast<uint64_t *>(&M.C->W);  // X0 sends (W, nxtP, overflow, prep)
  if (owner && nranks == 1) {  // one rank: its exchanges are its own payloads in place (no copies in the window)
    M.x0_recv = M.x0_send;
    M.x2_recv = M.x2_send;  // (with one rank no child is remote: X2 stays empty)
  }
  TRY(dalloc(h, &M.error, 4));
  M.log_cap = log_cap;
  TRY(dalloc(h, &M.log_ts, log_cap));
  TRY(dalloc(h, &M.log_uid, log_cap));
  TRY(dalloc(h, &M.log_ctx, log_cap));
  const uint64_t *c_ts;
  const uint32_t *c_uid, *c_ctx, *c_kind, *c_a;
  TRY(dupload(h, &c_ts, its.data(), its.size()));
  TRY(dupload(h, &c_uid, iuid.data(), iuid.size()));
  TRY(dupload(h, &c_ctx, ictx.data(), ictx.size()));
  TRY(dupload(h, &c_kind, ikind.data(), ikind.size()));
  TRY(dupload(h, &c_a, ia.data(), ia.size()));
  h->init_ts = (uint64_t *)c_ts;
  h->init_uid = (uint32_t *)c_uid;
  h->init_ctx = (uint32_t *)c_ctx;
  h->init_kind = (uint32_t *)c_kind;
  h->init_a = (uint32_t *)c_a;
  // run control after reset
  Ctl &C0 = h->C0;
  memset(&C0, 0, sizeof(C0));
  C0.uid = uid;
  // reduction of the initial pool: window 0 is bounded by red[1] (k2_pa / k2_handle fold later
  // pending sets in for the next windows)
  C0.red[0].tmin = C0.red[0].wend = C0.red[0].stopts = C0.red[0].wendw = ~0ull;
  C0.red[0].stopuid = 0;
  C0.red[1] = red0;
  C0.max_windows = h->max_windows;
  C0.done = red0.tmin == ~0ull ? 2 : 0;  // (no event anywhere)
  C0.P_end = C0.live = M.n_init;  // single engine: the in-place pool starts as the setup events
  C0.hts = ~0ull;                 // no host closure pending (nsgpu_p2p_advance sets one)
  C0.hrel = ~0ull;
  C0.rt = 0;                      // window 0 is bounded by red[1] and folds into red[0]
  C0.span_t = ~0ull >> 2;         // wide windows start at their widest (adapted to the capacity)
  if (hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking) != hipSuccess) {
    h->s = nullptr;
    nsgpu_p2p_destroy(h);
    return set_error(NSGPU_EHIP, "nsgpu_p2p_create: hipStreamCreate failed");
  }
  for (hipEvent_t *e : {&h->ev[0], &h->ev[1]})
    if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
      *e = nullptr;
      nsgpu_p2p_destroy(h);
      return set_error(NSGPU_EHIP, "nsgpu_p2p_create: hipEventCreate failed");
    }
  for (hipEvent_t *e : {&h->t0, &h->t1})
    if (hipEventCreate(e) != hipSuccess) {
      *e = nullptr;
      nsgpu_p2p_destroy(h);
      return set_error(NSGPU_EHIP, "nsgpu_p2p_create: hipEventCreate failed");
    }
  if (hipHostMalloc((void **)&h->snap, 2 * sizeof(Ctl), hipHostMallocDefault) != hipSuccess) {
    h->snap = nullptr;
    nsgpu_p2p_destroy(h);
    return set_error(NSGPU_ENOMEM, "nsgpu_p2p_create: hipHostMalloc failed");
  }
  if (const int rc = mdev_sync(h)) {
    nsgpu_p2p_destroy(h);
    return rc;
  }
  *out = h;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_create(const nsgpu_p2p_scenario *sc, uint64_t pool_cap, uint64_t log_cap,
                                nsgpu_p2p **out) {
  return create_engine(sc, nullptr, nullptr, 0, 1, nullptr, pool_cap, log_cap, out);
}
extern "C" int nsgpu_p2p_create_ex(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext, uint64_t pool_cap,
                                   uint64_t log_cap, nsgpu_p2p **out) {
  return create_engine(sc, ext, nullptr, 0, 1, nullptr, pool_cap, log_cap, out);
}

extern "C" int nsgpu_p2p_create_dist(const nsgpu_p2p_scenario *sc, const uint32_t *node_owner, int rank,
                                     int nranks, nsgpu_comm *comm, uint64_t pool_cap, uint64_t log_cap,
                                     nsgpu_p2p **out) {
  return nsgpu_p2p_create_dist_ex(sc, nullptr, node_owner, rank, nranks, comm, pool_cap, log_cap, out);
}
extern "C" int nsgpu_p2p_create_dist_ex(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext,
                                        const uint32_t *node_owner, int rank, int nranks, nsgpu_comm *comm,
                                        uint64_t pool_cap, uint64_t log_cap, nsgpu_p2p **out) {
  if (!node_owner) return set_error(NSGPU_EINVAL, "nsgpu_p2p_create_dist: null owner map");
  if (comm && (comm->nranks != nranks || comm->rank != rank))
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_create_dist: communicator is rank %d of %d", comm->rank, comm->nranks);
  return create_engine(sc, ext, node_owner, rank, nranks, comm, pool_cap, log_cap, out);
}

extern "C" int nsgpu_p2p_dist_plan(const nsgpu_p2p_scenario *sc, const uint32_t *node_owner, int rank, int nranks,
                                   uint64_t pool_cap, nsgpu_p2p_plan *out) {
  return nsgpu_p2p_dist_plan_ex(sc, nullptr, node_owner, rank, nranks, pool_cap, out);
}
extern "C" int nsgpu_p2p_dist_plan_ex(const nsgpu_p2p_scenario *sc, const nsgpu_p2p_scenario_ext *ext,
                                      const uint32_t *node_owner, int rank, int nranks, uint64_t pool_cap,
                                      nsgpu_p2p_plan *out) {
  if (!sc || !out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_dist_plan: null");
  static_assert(K_NKINDS <= 16, "nsgpu_p2p_plan holds 16 kinds");
  EnginePlan P;
  if (int rc = plan_engine(sc, ext, node_owner, rank, nranks, pool_cap, P)) return rc;
  memset(out, 0, sizeof(*out));
  out->wide = P.wide;
  out->maxc = P.maxc;
  out->wcap = WCAP;
  out->xlcap = XLCAP;
  if (node_owner) {
    out->x0_bytes = X0B;
    out->x1_bytes = X1B;
    out->x2_bytes = P.x2b;
    out->x2_records = P.capx;
  }
  out->n_kinds = K_NKINDS;
  for (int k = 0; k < K_NKINDS; k++) out->lookahead[k] = P.lookahead[k], out->lookw[k] = P.lookw[k];
  out->tx_min = P.tx_min;
  out->lx = P.lx;
  out->red0_tmin = P.red0.tmin;
  out->red0_wend = P.red0.wend;
  out->red0_wendw = P.red0.wendw;
  out->stop_ts = P.red0.stopts;
  out->stop_uid = P.red0.stopuid;
  out->uid_init = P.uid_init;
  out->n_init = P.n_init;
  out->pool_cap = P.pool_cap;
  return NSGPU_OK;
}

// Restores the initial (post-setup) state on the device, asynchronously.
extern "C" int nsgpu_p2p_reset(nsgpu_p2p *h, void *stream) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_reset: null");
  hipStream_t s = (hipStream_t)stream;
  P2PDev &M = h->M;
  const uint32_t A = M.n_apps, n0 = M.n_init;
  NSGPU_HIP(hipMemcpyAsync(M.ev_ts[0], h->init_ts, n0 * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemcpyAsync(M.ev_uid[0], h->init_uid, n0 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemcpyAsync(M.ev_ctx[0], h->init_ctx, n0 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemcpyAsync(M.ev_kind[0], h->init_kind, n0 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemcpyAsync(M.ev_a[0], h->init_a, n0 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemcpyAsync(M.dev, h->dev_init, h->dev_bytes, hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemsetAsync(M.app_flags, 0, A * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.app_send_gen, 0, A * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.app_ss_gen, 0, A * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.app_residual, 0, A * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.app_tot, 0, (h->has_trace_client ? 3 : 1) * (size_t)A * sizeof(uint32_t), s));
  // (the identifications, the FragNode indices and header, empty FragNodes; a monitored engine: the tables' bases
  // and sizes, empty flow records and tracked-packet tables)
  if (M.frag || M.flowmon) {
    NSGPU_HIP(hipMemsetAsync(M.node_ipid, 0, h->frag_bytes, s));
    NSGPU_HIP(hipMemcpyAsync(M.node_ipid, h->frag_init, h->frag_words * 4, hipMemcpyDeviceToDevice, s));
  } else {
    NSGPU_HIP(hipMemsetAsync(M.node_ipid, 0, M.n_nodes * sizeof(uint32_t), s));
  }
  if (M.trace) NSGPU_HIP(hipMemsetAsync(M.trace_n, 0, sizeof(unsigned long long), s));
  if (h->rv_init) NSGPU_HIP(hipMemcpyAsync(M.app_last_start, h->rv_init, h->rv_bytes, hipMemcpyDeviceToDevice, s));
  else NSGPU_HIP(hipMemsetAsync(M.app_last_start, 0, A * sizeof(uint64_t), s));
  NSGPU_HIP(hipMemsetAsync(M.appc, 0, A * sizeof(nsgpu_app_counters), s));
  if (h->loss_init)
    NSGPU_HIP(hipMemcpyAsync(loss_counters(M.appc, A), h->loss_init, A * sizeof(nsgpu_loss_counter),
                             hipMemcpyDeviceToDevice, s));
  NSGPU_HIP(hipMemsetAsync(M.node_tab, 0, (size_t)M.n_nodes * NTAB * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.wrank, 0, 2 * WTOT * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.lrank, 0, 2 * LMAX * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.lcnt, 0, NLR * sizeof(uint32_t), s));
  NSGPU_HIP(hipMemsetAsync(M.error, 0, 4 * sizeof(uint32_t), s));
  if (M.dist) {
    const size_t R = M.nranks;
    if (M.x0_recv != M.x0_send) NSGPU_HIP(hipMemsetAsync(M.x0_recv, 0, X0B * R, s));
    NSGPU_HIP(hipMemsetAsync(M.xk_send, 0, 16, s));
    NSGPU_HIP(hipMemsetAsync(M.xk_recv, 0, 16 * R, s));
    NSGPU_HIP(hipMemsetAsync(M.x1_recv, 0, X1B * R, s));
    NSGPU_HIP(hipMemsetAsync(M.x1_own, 0, X1OWN, s));
    NSGPU_HIP(hipMemcpyAsync(M.x1_send, &h->x1h0, sizeof(X1Hdr), hipMemcpyHostToDevice, s));  // (its own slot)
    NSGPU_HIP(hipMemsetAsync(M.x2_send, 0, M.x2b * R, s));
    if (M.x2_recv != M.x2_send) NSGPU_HIP(hipMemsetAsync(M.x2_recv, 0, M.x2b * R, s));
    NSGPU_HIP(hipMemsetAsync(M.gacc, 0, 4 * NACC * sizeof(uint32_t), s));
  }
  if (M.log_cap) {  // (partitioned: every rank writes only the entries it dispatches, the union is the log;
                    //  mixed runs: the ranks of host dispatches stay unwritten)
    NSGPU_HIP(hipMemsetAsync(M.log_ts, 0, M.log_cap * 8, s));
    NSGPU_HIP(hipMemsetAsync(M.log_uid, 0, M.log_cap * 4, s));
    NSGPU_HIP(hipMemsetAsync(M.log_ctx, 0, M.log_cap * 4, s));
  }
  NSGPU_HIP(hipMemcpyAsync(M.C, &h->C0, sizeof(Ctl), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_part_clear, dim3((NPARTS + 255) / 256), dim3(256), 0, s, M.C);  // (a run that failed may leave some)
  NSGPU_HIP(hipGetLastError());
  h->uid_hint = h->C0.uid;
  return NSGPU_OK;
}

// The window pipeline, in launch order (graph capture, eager runs and the per-kernel profile).
namespace {
constexpr int NKERN = 5;
const char *const KERNEL_NAMES[NKERN] = {"k2_pa", "k2_handle", "k2_rank", "k2_scan", "k_tpatch"};
// ev0 / ev1: optional HIP events the command processor records at the kernel's start and end
// (hipExtLaunchKernelGGL: no separate marker packets between the pipeline's kernels).
// Kernel k of the single engine's window (KERNEL_NAMES); a wide engine places its local records after
// its handlers (k2_rank) and, traced, patches their trace uids (k_tpatch).  Returns
// whether kernel k is part of this engine's window.
#define NSGPU_KLAUNCH(K, G, B, S, E0, E1, ...) hipExtLaunchKernelGGL(K, G, B, 0, S, E0, E1, 0, __VA_ARGS__)
bool launch_kernel(nsgpu_p2p *h, int k, hipStream_t s, bool df, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  const bool wide = h->M.wide != 0;
  switch (k) {
    case 0:
      if (df) NSGPU_KLAUNCH((k2_pa<false, true, true>), dim3(pa_grid_rt<true>(h->M)), dim3(TB), s, ev0, ev1, h->M);
      else if (wide) NSGPU_KLAUNCH((k2_pa<false, true>), dim3(pa_grid_rt<true>(h->M)), dim3(TB), s, ev0, ev1, h->M);
      else NSGPU_KLAUNCH((k2_pa<false, false>), dim3(pa_grid_rt<false>(h->M)), dim3(TB), s, ev0, ev1, h->M);
      return true;
    case 1:
      // (a scenario with ports, frag, a receive error model or per-flow statistics: the extended handlers — the
      // endpoint lookup, UdpClient, UdpServer, IPv4 fragmentation and reassembly, the error models, the flow monitor —
      // nsgpu_p2p_ports.hip)
      if (h->loss_init || h->M.frag || h->M.errm || h->M.flowmon || h->M.ranvar) launch_handle_ports(h->M, wide, false, df, K2_GRID, s, ev0, ev1);
      else if (df) NSGPU_KLAUNCH((k2_handle<true, false, true>), dim3(K2_GRID), dim3(HB), s, ev0, ev1, h->M);
      else if (wide) NSGPU_KLAUNCH(k2_handle<true>, dim3(K2_GRID), dim3(HB), s, ev0, ev1, h->M);
      else NSGPU_KLAUNCH(k2_handle<false>, dim3(K2_GRID), dim3(HB), s, ev0, ev1, h->M);
      return true;
    case 2:
      if (!wide) return false;
      if (df) NSGPU_KLAUNCH(k2_rank<true>, dim3(RK_GRID_DF), dim3(RKT_DF), s, ev0, ev1, h->M);
      else NSGPU_KLAUNCH(k2_rank<false>, dim3(RK_GRID), dim3(RKT), s, ev0, ev1, h->M);
      return true;
    case 3:
      if (df) return false;  // (the deferred pipeline: df_book and the accounting (df_sdef) in k2_rank)
      if (wide) NSGPU_KLAUNCH(k2_scan<true>, dim3(1), dim3(SCAN_THREADS), s, ev0, ev1, h->M);
      else NSGPU_KLAUNCH(k2_scan<false>, dim3(1), dim3(SCAN_THREADS), s, ev0, ev1, h->M);
      return true;
    default:
      if (!(wide && h->M.trace)) return false;
      NSGPU_KLAUNCH(k_tpatch, dim3(64), dim3(256), s, ev0, ev1, h->M);
      return true;
  }
}
#ifdef NSGPU_PHASE_PROF
// The invariant checker (diagnostic build only).  Eager launches with NSGPU_P2P_DEBUG=1: after every kernel
// the stream is drained (a fault is reported with the kernel and window that raised it) and k_dbg checks the
// engine's invariants (pool, free stack, fresh buffer, window records, children), so that a broken state is
// reported by the kernel that made it instead of faulting a later one.
// In graph mode (NSGPU_P2P_DEBUG=2) k_dbg runs after every kernel of the replay (`at`: window << 8 | kernel)
// and a broken invariant also ends the run (done = 2, error 1024) so that the next kernels do nothing.
// k: the pipeline kernel that ran last (KERNEL_NAMES).
__global__ __launch_bounds__(256) void k_dbg(const P2PDev M, unsigned long long *out, unsigned long long at = 0,
                                             int k = -1) {
  Ctl &C = *M.C;
  const uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x, st = (uint64_t)gridDim.x * 256;
  if (at && out[0]) return;  // (graph mode: the first violation is kept)
  auto bad = [&](unsigned long long code, unsigned long long a, unsigned long long b) {
    if (atomicCAS(&out[0], 0ull, code) == 0ull) {
      out[1] = a;
      out[2] = b;
      out[3] = at | ((unsigned long long)C.windows << 32);
      if (at) {
        atomicOr(M.error, 1024u);
        C.done = 2;
      }
    }
  };
  // (the deferred pipeline counts the forming window in wnf, the other one in W / nF: the idle pair is 0)
  const uint64_t Pe = C.P_end, nfree = C.nfree, nF = C.nF + (C.wnf >> 32), W = C.W + (uint32_t)C.wnf;
  if (i0 == 0) {
    if (Pe > M.pool_cap) bad(1, Pe, M.pool_cap);
    if (nfree + C.npush > M.pool_cap) bad(2, nfree, C.npush);
    if (C.live > Pe + nF) bad(3, C.live, Pe);
    if (nF > M.fcap) bad(4, nF, M.fcap);
    if (W > M.runcap) bad(5, W, M.runcap);
  }
  // the deferred pipeline's partial records are empty once k2_rank has run (the other pipeline stores none)
  if (k == 2 && i0 < (uint64_t)NPARTS) {
    const Part q = *part_rec(&C, (uint32_t)i0);
    if ((q.tmin & q.wend & q.wendw) != ~0ull || q.tot) bad(50, i0, q.tmin);
  }
  const uint64_t P = Pe < M.pool_cap ? Pe : M.pool_cap;
  for (uint64_t p = i0; p < P; p += st)
    if (M.ev_ts[0][p] != TOMB && ((M.ev_ctx[0][p] >= M.n_nodes && M.ev_ctx[0][p] != ~0u) ||
                                  (M.ev_kind[0][p] & 0xffu) >= (uint32_t)K_NKINDS))
      bad(10, p, M.ev_ctx[0][p]);
  const uint64_t F = nF < M.fcap ? nF : M.fcap;
  for (uint64_t f = i0; f < F; f += st)
    if (M.f_ctx[f] >= M.n_nodes && M.f_ctx[f] != ~0u) bad(30, f, M.f_ctx[f]);
  const uint64_t NF = nfree < M.pool_cap ? nfree : M.pool_cap;
  for (uint64_t j = i0; j < NF; j += st)
    if (M.fstack[j] >= P) bad(40, j, M.fstack[j]);
  const uint64_t Wm = W < (uint64_t)WCAP ? W : (uint64_t)WCAP;
  if (C.mode != MODE_RUN)
    for (uint64_t s = i0; s < Wm; s += st) {
      if (M.wctx[s] >= M.n_nodes && M.wctx[s] != ~0u) bad(20, s, M.wctx[s]);
      if (M.nchild[s] > M.maxc) bad(21, s, M.nchild[s]);
    }
}
unsigned long long *g_dbg_out = nullptr;
int dbg_alloc() {  // (before any capture)
  if (!g_dbg_out) {
    NSGPU_HIP(hipMalloc(&g_dbg_out, 4 * sizeof(unsigned long long)));
    NSGPU_HIP(hipMemset(g_dbg_out, 0, 4 * sizeof(unsigned long long)));
  }
  return NSGPU_OK;
}
int launch_windows_dbg(nsgpu_p2p *h, hipStream_t s, bool df) {
  if (const int rd = dbg_alloc()) return rd;
  unsigned long long *dout = g_dbg_out;
  if (!h->eager) {  // graph capture: checks as graph nodes
    for (int w = 0; w < NWIN; w++)
      for (int k = 0; k < NKERN; k++)
        if (launch_kernel(h, k, s, df)) hipLaunchKernelGGL(k_dbg, dim3(256), dim3(256), 0, s, h->M, dout, (unsigned long long)(w << 8 | k | 0x80000000u), k);
    return NSGPU_OK;
  }
  static int lines = 0;
  static const bool trace_c = getenv("NSGPU_P2P_DEBUG_TRACE") != nullptr;
  for (int w = 0; w < NWIN; w++) {
    Ctl c{};
    NSGPU_HIP(hipMemcpyAsync(&c, h->M.C, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipStreamSynchronize(s));
    if (trace_c && (lines < 400 || c.windows % 10000 == 0) && lines < 2000) {
      lines++;
      fprintf(stderr, "[p2p dbg] df %d win %llu mode %u done %u live %llu P_end %llu nfree %llu pvalid %u pchild %llu "
              "hts %llu hcap %u tmin %llu W %u K %llu uid %u stop %u\n", (int)df, (unsigned long long)c.windows, c.mode,
              c.done, (unsigned long long)c.live, (unsigned long long)c.P_end, (unsigned long long)c.nfree, c.pvalid,
              (unsigned long long)c.pchild, (unsigned long long)c.hts, c.hcap, (unsigned long long)c.tmin, c.W,
              (unsigned long long)c.K, c.uid, c.stop_seen);
    }
    for (int k = 0; k < NKERN; k++) {
      if (!launch_kernel(h, k, s, df)) continue;
      hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess)
        return set_error(NSGPU_EHIP, "nsgpu_p2p debug: %s faulted in window %llu (df %d, mode %u): %s", KERNEL_NAMES[k],
                         (unsigned long long)c.windows, (int)df, c.mode, hipGetErrorString(e));
      NSGPU_HIP(hipMemsetAsync(dout, 0, 4 * sizeof(unsigned long long), s));
      hipLaunchKernelGGL(k_dbg, dim3(256), dim3(256), 0, s, h->M, dout, 0ull, k);
      unsigned long long o[4] = {};
      NSGPU_HIP(hipMemcpyAsync(o, dout, sizeof(o), hipMemcpyDeviceToHost, s));
      NSGPU_HIP(hipStreamSynchronize(s));
      if (o[0])
        return set_error(NSGPU_EHIP, "nsgpu_p2p debug: invariant %llu broken after %s in window %llu (df %d, mode %u): "
                         "%llu %llu", o[0], KERNEL_NAMES[k], (unsigned long long)c.windows, (int)df, c.mode, o[1], o[2]);
    }
  }
  return NSGPU_OK;
}
#endif
int launch_windows(nsgpu_p2p *h, hipStream_t s, bool df, int nwin = NWIN) {
#ifdef NSGPU_PHASE_PROF
  static const int dbg = [] {
    const char *e = getenv("NSGPU_P2P_DEBUG");
    return e ? atoi(e) : 0;
  }();
  if ((dbg == 1 && h->eager) || (dbg == 2 && !h->eager)) return launch_windows_dbg(h, s, df);
#endif
  for (int w = 0; w < nwin; w++)
    for (int k = 0; k < NKERN; k++) launch_kernel(h, k, s, df);
  return NSGPU_OK;
}
// The deferred pipeline is used for untraced single wide engines.  (Not for a monitored one: a flow's first
// transmission records the uid of the event being run, which that pipeline's handlers know only provisionally.)
bool df_usable(const nsgpu_p2p *h) {
  return h->M.wide && !h->M.dist && !h->M.trace && !h->M.flowmon && h->M.maxc <= PROV_MAXC && h->M.n_nodes < (1u << 24);
}
// When the deferred pipeline paused itself (a sorted run, a compaction, a host closure) after window n's
// bookkeeping: window n's dispatch accounting from its records (k2_scan<true, true>: sinfo for the next
// k2_pa), and every provisional uid still pending resolved (k_xlate); the other pipeline can take over.
int df_flush(nsgpu_p2p *h, hipStream_t s) {
  hipLaunchKernelGGL((k2_scan<true, true>), dim3(1), dim3(SCAN_THREADS), 0, s, h->M);
  hipLaunchKernelGGL(k_xlate, dim3(1024), dim3(256), 0, s, h->M);
  NSGPU_HIP(hipGetLastError());
  return NSGPU_OK;
}
}  // namespace

// LSD radix sort of the n window keys (M.wkey) on stream s, 8 bits a pass over the bits the keys use (k_rs_or:
// drains the stream once to read them).  The passes write ka and kb in turn: ka first, or with `land` whichever
// makes the last pass write ka.  *key: the buffer the sorted keys are in; *perm: the window record each came from
// (null if no pass made one) — the caller gathers its records through it.
static int radix_sort(const P2PDev &M, uint64_t n, uint64_t *ka, uint64_t *kb, bool land, hipStream_t s,
                      const uint64_t **key, const uint32_t **perm) {
  NSGPU_HIP(hipMemsetAsync(M.cmp_cnt, 0, sizeof(uint64_t), s));
  hipLaunchKernelGGL(k_rs_or, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 2048)), dim3(256), 0, s, M.wkey, n,
                     (unsigned long long *)M.cmp_cnt);
  uint64_t kor = 0;
  NSGPU_HIP(hipMemcpyAsync(&kor, M.cmp_cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  const int bits = kor ? 64 - __builtin_clzll(kor) : 1;
  const int passes = (bits + 7) / 8;
  const uint32_t ntiles = (uint32_t)((n + RS_TILE - 1) / RS_TILE);
  if (land && !(passes & 1)) std::swap(ka, kb);
  const uint64_t *kin = M.wkey;
  uint64_t *kout = ka;
  uint32_t *vin = nullptr, *vout = M.s_val;
  for (int p = 0; p < passes; p++) {
    hipLaunchKernelGGL(k_rs_hist, dim3(ntiles), dim3(RS_T), 0, s, kin, n, 8 * p, M.s_hist, ntiles);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, M.s_hist, (uint64_t)256 * ntiles);
    hipLaunchKernelGGL(k_rs_scatter, dim3(ntiles), dim3(RS_T), 0, s, kin, vin, kout, vout, n, 8 * p, M.s_hist,
                       ntiles);
    kin = kout;
    kout = kout == ka ? kb : ka;
    vin = vout;
    vout = vin == M.s_val ? M.s_val2 : M.s_val;
  }
  *key = kin;
  *perm = vin;
  return NSGPU_OK;
}

// The host-driven steps of the single engine (rare; on the engine stream, after the pipeline has
// paused itself): the radix sort that turns an overflowing window into a sorted run, and the pool
// compaction.  `c` is the run control the pause left.
static int host_step(nsgpu_p2p *h, const Ctl &c, hipStream_t s) {
  const P2PDev &M = h->M;
  if (c.mode == MODE_SORT) {  // in place: the passes alternate between the scratch keys and the window's own
    const uint64_t n = c.rW;
    const uint64_t *kin;
    const uint32_t *vin;
    if (const int rc = radix_sort(M, n, M.s_key2, M.wkey, false, s, &kin, &vin)) return rc;
    if (kin != M.wkey) NSGPU_HIP(hipMemcpyAsync(M.wkey, kin, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if (vin) {
      const uint32_t gg = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192);
      for (uint32_t *a : {M.wctx, M.wkind, M.wa}) {
        hipLaunchKernelGGL(k_rs_gather<uint32_t>, dim3(gg), dim3(256), 0, s, vin, a, M.g_u32, n);
        NSGPU_HIP(hipMemcpyAsync(a, M.g_u32, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
      }
      hipLaunchKernelGGL(k_rs_gather<Pkt>, dim3(gg), dim3(256), 0, s, vin, M.wpkt, M.g_pkt, n);
      NSGPU_HIP(hipMemcpyAsync(M.wpkt, M.g_pkt, n * sizeof(Pkt), hipMemcpyDeviceToDevice, s));
    }
    if (c.renarrow) hipLaunchKernelGGL(k_renarrow, dim3(1), dim3(1024), 0, s, M);  // (a widened window)
    hipLaunchKernelGGL(k_after_sort, dim3(1), dim3(1024), 0, s, M);
    NSGPU_HIP(hipGetLastError());
  } else if (c.mode == MODE_UIDX) {  // (the deferred pipeline handed over: nothing to do on the host)
    hipLaunchKernelGGL(k_after_uidx, dim3(1), dim3(1), 0, s, M);
    NSGPU_HIP(hipGetLastError());
  } else if (c.mode == MODE_TRIM) {  // a run ends after a cut same-ts group: the rest goes back to the pool
    hipLaunchKernelGGL(k_trim, dim3(1), dim3(1024), 0, s, M);
    NSGPU_HIP(hipGetLastError());
  } else if (c.mode == MODE_COMPACT) {
    NSGPU_HIP(hipMemsetAsync(M.cmp_cnt, 0, sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_cmp, dim3(1024), dim3(256), 0, s, M, c.P_end);
    NSGPU_HIP(hipGetLastError());
    uint64_t live = 0;
    NSGPU_HIP(hipMemcpyAsync(&live, M.cmp_cnt, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipStreamSynchronize(s));
    if (live != c.live) return set_error(NSGPU_EHIP, "nsgpu_p2p: compaction found %llu live events, expected %llu",
                                          (unsigned long long)live, (unsigned long long)c.live);
    NSGPU_HIP(hipMemcpyAsync(M.ev_ts[0], M.ev_ts[1], live * 8, hipMemcpyDeviceToDevice, s));
    NSGPU_HIP(hipMemcpyAsync(M.ev_uid[0], M.ev_uid[1], live * 4, hipMemcpyDeviceToDevice, s));
    NSGPU_HIP(hipMemcpyAsync(M.ev_ctx[0], M.ev_ctx[1], live * 4, hipMemcpyDeviceToDevice, s));
    NSGPU_HIP(hipMemcpyAsync(M.ev_kind[0], M.ev_kind[1], live * 4, hipMemcpyDeviceToDevice, s));
    NSGPU_HIP(hipMemcpyAsync(M.ev_a[0], M.ev_a[1], live * 4, hipMemcpyDeviceToDevice, s));
    NSGPU_HIP(hipMemcpyAsync(M.ev_pkt[0], M.ev_pkt[1], live * sizeof(Pkt), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_after_compact, dim3(1), dim3(1), 0, s, M, live);
    NSGPU_HIP(hipGetLastError());
  }
  return NSGPU_OK;
}

// The exchanges of a partitioned window.  A one-rank job has nothing to exchange: its "all-gather" and
// "all-to-all" are a device copy of its own slot (no RCCL call, so the window graph is all kernels and copies).
static int x_allgather(nsgpu_p2p *h, const void *send, void *recv, size_t bytes, hipStream_t s) {
  if (h->M.nranks == 1) {
    if (send != recv) NSGPU_HIP(hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, s));
    return NSGPU_OK;
  }
  NCCL_TRY(ncclAllGather(send, recv, bytes, ncclUint8, h->comm->comm, s));
  return NSGPU_OK;
}
static int x_alltoall(nsgpu_p2p *h, const void *send, void *recv, size_t bytes, hipStream_t s) {
  if (h->M.nranks == 1) {
    if (send != recv && bytes) NSGPU_HIP(hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, s));
    return NSGPU_OK;
  }
  NCCL_TRY(ncclAllToAll(send, recv, bytes, ncclUint8, h->comm->comm, s));
  return NSGPU_OK;
}

// The partitioned window's kernels (narrow, or wide: local records ranked across the ranks through X1Loc).
static void dist_pa(const P2PDev &M, hipStream_t s) {
  if (M.wide) hipLaunchKernelGGL((k2_pa<true, true>), dim3(GRID_POOL_DIST), dim3(TB), 0, s, M);
  else hipLaunchKernelGGL((k2_pa<true, false>), dim3(GRID_POOL_DIST), dim3(TB), 0, s, M);
}
static void dist_handle(const P2PDev &M, hipStream_t s, bool ports) {
  if (M.wide) {
    if (ports) launch_handle_ports(M, true, true, false, K2_GRID_W, s, nullptr, nullptr);
    else hipLaunchKernelGGL((k2_handle<true, true>), dim3(K2_GRID_W), dim3(HB), 0, s, M);
    hipLaunchKernelGGL(k_xlcompact, dim3(NLR), dim3(HB), 0, s, M);
  }
  else if (ports) launch_handle_ports(M, false, false, false, K2_GRID, s, nullptr, nullptr);
  else hipLaunchKernelGGL(k2_handle<false>, dim3(K2_GRID), dim3(HB), 0, s, M);
}
// Before the X1 exchange: this rank's records ranked among themselves and, with more ranks, sorted into its X1.
static void dist_rank(const P2PDev &M, hipStream_t s) {
  if (M.wide) hipLaunchKernelGGL(k_gtile<true>, dim3(GTB), dim3(HB), 0, s, M);
  else hipLaunchKernelGGL(k_gtile<false>, dim3(GTB), dim3(HB), 0, s, M);
  if (M.nranks > 1) {
    if (M.wide) hipLaunchKernelGGL(k_gsort<true>, dim3(NACC / 256), dim3(256), 0, s, M);
    else hipLaunchKernelGGL(k_gsort<false>, dim3(NACC / 256), dim3(256), 0, s, M);
  }
}
// After it: the other ranks' records before each of this rank's (binary searches), then the window's books.
static void dist_rank_fin(const P2PDev &M, hipStream_t s) {
  if (M.nranks > 1) {
    const dim3 g(NACC / GS_T, M.nranks - 1);
    if (M.wide) hipLaunchKernelGGL(k_gsearch<true>, g, dim3(GS_T), 0, s, M);
    else hipLaunchKernelGGL(k_gsearch<false>, g, dim3(GS_T), 0, s, M);
  }
  if (M.wide) hipLaunchKernelGGL(k_dfin2<true>, dim3(DF2_FB + NACC / HB), dim3(HB), 0, s, M);
  else hipLaunchKernelGGL(k_dfin2<false>, dim3(DF2_FB + NHB), dim3(HB), 0, s, M);
}
// The partitioned window (one RCCL member): 4 kernels and 3 collectives, on stream s.
static int launch_windows_dist(nsgpu_p2p *h, hipStream_t s, int nwin = NWIN) {
  const P2PDev &M = h->M;
  int rc = NSGPU_OK;
  for (int w = 0; w < nwin && !rc; w++) {
    dist_pa(M, s);
    rc = x_allgather(h, M.x0_send, M.x0_recv, X0B, s);
    dist_handle(M, s, h->loss_init != nullptr || M.frag != 0 || M.errm != 0 || M.ranvar != 0);
    dist_rank(M, s);
    if (!rc) rc = x_allgather(h, M.x1_send, M.x1_recv, X1B, s);
    dist_rank_fin(M, s);
    if (!rc) rc = x_alltoall(h, M.x2_send, M.x2_recv, M.x2b, s);
  }
  return rc;
}

// The partitioned engine's host-driven steps (every rank makes the same ones: the pause that asks for them is
// decided from exchanged data): the pool compaction, and the start of a partitioned sorted run — a window some
// rank cannot hold (MODE_CUT): every rank sorts its candidates (drun_sort), the ranks' fitting keys are
// all-gathered and every rank moves the first chunk in (k_drun_first); the later chunks are formed by the window
// pipeline itself.
static int drun_sort(nsgpu_p2p *h, uint64_t W, hipStream_t s) {
  const P2PDev &M = h->M;
  const uint64_t n = W < M.runcap ? W : M.runcap;
  hipLaunchKernelGGL(k_drun_clear, dim3(64), dim3(256), 0, s, M);
  if (n) {  // the keys sorted so that the last pass writes rn_key, the records gathered into rn_*
    const uint64_t *kin;
    const uint32_t *vin;
    if (const int rc = radix_sort(M, n, M.rn_key, M.s_key2, true, s, &kin, &vin)) return rc;
    const uint32_t gg = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_rs_gather<uint32_t>, dim3(gg), dim3(256), 0, s, vin, M.wctx, M.rn_ctx, n);
    hipLaunchKernelGGL(k_rs_gather<uint32_t>, dim3(gg), dim3(256), 0, s, vin, M.wkind, M.rn_kind, n);
    hipLaunchKernelGGL(k_rs_gather<uint32_t>, dim3(gg), dim3(256), 0, s, vin, M.wa, M.rn_a, n);
    hipLaunchKernelGGL(k_rs_gather<uint32_t>, dim3(gg), dim3(256), 0, s, vin, M.wsrc, M.rn_src, n);
    hipLaunchKernelGGL(k_rs_gather<Pkt>, dim3(gg), dim3(256), 0, s, vin, M.wpkt, M.rn_pkt, n);
  }
  if (n && M.wide) hipLaunchKernelGGL(k_drun_trim, dim3(1), dim3(1024), 0, s, M, n);
  hipLaunchKernelGGL(k_drun_start, dim3(1), dim3(1), 0, s, M, n);
  if (n) hipLaunchKernelGGL(k_drun_red, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 1024)), dim3(256), 0, s, M, n);
  NSGPU_HIP(hipGetLastError());
  return NSGPU_OK;
}
static int host_step_dist(nsgpu_p2p *h, const Ctl &c, hipStream_t s) {
  if (c.mode != MODE_CUT) return host_step(h, c, s);
  int rc = drun_sort(h, c.W, s);
  if (!rc) rc = x_allgather(h, h->M.xk_send, h->M.xk_recv, 16, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_drun_first, dim3(WCAP / TB), dim3(TB), 0, s, h->M);
  NSGPU_HIP(hipGetLastError());
  return NSGPU_OK;
}

// Captures what `body` launches on stream s (capture mode `mode`) into an instantiated graph, *gx; `body` returns an
// nsgpu status.  A failure leaves *gx null, no graph behind and no pending HIP error; `who` names the path in its
// message.
template <class F>
static int capture_graph(hipStream_t s, hipStreamCaptureMode mode, const char *who, hipGraphExec_t *gx, F body) {
  hipGraph_t g = nullptr;
  NSGPU_HIP(hipStreamBeginCapture(s, mode));
  const int rc = body();
  hipError_t e = hipStreamEndCapture(s, &g);
  if (rc != NSGPU_OK || e != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    if (rc != NSGPU_OK) return rc;
    return set_error(NSGPU_EHIP, "%s: graph capture: %s", who, hipGetErrorString(e));
  }
  e = hipGraphInstantiate(gx, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) {
    *gx = nullptr;
    return set_error(NSGPU_EHIP, "%s: graph instantiate: %s", who, hipGetErrorString(e));
  }
  return NSGPU_OK;
}

static int build_graph(nsgpu_p2p *h, bool df = false, bool tail = false) {
  // NWIN windows of the pipeline (tail: NWIN_TAIL, single engine); kernels read every run-dependent value from the
  // device (Ctl), so one instantiated graph serves every run of this engine
  hipGraphExec_t &gx = tail ? h->gtail[df ? 1 : 0] : df ? h->gexec_df : h->gexec;
#ifdef NSGPU_PHASE_PROF
  if (const int rd = dbg_alloc()) return rd;  // (the invariant checker's buffer: allocated before any capture)
#endif
  const hipStreamCaptureMode mode = h->M.dist ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal;
  return capture_graph(h->s, mode, "nsgpu_p2p", &gx, [&] {
    return h->M.dist ? launch_windows_dist(h, h->s) : launch_windows(h, h->s, df, tail ? NWIN_TAIL : NWIN);
  });
}

// A run that set the engine's error word: capacity exceeded (the simulation is truncated).
static int engine_error(uint32_t err) {
  if (err & ERR_RANVAR_ATTEMPTS)
    return set_error(NSGPU_ERANGE, "nsgpu_p2p: a bounded ExponentialVariable was rejected %u times in one GetValue "
                     "(code %u)", NSGPU_RV_MAX_ATTEMPTS, err);
  if (err & ERR_TRACE_SEQ)
    return set_error(NSGPU_ERANGE, "nsgpu_p2p: a UdpTraceClient's m_sent would pass 2^24 (code %u: the packet descriptor "
                     "carries the SeqTsHeader's sequence number in 24 bits; it is never wrapped silently)", err);
  if (err & ERR_FLOWMON_ID)
    return set_error(NSGPU_ERANGE, "nsgpu_p2p: a monitored node's IPv4 identification reached the size of its "
                     "tracked-packet table (flowmon; code %u: at most 65536 datagrams a node, the 16-bit identification "
                     "would wrap there, which the per-flow statistics do not model)", err);
  return set_error((err & 2048u) ? NSGPU_ERANGE : NSGPU_ENOMEM, "nsgpu_p2p: engine capacity exceeded (code %u: 1 = event pool, 4 = window limit, "
                                 "8 = window cut, 16 = a window's remote events beyond the X2 capacity, 32 = local "
                                 "records, 64 = window records, 256 = deferred uid resolution (internal), 512 = uids "
                                 "beyond the deferred pipeline's range (internal), 2048 = the uid counter would pass "
                                 "0xfffffffe: DefaultSimulatorImpl's uint32 m_uid wraps there, which the engine does "
                                 "not replicate, 4096 = a node's IPv4 reassembly list would pass 128 fragments, 8192 = a fragment at a node "
                                 "without reassembly state (internal))", err);
}

// The replay loop of every driver: replays of a window pipeline on stream s until the run is over (done >= 2 in the
// run control C) or a pause says stop.  Two replays in flight: replay i+1 is queued (`launch(slot)`), the run
// control behind it copied into the pinned snap[slot] and ev[slot] recorded, before the snapshot after replay i is
// examined.  A pipeline that paused itself (mode >= MODE_SORT: a host-driven sort, cut or compaction, a host
// closure) makes the replay queued behind it a no-op; once that one has drained, `pause(slot, &stop)` runs the host
// step from its snapshot, snap[slot], or sets stop, and the loop starts over with no previous snapshot.  Any other
// snapshot goes to `seen(c)`.  The callables return an nsgpu status.
template <class L, class P, class O>
static int replay_loop(hipStream_t s, const Ctl *C, Ctl *snap, hipEvent_t *ev, L launch, P pause, O seen) {
  int cur = 0;
  bool have_prev = false;
  for (;;) {
    if (const int rc = launch(cur)) return rc;
    // (the run control into a pinned snapshot after the replay: a copy-engine transfer)
    NSGPU_HIP(hipMemcpyAsync(&snap[cur], C, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipEventRecord(ev[cur], s));
    if (have_prev) {
      NSGPU_HIP(hipEventSynchronize(ev[cur ^ 1]));
      const Ctl &c = snap[cur ^ 1];
      if (c.done >= 2) break;  // 2: the final window is appended
      if (c.mode >= MODE_SORT) {
        NSGPU_HIP(hipEventSynchronize(ev[cur]));
        bool stop = false;
        if (const int rc = pause(cur, &stop)) return rc;
        if (stop) break;
        have_prev = false;
        continue;
      }
      if (const int rc = seen(c)) return rc;
    }
    have_prev = true;
    cur ^= 1;
  }
  return NSGPU_OK;
}

// Replays the single engine's window pipeline until the run is over or the pipeline paused for a host closure
// (*paused), through replay_loop.
static int drive(nsgpu_p2p *h, bool *paused) {
  *paused = false;
  // the deferred pipeline while the engine runs normal windows; after a pause (which it flushes) the other
  // pipeline until a replay ends in a normal window
  const bool dfu = df_usable(h);
  bool df = dfu && h->uid_hint < UID_DF_SOFT;
  bool df_of[2] = {false, false};
  if (df && !h->eager && !h->gexec_df) {
    const int rc = build_graph(h, true);
    if (rc) return rc;
  }
  // The run's last windows in replays of NWIN_TAIL: a replay queued behind the final window is a no-op that still
  // launches its kernels (~1.5 x NWIN of them trail the run).  The tail starts once the examined snapshots' pace
  // (simulated ns a window) puts Simulator::Stop within the windows already queued plus one replay.  Speed only:
  // the windows are the same whatever a replay holds.
  const uint64_t stop_ts = h->C0.red[1].stopts;
  bool tail = false;
  uint64_t w_last = 0, t_last = 0;
  int queued = 0;  // windows of the replay in flight behind the examined one
  auto launch = [&](int slot) -> int {
    const int nw = tail ? NWIN_TAIL : NWIN;
    if (h->eager) {
      const int rc = launch_windows(h, h->s, df, nw);
      if (rc) return rc;
      NSGPU_HIP(hipGetLastError());
    } else {
      hipGraphExec_t gx = tail ? h->gtail[df ? 1 : 0] : df ? h->gexec_df : h->gexec;
      if (tail && !gx) {
        const int rc = build_graph(h, df, true);
        if (rc) return rc;
        gx = h->gtail[df ? 1 : 0];
      }
      NSGPU_HIP(hipGraphLaunch(gx, h->s));
    }
    queued = nw;
    df_of[slot] = df;
    return NSGPU_OK;
  };
  auto pause = [&](int slot, bool *stop) -> int {
    if (df_of[slot ^ 1]) {  // (the pause came from the deferred pipeline: its last window is not accounted yet)
      const int rc = df_flush(h, h->s);
      if (rc) return rc;
      NSGPU_HIP(hipMemcpyAsync(&h->snap[slot], h->M.C, sizeof(Ctl), hipMemcpyDeviceToHost, h->s));
      NSGPU_HIP(hipStreamSynchronize(h->s));
    }
    df = false;
    if (h->snap[slot].mode == MODE_HOST) {
      *paused = *stop = true;
      return NSGPU_OK;
    }
    return host_step(h, h->snap[slot], h->s);
  };
  auto seen = [&](const Ctl &c) -> int {
    if (!tail && stop_ts != ~0ull && c.mode == MODE_NORMAL && c.windows > w_last && c.tmin > t_last &&
        c.tmin != ~0ull && t_last != 0) {
      const double pace = (double)(c.tmin - t_last) / (double)(c.windows - w_last);
      const double left = stop_ts > c.tmin ? (double)(stop_ts - c.tmin) / pace : 0.0;
      if (left < (double)(queued + NWIN)) tail = true;
    }
    if (c.mode == MODE_NORMAL && c.tmin != ~0ull) w_last = c.windows, t_last = c.tmin;
    if (!df && dfu && c.mode == MODE_NORMAL && c.uid < UID_DF_SOFT) {  // a normal window ended the replay: back
                                                                      // to the deferred pipeline
      // (not in a sorted run's chunks: those belong to the other pipeline until the run is over)
      if (!h->eager && !h->gexec_df) {
        const int rc = build_graph(h, true);
        if (rc) return rc;
      }
      df = true;
    }
    return NSGPU_OK;
  };
  if (const int rc = replay_loop(h->s, h->M.C, h->snap, h->ev, launch, pause, seen)) return rc;
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

// Replays the partitioned window pipeline until the run is over, as drive(): two replays in flight;
// a pause (a cut, a compaction: every rank pauses in the same window) runs its host step once the
// replay queued behind it has drained.
static int drive_dist(nsgpu_p2p *h) {
  auto launch = [h](int) -> int {
    if (h->eager) {
      const int rc = launch_windows_dist(h, h->s);
      if (rc) return rc;
      NSGPU_HIP(hipGetLastError());
    } else {
      NSGPU_HIP(hipGraphLaunch(h->gexec, h->s));
    }
    return NSGPU_OK;
  };
  auto pause = [h](int slot, bool *) -> int { return host_step_dist(h, h->snap[slot], h->s); };
  auto seen = [](const Ctl &) -> int { return NSGPU_OK; };
  if (const int rc = replay_loop(h->s, h->M.C, h->snap, h->ev, launch, pause, seen)) return rc;
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

// ---- mixed host / device runs: the host-closure runtime (nsgpu_sim) drives the engine ----
uint32_t nsgpu::p2p_first_uid(const nsgpu_p2p *h) { return h->sc.uid_first ? h->sc.uid_first : 4u; }

// The engine stream takes over from the caller's (join_in: what the caller queued on cs runs before anything queued
// on the engine stream from here on) and hands back (join_out).
static int join_in(nsgpu_p2p *h, hipStream_t cs) {
  NSGPU_HIP(hipEventRecord(h->ev[0], cs));
  NSGPU_HIP(hipStreamWaitEvent(h->s, h->ev[0], 0));
  return NSGPU_OK;
}
static int join_out(nsgpu_p2p *h, hipStream_t cs) {
  NSGPU_HIP(hipEventRecord(h->ev[0], h->s));
  NSGPU_HIP(hipStreamWaitEvent(cs, h->ev[0], 0));
  return NSGPU_OK;
}
// The run control as the engine stream has left it, into snap[0] (and the engine's error word into *err): drains
// the engine stream.
static int read_ctl(nsgpu_p2p *h, uint32_t *err = nullptr) {
  NSGPU_HIP(hipMemcpyAsync(&h->snap[0], h->M.C, sizeof(Ctl), hipMemcpyDeviceToHost, h->s));
  if (err) NSGPU_HIP(hipMemcpyAsync(err, h->M.error, 4, hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_setup_uid(nsgpu_p2p *h, uint32_t *uid) {
  if (!h || !uid) return set_error(NSGPU_EINVAL, "nsgpu_p2p_setup_uid: null");
  // (nsgpu_sim_attach_p2p / _adopt_p2p start here: a frag engine stays outside mixed host / device runs — a host
  // closure's send is one packet with the node's whole identification counter, and no test covers the combination)
  if (h->M.frag)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_setup_uid: a scenario with IPv4 fragmentation (frag) cannot be attached "
                     "to a host-closure runtime");
  if (h->M.flowmon)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_setup_uid: a scenario with per-flow statistics (flowmon) cannot be attached "
                     "to a host-closure runtime");
  // (... and so does an engine with a receive error model: no test covers the combination)
  if (h->M.errm)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_setup_uid: a scenario with a receive error model cannot be attached to a "
                     "host-closure runtime");
  if (h->has_trace_client)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_setup_uid: a scenario with a UdpTraceClient cannot be attached to a "
                     "host-closure runtime");
  if (h->M.ranvar)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_setup_uid: a scenario with a random OnOff time cannot be attached to a "
                     "host-closure runtime");
  *uid = h->C0.uid;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_advance(nsgpu_p2p *h, uint64_t hts, uint32_t huid, uint32_t *uid, uint64_t *dispatched,
                                 int *ended, void *stream) {
  if (!h || !uid || !dispatched || !ended) return set_error(NSGPU_EINVAL, "nsgpu_p2p_advance: null");
  if (h->M.dist) return set_error(NSGPU_ESTATE, "nsgpu_p2p_advance: single-device engines only");
  *ended = 0;
  if (!h->eager && !h->gexec) {
    const int rc = build_graph(h);
    if (rc) return rc;
  }
  hipStream_t cs = (hipStream_t)stream;
  uint32_t err = 0;
  if (const int rc = join_in(h, cs)) return rc;
  if (const int rc = read_ctl(h, &err)) return rc;
  if (err) return engine_error(err);  // (sticky: e.g. a refused inject_send at the uid limit)
  if (h->snap[0].done >= 2) {
    *ended = 1;
    return NSGPU_OK;
  }
  hipLaunchKernelGGL(k_host_resume, dim3(1), dim3(1), 0, h->s, h->M, hts, huid, *uid, *dispatched);
  NSGPU_HIP(hipGetLastError());
  h->uid_hint = *uid;
  bool paused = false;
  if (const int rc = drive(h, &paused)) return rc;
  if (const int rc = read_ctl(h, &err)) return rc;
  if (err) return engine_error(err);
  *uid = h->snap[0].uid;
  h->uid_hint = *uid;
  *dispatched = h->snap[0].K;
  *ended = paused ? 0 : 1;
  return join_out(h, cs);
}

// The attached engine's pending device events (Next / IsFinished of the runtime): how many, the
// smallest timestamp among them, and whether a device-dispatched Simulator::Stop ended the run.
extern "C" int nsgpu_p2p_pending(nsgpu_p2p *h, uint64_t *n, uint64_t *next_ts, int *stopped, void *stream) {
  if (!h || !n || !next_ts || !stopped) return set_error(NSGPU_EINVAL, "nsgpu_p2p_pending: null");
  if (h->M.dist) return set_error(NSGPU_ESTATE, "nsgpu_p2p_pending: single-device engines only");
  if (const int rc = join_in(h, (hipStream_t)stream)) return rc;
  if (const int rc = read_ctl(h)) return rc;
  const Ctl &c = h->snap[0];
  *stopped = c.stop_seen ? 1 : 0;
  if (c.done >= 1) {  // (1: the final window is dispatched, its children are not queued)
    *n = 0;
    *next_ts = ~0ull;
    return NSGPU_OK;
  }
  *n = c.live + (c.pvalid ? c.pchild : 0) + (c.mode == MODE_RUN ? c.rW - c.r0 : 0);
  *next_ts = c.red[0].tmin < c.red[1].tmin ? c.red[0].tmin : c.red[1].tmin;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_inject_send(nsgpu_p2p *h, uint32_t app, uint64_t now, uint32_t cur_uid, uint32_t cur_ctx,
                                     uint32_t *uid, uint32_t *trace_seq, void *stream) {
  if (!h || !uid || !trace_seq) return set_error(NSGPU_EINVAL, "nsgpu_p2p_inject_send: null");
  if (h->M.dist) return set_error(NSGPU_ESTATE, "nsgpu_p2p_inject_send: single-device engines only");
  if (app >= h->M.n_apps || h->app_kind[app] != NSGPU_APP_ONOFF)
    return set_error(NSGPU_EINVAL, "nsgpu_p2p_inject_send: app %u is not an OnOff flow", app);
  // (a host closure's send is one packet with the node's whole identification counter: it stays outside frag mode,
  // whose receivers read the upper half of a descriptor's identification as fragment fields)
  if (h->M.frag)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_inject_send: not available in a scenario with IPv4 fragmentation (frag)");
  if (h->M.errm)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_inject_send: not available in a scenario with a receive error model");
  if (h->M.ranvar)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_inject_send: not available in a scenario with a random OnOff time");
  // (... nor on a monitored engine: the injected datagram would pass no ReportFirstTx)
  if (h->M.flowmon)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_inject_send: not available in a scenario with per-flow statistics (flowmon)");
  hipStream_t s = h->s;
  if (const int rc = join_in(h, (hipStream_t)stream)) return rc;
  if (const int rc = read_ctl(h)) return rc;
  if (h->snap[0].mode != MODE_HOST) return set_error(NSGPU_ESTATE, "nsgpu_p2p_inject_send: the engine is not paused for a host closure");
  hipLaunchKernelGGL(k_set_uid, dim3(1), dim3(1), 0, s, h->M, *uid);  // (the host closures' Schedule calls)
  // (the room is checked on the device before any child is written: a refused send leaves the sticky uid error)
  if ((uint64_t)*uid > UID_MAX_NEXT) return nsgpu::uid_range_error("nsgpu_p2p_inject_send");
  hipLaunchKernelGGL(k_inject, dim3(1), dim3(1), 0, s, h->M, app, now, cur_uid, cur_ctx, *trace_seq,
                     (uint64_t)(UID_MAX_NEXT - *uid), h->M.s_val);
  NSGPU_HIP(hipGetLastError());
  uint32_t outv[3];
  NSGPU_HIP(hipMemcpyAsync(outv, h->M.s_val, sizeof(outv), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  if (outv[2]) return nsgpu::uid_range_error("nsgpu_p2p_inject_send");
  *uid = outv[0];
  *trace_seq = outv[1];
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_counters(nsgpu_p2p *h, nsgpu_dev_counters *devc, nsgpu_app_counters *appc, void *stream) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_counters: null");
  hipStream_t cs = (hipStream_t)stream;
  NSGPU_HIP(hipStreamSynchronize(h->s));
  if (devc)
    NSGPU_HIP(hipMemcpy2DAsync(devc, sizeof(*devc), &h->M.dev[0].c, sizeof(DevRec), sizeof(*devc), h->M.n_devices,
                               hipMemcpyDeviceToHost, cs));
  if (appc) NSGPU_HIP(hipMemcpyAsync(appc, h->M.appc, h->M.n_apps * sizeof(*appc), hipMemcpyDeviceToHost, cs));
  NSGPU_HIP(hipStreamSynchronize(cs));
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_run(nsgpu_p2p *h, void *stream) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_run: null");
  if (h->M.dist && !h->comm)
    return set_error(NSGPU_ESTATE, "nsgpu_p2p_run: a loopback partition runs with its group (nsgpu_p2p_group_run)");
  if (!h->eager && !h->gexec) {
    int rc = build_graph(h);
    if (rc && h->M.dist) {  // RCCL collectives that refuse stream capture: launch them eagerly
      h->eager = true;
      rc = NSGPU_OK;
    }
    if (rc) return rc;
  }
  hipStream_t cs = (hipStream_t)stream;
  if (const int rc = join_in(h, cs)) return rc;
  NSGPU_HIP(hipEventRecord(h->t0, h->s));
  if (h->M.dist) {
    const int rc = drive_dist(h);
    if (rc) return rc;
  } else {
    bool paused = false;
    const int rc = drive(h, &paused);
    if (rc) return rc;
    if (paused) return set_error(NSGPU_ESTATE, "nsgpu_p2p_run: paused for a host closure (use nsgpu_p2p_advance)");
  }
  NSGPU_HIP(hipEventRecord(h->t1, h->s));
  uint32_t err = 0;
  NSGPU_HIP(hipMemcpyAsync(&err, h->M.error, 4, hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipEventSynchronize(h->t1));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  NSGPU_HIP(hipEventElapsedTime(&h->last_ms, h->t0, h->t1));
#ifdef NSGPU_PHASE_PROF
  if (err & 1024u) {  // (debug mode 2: a graph-resident check stopped the run)
    unsigned long long o[4] = {};
    NSGPU_HIP(hipMemcpy(o, g_dbg_out, sizeof(o), hipMemcpyDeviceToHost));
    return set_error(NSGPU_EHIP, "nsgpu_p2p debug (graph): invariant %llu broken after %s (window %llu of the replay, "
                     "C.windows %llu): %llu %llu", o[0], KERNEL_NAMES[o[3] & 0xff], (o[3] >> 8) & 0xff, o[3] >> 32, o[1],
                     o[2]);
  }
#endif
  if (err) return engine_error(err);
  return join_out(h, cs);
}

extern "C" int nsgpu_p2p_phase_read(uint64_t *out, int n, int reset) {
#ifdef NSGPU_PHASE_PROF
  if (!out || n <= 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_phase_read: null");
  if (n > 64) {  // the rest: the per-block times of the sampled window (g_blk)
    const int nb = std::min(n - 64, 3 * BLK_MAX * 2);
    NSGPU_HIP(hipMemcpyFromSymbol(out + 64, HIP_SYMBOL(g_blk), nb * sizeof(uint64_t)));
    const int ng = std::min(n - 64 - 3 * BLK_MAX * 2, GT_BLK_MAX * 8);  // (then k_gtile's stamps)
    if (ng > 0) NSGPU_HIP(hipMemcpyFromSymbol(out + 64 + 3 * BLK_MAX * 2, HIP_SYMBOL(g_gt), ng * sizeof(uint64_t)));
    // (then the holder blocks' kind counts: BLKK_MAX x BLKK_N 32-bit words, two to an output word)
    const int nk = std::min(n - 64 - 3 * BLK_MAX * 2 - GT_BLK_MAX * 8, BLKK_MAX * BLKK_N / 2);
    if (nk > 0)
      NSGPU_HIP(hipMemcpyFromSymbol(out + 64 + 3 * BLK_MAX * 2 + GT_BLK_MAX * 8, HIP_SYMBOL(g_blkk), nk * sizeof(uint64_t)));
    n = 64;
  }
  NSGPU_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), n * sizeof(uint64_t)));
  if (reset) {
    uint64_t z[64] = {0};
    NSGPU_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)));
  }
  if (reset < 0) {  // (-w: the window the per-block stamps sample from now on; its old stamps cleared)
    const uint64_t w = (uint64_t)(-(int64_t)reset);
    NSGPU_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_blk_win), &w, sizeof(w)));
    std::vector<uint64_t> zb(3 * BLK_MAX * 2, 0);
    NSGPU_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_blk), zb.data(), zb.size() * sizeof(uint64_t)));
    NSGPU_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_blkk), zb.data(), sizeof(uint32_t) * BLKK_MAX * BLKK_N));
  }
  return NSGPU_OK;
#else
  (void)out, (void)n, (void)reset;
  return set_error(NSGPU_ESTATE, "nsgpu_p2p_phase_read: library built without NSGPU_PHASE_PROF");
#endif
}

// Trace sink records (ascii/pcap replay): a device buffer of `cap` records, cleared by every reset.
// The kernels take the engine descriptor by value, so an instantiated graph is rebuilt.
extern "C" int nsgpu_p2p_set_trace(nsgpu_p2p *h, uint64_t cap) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_set_trace: null");
  if (h->M.trace) return set_error(NSGPU_ESTATE, "nsgpu_p2p_set_trace: tracing is already on");
  if (cap == 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_set_trace: zero capacity");
  nsgpu_trace_record *tb = nullptr;
  unsigned long long *tn = nullptr;
  int rc = dalloc(h, &tb, cap);
  if (!rc) rc = dalloc(h, &tn, 1);
  if (rc) return rc;
  h->M.trace = tb;
  h->M.trace_n = tn;
  if (h->M.dist) h->M.wide = 0;  // (a traced partitioned engine runs narrow windows: its local records' trace
                                 //  uids would need the single engine's patch pass)
  NSGPU_HIP(hipMemset(h->M.trace_n, 0, sizeof(unsigned long long)));
  h->M.trace_cap = cap;
  if (const int rc2 = mdev_sync(h)) return rc2;
  if (h->gexec) {
    (void)hipGraphExecDestroy(h->gexec);
    h->gexec = nullptr;
  }
  if (h->gexec_df) {  // (traced engines run the other pipeline)
    (void)hipGraphExecDestroy(h->gexec_df);
    h->gexec_df = nullptr;
  }
  for (hipGraphExec_t &g : h->gtail)
    if (g) {
      (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
  return NSGPU_OK;
}

// Which trace sinks the runs record (bit k = nsgpu_trace_kind k).
extern "C" int nsgpu_p2p_set_trace_kinds(nsgpu_p2p *h, uint32_t mask) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_set_trace_kinds: null");
  if (mask & ~0x7fu) return set_error(NSGPU_EINVAL, "nsgpu_p2p_set_trace_kinds: unknown kind bits 0x%x", mask);
  h->M.trace_kinds = mask;
  if (const int rc = mdev_sync(h)) return rc;
  for (hipGraphExec_t *g : {&h->gexec, &h->gexec_df, &h->gtail[0], &h->gtail[1]})
    if (*g) {
      (void)hipGraphExecDestroy(*g);
      *g = nullptr;
    }
  return NSGPU_OK;
}

// Copies the trace records of the last run (unordered; *n = how many the run made, which may exceed
// both the buffer and `cap`: NSGPU_ENOMEM then).
extern "C" int nsgpu_p2p_trace_read(nsgpu_p2p *h, nsgpu_trace_record *out, uint64_t cap, uint64_t *n, void *stream) {
  if (!h || !n) return set_error(NSGPU_EINVAL, "nsgpu_p2p_trace_read: null");
  if (!h->M.trace) return set_error(NSGPU_ESTATE, "nsgpu_p2p_trace_read: tracing is off (nsgpu_p2p_set_trace)");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long total = 0;
  NSGPU_HIP(hipMemcpyAsync(&total, h->M.trace_n, sizeof(total), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  *n = total;
  const uint64_t m = std::min<uint64_t>(std::min<uint64_t>(total, h->M.trace_cap), cap);
  if (m && out) {
    NSGPU_HIP(hipMemcpyAsync(out, h->M.trace, m * sizeof(nsgpu_trace_record), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipStreamSynchronize(s));
  }
  if (total > h->M.trace_cap || (out && total > cap))
    return set_error(NSGPU_ENOMEM, "nsgpu_p2p_trace_read: %llu records, buffer %llu", total,
                     (unsigned long long)std::min<uint64_t>(h->M.trace_cap, cap));
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_set_eager(nsgpu_p2p *h, int eager) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_set_eager: null");
  h->eager = eager != 0;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_kernel_count(int *n) {
  if (!n) return set_error(NSGPU_EINVAL, "nsgpu_p2p_kernel_count: null");
  *n = NKERN;
  return NSGPU_OK;
}

extern "C" const char *nsgpu_p2p_kernel_name(int k) { return k >= 0 && k < NKERN ? KERNEL_NAMES[k] : nullptr; }

// Per-kernel device time: runs the simulation to completion with the pipeline's kernels launched
// one by one on the engine stream; in every `sample_every`-th window each kernel is bracketed by
// two HIP events on that stream, and kernel_ms[k] / launches[k] accumulate the bracketed time and
// the bracketed launches of kernel k (NKERN entries each).  Other windows run unbracketed.
extern "C" int nsgpu_p2p_profile(nsgpu_p2p *h, void *stream, uint32_t sample_every, double *kernel_ms,
                                 uint64_t *launches) {
  if (!h || !kernel_ms || !launches) return set_error(NSGPU_EINVAL, "nsgpu_p2p_profile: null");
  if (h->M.dist) return set_error(NSGPU_ESTATE, "nsgpu_p2p_profile: single-device engines only");
  if (sample_every == 0) sample_every = 1;
  for (int k = 0; k < NKERN; k++) kernel_ms[k] = 0.0, launches[k] = 0;
  // up to NS sampled windows; the events are read after the run (no synchronisation in between
  // beyond the done-flag checks every NWIN windows that nsgpu_p2p_run makes too)
  constexpr int NS = 512;
  std::vector<hipEvent_t> ev(2 * NKERN * NS, nullptr);
  int rc = NSGPU_OK;
  for (auto &e : ev)
    if (hipEventCreate(&e) != hipSuccess) {
      e = nullptr;
      rc = set_error(NSGPU_EHIP, "nsgpu_p2p_profile: hipEventCreate failed");
      break;
    }
  hipStream_t cs = (hipStream_t)stream;
  if (rc == NSGPU_OK) rc = join_in(h, cs);
  int ns = 0;
  bool used[NKERN] = {};  // the engine's window launches kernel k (its events are recorded)
  const bool dfu = df_usable(h);
  bool df = dfu && h->uid_hint < UID_DF_SOFT;
  // the run control is read after every window (so no sampled pass is a paused no-op and the
  // host-driven steps run as soon as the pipeline asks)
  for (uint64_t w = 0; rc == NSGPU_OK; w++) {
    const bool sample = (w % sample_every) == 0 && ns < NS;
    for (int k = 0; k < NKERN; k++) {
      if (sample) used[k] |= launch_kernel(h, k, h->s, df, ev[(2 * ns) * NKERN + k], ev[(2 * ns + 1) * NKERN + k]);
      else launch_kernel(h, k, h->s, df);
    }
    if (sample) ns++;
    if (hipGetLastError() != hipSuccess) {
      rc = set_error(NSGPU_EHIP, "nsgpu_p2p_profile: launch failed");
      break;
    }
    if ((rc = read_ctl(h))) break;
    if (h->snap[0].done >= 2) break;  // the final window is appended
    if (h->snap[0].mode >= MODE_SORT) {
      if (df) {  // (the deferred pipeline paused: flush its last window first)
        rc = df_flush(h, h->s);
        if (rc == NSGPU_OK) rc = read_ctl(h);
        df = false;
      }
      if (rc == NSGPU_OK) rc = host_step(h, h->snap[0], h->s);
    } else if (!df && dfu && h->snap[0].mode == MODE_NORMAL && h->snap[0].uid < UID_DF_SOFT) {  // (sorted-run
                                                                                             //  chunks stay on the other pipeline)
      df = true;
    }
  }
  if (rc == NSGPU_OK) {
    for (int i = 0; i < ns; i++)
      for (int k = 0; k < NKERN; k++) {
        float ms = 0.f;
        if (used[k] && hipEventElapsedTime(&ms, ev[(2 * i) * NKERN + k], ev[(2 * i + 1) * NKERN + k]) == hipSuccess) {
          kernel_ms[k] += ms;
          launches[k]++;
        }
      }
  }
  for (auto e : ev)
    if (e) (void)hipEventDestroy(e);
  (void)hipEventRecord(h->ev[0], h->s);  // (join_out, keeping rc and its message)
  (void)hipStreamWaitEvent(cs, h->ev[0], 0);
  return rc;
}

// Whether the engine runs wide windows (node degree <= LQ, not NSGPU_P2P_NARROW=1; a traced partitioned engine
// runs narrow ones).
extern "C" int nsgpu_p2p_get_wide(nsgpu_p2p *h, int *wide) {
  if (!h || !wide) return set_error(NSGPU_EINVAL, "nsgpu_p2p_get_wide: null");
  *wide = h->M.wide ? 1 : 0;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_last_run_ms(nsgpu_p2p *h, double *gpu_ms) {
  if (!h || !gpu_ms) return set_error(NSGPU_EINVAL, "nsgpu_p2p_last_run_ms: null");
  *gpu_ms = h->last_ms;
  return NSGPU_OK;
}

// UdpServer::GetReceived / GetLost of every application (zeros for other kinds, and for a scenario without ports).
extern "C" int nsgpu_p2p_udp_servers(nsgpu_p2p *h, nsgpu_udp_server_record *out, void *stream) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_udp_servers: null");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t A = h->M.n_apps;
  memset(out, 0, A * sizeof(*out));
  if (!h->loss_init) return NSGPU_OK;
  std::vector<nsgpu_loss_counter> lc(A);
  NSGPU_HIP(hipMemcpyAsync(lc.data(), loss_counters(h->M.appc, A), A * sizeof(nsgpu_loss_counter),
                           hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (uint32_t a = 0; a < A; a++)
    if (h->app_kind[a] == NSGPU_APP_UDP_SERVER)
      out[a] = nsgpu_udp_server_record{lc[a].received, lc[a].lost, lc[a].last_max_seq, 0};
  return NSGPU_OK;
}

// UdpTraceClient's m_sent, m_currentEntry and Send events run, per application (zeros for every other kind).
extern "C" int nsgpu_p2p_udp_trace_clients(nsgpu_p2p *h, nsgpu_udp_trace_client_record *out, void *stream) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_udp_trace_clients: null");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t A = h->M.n_apps;
  memset(out, 0, A * sizeof(*out));
  if (!h->has_trace_client) return NSGPU_OK;
  std::vector<uint32_t> w(3 * (size_t)A);
  NSGPU_HIP(hipMemcpyAsync(w.data(), h->M.app_tot, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (uint32_t a = 0; a < A; a++)
    if (h->app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT)
      out[a] = nsgpu_udp_trace_client_record{w[a], w[A + a], w[2 * (size_t)A + a], 0};
  return NSGPU_OK;
}

// What UdpTraceClient::LoadDefaultTrace (udp-trace-client.cc:211-232) leaves in m_entries: the ten built-in frames
// (:41-53) with a B frame's timeToSend 0 and every other frame's the delta to the frame before it that is no B frame.
namespace {
const nsgpu_udp_trace_entry k_default_trace[] = {{0, 534},  {40, 1542}, {0, 134},  {0, 390}, {200, 765},
                                                 {0, 407},  {0, 504},   {120, 903}, {0, 421}, {0, 587}};
void load_default_trace(std::vector<nsgpu_udp_trace_entry> &v) {
  v.assign(std::begin(k_default_trace), std::end(k_default_trace));
}
int trace_out(const std::vector<nsgpu_udp_trace_entry> &v, nsgpu_udp_trace_entry *out, uint64_t cap, uint64_t *n) {
  *n = v.size();
  for (uint64_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
  return NSGPU_OK;
}
}  // namespace
extern "C" int nsgpu_udp_trace_default(nsgpu_udp_trace_entry *out, uint64_t cap, uint64_t *n) {
  if (!n || (cap && !out)) return set_error(NSGPU_EINVAL, "nsgpu_udp_trace_default: null");
  std::vector<nsgpu_udp_trace_entry> v;
  load_default_trace(v);
  return trace_out(v, out, cap, n);
}
// UdpTraceClient::LoadTrace (:176-209) with its own extraction idiom, types and loop condition: a file that ends in
// whitespace is good () after its last line, so one more round runs; its first extraction meets the end of the file
// while skipping whitespace and every one fails before it stores anything, so the variables keep the last line's values
// — the last entry once more, with timeToSend time - prevTime = 0 (or a B frame's 0).  time - prevTime is unsigned and
// may wrap.  (The reference leaves its variables uninitialised, which shows only for an empty file; here they are 0.)
extern "C" int nsgpu_udp_trace_load(const char *path, nsgpu_udp_trace_entry *out, uint64_t cap, uint64_t *n) {
  if (!path || !n || (cap && !out)) return set_error(NSGPU_EINVAL, "nsgpu_udp_trace_load: null");
  std::vector<nsgpu_udp_trace_entry> v;
  uint32_t time = 0, index = 0, prevTime = 0;
  uint16_t size = 0;
  char frameType = 0;
  std::ifstream ifTraceFile;
  ifTraceFile.open(path, std::ifstream::in);
  if (!ifTraceFile.good()) load_default_trace(v);
  while (ifTraceFile.good()) {
    ifTraceFile >> index >> frameType >> time >> size;
    nsgpu_udp_trace_entry entry;
    if (frameType == 'B') {
      entry.time_to_send_ms = 0;
    } else {
      entry.time_to_send_ms = time - prevTime;
      prevTime = time;
    }
    entry.packet_size = size;
    v.push_back(entry);
  }
  ifTraceFile.close();
  return trace_out(v, out, cap, n);
}

// The fragmentation counters of a frag scenario (zeros without frag): the senders' from the device records, the
// receivers' from the nodes' reassembly state.  A partitioned engine reports what its own nodes did (another
// rank's nodes and devices stay zero here), so a group's totals are the ranks' sums and the largest max_list.
extern "C" int nsgpu_p2p_frag_stats(nsgpu_p2p *h, nsgpu_frag_stats *out, void *stream) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_frag_stats: null");
  hipStream_t s = (hipStream_t)stream;
  memset(out, 0, sizeof(*out));
  const P2PDev &M = h->M;
  if (!M.frag) return NSGPU_OK;
  std::vector<uint64_t> dv(2 * (size_t)M.n_devices);
  std::vector<FragNode> fn(h->frag_nf);
  if (M.n_devices)
    NSGPU_HIP(hipMemcpy2DAsync(dv.data(), 16, &M.dev[0].frag_dgrams, sizeof(DevRec), 16, M.n_devices,
                               hipMemcpyDeviceToHost, s));
  if (h->frag_nf)
    NSGPU_HIP(hipMemcpyAsync(fn.data(), frag_nodes(M.node_ipid, M.n_nodes), fn.size() * sizeof(FragNode),
                             hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (uint32_t d = 0; d < M.n_devices; d++) out->fragmented += dv[2 * d], out->fragments_sent += dv[2 * d + 1];
  for (const FragNode &f : fn) {
    out->reassembled += f.reassembled;
    out->timeouts += f.timeouts;
    out->cancelled_timers += f.cancelled;
    out->max_list = std::max<uint64_t>(out->max_list, f.maxlen);
  }
  return NSGPU_OK;
}

// The receive error models' counters per device (zeros without an enabled model).  A partitioned engine's models
// advance on the rank that owns the device's node; another rank's stay at zero here.
extern "C" int nsgpu_p2p_error_models(nsgpu_p2p *h, nsgpu_error_model_record *out, void *stream) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_error_models: null");
  hipStream_t s = (hipStream_t)stream;
  const P2PDev &M = h->M;
  memset(out, 0, M.n_devices * sizeof(*out));
  if (!h->em_models) return NSGPU_OK;
  std::vector<EmRec> er(h->em_models);
  NSGPU_HIP(hipMemcpyAsync(er.data(), em_recs(M.dev, M.n_devices), er.size() * sizeof(EmRec), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (const EmRec &r : er) out[r.dev] = nsgpu_error_model_record{r.invoked, r.corrupted};
  return NSGPU_OK;
}

// FlowMonitor's FlowStats per flow (zeros for an unmonitored engine): the three parts of each flow's record, and
// CheckForLostPackets (max_delay_ns) at the run's last dispatched time by the sweep kernel, which only reads.
extern "C" int nsgpu_p2p_flow_stats(nsgpu_p2p *h, int64_t max_delay_ns, nsgpu_flow_record *out, void *stream) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_p2p_flow_stats: null");
  if (max_delay_ns < 0) return set_error(NSGPU_EINVAL, "nsgpu_p2p_flow_stats: negative max_delay_ns");
  hipStream_t s = (hipStream_t)stream;
  const P2PDev &M = h->M;
  const uint32_t F = 2 * M.n_apps;
  memset(out, 0, (size_t)F * sizeof(*out));
  if (!M.flowmon || !F) return NSGPU_OK;
  Ctl c;
  NSGPU_HIP(hipMemcpyAsync(&c, M.C, sizeof(Ctl), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));  // (Simulator::Now () after Run: the sweep's `now`)
  NSGPU_HIP(hipMemsetAsync(h->fm_lost, 0, (size_t)F * sizeof(unsigned long long), s));
  launch_flow_sweep(M, (int64_t)c.last_ts, max_delay_ns, h->fm_entries, h->fm_lost, s);
  NSGPU_HIP(hipGetLastError());
  std::vector<FmTx> tx(F);
  std::vector<FmRx> rx(F);
  std::vector<FmDrop> dr(F);
  std::vector<unsigned long long> lost(F);
  static_assert(sizeof(FmTx) == sizeof(FmRx) && sizeof(FmRx) == sizeof(FmDrop), "the flows' records are one copy");
  NSGPU_HIP(hipMemcpyAsync(tx.data(), fm_tx(M.node_ipid, M.n_nodes), (size_t)F * sizeof(FmTx), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipMemcpyAsync(rx.data(), fm_rx(M.node_ipid, M.n_nodes, F), (size_t)F * sizeof(FmRx), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipMemcpyAsync(dr.data(), fm_drops(M.node_ipid, M.n_nodes, F), (size_t)F * sizeof(FmDrop), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipMemcpyAsync(lost.data(), h->fm_lost, (size_t)F * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (uint32_t f = 0; f < F; f++) {
    nsgpu_flow_record &o = out[f];
    o.tx_packets = tx[f].packets, o.tx_bytes = tx[f].bytes;
    o.time_first_tx_ns = tx[f].t_first, o.time_last_tx_ns = tx[f].t_last;
    o.first_tx_ts = tx[f].first_ts, o.first_tx_uid = tx[f].first_uid;
    o.rx_packets = rx[f].packets, o.rx_bytes = rx[f].bytes;
    o.delay_sum_ns = rx[f].delay_sum, o.jitter_sum_ns = rx[f].jitter_sum, o.last_delay_ns = rx[f].last_delay;
    o.time_first_rx_ns = rx[f].t_first, o.time_last_rx_ns = rx[f].t_last;
    o.times_forwarded = rx[f].forwarded;
    o.lost_packets = dr[f].lost + lost[f];
    for (uint32_t k = 0; k < NSGPU_FLOW_DROP_REASONS; k++)
      o.packets_dropped[k] = dr[f].packets[k], o.bytes_dropped[k] = dr[f].bytes[k];
  }
  return NSGPU_OK;
}

// The random OnOff times' draw counts per application (zeros without a random variable).  A partitioned engine's
// variables advance on the rank that owns the application's node; another rank's stay at zero here.
extern "C" int nsgpu_p2p_onoff_draws(nsgpu_p2p *h, nsgpu_onoff_draw_record *out, uint32_t n_apps, void *stream) {
  if (!h || (n_apps && !out)) return set_error(NSGPU_EINVAL, "nsgpu_p2p_onoff_draws: null");
  if (n_apps != h->M.n_apps) return set_error(NSGPU_EINVAL, "nsgpu_p2p_onoff_draws: the engine has %u applications", h->M.n_apps);
  hipStream_t s = (hipStream_t)stream;
  const P2PDev &M = h->M;
  memset(out, 0, (size_t)n_apps * sizeof(*out));
  if (!M.ranvar) return NSGPU_OK;
  std::vector<RvRec> rr(2 * (size_t)n_apps);
  NSGPU_HIP(hipMemcpyAsync(rr.data(), rv_recs(M.app_last_start, n_apps), rr.size() * sizeof(RvRec), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (uint32_t a = 0; a < n_apps; a++)
    out[a] = nsgpu_onoff_draw_record{rr[2 * a].draws, rr[2 * a + 1].draws, rr[2 * a].ambiguous + rr[2 * a + 1].ambiguous, 0};
  return NSGPU_OK;
}
// The log of ambiguous attempts: *n records (at most cap are written to out; out may be NULL with cap 0 to ask for
// the count) and the attempts beyond the log's NSGPU_RV_AMBIGUOUS_CAP records.
extern "C" int nsgpu_p2p_onoff_ambiguous(nsgpu_p2p *h, nsgpu_ambiguous_draw *out, uint64_t cap, uint64_t *n,
                                         uint64_t *overflow, void *stream) {
  if (!h || !n || !overflow || (cap && !out)) return set_error(NSGPU_EINVAL, "nsgpu_p2p_onoff_ambiguous: null");
  *n = *overflow = 0;
  const P2PDev &M = h->M;
  if (!M.ranvar) return NSGPU_OK;
  hipStream_t s = (hipStream_t)stream;
  RvHdr H;
  NSGPU_HIP(hipMemcpyAsync(&H, rv_hdr(M.app_last_start, M.n_apps), sizeof(H), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  const uint32_t cnt = std::min(H.log_n, NSGPU_RV_AMBIGUOUS_CAP);
  *n = cnt;
  *overflow = H.log_over;
  const uint64_t m = std::min<uint64_t>(cnt, cap);
  if (m) {
    NSGPU_HIP(hipMemcpyAsync(out, rv_log(M.app_last_start, M.n_apps), m * sizeof(*out), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipStreamSynchronize(s));
  }
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_results(nsgpu_p2p *h, nsgpu_p2p_stats *stats, nsgpu_dev_counters *devc,
                                 nsgpu_app_counters *appc, uint64_t *log_ts, uint32_t *log_uid, uint32_t *log_ctx,
                                 uint64_t log_n, uint32_t *error, void *stream) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_p2p_results: null");
  hipStream_t s = (hipStream_t)stream;
  const P2PDev &M = h->M;
  Ctl c;
  NSGPU_HIP(hipMemcpyAsync(&c, M.C, sizeof(Ctl), hipMemcpyDeviceToHost, s));
  if (devc)
    NSGPU_HIP(hipMemcpy2DAsync(devc, sizeof(*devc), &M.dev[0].c, sizeof(DevRec), sizeof(*devc), M.n_devices,
                               hipMemcpyDeviceToHost, s));
  if (appc) NSGPU_HIP(hipMemcpyAsync(appc, M.appc, M.n_apps * sizeof(*appc), hipMemcpyDeviceToHost, s));
  if (log_n > M.log_cap) log_n = M.log_cap;
  if (log_ts && log_n) NSGPU_HIP(hipMemcpyAsync(log_ts, M.log_ts, log_n * 8, hipMemcpyDeviceToHost, s));
  if (log_uid && log_n) NSGPU_HIP(hipMemcpyAsync(log_uid, M.log_uid, log_n * 4, hipMemcpyDeviceToHost, s));
  if (log_ctx && log_n) NSGPU_HIP(hipMemcpyAsync(log_ctx, M.log_ctx, log_n * 4, hipMemcpyDeviceToHost, s));
  uint32_t err = 0;
  NSGPU_HIP(hipMemcpyAsync(&err, M.error, 4, hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->dispatched = c.K;
    stats->digest = c.digest;
    stats->cancelled = c.cancelled;
    stats->final_ts = c.last_ts;
    stats->next_uid = c.uid;
    stats->windows = (uint32_t)c.windows;
    stats->ttl_drops = c.ttl_drops;
    stats->no_route_drops = c.no_route;
    stats->max_window = c.max_window;
    stats->unreach_drops = c.unreach;
    stats->icmp_sent = c.icmp;
    stats->refits = c.refits;
  }
  if (error) *error = err;
  if (err) return engine_error(err);
  return NSGPU_OK;
}

// ====================================================================================================
// Loopback group: every partition of one scenario on this device, the collectives replaced by
// device-to-device copies (k_copies) on one stream — the partitioned algorithm's parity harness on
// a single GPU.  Members are nsgpu_p2p_create_dist engines with comm == NULL, rank i at index i.
// ====================================================================================================
struct nsgpu_p2p_group {
  std::vector<nsgpu_p2p *> m;
  CopyDesc *d_x[4] = {nullptr, nullptr, nullptr, nullptr};  // X0, X1, X2, the cut's keys: n x n copies each
  hipStream_t s = nullptr;
  hipGraphExec_t gexec = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  Ctl *snap = nullptr;  // pinned, 2 run-control snapshots of member 0 (the pauses are run-global)
};

static void launch_windows_group(nsgpu_p2p_group *g, hipStream_t s, int nwin = NWIN) {
  const unsigned n = (unsigned)g->m.size();
  for (int w = 0; w < nwin; w++) {
    for (auto *h : g->m) dist_pa(h->M, s);
    hipLaunchKernelGGL(k_copies, dim3(n * n), dim3(256), 0, s, (const CopyDesc *)g->d_x[0]);
    for (auto *h : g->m) dist_handle(h->M, s, h->loss_init != nullptr || h->M.frag != 0 || h->M.errm != 0 || h->M.ranvar != 0);
    for (auto *h : g->m) dist_rank(h->M, s);
    hipLaunchKernelGGL(k_copies, dim3(n * n), dim3(256), 0, s, (const CopyDesc *)g->d_x[1]);
    for (auto *h : g->m) dist_rank_fin(h->M, s);
    hipLaunchKernelGGL(k_copies, dim3(n * n), dim3(256), 0, s, (const CopyDesc *)g->d_x[2]);
  }
}

extern "C" int nsgpu_p2p_group_destroy(nsgpu_p2p_group *g) {
  if (!g) return NSGPU_OK;
  if (g->s) (void)hipStreamSynchronize(g->s);
  if (g->gexec) (void)hipGraphExecDestroy(g->gexec);
  for (hipEvent_t e : {g->ev[0], g->ev[1]})
    if (e) (void)hipEventDestroy(e);
  if (g->snap) (void)hipHostFree(g->snap);
  for (CopyDesc *d : g->d_x)
    if (d) (void)hipFree(d);
  if (g->s) (void)hipStreamDestroy(g->s);
  delete g;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_group_create(nsgpu_p2p **members, int n, nsgpu_p2p_group **out) {
  if (!members || !out || n < 1) return set_error(NSGPU_EINVAL, "nsgpu_p2p_group_create: bad arguments");
  *out = nullptr;
  for (int i = 0; i < n; i++) {
    const nsgpu_p2p *h = members[i];
    if (!h || !h->M.dist || h->comm || h->M.nranks != (uint32_t)n || h->M.rank != (uint32_t)i)
      return set_error(NSGPU_EINVAL, "nsgpu_p2p_group_create: member %d is not loopback partition %d of %d", i, i, n);
  }
  nsgpu_p2p_group *g = new nsgpu_p2p_group();
  g->m.assign(members, members + n);
  std::vector<CopyDesc> x[4];
  for (int r = 0; r < n; r++)
    for (int q = 0; q < n; q++) {
      const P2PDev &R = members[r]->M, &Q = members[q]->M;
      x[0].push_back(CopyDesc{(const uint8_t *)Q.x0_send, (uint8_t *)(R.x0_recv + 2 * q), X0B});
      x[1].push_back(CopyDesc{Q.x1_send, R.x1_recv + (size_t)q * X1B, X1B});
      x[2].push_back(CopyDesc{Q.x2_send + (size_t)r * Q.x2b, R.x2_recv + (size_t)q * R.x2b, Q.x2b});
      x[3].push_back(CopyDesc{(const uint8_t *)Q.xk_send, (uint8_t *)(R.xk_recv + 2 * q), 16});
    }
  for (int k = 0; k < 4; k++) {
    if (hipMalloc(&g->d_x[k], x[k].size() * sizeof(CopyDesc)) != hipSuccess ||
        hipMemcpy(g->d_x[k], x[k].data(), x[k].size() * sizeof(CopyDesc), hipMemcpyHostToDevice) != hipSuccess) {
      nsgpu_p2p_group_destroy(g);
      return set_error(NSGPU_ENOMEM, "nsgpu_p2p_group_create: copy descriptors");
    }
  }
  if (hipStreamCreateWithFlags(&g->s, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&g->ev[1], hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc((void **)&g->snap, 2 * sizeof(Ctl), hipHostMallocDefault) != hipSuccess) {
    nsgpu_p2p_group_destroy(g);
    return set_error(NSGPU_EHIP, "nsgpu_p2p_group_create: stream / events");
  }
  *out = g;
  return NSGPU_OK;
}

extern "C" int nsgpu_p2p_group_reset(nsgpu_p2p_group *g, void *stream) {
  if (!g) return set_error(NSGPU_EINVAL, "nsgpu_p2p_group_reset: null");
  for (nsgpu_p2p *h : g->m) {
    const int rc = nsgpu_p2p_reset(h, stream);
    if (rc) return rc;
  }
  return NSGPU_OK;
}

// The host-driven steps of a group (host_step_dist's, every member): the cut's keys go through k_copies.
static int group_host_step(nsgpu_p2p_group *g, const Ctl &c0) {
  hipStream_t s = g->s;
  const bool cut = c0.mode == MODE_CUT;  // a partitioned sorted run starts
  for (auto *h : g->m) {  // (every member from its own run control)
    Ctl c;
    NSGPU_HIP(hipMemcpyAsync(&c, h->M.C, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipStreamSynchronize(s));
    const int rc = cut ? drun_sort(h, c.W, s) : host_step(h, c, s);
    if (rc) return rc;
  }
  if (!cut) return NSGPU_OK;
  const unsigned n = (unsigned)g->m.size();
  hipLaunchKernelGGL(k_copies, dim3(n * n), dim3(256), 0, s, (const CopyDesc *)g->d_x[3]);
  for (auto *h : g->m) hipLaunchKernelGGL(k_drun_first, dim3(WCAP / TB), dim3(TB), 0, s, h->M);
  NSGPU_HIP(hipGetLastError());
  return NSGPU_OK;
}

// Runs every partition to the end of the simulation (blocking), like nsgpu_p2p_run.
extern "C" int nsgpu_p2p_group_run(nsgpu_p2p_group *g, void *stream) {
  if (!g) return set_error(NSGPU_EINVAL, "nsgpu_p2p_group_run: null");
  static const bool eager = env_eager();
  if (!eager && !g->gexec) {
    const int rc = capture_graph(g->s, hipStreamCaptureModeThreadLocal, "nsgpu_p2p_group", &g->gexec, [g] {
      launch_windows_group(g, g->s);
      return NSGPU_OK;
    });
    if (rc) return rc;
  }
  hipStream_t cs = (hipStream_t)stream;
  NSGPU_HIP(hipEventRecord(g->ev[0], cs));
  NSGPU_HIP(hipStreamWaitEvent(g->s, g->ev[0], 0));
  auto launch = [g](int) -> int {
    if (eager) launch_windows_group(g, g->s);
    else NSGPU_HIP(hipGraphLaunch(g->gexec, g->s));
    NSGPU_HIP(hipGetLastError());
    return NSGPU_OK;
  };
  auto pause = [g](int slot, bool *) -> int { return group_host_step(g, g->snap[slot]); };
  auto seen = [](const Ctl &) -> int { return NSGPU_OK; };
  // as drive_dist: member 0's run control decides (done and the pauses are run-global)
  if (const int rc = replay_loop(g->s, g->m[0]->M.C, g->snap, g->ev, launch, pause, seen)) return rc;
  NSGPU_HIP(hipEventRecord(g->ev[0], g->s));
  NSGPU_HIP(hipEventSynchronize(g->ev[0]));
  NSGPU_HIP(hipStreamWaitEvent(cs, g->ev[0], 0));
  uint32_t err = 0;
  for (nsgpu_p2p *m : g->m) {  // (as nsgpu_p2p_run: a member's error word fails the run)
    uint32_t e = 0;
    NSGPU_HIP(hipMemcpy(&e, m->M.error, 4, hipMemcpyDeviceToHost));
    err |= e;
  }
  if (err) return engine_error(err);
  return NSGPU_OK;
}
