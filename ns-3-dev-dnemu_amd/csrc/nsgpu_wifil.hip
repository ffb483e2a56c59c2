// nsgpu_wifil.hip — the closed-loop Wi-Fi PHY on the device (include/nsgpu.h: nsgpu_wifil_*, and
// nsgpu_sim_attach_wifi / nsgpu_sim_wifi_send / nsgpu_sim_wifi_state in nsgpu_simimpl.hip).
//
// Replaces, for transmissions that host closures start at run time (a MAC on the host):
// YansWifiPhy::SendPacket (yans-wifi-phy.cc:499-522) -> YansWifiChannel::Send (yans-wifi-channel.cc:77-115)
// -> YansWifiPhy::StartReceivePacket (yans-wifi-phy.cc:399-496) with InterferenceHelper::Add / AppendEvent /
// GetEnergyDuration (interference-helper.cc:129-212), the WifiPhyStateHelper transitions
// (wifi-phy-state-helper.cc:122-183, 254-322, 391-423), and YansWifiPhy::EndReceive (yans-wifi-phy.cc:770-799)
// with InterferenceHelper::CalculateSnrPer (interference-helper.cc:215-353) and the error-rate models
// (nist-error-rate-model.cc, yans-error-rate-model.cc, dsss-error-rate-model.cc).  EndReceive's m_random
// draw (:783) is the host's: each EndReceive's (snr, per) goes back to it (nsgpu_wifil_read_ends).
//
// Epochs.  The host runtime (nsgpu_sim) owns the uid counter and the dispatch order; before it runs a host
// closure with key (T, u) it advances the device to that key (nsgpu_wifil_advance): every phy's wave runs
// its pending Receive / EndReceive events with keys below (T, u), in (ts, uid) order, then the epoch's
// syncs get their EndReceive uids.  A host closure's SendPacket (nsgpu_wifil_send) applies the sender's
// state switch at once and queues one Receive per receiver, with the uids the runtime hands out.
// Order inside one phy needs no global rank: every Receive's uid is known when it is queued (the runtime's
// counter at the SendPacket), and an EndReceive scheduled in the running epoch has a uid above every uid
// handed out before the epoch — so it sorts after those at equal ts, and among themselves by their syncing
// Receives' keys (uids follow the dispatch order of the events that schedule them).
//
// State per phy lives in HBM between epochs: the InterferenceHelper list as a time-sorted ring (the r02
// RingNi layout of nsgpu_wifi.hip, with its eager prefix cursor), the state helper's end times, the pending
// Receive queue (sorted by (arrival, uid)) and up to LPE_CAP pending EndReceive records.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "nsgpu_waypool.h"
#include "nsgpu_wifil_dev.h"

using namespace nsgpu;

// ---- a partitioned PHY (nsgpu_wifil_create_dist / nsgpu_wifil_create_group): its handle is the host side
// every rank replicates (the MAC's closures, the uids, GetState, the ends) and owns one of these; `mem` are the
// partitions it runs — one (RCCL: `comm`, the others on other GPUs) or all of them (a loopback group on this
// device) — each an engine over its phys [lo, hi) with every array indexed by the global phy, launched on the
// handle's stream (a member has no stream, second stream or events of its own).  The device arrays named here are
// in the handle's `allocs`.
struct WlGroup {
  std::vector<nsgpu_wifil *> mem;
  nsgpu_comm *comm = nullptr;
  std::vector<int64_t> plo, phi;  // every partition's phys (RCCL: gathered at create)
  int64_t pmax = 0;               // the largest partition (the gathers' padding)
  WDev U{};                       // the order over every partition's events (k_wl_tsort / k_wl_rank)
  LSync *xsync = nullptr;         // every partition's syncs of the epoch
  LSync *xsr = nullptr;           // (RCCL) their gather, padded
  LEv *xev = nullptr;             // (RCCL) the events' gather, padded
  nsgpu_wifil_end *uend = nullptr, *xend = nullptr;  // every partition's end records; (RCCL) their gather, padded
  WMir *xmir = nullptr, *dmir = nullptr, *smir = nullptr;  // (RCCL) mirror: gather, the partition's, send staging
  uint8_t *xps = nullptr, *sps = nullptr;                  // (RCCL) phy states for read_phys: gather, staging
  unsigned long long *xsm = nullptr, *ssm = nullptr;       // (RCCL) small per-rank words: gather, send
  uint64_t g_sync_cap = 0;                                 // the single engine's sync capacity (the union's)
};

struct nsgpu_wifil {
  WDev D{};
  hipStream_t s = nullptr;
  std::vector<void *> allocs;
  std::vector<uint32_t> recv;  // fan-out uids of one SendPacket per phy
  uint64_t n_tx = 0, tx_cap = 0;
  SendBatch sb{};  // SendPackets not yet applied (the next epoch launch applies them; k_wl_send past NSEND)
  // mapped host memory: the epoch's status block — counters, digest sum, first END_STAGE end records (the
  // device's D.cnt / D.edig / D.ends are laid out the same way in one allocation) — k_wl_rank writes it
  uint8_t *h_stat = nullptr, *d_stat = nullptr;  // (mapped: k_wl_rank writes it; d_stat is its device address)
  uint8_t *stat[2] = {nullptr, nullptr};  // the device's status blocks, by epoch parity (the next one is zeroed
  uint32_t par = 0;                       //   by the running epoch's k_wl_tsort: no fills between epochs)
  uint32_t *evc[2] = {nullptr, nullptr};  // the event-list stripe counters, by epoch parity (likewise)
  uint32_t *h_cnt = nullptr;
  LEv *evb[2] = {nullptr, nullptr};      // the event lists, by epoch parity (the order reads them an epoch behind)
  LEv *evpb[2] = {nullptr, nullptr};     // the phys' own event slots, by epoch parity (likewise)
  uint32_t *evnb[2] = {nullptr, nullptr};
  uint32_t *evtb[2] = {nullptr, nullptr};  // their striped totals, by epoch parity
  LSync *syncb[2] = {nullptr, nullptr};  // the syncs, by epoch parity (likewise)
  hipStream_t s2 = nullptr;              // the epochs' order (k_wl_tsort / k_wl_rank)
  hipEvent_t ev_fin[2] = {nullptr, nullptr}, ev_ord[2] = {nullptr, nullptr};
  bool ord_pending[2] = {false, false};  // an order of this parity's epoch was launched and not yet waited for
  unsigned long long *h_digtot = nullptr, *d_digtot = nullptr;  // (mapped) the ordered epochs' digest sum
  uint64_t dig_added = 0;                // the part of it already added to a caller's digest
  uint32_t seq = 0;                      // epochs launched (the close's flag)
  nsgpu_wifil_end *h_ends = nullptr;
  WMir *h_mir = nullptr;                 // mapped host memory: every phy's state fields (D.mir; GetState)
  std::vector<uint32_t> erank;
  unsigned long long *d_pend = nullptr, *h_pend = nullptr;
  std::vector<LEv> ev;
  std::vector<nsgpu_wifil_end> ends, ends_epoch;
  // the EndReceive hand-back: listened phys (a flag each, and the list the device scans), each phy's node
  std::vector<uint8_t> lis_on;
  std::vector<uint32_t> lis_list, node_h;
  bool lis_dirty = false;
  uint32_t *d_lis = nullptr;
  unsigned long long *d_next = nullptr, *h_next = nullptr;
  // RxStart / CCA-busy notifications: the notifying phys (a flag each; their count picks the epoch kernel), the
  // notes of the epochs advanced and not yet read, and the last epoch's (sorted by (ts, uid))
  std::vector<uint8_t> note_on;
  uint64_t n_note_on = 0;
  uint32_t *d_note_on = nullptr;
  std::vector<nsgpu_wifil_note> notes, notes_epoch;
  // mobility: every phy's model kind (MOVE_*; empty until the first install; the count of phys with one decides
  // whether a send launches k_wl_move), the waypoint phys' lists and segments of the pool D.wpool (nsgpu_waypool.h;
  // the pool is not in `allocs`: it is replaced when it grows), and the device word the three reads come back through
  std::vector<uint8_t> mov_kind;
  uint64_t n_mov = 0;
  std::vector<WaySeg> seg;
  WayPool wpool;
  MoveOut *d_movout = nullptr;
  // channel switching (nsgpu_wifil_set_channel): every phy's current channel number (the receiver counts in `recv`
  // follow it), the switches made (non-zero: the epochs launch the SW instantiation) and k_wl_rechan's count word
  // (allocated at the first call)
  std::vector<uint32_t> chan_h;
  uint64_t n_switches = 0;
  uint32_t *d_nbefore = nullptr;
  // the extended loss chain (nsgpu_wifil_set_loss): one device block [LossX | loss | row | col] of lx_cap bytes, written
  // on `s` from the pinned block lx_pin (lx_up: the last upload, waited for before lx_pin is written again); D.lx
  // names the device block while a chain is installed
  uint8_t *lx_dev = nullptr, *lx_pin = nullptr;
  size_t lx_cap = 0;
  hipEvent_t lx_up = nullptr;
  std::vector<unsigned long long> words;  // the between-epoch queries' words, k a partition (wl_words)
  WlGroup *grp = nullptr;         // a partitioned PHY's handle: its partitions and exchange buffers (else null)
};

// Blocks of b threads over n phys (at least one: a partition with no phys still records a transmission, and
// its kernels return at once).
static unsigned wl_grid(int64_t n, int b) { return (unsigned)std::max<int64_t>((n + b - 1) / b, 1); }

// The epoch's status block (counters, digest, end records) is stat[b].
static void wl_use_stat(nsgpu_wifil *h, uint32_t b) {
  h->par = b;
  h->D.cnt = reinterpret_cast<uint32_t *>(h->stat[b]);
  h->D.ev = h->evb[b];
  h->D.evp = h->evpb[b];
  h->D.evn = h->evnb[b];
  h->D.evt = h->evtb[b];
  h->D.sync = h->syncb[b];
  h->D.ends = reinterpret_cast<nsgpu_wifil_end *>(h->stat[b] + STAT_HDR);
  h->D.evc = h->evc[b];
}

template <class T>
static int wl_alloc(nsgpu_wifil *h, T **p, size_t n, const T *src = nullptr) {
  void *v = nullptr;
  NSGPU_HIP(hipMalloc(&v, std::max<size_t>(n, 1) * sizeof(T)));
  h->allocs.push_back(v);
  if (src && n) NSGPU_HIP(hipMemcpy(v, src, n * sizeof(T), hipMemcpyHostToDevice));
  else NSGPU_HIP(hipMemset(v, 0, std::max<size_t>(n, 1) * sizeof(T)));
  *p = (T *)v;
  return NSGPU_OK;
}

extern "C" int nsgpu_wifil_destroy(nsgpu_wifil *h) {
  if (!h) return NSGPU_OK;
  if (h->s) (void)hipStreamSynchronize(h->s);
  if (h->grp) {
    for (nsgpu_wifil *m : h->grp->mem) {  // (a partition runs on this handle's stream)
      m->s = nullptr;
      nsgpu_wifil_destroy(m);
    }
    delete h->grp;
  }
  for (hipStream_t q : {h->s, h->s2})
    if (q) {
      (void)hipStreamSynchronize(q);
      (void)hipStreamDestroy(q);
    }
  for (int b = 0; b < 2; b++) {
    if (h->ev_fin[b]) (void)hipEventDestroy(h->ev_fin[b]);
    if (h->ev_ord[b]) (void)hipEventDestroy(h->ev_ord[b]);
  }
  if (h->h_digtot) (void)hipHostFree(h->h_digtot);
  for (void *p : h->allocs) (void)hipFree(p);
  if (h->D.wpool) (void)hipFree(h->D.wpool);
  if (h->lx_dev) (void)hipFree(h->lx_dev);
  if (h->lx_pin) (void)hipHostFree(h->lx_pin);
  if (h->lx_up) (void)hipEventDestroy(h->lx_up);
  if (h->h_stat) (void)hipHostFree(h->h_stat);
  if (h->h_mir) (void)hipHostFree(h->h_mir);
  if (h->h_pend) (void)hipHostFree(h->h_pend);
  if (h->h_next) (void)hipHostFree(h->h_next);
  delete h;
  return NSGPU_OK;
}

// (hipDeviceGetStreamPriorityRange: greatest = the most urgent, a smaller number)
static int wl_prio(bool high) {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
  return high ? greatest : least;
}

// Each phy's place among the phys of its channel (YansWifiChannel::Send's receiver loop, m_phyList order) and the
// Receives one SendPacket of it schedules (the other phys of its channel).
static void wl_channel_ranks(const nsgpu_wifil_config *c, std::vector<uint32_t> &rank, std::vector<uint32_t> &recv) {
  const int64_t N = c->n_phy;
  rank.assign((size_t)N, 0);
  recv.assign((size_t)N, 0);
  std::vector<std::pair<uint32_t, uint32_t>> cnt;  // (channel, count so far)
  for (int64_t j = 0; j < N; j++) {
    auto it = std::find_if(cnt.begin(), cnt.end(), [&](const std::pair<uint32_t, uint32_t> &p) { return p.first == c->channel[j]; });
    if (it == cnt.end()) cnt.emplace_back(c->channel[j], 0), it = cnt.end() - 1;
    rank[j] = it->second++;
  }
  for (int64_t j = 0; j < N; j++)
    for (auto &p : cnt)
      if (p.first == c->channel[j]) recv[j] = p.second - 1;
}

// An engine over phys [j0, j0 + nown) of the config (the single engine: all of them); its epoch lists are sized
// for capn phys (a partition: the largest partition's, so that every rank's lists hold a gather's padding).  `on`:
// the stream a partition's handle runs it on (it then makes no stream, second stream or events: it launches no
// order of its own); null: the single engine, on streams of its own.
static int wl_create(const nsgpu_wifil_config *c, int64_t j0, int64_t nown, int64_t capn, hipStream_t on, nsgpu_wifil **out) {
  if (!c || !out || c->n_phy <= 0 || !c->x || !c->y || !c->z || !c->channel || !c->node)
    return set_error(NSGPU_EINVAL, "nsgpu_wifil_create: bad config");
  const auto pow2 = [](uint32_t v) { return v >= 2 && (v & (v - 1)) == 0; };
  if (!pow2(c->ni_cap) || !pow2(c->rxq_cap) || c->tx_cap == 0 || c->tx_cap >= 0xffffffffull || c->loss.n < 0 ||
      c->loss.n > NSGPU_MAX_LOSS_CHAIN || c->error_model > NSGPU_WIFIL_YANS)
    return set_error(NSGPU_EINVAL, "nsgpu_wifil_create: ni_cap / rxq_cap must be powers of two >= 2, tx_cap in (0, 2^32)");
  nsgpu_wifil *h = new nsgpu_wifil();
  const int64_t N = c->n_phy;
  WDev &D = h->D;
  D.nphy = N;
  D.j0 = j0;
  D.nown = nown;
  D.loss = c->loss;
  D.speed = c->speed;
  D.rx_gain_db = c->rx_gain_db;
  D.edW = pow(10.0, c->ed_threshold_dbm / 10.0) / 1000.0;   // SetEdThreshold (yans-wifi-phy.cc:228-232)
  D.ccaW = pow(10.0, c->cca_threshold_dbm / 10.0) / 1000.0; // SetCcaMode1Threshold (:234-238)
  D.nf = pow(10.0, c->rx_noise_figure_db / 10.0);           // SetRxNoiseFigure: DbToRatio (:192-197)
  D.model = c->error_model;
  D.ni_mask = c->ni_cap - 1;
  D.rq_mask = c->rxq_cap - 1;
  const u128 inv = invert(1000000000ull);
  D.inv_hi = (uint64_t)(inv >> 64);
  D.inv_lo = (uint64_t)inv;
  // the receiver loop's order on each channel (m_phyList order)
  std::vector<uint32_t> rank;
  wl_channel_ranks(c, rank, h->recv);
  const uint64_t ev_cap = (uint64_t)capn * 64 + 4096, sync_cap = (uint64_t)capn * LPE_CAP + 1024;
  int rc;
#define WL_TRY(x)                \
  if ((rc = (x)) != NSGPU_OK) {  \
    nsgpu_wifil_destroy(h);      \
    return rc;                   \
  }
  WL_TRY(wl_alloc(h, (double **)&D.x, N, c->x));
  WL_TRY(wl_alloc(h, (double **)&D.y, N, c->y));
  WL_TRY(wl_alloc(h, (double **)&D.z, N, c->z));
  WL_TRY(wl_alloc(h, (uint32_t **)&D.chan, N, c->channel));
  WL_TRY(wl_alloc(h, (uint32_t **)&D.node, N, c->node));
  WL_TRY(wl_alloc(h, (uint32_t **)&D.chan_rank, N, rank.data()));
  std::vector<LPhy> ps((size_t)N);
  for (auto &p : ps) p.live = NONE;
  WL_TRY(wl_alloc(h, &D.ps, N, ps.data()));
  WL_TRY(wl_alloc(h, &D.ni, (size_t)N * c->ni_cap));
  WL_TRY(wl_alloc(h, &D.rq, (size_t)N * c->rxq_cap));
  WL_TRY(wl_alloc(h, &D.pe, (size_t)N * LPE_CAP));
  WL_TRY(wl_alloc(h, &D.tx, c->tx_cap));
  WL_TRY(wl_alloc(h, &D.edig, 1));
  for (int b = 0; b < 2; b++) {  // [cnt x 5 | pad | edig | ends x sync_cap], two of them (epoch parity)
    WL_TRY(wl_alloc(h, &h->stat[b], STAT_HDR + sync_cap * sizeof(nsgpu_wifil_end)));
    WL_TRY(wl_alloc(h, &h->evc[b], (size_t)EV_STRIPES * EV_STRIDE));
    WL_TRY(wl_alloc(h, &h->evb[b], ev_cap));
    WL_TRY(wl_alloc(h, &h->evpb[b], (size_t)N * EVB));
    WL_TRY(wl_alloc(h, &h->evnb[b], (size_t)N));
    WL_TRY(wl_alloc(h, &h->evtb[b], (size_t)EV_STRIPES * EV_STRIDE));
    WL_TRY(wl_alloc(h, &h->syncb[b], sync_cap));
  }
  WL_TRY(wl_alloc(h, &D.evd, (size_t)N * EVB + ev_cap));  // (the slots' events, then the stripes')
  D.ev_scap = ev_cap / EV_STRIPES;
  wl_use_stat(h, 0);
  WL_TRY(wl_alloc(h, &D.end_sslot, sync_cap));
  WL_TRY(wl_alloc(h, &D.eck, sync_cap));
  // deferred chunks an epoch (~100-600 an EndReceive): 64 MB, or 512 a phy (k_wl_stepw has no inline
  // fallback — its error-rate models would take ~130 more VGPRs and scratch from every lane: a full pool
  // fails the run, WE_CKCAP)
  D.ck_cap = std::max<uint64_t>(1ull << 22, (uint64_t)capn * 512);
  WL_TRY(wl_alloc(h, &D.ck, (size_t)D.ck_cap));
  WL_TRY(wl_alloc(h, &D.erank, std::min<uint64_t>(ev_cap, ERANK_MAX)));
  WL_TRY(wl_alloc(h, &D.ticket, 1));
  WL_TRY(wl_alloc(h, &D.mticket, 1));
  WL_TRY(wl_alloc(h, &D.gtot, 1));
  WL_TRY(wl_alloc(h, &D.rxb, (size_t)NSEND * N));
  WL_TRY(wl_alloc(h, &D.evg, std::min<uint64_t>(ev_cap, ERANK_MAX)));
  WL_TRY(wl_alloc(h, &h->d_pend, 2));
  WL_TRY(wl_alloc(h, &h->d_next, 4));
  WL_TRY(wl_alloc(h, &h->d_lis, (size_t)N));
  D.lis = h->d_lis;
  D.nlis = 0;
  h->lis_on.assign((size_t)N, 0);
  h->node_h.assign(c->node, c->node + N);
  h->chan_h.assign(c->channel, c->channel + N);
#undef WL_TRY
  D.sync_cap = sync_cap;
  D.ev_cap = ev_cap;
  D.end_cap = sync_cap;
  h->tx_cap = c->tx_cap;
  // the PHY's epochs on a high-priority stream, the order behind them on a low-priority one: streams of
  // different priorities never share a hardware queue (with GPU_MAX_HW_QUEUES = 4 and other engines' streams
  // alive, two normal streams could land on one queue, and the order's ~55 us would then run in line with
  // the next epoch: 75 -> 112 us an epoch, VERDICT r05 item 2, scripts/wifil_interference.py)
  const auto own_streams = [h] {
    return hipStreamCreateWithPriority(&h->s, hipStreamNonBlocking, wl_prio(true)) == hipSuccess &&
           hipStreamCreateWithPriority(&h->s2, hipStreamNonBlocking, wl_prio(false)) == hipSuccess &&
           hipEventCreateWithFlags(&h->ev_fin[0], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&h->ev_fin[1], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&h->ev_ord[0], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&h->ev_ord[1], hipEventDisableTiming) == hipSuccess;
  };
  if (hipHostMalloc((void **)&h->h_stat, STAT_HDR + END_STAGE * sizeof(nsgpu_wifil_end),
                    hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void **)&h->d_stat, h->h_stat, 0) != hipSuccess ||
      hipHostMalloc((void **)&h->h_mir, (size_t)N * sizeof(WMir), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void **)&D.mir, h->h_mir, 0) != hipSuccess ||
      hipHostMalloc((void **)&h->h_pend, 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&h->h_next, 4 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void **)&h->h_digtot, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void **)&h->d_digtot, h->h_digtot, 0) != hipSuccess ||
      (!on && !own_streams())) {
    nsgpu_wifil_destroy(h);
    return set_error(NSGPU_EHIP, "nsgpu_wifil_create: host buffers / stream");
  }
  if (on) h->s = on;
  h->h_cnt = reinterpret_cast<uint32_t *>(h->h_stat);
  h->h_ends = reinterpret_cast<nsgpu_wifil_end *>(h->h_stat + STAT_HDR);
  *h->h_digtot = 0;
  std::memset(h->h_mir, 0, (size_t)N * sizeof(WMir));  // (the phys' initial state: every end time 0, not receiving)
  *out = h;
  return NSGPU_OK;
}

extern "C" int nsgpu_wifil_create(const nsgpu_wifil_config *c, nsgpu_wifil **out) {
  if (!c || !out) return set_error(NSGPU_EINVAL, "nsgpu_wifil_create: bad config");
  return wl_create(c, 0, c->n_phy, c->n_phy, nullptr, out);
}

extern "C" int nsgpu_wifil_receivers(nsgpu_wifil *h, uint32_t phy, uint32_t *n) {
  if (!h || !n || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_receivers: bad phy");
  *n = h->recv[phy];
  return NSGPU_OK;
}

// YansWifiChannel::Send's ScheduleWithContext calls for one SendPacket of `sender` (yans-wifi-channel.cc:77-115),
// on the host: every other phy of m_phyList on the sender's channel number, in list order, gets the Receive with
// uid uid_base + its place and the context of its device's node (0xffffffff: a phy without a device).  This is the
// uid-critical half of a binding's Send (nsgpu_sim_wifi_send hands out the same block); no device is touched.
extern "C" int nsgpu_wifil_send_plan(const nsgpu_wifil_config *c, uint32_t sender, uint32_t uid_base, uint32_t *rx_phy,
                                     uint32_t *rx_uid, uint32_t *rx_ctx, uint64_t cap, uint64_t *n) {
  if (!c || !n || !c->channel || !c->node || (int64_t)sender >= c->n_phy)
    return set_error(NSGPU_EINVAL, "nsgpu_wifil_send_plan: bad config / sender");
  uint64_t k = 0;
  for (int64_t j = 0; j < c->n_phy; j++) {
    if ((uint32_t)j == sender || c->channel[j] != c->channel[sender]) continue;  // (:86-91)
    if ((uint64_t)uid_base + k >= nsgpu::UID_NEXT_MAX) return nsgpu::uid_range_error("nsgpu_wifil_send_plan");
    if (k < cap) {
      if (rx_phy) rx_phy[k] = (uint32_t)j;
      if (rx_uid) rx_uid[k] = uid_base + (uint32_t)k;
      if (rx_ctx) rx_ctx[k] = c->node[j];  // dstNode (:101-110)
    }
    k++;
  }
  *n = k;
  return NSGPU_OK;
}

static int wl_check_bits(uint32_t e, const char *what) {
  if (!e) return NSGPU_OK;
  if (e & WE_TX_IN_TX)
    return set_error(NSGPU_ESTATE, "%s: SendPacket while transmitting (yans-wifi-phy.cc:508 NS_ASSERT)", what);
  if (e & WE_TX_IN_SWITCHING)
    return set_error(NSGPU_ESTATE, "%s: SendPacket while switching channels (yans-wifi-phy.cc:508 NS_ASSERT)", what);
  return set_error(NSGPU_ENOMEM, "%s: capacity exceeded (bits %u: 2 NiChanges ring, 4 Receive queue, 8 pending "
                                 "EndReceive records, 16 epoch lists, 32 CalculatePer chunk pool, 64 epoch notes)", what, e);
}
static int wl_check(nsgpu_wifil *h, const char *what) { return wl_check_bits(h->h_cnt[3], what); }

// What a partitioned handle refuses (`feature`: "mobility is", ...), with the entry point's own code.
static int wl_single_only(const nsgpu_wifil *h, int code, const char *what, const char *feature) {
  if (!h->grp) return NSGPU_OK;
  return set_error(code, "%s: %s single-engine for now (a partitioned handle)", what, feature);
}

// The batched SendPackets as k_wl_send launches (before anything that reads the phys or moves one).
static int wl_flush_sends(nsgpu_wifil *h) {
  const unsigned g = wl_grid(h->D.nown, 256);
  const auto kern = h->D.lx ? k_wl_send<true> : k_wl_send<false>;  // (an extended chain is installed: its instantiation)
  for (uint32_t i = 0; i < h->sb.n; i++)
    hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, h->s, h->D, h->sb.k0 + i, h->sb.t[i], h->sb.dbm[i], h->sb.base[i]);
  h->sb.n = 0;
  NSGPU_HIP(hipGetLastError());
  return NSGPU_OK;
}

static int wl_queue_send(nsgpu_wifil *h, const LTx &t, double dbm, uint32_t uid_base);

// YansWifiPhy::SendPacket of `phy` from the host closure running at (now, closure uid); its fan-out takes
// the uids uid_base .. uid_base + receivers - 1 (nsgpu_wifil_receivers).
extern "C" int nsgpu_wifil_send(nsgpu_wifil *h, uint64_t now, uint32_t uid_base, uint32_t phy, uint32_t size, double dbm,
                                uint32_t modclass, uint64_t rate, uint32_t bw, uint32_t preamble) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_send: bad phy");
  if (h->n_tx >= h->tx_cap) return set_error(NSGPU_ENOMEM, "nsgpu_wifil_send: tx_cap SendPacket calls");
  uint32_t nrx = 0;
  int rc0 = nsgpu_wifil_receivers(h, phy, &nrx);
  if (rc0) return rc0;
  if ((uint64_t)uid_base + nrx > nsgpu::UID_NEXT_MAX) return nsgpu::uid_range_error("nsgpu_wifil_send");
  int64_t dur = 0;
  int rc = nsgpu_wifi_tx_duration_ns(size, modclass, rate, bw, preamble, &dur);  // CalculateTxDuration
  if (rc) return rc;
  const LTx t{now, dur, rate, phy, modclass, bw, preamble};
  WMir &mr = h->h_mir[phy];  // the sender's switch (k_wl_send's), in the host's copy of its state fields
  if (!(mr.endTx > (int64_t)now) && !(mr.endSw > (int64_t)now)) {
    if (mr.rxing) mr.rxing = 0, mr.endRx = (int64_t)now;
    mr.endTx = (int64_t)now + dur;
  }
  if (!h->grp) return wl_queue_send(h, t, dbm, uid_base);
  h->n_tx++;
  for (nsgpu_wifil *m : h->grp->mem)  // (every partition records the transmission; its receivers take their Receives)
    if (int rcm = wl_queue_send(m, t, dbm, uid_base)) return rcm;
  return NSGPU_OK;
}

// A SendPacket into the engine's batch (applied by its next epoch launch), its Receives computed now (k_wl_rx).
static int wl_queue_send(nsgpu_wifil *h, const LTx &t, double dbm, uint32_t uid_base) {
  if (h->sb.n == NSEND) {
    int rcf = wl_flush_sends(h);
    if (rcf) return rcf;
  }
  if (h->n_mov) {
    // Mobility and the batch: a flushed send's receptions are re-derived by k_wl_send from the positions held at
    // the flush, so the batch is flushed before anything that can change a position — this send's updates here,
    // and every host call on a phy's model (wl_move_op; as nsgpu_wifil_set_position always did).  Each send is then
    // applied from the positions of its own send.
    if (int rcf = wl_flush_sends(h)) return rcf;
    hipLaunchKernelGGL(k_wl_move, dim3(wl_grid(h->D.nphy, 256)), dim3(256), 0, h->s, h->D, t.phy, (int64_t)t.ts,
                       h->recv[t.phy] ? 1u : 0u);
  }
  const uint32_t k = (uint32_t)h->n_tx++;
  if (h->sb.n == 0) h->sb.k0 = k;
  hipLaunchKernelGGL(h->D.lx ? k_wl_rx<true> : k_wl_rx<false>, dim3(wl_grid(h->D.nown, 256)), dim3(256), 0, h->s, h->D,
                     h->D.rxb + (uint64_t)h->sb.n * h->D.nphy, t, k, dbm, uid_base);
  NSGPU_HIP(hipGetLastError());
  h->sb.t[h->sb.n] = t;
  h->sb.dbm[h->sb.n] = dbm;
  h->sb.base[h->sb.n] = uid_base;
  h->sb.n++;
  return NSGPU_OK;  // (applied by the next epoch launch: its error bits, if any, fail that nsgpu_wifil_advance)
}

// ---- the epoch's host steps, shared by the single engine's driver (nsgpu_wifil_advance) and the partitioned
// handle's (wlg_advance); each driver does its own launches, copies and waits ----
// The (ts, uid) dispatch order, over events, end records and notes.
template <class T>
struct KeyLess {
  bool operator()(const T &a, const T &b) const { return a.ts != b.ts ? a.ts < b.ts : a.uid < b.uid; }
};
// The epoch's records (ends, notes) in (ts, uid) order, onto the list the host reads them back from.
template <class T>
static void wl_sort_append(std::vector<T> &epoch, std::vector<T> &all) {
  std::sort(epoch.begin(), epoch.end(), KeyLess<T>());
  all.insert(all.end(), epoch.begin(), epoch.end());
}

// The caller's log (null pointers: none): a dispatch's (ts, uid, context) at its rank, below cap.
struct WlLog {
  uint64_t *ts;
  uint32_t *uid, *ctx;
  uint64_t cap;
  bool on() const { return ts && uid && ctx; }
  void put(uint64_t rank, const LEv &e) const {
    if (rank < cap) ts[rank] = e.ts, uid[rank] = e.uid, ctx[rank] = e.ctx;
  }
};

// k_wl_stepw's instantiation: the notifying one only while some phy notifies, the switching one only once some phy
// has switched channels (the default path's kernel holds neither).
using WlStep = void (*)(const WDev, uint64_t, uint32_t, const SendBatch);
static WlStep wl_step_kernel(bool noting, bool switching) {
  if (noting) return switching ? k_wl_stepw<true, true> : k_wl_stepw<true, false>;
  return switching ? k_wl_stepw<false, true> : k_wl_stepw<false, false>;
}

// An engine's epoch counts against its arrays (part >= 0: partition `part` of a handle, whose syncs and notes are
// checked elsewhere / do not exist).  The order zeroes the epoch counters for the epoch two on; were that zeroing
// ever missed, nev would grow epoch by epoch past the dense array, as in fault r05z4n — a count beyond it is an
// engine fault, reported as one.
static int wl_check_counts(const WDev &D, int part, uint64_t nev, uint64_t nsync, uint64_t nend, uint64_t nnote) {
  if (nev <= (uint64_t)D.nphy * EVB + D.ev_cap && nend <= D.end_cap && nsync <= D.sync_cap && nnote <= D.note_cap)
    return NSGPU_OK;
  if (part < 0)
    return set_error(NSGPU_ESTATE, "nsgpu_wifil_advance: epoch counts beyond the engine's arrays (events %u, syncs "
                                   "%u, ends %u, notes %u): the epoch counters were not reset", (uint32_t)nev,
                     (uint32_t)nsync, (uint32_t)nend, (uint32_t)nnote);
  return set_error(NSGPU_ESTATE, "nsgpu_wifil_advance: partition %d's epoch counts beyond its arrays (events %llu, "
                                 "ends %llu)", part, (unsigned long long)nev, (unsigned long long)nend);
}
//  the uid range before anything of the epoch is published (ends, dispatch count, digest): the
// epoch's EndReceives are queued, none dispatched; the caller makes the error sticky (nsgpu_sim: uid_spent)
static int wl_check_uids(uint32_t uid, uint64_t nsync) {
  return (uint64_t)uid + nsync > nsgpu::UID_NEXT_MAX ? nsgpu::uid_range_error("nsgpu_wifil_advance") : NSGPU_OK;
}

// The dense events of an epoch the host orders (nev > ERANK_MAX) or logs, with their ranks in the latter case, from
// the arrays of D (the engine's own, or the union of a handle's partitions) into h->ev / h->erank; waited for.
static int wl_fetch_events(nsgpu_wifil *h, const WDev &D, uint64_t nev) {
  h->ev.resize(nev);
  NSGPU_HIP(hipMemcpyAsync(h->ev.data(), D.evd, nev * sizeof(LEv), hipMemcpyDeviceToHost, h->s));
  if (nev <= ERANK_MAX) {
    h->erank.resize(nev);
    NSGPU_HIP(hipMemcpyAsync(h->erank.data(), D.erank, nev * sizeof(uint32_t), hipMemcpyDeviceToHost, h->s));
  }
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

// The epoch's nev dispatches into the caller's count, digest and log.  A large epoch (nev > ERANK_MAX) is ordered
// here, from its fetched events, and its digest terms added; otherwise the device ranked it (its digest terms come
// through wl_digest_catchup) and, when logging, the fetched events go to the log at their ranks.
static void wl_publish(std::vector<LEv> &ev, const std::vector<uint32_t> &erank, uint64_t nev, bool logging,
                       const WlLog &log, uint64_t *dispatched, uint64_t *digest) {
  if (nev > ERANK_MAX) {
    std::sort(ev.begin(), ev.end(), KeyLess<LEv>());
    for (const LEv &e : ev) {
      const uint64_t rank = (*dispatched)++;
      *digest += nsgpu_dispatch_digest_term(rank, e.ts, e.uid);
      if (log.on()) log.put(rank, e);
    }
    return;
  }
  if (logging)
    for (uint64_t i = 0; i < nev; i++) log.put(*dispatched + erank[i], ev[i]);
  *dispatched += nev;
}

// The digest terms the device's order has summed since the last call (one aligned 8-byte store's value).
static void wl_digest_catchup(nsgpu_wifil *h, uint64_t *digest) {
  const uint64_t tot = *h->h_digtot;
  *digest += tot - h->dig_added;
  h->dig_added = tot;
}

// The dispatch order of an epoch (gather, tile sort, rank) on the second stream behind the epoch's close; the
// event lets the epoch two on (same parity) wait for it.  Launched before the host waits for the close: the
// launches' API time overlaps the epoch's kernels.
static int wl_launch_order(nsgpu_wifil *h, const WDev &D, uint32_t b, uint64_t K0, int keep) {
  NSGPU_HIP(hipEventRecord(h->ev_fin[b], h->s));
  NSGPU_HIP(hipStreamWaitEvent(h->s2, h->ev_fin[b], 0));
  hipLaunchKernelGGL(k_wl_gather, dim3(wl_grid(D.nown, 256)), dim3(256), 0, h->s2, D);
  hipLaunchKernelGGL(k_wl_tsort, dim3(NTILE), dim3(TS_T), 0, h->s2, D);
  hipLaunchKernelGGL(k_wl_rank, dim3(NTILE), dim3(TS_T), 0, h->s2, D, K0, keep, h->d_digtot);
  NSGPU_HIP(hipGetLastError());
  NSGPU_HIP(hipEventRecord(h->ev_ord[b], h->s2));
  h->ord_pending[b] = true;
  return NSGPU_OK;
}

static int wlg_advance(nsgpu_wifil *G, uint64_t bts, uint32_t buid, uint32_t *uid, uint64_t *dispatched, uint64_t *digest,
                       const WlLog &log);

// Every device event with a key below (bound_ts, bound_uid) (~0: all of them): dispatched in (ts, uid) order
// from rank *dispatched on; the syncs' EndReceives take the uids from *uid on.  The dispatches are added to
// the caller's digest (nsgpu_dispatch_digest_term) and log (at their ranks, below log_cap).
extern "C" int nsgpu_wifil_advance(nsgpu_wifil *h, uint64_t bound_ts, uint32_t bound_uid, uint32_t *uid,
                                   uint64_t *dispatched, uint64_t *digest, uint64_t *log_ts, uint32_t *log_uid,
                                   uint32_t *log_ctx, uint64_t log_cap) {
  if (!h || !uid || !dispatched || !digest) return set_error(NSGPU_EINVAL, "nsgpu_wifil_advance: null");
  const WlLog log{log_ts, log_uid, log_ctx, log_cap};
  if (h->grp) return wlg_advance(h, bound_ts, bound_uid, uid, dispatched, digest, log);
  const WDev D = h->D;  // (this epoch's parity: its status block, lists, syncs; zeroed by the order two epochs back)
  const uint32_t b = h->par;
  if (h->ord_pending[b]) {  // (that order is their last reader; it has had a whole epoch: usually done, then the
    const hipError_t q = hipEventQuery(h->ev_ord[b]);  //  stream needs no wait packet before this epoch's kernels)
    if (q == hipErrorNotReady) NSGPU_HIP(hipStreamWaitEvent(h->s, h->ev_ord[b], 0));
    else NSGPU_HIP(q);
    h->ord_pending[b] = false;
  }
  // epoch: the phys' waves, then the tail (PER products + sync ranks + the close), then the order behind it
  hipLaunchKernelGGL(wl_step_kernel(h->n_note_on != 0, h->n_switches != 0), dim3(wl_grid(D.nown, 1)), dim3(64), 0, h->s,
                     D, bound_ts, bound_uid, h->sb);
  h->sb.n = 0;
#ifdef NSGPU_PHASE_PROF
  hipLaunchKernelGGL(k_wl_prof_epoch, dim3(1), dim3(1), 0, h->s);
#endif
  const uint32_t seq = ++h->seq;  // (the close writes it into the host's status block last: the epoch's flag)
  hipLaunchKernelGGL(k_wl_mid, dim3(MID_PER + MID_RANK), dim3(256), 0, h->s, D, *uid, h->d_stat, seq);
  NSGPU_HIP(hipGetLastError());
  const bool logging = log.on() && *dispatched < log_cap;
  if (int rco = wl_launch_order(h, D, b, *dispatched, logging ? 1 : 0)) return rco;
  {  // the epoch's flag in the mapped status block (a spin: a stream synchronize's wake-up took microseconds);
     // the stream is queried now and then, so a failed kernel (no flag) ends the wait with its error
    volatile uint32_t *flag = reinterpret_cast<volatile uint32_t *>(h->h_stat) + 6;
    for (uint64_t n = 1; *flag != seq; n++) {
      if ((n & 1023) == 0) {
        const hipError_t q = hipStreamQuery(h->s);
        if (q == hipErrorNotReady) continue;
        NSGPU_HIP(q);
        if (*flag != seq) return set_error(NSGPU_EHIP, "nsgpu_wifil_advance: the epoch's kernels ended without its flag");
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  wl_use_stat(h, b ^ 1);  // (the next epoch's block; SendPackets until then report their errors there)
  int rc = wl_check(h, "nsgpu_wifil_advance");
  if (rc) return rc;
  const uint32_t nev = h->h_cnt[0], nsync = h->h_cnt[1], nend = h->h_cnt[2], nnote = h->h_cnt[5];
  if ((rc = wl_check_counts(D, -1, nev, nsync, nend, nnote))) return rc;
  if ((rc = wl_check_uids(*uid, nsync))) return rc;
  h->notes_epoch.resize(nnote);  // (before the next epoch's kernel reuses the array; waited for below)
  if (nnote) NSGPU_HIP(hipMemcpyAsync(h->notes_epoch.data(), D.notes, nnote * sizeof(nsgpu_wifil_note), hipMemcpyDeviceToHost, h->s));
  h->ends_epoch.resize(nend);
  if (nend > END_STAGE) {
    NSGPU_HIP(hipMemcpyAsync(h->ends_epoch.data(), D.ends, nend * sizeof(nsgpu_wifil_end), hipMemcpyDeviceToHost, h->s));
  } else if (nend) {
    std::copy(h->h_ends, h->h_ends + nend, h->ends_epoch.begin());
  }
  if (nev > ERANK_MAX || (logging && nev)) {  // (the dense events / ranks: behind the order)
    NSGPU_HIP(hipStreamSynchronize(h->s2));
    if ((rc = wl_fetch_events(h, D, nev))) return rc;
  }
  wl_publish(h->ev, h->erank, nev, logging, log, dispatched, digest);
  wl_digest_catchup(h, digest);  // (the ordered epochs' terms so far)
  if (nend > END_STAGE || nnote) NSGPU_HIP(hipStreamSynchronize(h->s));
  if (nnote) wl_sort_append(h->notes_epoch, h->notes);  // (the notifying phys' only: a small set)
  wl_sort_append(h->ends_epoch, h->ends);
  *uid += nsync;
  return NSGPU_OK;
}

// Waits for the epochs' order behind the PHY (k_wl_tsort / k_wl_rank on the second stream) and adds the
// digest terms it summed since the last advance / flush.
extern "C" int nsgpu_wifil_flush(nsgpu_wifil *h, uint64_t *digest) {
  if (!h || !digest) return set_error(NSGPU_EINVAL, "nsgpu_wifil_flush: null");
  NSGPU_HIP(hipStreamSynchronize(h->grp ? h->s : h->s2));  // (a partitioned PHY orders every epoch at once)
  wl_digest_catchup(h, digest);
  return NSGPU_OK;
}

// (the phy's mobility model: MOVE_NONE, MOVE_VEL, MOVE_WAY or MOVE_ACC)
static uint32_t wl_kind(const nsgpu_wifil *h, uint32_t phy) { return phy < h->mov_kind.size() ? h->mov_kind[phy] : MOVE_NONE; }

// MobilityModel::SetPosition of `phy`'s node (mobility-model.cc SetPosition -> DoSetPosition; e.g. a host closure
// at run time): YansWifiChannel::Send reads the positions at each send (yans-wifi-channel.cc:92-96), so the
// later sends' fan-outs see it; receptions already scheduled keep their delay and power.  In stream order with
// the sends.
extern "C" int nsgpu_wifil_set_position(nsgpu_wifil *h, uint32_t phy, double x, double y, double z) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_position: bad phy");
  if (wl_kind(h, phy))
    return set_error(NSGPU_ESTATE, "nsgpu_wifil_set_position: phy %u has a mobility model, whose SetPosition reads Now: "
                                   "use nsgpu_wifil_set_position_at", phy);
  if (h->grp) {  // (every partition holds every position)
    for (nsgpu_wifil *m : h->grp->mem)
      if (int rcm = nsgpu_wifil_set_position(m, phy, x, y, z)) return rcm;
    return NSGPU_OK;
  }
  if (int rcf = wl_flush_sends(h)) return rcf;  // (the sends so far see the positions they were made with)
  const double v[3] = {x, y, z};
  double *dst[3] = {const_cast<double *>(h->D.x), const_cast<double *>(h->D.y), const_cast<double *>(h->D.z)};
  for (int c = 0; c < 3; c++)
    NSGPU_HIP(hipMemcpyAsync(dst[c] + phy, &v[c], sizeof(double), hipMemcpyHostToDevice, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));  // (v is on this stack)
  return NSGPU_OK;
}

// ---- mobility: constant velocity, waypoints, constant acceleration ----
// One k_wl_mop call on phy's model (the batch first: see wl_queue_send).  The host's copy of the record's kind, and
// the count of phys with a model, follow the op: an install sets the kind, the remove clears it.
static int wl_move_op(nsgpu_wifil *h, uint32_t op, uint32_t phy, uint64_t now, const MoveArg &a) {
  if (int rcf = wl_flush_sends(h)) return rcf;
  hipLaunchKernelGGL(k_wl_mop, dim3(1), dim3(1), 0, h->s, h->D, op, phy, (int64_t)now, a, h->d_movout);
  NSGPU_HIP(hipGetLastError());
  uint8_t &kind = h->mov_kind[phy];
  const uint8_t is = op == MOP_REMOVE ? MOVE_NONE : op == MOP_VEL_INSTALL ? MOVE_VEL : op == MOP_WAY_INSTALL ? MOVE_WAY
                     : op == MOP_ACC_INSTALL ? MOVE_ACC : kind;
  h->n_mov += (is != MOVE_NONE) - (kind != MOVE_NONE);
  kind = is;
  return NSGPU_OK;
}
// The argument checks every install / remove call makes first and, ahead of an install, the records: sized at the
// first install of any model, as nsgpu_wifil_notify sizes its flags.
static int wl_move_begin(nsgpu_wifil *h, uint32_t phy, const char *what, bool install) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "%s: bad phy", what);  // (before anything is sized)
  if (int rc = wl_single_only(h, NSGPU_EINVAL, what, "mobility is")) return rc;
  if (!install || !h->mov_kind.empty()) return NSGPU_OK;
  int rc = wl_alloc(h, &h->D.mov, (size_t)h->D.nphy);
  if (!rc) rc = wl_alloc(h, &h->d_movout, 1);
  if (rc) return rc;
  h->mov_kind.assign((size_t)h->D.nphy, MOVE_NONE);
  h->seg.resize((size_t)h->D.nphy);
  return NSGPU_OK;
}

// Installs ConstantVelocityHelper state on `phy`, in place of whatever model it had (m == NULL: removes a
// constant-velocity model; the phy stays where it is, a constant position again).
extern "C" int nsgpu_wifil_set_mobility(nsgpu_wifil *h, uint32_t phy, const nsgpu_mobility *m) {
  if (int rc = wl_move_begin(h, phy, "nsgpu_wifil_set_mobility", m != nullptr)) return rc;
  if (!m) return wl_kind(h, phy) == MOVE_VEL ? wl_move_op(h, MOP_REMOVE, phy, 0, MoveArg{}) : NSGPU_OK;
  MoveArg a{};
  for (int c = 0; c < 3; c++) a.w.pos[c] = m->pos[c], a.v[c] = m->vel[c];
  a.time = m->last_update, a.paused = m->paused;
  return wl_move_op(h, MOP_VEL_INSTALL, phy, 0, a);
}

extern "C" int nsgpu_wifil_set_velocity(nsgpu_wifil *h, uint64_t now, uint32_t phy, const double v[3]) {
  if (!h || !v || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_velocity: bad phy");
  if (wl_kind(h, phy) != MOVE_VEL) return set_error(NSGPU_ESTATE, "nsgpu_wifil_set_velocity: phy %u has no mobility model", phy);
  MoveArg a{};
  a.v[0] = v[0], a.v[1] = v[1], a.v[2] = v[2];
  return wl_move_op(h, MOP_VEL_SET, phy, now, a);
}

extern "C" int nsgpu_wifil_pause(nsgpu_wifil *h, uint64_t now, uint32_t phy, uint32_t paused) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_pause: bad phy");
  if (wl_kind(h, phy) != MOVE_VEL) return set_error(NSGPU_ESTATE, "nsgpu_wifil_pause: phy %u has no mobility model", phy);
  MoveArg a{};
  a.paused = paused;
  return wl_move_op(h, MOP_VEL_PAUSE, phy, now, a);
}

// The phy's model's SetPosition at `now` (ConstantVelocityHelper::SetPosition, constant-velocity-helper.cc:43-49;
// WaypointMobilityModel / ConstantAccelerationMobilityModel::DoSetPosition).
extern "C" int nsgpu_wifil_set_position_at(nsgpu_wifil *h, uint64_t now, uint32_t phy, double x, double y, double z) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_position_at: bad phy");
  if (!wl_kind(h, phy)) return nsgpu_wifil_set_position(h, phy, x, y, z);  // (ConstantPositionMobilityModel: no time)
  MoveArg a{};
  a.w.pos[0] = x, a.w.pos[1] = y, a.w.pos[2] = z;
  return wl_move_op(h, MOP_SET_POSITION, phy, now, a);
}

extern "C" int nsgpu_wifil_get_mobility(nsgpu_wifil *h, uint64_t now, uint32_t phy, nsgpu_mobility *out) {
  if (!h || !out || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_get_mobility: bad phy");
  if (wl_kind(h, phy) != MOVE_VEL) return set_error(NSGPU_ESTATE, "nsgpu_wifil_get_mobility: phy %u has no mobility model", phy);
  if (int rc = wl_move_op(h, MOP_VEL_GET, phy, now, MoveArg{})) return rc;
  NSGPU_HIP(hipMemcpyAsync(out, &h->d_movout->vel, sizeof(nsgpu_mobility), hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

// Room for `need` slots in phy's segment of the pool (nsgpu_waypool.h), in stream order: a full pool is replaced once
// the stream has drained (as the Matrix table grows: rare, and not on the send path), a full segment is copied to
// the pool's end behind every kernel that reads the old one.
static int wl_way_reserve(nsgpu_wifil *h, WaySeg &s, uint64_t need) {
  const uint64_t old_end = h->wpool.end;
  const WayPlan p = h->wpool.reserve(s, need);
  if (p.grow) {
    nsgpu_waypoint *np = nullptr;
    NSGPU_HIP(hipStreamSynchronize(h->s));
    NSGPU_HIP(hipMalloc((void **)&np, p.pool_cap * sizeof(nsgpu_waypoint)));
    if (h->D.wpool) {
      NSGPU_HIP(hipMemcpy(np, h->D.wpool, old_end * sizeof(nsgpu_waypoint), hipMemcpyDeviceToDevice));
      NSGPU_HIP(hipFree(h->D.wpool));
    }
    h->D.wpool = np;
  }
  if (p.move)
    NSGPU_HIP(hipMemcpyAsync(h->D.wpool + p.off, h->D.wpool + p.old_off, (size_t)s.cnt * sizeof(nsgpu_waypoint),
                             hipMemcpyDeviceToDevice, h->s));
  return NSGPU_OK;
}
// Waypoints into the slots [at, at + n) of the pool, WP_CHUNK a launch, carried as kernel arguments.
static int wl_way_put(nsgpu_wifil *h, uint64_t at, const nsgpu_waypoint *wp, uint64_t n) {
  for (uint64_t i = 0; i < n; i += WP_CHUNK) {
    WpChunk c{};
    const uint32_t k = (uint32_t)std::min<uint64_t>(WP_CHUNK, n - i);
    std::copy(wp + i, wp + i + k, c.w);
    hipLaunchKernelGGL(k_wl_wput, dim3(1), dim3(WP_CHUNK), 0, h->s, h->D.wpool + at + i, c, k);
  }
  NSGPU_HIP(hipGetLastError());
  return NSGPU_OK;
}

extern "C" int nsgpu_wifil_set_waypoints(nsgpu_wifil *h, uint32_t phy, const nsgpu_waypoint *wp, uint64_t n) {
  if (int rc = wl_move_begin(h, phy, "nsgpu_wifil_set_waypoints", n != 0)) return rc;
  if (n && !wp) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_waypoints: null");
  if (n > 0xffffffffull || !ascending(wp, n))
    return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_waypoints: waypoints must be given in ascending time order "
                                   "(waypoint-mobility-model.cc:91 NS_ABORT_MSG_IF)");
  if (n == 0)  // (a waypoint or an acceleration model: either goes)
    return wl_kind(h, phy) >= MOVE_WAY ? wl_move_op(h, MOP_REMOVE, phy, 0, MoveArg{}) : NSGPU_OK;
  if (int rcf = wl_flush_sends(h)) return rcf;
  WaySeg &s = h->seg[phy];
  s.cnt = 0;  // (a fresh model: nothing of the old list moves with the segment)
  if (int rc = wl_way_reserve(h, s, n - 1)) return rc;
  if (int rc = wl_way_put(h, s.off, wp + 1, n - 1)) return rc;
  s.cnt = (uint32_t)(n - 1);
  s.first = false, s.any = true, s.last = wp[n - 1].time;
  s.list.assign(wp, wp + n);
  MoveArg a{};
  a.w = wp[0], a.off = (uint32_t)s.off, a.cnt = s.cnt;
  return wl_move_op(h, MOP_WAY_INSTALL, phy, 0, a);
}

extern "C" int nsgpu_wifil_add_waypoint(nsgpu_wifil *h, uint32_t phy, const nsgpu_waypoint *wp) {
  if (!h || !wp || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_add_waypoint: bad phy");
  if (wl_kind(h, phy) != MOVE_WAY) return set_error(NSGPU_ESTATE, "nsgpu_wifil_add_waypoint: phy %u has no waypoint model", phy);
  WaySeg &s = h->seg[phy];
  if (!s.first && s.any && wp->time <= s.last)
    return set_error(NSGPU_EINVAL, "nsgpu_wifil_add_waypoint: waypoints must be added in ascending time order "
                                   "(waypoint-mobility-model.cc:91 NS_ABORT_MSG_IF)");
  if (int rcf = wl_flush_sends(h)) return rcf;
  if (!s.first) {  // (queued: one slot, behind every kernel that may read the old count)
    if (s.cnt == 0xffffffffu) return set_error(NSGPU_ENOMEM, "nsgpu_wifil_add_waypoint: 2^32 waypoints");
    if (int rc = wl_way_reserve(h, s, (uint64_t)s.cnt + 1)) return rc;
    if (int rc = wl_way_put(h, s.off + s.cnt, wp, 1)) return rc;
    s.cnt++;
  }
  s.first = false, s.any = true, s.last = wp->time;
  s.list.push_back(*wp);
  MoveArg a{};
  a.w = *wp, a.off = (uint32_t)s.off, a.cnt = s.cnt;
  return wl_move_op(h, MOP_WAY_ADD, phy, 0, a);
}

extern "C" int nsgpu_wifil_end_waypoints(nsgpu_wifil *h, uint32_t phy) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_end_waypoints: bad phy");
  if (wl_kind(h, phy) != MOVE_WAY) return set_error(NSGPU_ESTATE, "nsgpu_wifil_end_waypoints: phy %u has no waypoint model", phy);
  WaySeg &s = h->seg[phy];
  s.first = true, s.any = false;
  return wl_move_op(h, MOP_WAY_END, phy, 0, MoveArg{});
}

extern "C" int nsgpu_wifil_get_waypoints(nsgpu_wifil *h, uint64_t now, uint32_t phy, nsgpu_waypoint_state *out) {
  if (!h || !out || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_get_waypoints: bad phy");
  if (wl_kind(h, phy) != MOVE_WAY) return set_error(NSGPU_ESTATE, "nsgpu_wifil_get_waypoints: phy %u has no waypoint model", phy);
  if (int rc = wl_move_op(h, MOP_WAY_GET, phy, now, MoveArg{})) return rc;
  NSGPU_HIP(hipMemcpyAsync(out, &h->d_movout->way, sizeof(nsgpu_waypoint_state), hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

extern "C" int nsgpu_wifil_set_acceleration(nsgpu_wifil *h, uint32_t phy, const nsgpu_accel *acc) {
  if (int rc = wl_move_begin(h, phy, "nsgpu_wifil_set_acceleration", acc != nullptr)) return rc;
  if (!acc)  // (a waypoint or an acceleration model: either goes)
    return wl_kind(h, phy) >= MOVE_WAY ? wl_move_op(h, MOP_REMOVE, phy, 0, MoveArg{}) : NSGPU_OK;
  MoveArg a{};
  for (int c = 0; c < 3; c++) a.w.pos[c] = acc->pos[c], a.v[c] = acc->vel[c], a.a[c] = acc->acc[c];
  a.time = acc->base_time;
  return wl_move_op(h, MOP_ACC_INSTALL, phy, 0, a);
}

extern "C" int nsgpu_wifil_set_velocity_and_acceleration(nsgpu_wifil *h, uint64_t now, uint32_t phy, const double v[3],
                                                         const double acc[3]) {
  if (!h || !v || !acc || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_velocity_and_acceleration: bad phy");
  if (wl_kind(h, phy) != MOVE_ACC)
    return set_error(NSGPU_ESTATE, "nsgpu_wifil_set_velocity_and_acceleration: phy %u has no acceleration model", phy);
  MoveArg a{};
  for (int c = 0; c < 3; c++) a.v[c] = v[c], a.a[c] = acc[c];
  return wl_move_op(h, MOP_ACC_SET, phy, now, a);
}

extern "C" int nsgpu_wifil_get_acceleration(nsgpu_wifil *h, uint64_t now, uint32_t phy, nsgpu_accel *out) {
  if (!h || !out || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_get_acceleration: bad phy");
  if (wl_kind(h, phy) != MOVE_ACC) return set_error(NSGPU_ESTATE, "nsgpu_wifil_get_acceleration: phy %u has no acceleration model", phy);
  if (int rc = wl_move_op(h, MOP_ACC_GET, phy, now, MoveArg{})) return rc;
  NSGPU_HIP(hipMemcpyAsync(out, &h->d_movout->acc, sizeof(nsgpu_accel), hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

// WifiPhyStateHelper::GetState (wifi-phy-state-helper.cc:159-183) from a phy's mirrored fields.
static uint32_t wl_state(const WMir &P, int64_t nw) {
  return P.endTx > nw ? NSGPU_WIFIL_TX : P.rxing ? NSGPU_WIFIL_RX : P.endSw > nw ? NSGPU_WIFIL_SWITCHING
         : P.endCca > nw ? NSGPU_WIFIL_CCA_BUSY : NSGPU_WIFIL_IDLE;
}

// YansWifiPhy::SetChannelNumber (nch) of `phy` from the host closure running at `now` (yans-wifi-phy.cc:327-374),
// after every earlier send of that closure.  The outcome follows from the phy's state at `now`, which the mirror
// holds (the runtime advanced the device to the closure; the closure's own sends are applied to it).  TX: nothing
// is touched — ns-3 schedules the retry (:349-352), an event with a uid, so the caller does.  Otherwise: the batch is
// flushed (its sends keep the receivers their channels had), then k_wl_rechan (when the number changes) and
// k_wl_switch; the host's channel numbers, receiver counts and mirror follow.
extern "C" int nsgpu_wifil_set_channel(nsgpu_wifil *h, uint64_t now, uint32_t phy, uint32_t nch, int64_t switch_delay_ns,
                                       nsgpu_wifil_switch *out) {
  if (!h || !out || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_channel: bad phy");
  if (switch_delay_ns < 0) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_channel: negative ChannelSwitchDelay");
  if (int rc = wl_single_only(h, NSGPU_ESTATE, "nsgpu_wifil_set_channel", "channel switching is")) return rc;
  WMir &mr = h->h_mir[phy];
  const int64_t nw = (int64_t)now;
  const uint32_t st = wl_state(mr, nw);
  const bool init = now == 0;  // "this is not channel switch, this is initialization" (:330-336)
  if (!init && st == NSGPU_WIFIL_SWITCHING)  // NS_ASSERT (!IsStateSwitching ()) (:338)
    return set_error(NSGPU_ESTATE, "nsgpu_wifil_set_channel: phy %u is switching channels (yans-wifi-phy.cc:338 NS_ASSERT)", phy);
  *out = nsgpu_wifil_switch{NSGPU_WIFIL_SWITCH_DONE, st, 0};
  if (!init && st == NSGPU_WIFIL_TX) {
    out->outcome = NSGPU_WIFIL_SWITCH_POSTPONED;
    out->retry_delay = mr.endTx - nw;  // GetDelayUntilIdle ()
    return NSGPU_OK;
  }
  if (init) out->outcome = NSGPU_WIFIL_SWITCH_INIT;
  if (!h->d_nbefore) {
    if (int rc = wl_alloc(h, &h->d_nbefore, 1)) return rc;
    NSGPU_HIP(hipDeviceSynchronize());  // (once: the word's zeroing, on the null stream, before h->s reads it)
  }
  if (int rcf = wl_flush_sends(h)) return rcf;
  const uint32_t old = h->chan_h[phy];
  const bool moved = old != nch;
  if (moved) {
    hipLaunchKernelGGL(k_wl_rechan, dim3(wl_grid(h->D.nphy, 256)), dim3(256), 0, h->s, h->D, phy, old, nch, h->d_nbefore);
    uint32_t on_new = 0;  // the receiver counts behind nsgpu_wifil_receivers
    for (size_t i = 0; i < h->chan_h.size(); i++) {
      if (i == phy) continue;
      if (h->chan_h[i] == old) h->recv[i]--;
      else if (h->chan_h[i] == nch) h->recv[i]++, on_new++;
    }
    h->recv[phy] = on_new;
    h->chan_h[phy] = nch;
  }
  hipLaunchKernelGGL(k_wl_switch, dim3(1), dim3(1), 0, h->s, h->D, phy, nw, switch_delay_ns, nch, init ? 0u : 1u,
                     moved ? 1u : 0u, h->d_nbefore);
  NSGPU_HIP(hipGetLastError());
  if (!init) {  // k_wl_switch's state changes, in the host's copy
    if (mr.rxing) mr.rxing = 0, mr.endRx = nw;
    if (nw < mr.endCca) mr.endCca = nw;
    mr.endSw = nw + switch_delay_ns;
    h->n_switches++;
  }
  return NSGPU_OK;
}

// GetChannelNumber () of `phy`, its m_startSwitching / m_endSwitching and its switching counters (one device trip).
extern "C" int nsgpu_wifil_get_channel(nsgpu_wifil *h, uint32_t phy, nsgpu_wifil_channel *out) {
  if (!h || !out || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_get_channel: bad phy");
  if (int rc = wl_single_only(h, NSGPU_ESTATE, "nsgpu_wifil_get_channel", "channel switching is")) return rc;
  if (int rcf = wl_flush_sends(h)) return rcf;
  LPhy p;
  NSGPU_HIP(hipMemcpyAsync(&p, h->D.ps + phy, sizeof(LPhy), hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  *out = nsgpu_wifil_channel{h->chan_h[phy], 0, p.startSw, p.endSw, p.switches, p.drop_switching};
  return NSGPU_OK;
}

// ---- the extended loss chain (nsgpu_wifil_set_loss, nsgpu_lossx_calc) ----
// What makes a nsgpu_lossx unusable (n_phy < 0: no bound on the entries' phys); nothing is touched before it passes.
static int lossx_check(const nsgpu_lossx *lx, int64_t n_phy, const char *what) {
  if (lx->n < 0 || lx->n > NSGPU_MAX_LOSS_CHAIN) return set_error(NSGPU_EINVAL, "%s: %d links (0 .. %d)", what, lx->n, NSGPU_MAX_LOSS_CHAIN);
  int matrices = 0;
  for (int i = 0; i < lx->n; i++) {
    const nsgpu_lossx_model &m = lx->m[i];
    if (m.kind < 0 || m.kind > NSGPU_LOSSX_MATRIX) return set_error(NSGPU_EINVAL, "%s: link %d has unknown kind %d", what, i, m.kind);
    if (m.kind == NSGPU_LOSSX_MATRIX) {  // (its one parameter, DefaultLoss, may be anything: the reference's is DBL_MAX)
      if (++matrices > 1) return set_error(NSGPU_EINVAL, "%s: more than one MATRIX link", what);
      continue;
    }
    const int np = m.kind == NSGPU_LOSSX_THREE_LOG ? 7 : m.kind == NSGPU_LOSSX_TWO_RAY_GROUND ? 4 : 3;
    for (int q = 0; q < np; q++)
      if (!std::isfinite(m.p[q])) return set_error(NSGPU_EINVAL, "%s: link %d's p%d is not finite", what, i, q);
  }
  if (lx->n_entry > 0xffffffffull) return set_error(NSGPU_EINVAL, "%s: more than 2^32 - 1 entries (the table's offsets are 32-bit)", what);
  if (lx->n_entry && !lx->entry) return set_error(NSGPU_EINVAL, "%s: %llu entries and no entry array", what, (unsigned long long)lx->n_entry);
  if (n_phy >= 0)
    for (uint64_t e = 0; e < lx->n_entry; e++)
      if (lx->entry[e].a >= n_phy || lx->entry[e].b >= n_phy)
        return set_error(NSGPU_EINVAL, "%s: entry %llu names phy (%u, %u) of %lld", what, (unsigned long long)e, lx->entry[e].a,
                         lx->entry[e].b, (long long)n_phy);
  return NSGPU_OK;
}
static bool lossx_has_matrix(const nsgpu_lossx *lx) {
  for (int i = 0; i < lx->n; i++)
    if (lx->m[i].kind == NSGPU_LOSSX_MATRIX) return true;
  return false;
}
// MatrixPropagationLossModel's map as the per-sender table of LossTable: row[n_phy + 1], then each sender's receivers
// ascending with their losses; of several entries for one (a, b) the last one given stays (SetLoss overwrites, :762-765).
static void lossx_table(const nsgpu_lossx *lx, int64_t n_phy, std::vector<uint32_t> &row, std::vector<uint32_t> &col,
                        std::vector<double> &loss) {
  std::vector<uint64_t> ord((size_t)lx->n_entry);
  for (uint64_t e = 0; e < lx->n_entry; e++) ord[e] = e;
  const nsgpu_lossx_entry *en = lx->entry;
  std::stable_sort(ord.begin(), ord.end(), [en](uint64_t p, uint64_t q) {
    return en[p].a != en[q].a ? en[p].a < en[q].a : en[p].b < en[q].b;
  });
  row.assign((size_t)n_phy + 1, 0);
  col.clear();
  loss.clear();
  for (size_t i = 0; i < ord.size(); i++) {
    const nsgpu_lossx_entry &x = en[ord[i]];
    if (i + 1 < ord.size() && en[ord[i + 1]].a == x.a && en[ord[i + 1]].b == x.b) continue;  // (a later one follows)
    col.push_back(x.b);
    loss.push_back(x.loss_db);
    row[(size_t)x.a + 1]++;
  }
  for (int64_t s = 0; s < n_phy; s++) row[(size_t)s + 1] += row[(size_t)s];
}

// CalcRxPower (tx_dbm, a, b) over an extended chain on the host: the table nsgpu_wifil_set_loss builds, the function
// the kernels call.  pa / pb: the positions of phys a (the sender) and b.
extern "C" int nsgpu_lossx_calc(const nsgpu_lossx *lx, uint32_t a, uint32_t b, const double pa[3], const double pb[3],
                                double tx_dbm, double *rx_dbm) {
  if (!lx || !pa || !pb || !rx_dbm) return set_error(NSGPU_EINVAL, "nsgpu_lossx_calc: null argument");
  if (int rc = lossx_check(lx, -1, "nsgpu_lossx_calc")) return rc;
  std::vector<uint32_t> row, col;
  std::vector<double> loss;
  LossTable tb{nullptr, nullptr, nullptr};
  if (lossx_has_matrix(lx) && lx->n_entry) {
    int64_t n_phy = (int64_t)std::max(a, b) + 1;
    for (uint64_t e = 0; e < lx->n_entry; e++) n_phy = std::max<int64_t>(n_phy, (int64_t)std::max(lx->entry[e].a, lx->entry[e].b) + 1);
    lossx_table(lx, n_phy, row, col, loss);
    tb = LossTable{row.data(), col.data(), loss.data()};
  }
  const double dist = distance3(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2]);  // a->GetDistanceFrom (b)
  *rx_dbm = calc_rx_power_x(lx->m, lx->n, tb, tx_dbm, a, b, pa[2], pb[2], dist);
  return NSGPU_OK;
}

// The handle's loss chain from now on (null: the config's again).  The batch is flushed first — k_wl_send launches,
// which take the chain in force by value — so every send so far keeps the powers of its own Now.  The device block is
// rewritten in stream order on h->s, the stream of every kernel that reads it: the copy runs after the last of them.
// A larger block replaces it once the stream has drained.
extern "C" int nsgpu_wifil_set_loss(nsgpu_wifil *h, const nsgpu_lossx *lx) {
  if (!h) return set_error(NSGPU_EINVAL, "nsgpu_wifil_set_loss: null handle");
  if (int rc = wl_single_only(h, NSGPU_ESTATE, "nsgpu_wifil_set_loss", "the extended loss chain is")) return rc;
  if (lx)
    if (int rc = lossx_check(lx, h->D.nphy, "nsgpu_wifil_set_loss")) return rc;
  if (int rcf = wl_flush_sends(h)) return rcf;
  if (!lx) {
    h->D.lx = nullptr;
    return NSGPU_OK;
  }
  std::vector<uint32_t> row, col;
  std::vector<double> loss;
  const bool table = lossx_has_matrix(lx) && lx->n_entry;
  if (table) lossx_table(lx, h->D.nphy, row, col, loss);
  const size_t o_loss = sizeof(LossX), o_row = o_loss + loss.size() * sizeof(double),
               o_col = o_row + row.size() * sizeof(uint32_t), size = o_col + col.size() * sizeof(uint32_t);
  static_assert(sizeof(LossX) % 8 == 0, "the losses follow the links, 8-aligned");
  if (size > h->lx_cap) {
    NSGPU_HIP(hipStreamSynchronize(h->s));  // (no queued kernel reads the old block, no copy reads the old pinned one)
    if (h->lx_dev) (void)hipFree(h->lx_dev);
    if (h->lx_pin) (void)hipHostFree(h->lx_pin);
    h->lx_dev = h->lx_pin = nullptr;
    h->lx_cap = 0;
    h->D.lx = nullptr;
    const size_t cap = size + size / 2;  // (a table that grows entry by entry: not a new block each call)
    NSGPU_HIP(hipMalloc((void **)&h->lx_dev, cap));
    NSGPU_HIP(hipHostMalloc((void **)&h->lx_pin, cap, hipHostMallocDefault));
    h->lx_cap = cap;
    if (!h->lx_up) NSGPU_HIP(hipEventCreateWithFlags(&h->lx_up, hipEventDisableTiming));
  } else {
    NSGPU_HIP(hipEventSynchronize(h->lx_up));  // (the last upload has left the pinned block)
  }
  LossX X{};
  X.n = lx->n;
  for (int i = 0; i < lx->n; i++) X.m[i] = lx->m[i];
  if (table)
    X.tb = LossTable{reinterpret_cast<const uint32_t *>(h->lx_dev + o_row), reinterpret_cast<const uint32_t *>(h->lx_dev + o_col),
                     reinterpret_cast<const double *>(h->lx_dev + o_loss)};
  std::memcpy(h->lx_pin, &X, sizeof(LossX));
  if (table) {
    std::memcpy(h->lx_pin + o_loss, loss.data(), loss.size() * sizeof(double));
    std::memcpy(h->lx_pin + o_row, row.data(), row.size() * sizeof(uint32_t));
    std::memcpy(h->lx_pin + o_col, col.data(), col.size() * sizeof(uint32_t));
  }
  NSGPU_HIP(hipMemcpyAsync(h->lx_dev, h->lx_pin, size, hipMemcpyHostToDevice, h->s));
  NSGPU_HIP(hipEventRecord(h->lx_up, h->s));
  h->D.lx = reinterpret_cast<const LossX *>(h->lx_dev);
  return NSGPU_OK;
}

// WifiPhyStateHelper::GetState / GetDelayUntilIdle of `phy` at `now` (wifi-phy-state-helper.cc:122-183).
extern "C" int nsgpu_wifil_get_state(nsgpu_wifil *h, uint32_t phy, uint64_t now, nsgpu_wifil_phy_state *out) {
  if (!h || !out || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_get_state: bad phy");
  // the state fields as the last epoch's kernels (their lanes write a changed phy's) and the host's SendPackets
  // left them: every event before `now` has run (the runtime advanced the device to the running closure)
  const WMir P = h->h_mir[phy];
  const int64_t nw = (int64_t)now;
  out->state = wl_state(P, nw);
  out->rxing = P.rxing;
  out->end_tx = P.endTx;
  out->end_rx = P.endRx;
  out->end_cca_busy = P.endCca;
  int64_t r = 0;
  if (out->state == NSGPU_WIFIL_RX) r = P.endRx - nw;
  else if (out->state == NSGPU_WIFIL_TX) r = P.endTx - nw;
  else if (out->state == NSGPU_WIFIL_SWITCHING) r = P.endSw - nw;
  else if (out->state == NSGPU_WIFIL_CCA_BUSY) r = P.endCca - nw;
  out->delay_until_idle = r > 0 ? r : 0;
  return NSGPU_OK;
}

// The first min(cap, size) records of a hand-back list, taken off it (cap 0 or no `out`: the count only, kept).
template <class T>
static int wl_drain(std::vector<T> &v, T *out, uint64_t cap, uint64_t *n) {
  *n = v.size();
  if (!out || cap == 0) return NSGPU_OK;
  const uint64_t k = std::min<uint64_t>(cap, v.size());
  std::copy(v.begin(), v.begin() + (ptrdiff_t)k, out);
  v.erase(v.begin(), v.begin() + (ptrdiff_t)k);
  *n = k;
  return NSGPU_OK;
}

// The EndReceive records dispatched since the last call, in dispatch order.
extern "C" int nsgpu_wifil_read_ends(nsgpu_wifil *h, nsgpu_wifil_end *out, uint64_t cap, uint64_t *n) {
  if (!h || !n) return set_error(NSGPU_EINVAL, "nsgpu_wifil_read_ends: null");
  return wl_drain(h->ends, out, cap, n);
}

// RxStart / CCA-busy notifications of phy, from the next advance on (in stream order with the epochs).  The flags
// and the epoch's note array are sized at the first opt-in: a Receive leaves at most one note, so the array holds
// what the epoch's event lists hold.
extern "C" int nsgpu_wifil_notify(nsgpu_wifil *h, uint32_t phy, int on) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_notify: bad phy");  // (before anything is sized)
  if (int rc = wl_single_only(h, NSGPU_ESTATE, "nsgpu_wifil_notify", "notifications are")) return rc;
  const uint8_t v = on ? 1 : 0;
  if (h->note_on.empty()) {
    if (!v) return NSGPU_OK;
    const uint64_t cap = (uint64_t)h->D.nphy * EVB + h->D.ev_cap;
    int rc = wl_alloc(h, &h->d_note_on, (size_t)h->D.nphy);
    if (!rc) rc = wl_alloc(h, &h->D.notes, (size_t)cap);
    if (rc) return rc;
    h->D.note_on = h->d_note_on;
    h->D.note_cap = cap;
    h->note_on.assign((size_t)h->D.nphy, 0);
  }
  if (h->note_on[phy] == v) return NSGPU_OK;
  hipLaunchKernelGGL(k_wl_set, dim3(1), dim3(1), 0, h->s, h->d_note_on + phy, (uint32_t)v);
  NSGPU_HIP(hipGetLastError());
  h->note_on[phy] = v;
  h->n_note_on += v ? 1 : (uint64_t)-1;
  return NSGPU_OK;
}

// The notes of the epochs advanced since the last call, in (ts, uid) order.
extern "C" int nsgpu_wifil_read_notes(nsgpu_wifil *h, nsgpu_wifil_note *out, uint64_t cap, uint64_t *n) {
  if (!h || !n) return set_error(NSGPU_EINVAL, "nsgpu_wifil_read_notes: null");
  return wl_drain(h->notes, out, cap, n);
}

// (runtime) The last epoch's EndReceive with this uid, and a phy's node (the hand-back's context).
bool nsgpu::wifil_epoch_end(const nsgpu_wifil *h, uint32_t uid, nsgpu_wifil_end *out) {
  for (const nsgpu_wifil_end &e : h->ends_epoch)
    if (e.uid == uid) {
      *out = e;
      return true;
    }
  return false;
}
uint32_t nsgpu::wifil_node(const nsgpu_wifil *h, uint32_t phy) {
  return phy < h->node_h.size() ? h->node_h[phy] : 0xffffffffu;
}

// ---------------- the partitioned PHY (SURVEY 8(e) for the closed loop: YansWifiChannel::Send's receivers
// split over GPUs) ----------------
// Every rank runs the same host program — the MAC's closures, the runtime's uids and order, GetState — over a
// replicated host handle (the one these functions take); the device work of a phy (its Receives,
// InterferenceHelper, state machine, EndReceive walks and PER chunks) runs on the partition that owns it.  A phy's
// chain needs no other phy's state, so the partitions exchange only per epoch: (1) the epoch's syncs — an
// EndReceive's uid is its sync's rank among every partition's syncs; (2) the counters, the end records (the
// host's m_random draws and hand-backs) and the phys' state fields (GetState, DcfManager's CCA queries); (3) the
// dispatched events, ordered over all partitions for the digest and the log.  The epochs run on one stream and
// the host waits for each exchange (no order behind the epoch: every partition's events are needed first).
// RCCL (nsgpu_wifil_create_dist): this rank's partition, the exchanges as all-gathers padded to the largest
// partition's count (every rank's lists are sized for the largest partition); loopback (nsgpu_wifil_create_group):
// every partition on this device, the exchanges as device copies.

// k words of every partition (partition order), each written by fn on its engine: a single engine is its own one
// partition; loopback from each member; RCCL this rank's, all-gathered.
template <class F>
static int wl_words(nsgpu_wifil *h, int k, F fn, std::vector<unsigned long long> &out) {
  if (!h->grp) {
    out.assign((size_t)k, 0ull);
    return fn(h, out.data());
  }
  const WlGroup &g = *h->grp;
  const int P = (int)g.plo.size();
  out.assign((size_t)P * k, 0ull);
  if (!g.comm) {
    for (int q = 0; q < P; q++)
      if (int rc = fn(g.mem[q], &out[(size_t)q * k])) return rc;
    return NSGPU_OK;
  }
  std::vector<unsigned long long> mine((size_t)k, 0ull);
  if (int rc = fn(g.mem[0], mine.data())) return rc;
  NSGPU_HIP(hipMemcpyAsync(g.ssm, mine.data(), (size_t)k * 8, hipMemcpyHostToDevice, h->s));
  NCCL_TRY(ncclAllGather(g.ssm, g.xsm, (size_t)k, ncclUint64, g.comm->comm, h->s));
  NSGPU_HIP(hipMemcpyAsync(out.data(), g.xsm, (size_t)P * k * 8, hipMemcpyDeviceToHost, h->s));
  NSGPU_HIP(hipStreamSynchronize(h->s));
  return NSGPU_OK;
}

// Every partition's first cnt[q] elements (esz bytes) of a device array, concatenated in partition order into
// dst: loopback from each member's array src(m), RCCL from this rank's, all-gathered padded to the largest count
// through xbuf (P x that count; every partition's array holds it: equal capacities).
template <class S>
static int wlg_cat(nsgpu_wifil *G, const std::vector<uint64_t> &cnt, size_t esz, S src, void *xbuf, void *dst) {
  const WlGroup &g = *G->grp;
  const hipStream_t s = G->s;
  const int P = (int)cnt.size();
  uint64_t off = 0;
  if (!g.comm) {
    for (int q = 0; q < P; q++) {
      if (cnt[q])
        NSGPU_HIP(hipMemcpyAsync((uint8_t *)dst + off * esz, src(g.mem[q]), cnt[q] * esz, hipMemcpyDeviceToDevice, s));
      off += cnt[q];
    }
    return NSGPU_OK;
  }
  uint64_t maxc = 0;
  for (uint64_t c : cnt) maxc = std::max(maxc, c);
  if (!maxc) return NSGPU_OK;
  NCCL_TRY(ncclAllGather(src(g.mem[0]), xbuf, maxc * esz, ncclUint8, g.comm->comm, s));
  for (int q = 0; q < P; q++) {
    if (cnt[q])
      NSGPU_HIP(hipMemcpyAsync((uint8_t *)dst + off * esz, (const uint8_t *)xbuf + (uint64_t)q * maxc * esz, cnt[q] * esz,
                               hipMemcpyDeviceToDevice, s));
    off += cnt[q];
  }
  return NSGPU_OK;
}

// The phys' state fields of every partition into the host's copy (RCCL; a loopback group's partitions write the
// one mapped copy themselves).
static int wlg_mirror(nsgpu_wifil *G) {
  const WlGroup &g = *G->grp;
  if (!g.comm) return NSGPU_OK;
  const hipStream_t s = G->s;
  const int P = (int)g.plo.size(), r = g.comm->rank;
  const int64_t lo = g.plo[r], n = g.phi[r] - g.plo[r];
  if (n) NSGPU_HIP(hipMemcpyAsync(g.smir, g.dmir + lo, (size_t)n * sizeof(WMir), hipMemcpyDeviceToDevice, s));
  NCCL_TRY(ncclAllGather(g.smir, g.xmir, (size_t)g.pmax * sizeof(WMir), ncclUint8, g.comm->comm, s));
  for (int q = 0; q < P; q++) {
    const int64_t nq = g.phi[q] - g.plo[q];
    if (nq)
      NSGPU_HIP(hipMemcpyAsync(G->h_mir + g.plo[q], g.xmir + (uint64_t)q * g.pmax, (size_t)nq * sizeof(WMir),
                               hipMemcpyDeviceToHost, s));
  }
  NSGPU_HIP(hipStreamSynchronize(s));
  return NSGPU_OK;
}

static int wlg_advance(nsgpu_wifil *G, uint64_t bts, uint32_t buid, uint32_t *uid, uint64_t *dispatched, uint64_t *digest,
                       const WlLog &log) {
  WlGroup &g = *G->grp;
  const hipStream_t s = G->s;
  const int P = (int)g.plo.size();
  // (1) every partition's epoch: the batched SendPackets, then its phys' events below the bound
  const WlStep step = wl_step_kernel(false, false);  // (a partitioned handle refuses notifications and switching)
  for (nsgpu_wifil *m : g.mem) {
    if (m->D.nown) hipLaunchKernelGGL(step, dim3((unsigned)m->D.nown), dim3(64), 0, s, m->D, bts, buid, m->sb);
    m->sb.n = 0;
  }
  NSGPU_HIP(hipGetLastError());
  // (2) the syncs of every partition
  std::vector<unsigned long long> &w = G->words;
  int rc = wl_words(G, 1, [&](nsgpu_wifil *m, unsigned long long *o) -> int {
    uint32_t c = 0;
    NSGPU_HIP(hipMemcpyAsync(&c, m->D.cnt + 1, sizeof(c), hipMemcpyDeviceToHost, s));
    NSGPU_HIP(hipStreamSynchronize(s));
    o[0] = std::min<uint64_t>(c, m->D.sync_cap);
    return NSGPU_OK;
  }, w);
  if (rc) return rc;
  std::vector<uint64_t> cnt((size_t)P);
  uint64_t tsy = 0;
  for (int q = 0; q < P; q++) cnt[q] = w[q], tsy += w[q];
  uint32_t xerr = 0;
  if (tsy > g.g_sync_cap) {  // (the single engine's capacity: the run fails as it would there)
    xerr |= WE_CAP;
    tsy = 0;
  } else if ((rc = wlg_cat(G, cnt, sizeof(LSync), [](nsgpu_wifil *m) { return (const void *)m->D.sync; }, g.xsr, g.xsync))) {
    return rc;
  }
  // (3) each partition's tail: PER products, its syncs' EndReceive uids (ranks among all), the close
  for (nsgpu_wifil *m : g.mem) {
    WDev Dm = m->D;
    Dm.xsync = g.xsync;
    Dm.xn = (uint32_t)tsy;
    hipLaunchKernelGGL(k_wl_mid, dim3(MID_PER + MID_RANK), dim3(256), 0, s, Dm, *uid, m->d_stat, ++m->seq);
  }
  NSGPU_HIP(hipGetLastError());
  NSGPU_HIP(hipStreamSynchronize(s));
  // (4) every partition's counters (the close's status block), then the checks before anything is published
  if ((rc = wl_words(G, 4, [&](nsgpu_wifil *m, unsigned long long *o) -> int {
         for (int i = 0; i < 4; i++) o[i] = m->h_cnt[i];
         return NSGPU_OK;
       }, w)))
    return rc;
  std::vector<uint64_t> nevq((size_t)P), nendq((size_t)P);
  uint64_t nev = 0, nend = 0, nsync = 0;
  uint32_t err = xerr;
  for (int q = 0; q < P; q++) {
    nevq[q] = w[(size_t)q * 4], nsync += w[(size_t)q * 4 + 1], nendq[q] = w[(size_t)q * 4 + 2];
    err |= (uint32_t)w[(size_t)q * 4 + 3];
    if ((rc = wl_check_counts(g.mem[0]->D, q, nevq[q], 0, nendq[q], 0))) return rc;  // (equal capacities)
    nev += nevq[q], nend += nendq[q];
  }
  if ((rc = wl_check_bits(err, "nsgpu_wifil_advance"))) return rc;
  if (nsync != tsy) return set_error(NSGPU_ESTATE, "nsgpu_wifil_advance: sync counts changed in the close");
  if ((rc = wl_check_uids(*uid, nsync))) return rc;
  // the end records (EndReceive uids patched by the closes) and the state fields
  if ((rc = wlg_cat(G, nendq, sizeof(nsgpu_wifil_end), [](nsgpu_wifil *m) { return (const void *)m->D.ends; }, g.xend,
                    g.uend)))
    return rc;
  G->ends_epoch.resize(nend);
  if (nend) NSGPU_HIP(hipMemcpyAsync(G->ends_epoch.data(), g.uend, nend * sizeof(nsgpu_wifil_end), hipMemcpyDeviceToHost, s));
  if ((rc = wlg_mirror(G))) return rc;
  // (5) the order over every partition's events: each gathers its own (uids resolved), the union is ranked once
  for (nsgpu_wifil *m : g.mem)
    if (m->D.nown) hipLaunchKernelGGL(k_wl_gather, dim3(wl_grid(m->D.nown, 256)), dim3(256), 0, s, m->D);
  if ((rc = wlg_cat(G, nevq, sizeof(LEv), [](nsgpu_wifil *m) { return (const void *)m->D.evd; }, g.xev, g.U.evd))) return rc;
  for (nsgpu_wifil *m : g.mem) hipLaunchKernelGGL(k_wl_zero, dim3(1), dim3(64), 0, s, m->D);
  const bool logging = log.on() && *dispatched < log.cap;
  hipLaunchKernelGGL(k_wl_set, dim3(1), dim3(1), 0, s, g.U.cnt, (uint32_t)nev);
  hipLaunchKernelGGL(k_wl_tsort, dim3(NTILE), dim3(TS_T), 0, s, g.U);
  hipLaunchKernelGGL(k_wl_rank, dim3(NTILE), dim3(TS_T), 0, s, g.U, *dispatched, logging ? 1 : 0, G->d_digtot);
  NSGPU_HIP(hipGetLastError());
  NSGPU_HIP(hipStreamSynchronize(s));
  if (nev > ERANK_MAX || (logging && nev))
    if ((rc = wl_fetch_events(G, g.U, nev))) return rc;
  wl_publish(G->ev, G->erank, nev, logging, log, dispatched, digest);
  wl_digest_catchup(G, digest);
  wl_sort_append(G->ends_epoch, G->ends);
  *uid += (uint32_t)nsync;
  return NSGPU_OK;
}

// ---------------- the between-epoch queries, of a single engine or of a partitioned handle ----------------
// Each has one probe per engine (the launch, the result words' copy back and the wait), run on the engine itself or
// on every partition (wl_words), and one reduction over the partitions' words.

// Pending Receive / EndReceive events and the smallest ts among them (~0: none).
static int wl_probe_pending(nsgpu_wifil *e, unsigned long long *o) {
  if (int rcf = wl_flush_sends(e)) return rcf;
  const unsigned long long init[2] = {0ull, ~0ull};
  NSGPU_HIP(hipMemcpyAsync(e->d_pend, init, sizeof(init), hipMemcpyHostToDevice, e->s));
  if (e->D.nown) hipLaunchKernelGGL(k_wl_pending, dim3(wl_grid(e->D.nown, 256)), dim3(256), 0, e->s, e->D, e->d_pend);
  NSGPU_HIP(hipGetLastError());
  NSGPU_HIP(hipMemcpyAsync(e->h_pend, e->d_pend, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->s));
  NSGPU_HIP(hipStreamSynchronize(e->s));
  o[0] = e->h_pend[0], o[1] = e->h_pend[1];
  return NSGPU_OK;
}
extern "C" int nsgpu_wifil_pending(nsgpu_wifil *h, uint64_t *n, uint64_t *next_ts) {
  if (!h || !n || !next_ts) return set_error(NSGPU_EINVAL, "nsgpu_wifil_pending: null");
  const std::vector<unsigned long long> &w = h->words;
  if (int rc = wl_words(h, 2, wl_probe_pending, h->words)) return rc;
  *n = 0;
  *next_ts = ~0ull;
  for (size_t q = 0; q < w.size() / 2; q++) *n += w[2 * q], *next_ts = std::min<uint64_t>(*next_ts, w[2 * q + 1]);
  return NSGPU_OK;
}

// The EndReceive hand-back: the host takes phy's EndReceives back (on = 1) or not.
extern "C" int nsgpu_wifil_listen(nsgpu_wifil *h, uint32_t phy, int on) {
  if (!h || phy >= h->D.nphy) return set_error(NSGPU_EINVAL, "nsgpu_wifil_listen: bad phy");
  const uint8_t v = on ? 1 : 0;
  if (h->lis_on[phy] != v) {
    h->lis_on[phy] = v;
    h->lis_dirty = true;
  }
  return NSGPU_OK;
}
// The listened phys among the engine's own, as the list its k_wl_nextend scans (uploaded on its stream; e->lis_list
// stays alive behind the copy).
static int wl_upload_listened(nsgpu_wifil *e, const std::vector<uint8_t> &on) {
  e->lis_list.clear();
  for (int64_t j = e->D.j0; j < e->D.j0 + e->D.nown; j++)
    if (on[(size_t)j]) e->lis_list.push_back((uint32_t)j);
  if (!e->lis_list.empty())
    NSGPU_HIP(hipMemcpyAsync(e->d_lis, e->lis_list.data(), e->lis_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, e->s));
  e->D.nlis = (uint32_t)e->lis_list.size();
  return NSGPU_OK;
}
static int wl_probe_next_end(nsgpu_wifil *e, unsigned long long *o) {
  hipLaunchKernelGGL(k_wl_nextend, dim3(1), dim3(256), 0, e->s, e->D, e->sb.n, e->d_next);
  NSGPU_HIP(hipGetLastError());
  NSGPU_HIP(hipMemcpyAsync(e->h_next, e->d_next, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->s));
  NSGPU_HIP(hipStreamSynchronize(e->s));
  for (int i = 0; i < 3; i++) o[i] = e->h_next[i];
  return NSGPU_OK;
}
// The next EndReceive of a listened phy (k_wl_nextend): a pending one (not cancelled) and the earliest time a
// sync not yet made could put one (see the kernel).  Valid between advances.
extern "C" int nsgpu_wifil_next_end(nsgpu_wifil *h, nsgpu_wifil_next *out) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_wifil_next_end: null");
  if (h->lis_dirty) {  // (each partition scans its own listened phys)
    if (!h->grp) {
      if (int rc = wl_upload_listened(h, h->lis_on)) return rc;
    } else {
      for (nsgpu_wifil *m : h->grp->mem)
        if (int rc = wl_upload_listened(m, h->lis_on)) return rc;
      // the handle's count is of every listened phy, not of this rank's: the same on every rank, so all of them
      // enter wl_words' gather below or none does
      h->D.nlis = (uint32_t)std::count(h->lis_on.begin(), h->lis_on.end(), (uint8_t)1);
    }
    h->lis_dirty = false;
  }
  memset(out, 0, sizeof(*out));
  out->ts = out->ts_potential = ~0ull;
  if (h->D.nlis == 0) return NSGPU_OK;
  const std::vector<unsigned long long> &w = h->words;
  if (int rc = wl_words(h, 3, wl_probe_next_end, h->words)) return rc;
  uint64_t bts = ~0ull, bkey = ~0ull;  // the earliest (ts, uid) among the partitions' (key: phy << 32 | uid, ~0: none)
  for (size_t q = 0; q < w.size() / 3; q++) {
    const uint64_t ts = w[3 * q], key = w[3 * q + 1];
    if (key != ~0ull && (ts < bts || (ts == bts && (uint32_t)key < (uint32_t)bkey))) bts = ts, bkey = key;
    out->ts_potential = std::min<uint64_t>(out->ts_potential, w[3 * q + 2]);
  }
  if (bkey != ~0ull) {
    out->found = 1;
    out->ts = bts;
    out->uid = (uint32_t)bkey;
    out->phy = (uint32_t)(bkey >> 32);
  }
  return NSGPU_OK;
}

static nsgpu_wifi_phy_counters wl_counters(const LPhy &p) {
  nsgpu_wifi_phy_counters c = p.c;
  c.ni_len = p.len;
  c.ni_max = p.ni_max;
  c.end_tx = p.endTx;
  c.end_rx = p.endRx;
  c.end_cca_busy = p.endCca;
  c.first_power = p.firstPower;
  c.rxing = p.rxing;
  return c;
}
// The engine's own phys' counters into out (indexed by the global phy): one copy, waited for.
static int wl_read_own(nsgpu_wifil *e, nsgpu_wifi_phy_counters *out) {
  std::vector<LPhy> ps((size_t)e->D.nown);
  if (e->D.nown)
    NSGPU_HIP(hipMemcpyAsync(ps.data(), e->D.ps + e->D.j0, ps.size() * sizeof(LPhy), hipMemcpyDeviceToHost, e->s));
  NSGPU_HIP(hipStreamSynchronize(e->s));
  for (size_t i = 0; i < ps.size(); i++) out[e->D.j0 + (int64_t)i] = wl_counters(ps[i]);
  return NSGPU_OK;
}

// Every phy's counters: the single engine's own, a loopback group's member by member, an RCCL handle's all-gathered
// (padded to the largest partition).
extern "C" int nsgpu_wifil_read_phys(nsgpu_wifil *h, nsgpu_wifi_phy_counters *out) {
  if (!h || !out) return set_error(NSGPU_EINVAL, "nsgpu_wifil_read_phys: null");
  if (!h->grp) {
    if (int rcf = wl_flush_sends(h)) return rcf;
    return wl_read_own(h, out);
  }
  const WlGroup &g = *h->grp;
  const hipStream_t s = h->s;
  for (nsgpu_wifil *m : g.mem)
    if (int rcf = wl_flush_sends(m)) return rcf;
  if (!g.comm) {
    for (nsgpu_wifil *m : g.mem)
      if (int rc = wl_read_own(m, out)) return rc;
    return NSGPU_OK;
  }
  const int P = (int)g.plo.size();
  const nsgpu_wifil *m = g.mem[0];
  if (m->D.nown)
    NSGPU_HIP(hipMemcpyAsync(g.sps, m->D.ps + m->D.j0, (size_t)m->D.nown * sizeof(LPhy), hipMemcpyDeviceToDevice, s));
  NCCL_TRY(ncclAllGather(g.sps, g.xps, (size_t)g.pmax * sizeof(LPhy), ncclUint8, g.comm->comm, s));
  std::vector<LPhy> ps((size_t)P * g.pmax);
  NSGPU_HIP(hipMemcpyAsync(ps.data(), g.xps, ps.size() * sizeof(LPhy), hipMemcpyDeviceToHost, s));
  NSGPU_HIP(hipStreamSynchronize(s));
  for (int q = 0; q < P; q++)
    for (int64_t i = 0; i < g.phi[q] - g.plo[q]; i++) out[g.plo[q] + i] = wl_counters(ps[(size_t)q * g.pmax + i]);
  return NSGPU_OK;
}

// The replicated host handle over partitions lo[q] .. hi[q] (contiguous, covering every phy): every partition on
// this device (comm null), or this rank's (comm).
static int wlg_make(const nsgpu_wifil_config *c, const std::vector<int64_t> &lo, const std::vector<int64_t> &hi,
                    nsgpu_comm *comm, nsgpu_wifil **out) {
  const int P = (int)lo.size();
  const int64_t N = c->n_phy;
  for (int q = 0; q < P; q++)
    if (lo[q] > hi[q] || (q == 0 ? lo[q] != 0 : lo[q] != hi[q - 1]) || (q == P - 1 && hi[q] != N))
      return set_error(NSGPU_EINVAL, "nsgpu_wifil partitions: [%lld, %lld) of partition %d does not continue the ones "
                                     "before it over [0, %lld)", (long long)lo[q], (long long)hi[q], q, (long long)N);
  nsgpu_wifil *G = new nsgpu_wifil();
  WlGroup &g = *(G->grp = new WlGroup());
  int rc;
#define WG_TRY(x)                \
  if ((rc = (x)) != NSGPU_OK) {  \
    nsgpu_wifil_destroy(G);      \
    return rc;                   \
  }
  g.comm = comm;
  g.plo = lo;
  g.phi = hi;
  for (int q = 0; q < P; q++) g.pmax = std::max<int64_t>(g.pmax, hi[q] - lo[q]);
  G->D.nphy = N;
  G->D.j0 = 0;
  G->D.nown = 0;  // (the handle runs no phy itself)
  std::vector<uint32_t> rank;
  wl_channel_ranks(c, rank, G->recv);
  G->node_h.assign(c->node, c->node + N);
  G->lis_on.assign((size_t)N, 0);
  G->tx_cap = c->tx_cap;
  if (hipStreamCreateWithPriority(&G->s, hipStreamNonBlocking, wl_prio(true)) != hipSuccess ||
      hipHostMalloc((void **)&G->h_mir, (size_t)N * sizeof(WMir), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostMalloc((void **)&G->h_digtot, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void **)&G->d_digtot, G->h_digtot, 0) != hipSuccess) {
    nsgpu_wifil_destroy(G);
    return set_error(NSGPU_EHIP, "nsgpu_wifil partitions: host buffers / stream");
  }
  std::memset(G->h_mir, 0, (size_t)N * sizeof(WMir));
  *G->h_digtot = 0;
  WMir *mir_dev = nullptr;  // (loopback: the partitions' lanes write the host's mapped copy)
  if (!comm && hipHostGetDevicePointer((void **)&mir_dev, G->h_mir, 0) != hipSuccess) {
    nsgpu_wifil_destroy(G);
    return set_error(NSGPU_EHIP, "nsgpu_wifil partitions: mapped mirror");
  }
  for (int q = 0; q < P; q++) {
    if (comm && q != comm->rank) continue;
    nsgpu_wifil *m = nullptr;
    WG_TRY(wl_create(c, lo[q], hi[q] - lo[q], g.pmax, G->s, &m));  // (every partition's kernels and copies in one order)
    g.mem.push_back(m);
  }
  if (comm) {
    WG_TRY(wl_alloc(G, &g.dmir, (size_t)N));
    mir_dev = g.dmir;
  }
  for (nsgpu_wifil *m : g.mem) m->D.mir = mir_dev;
  const nsgpu_wifil *m0 = g.mem[0];
  g.g_sync_cap = (uint64_t)N * LPE_CAP + 1024;  // (the single engine's)
  const uint64_t ev_per = (uint64_t)m0->D.nphy * EVB + m0->D.ev_cap;  // (a partition's dense events at most)
  const uint64_t u_evcap = (uint64_t)P * ev_per;
  WG_TRY(wl_alloc(G, &g.xsync, (size_t)g.g_sync_cap));
  WG_TRY(wl_alloc(G, &g.uend, (size_t)P * m0->D.end_cap));
  WDev &U = g.U;
  WG_TRY(wl_alloc(G, &U.evd, (size_t)u_evcap));
  WG_TRY(wl_alloc(G, &U.evg, (size_t)std::min<uint64_t>(u_evcap, ERANK_MAX)));
  WG_TRY(wl_alloc(G, &U.erank, (size_t)std::min<uint64_t>(u_evcap, ERANK_MAX)));
  WG_TRY(wl_alloc(G, &U.cnt, 8));
  WG_TRY(wl_alloc(G, &U.ticket, 1));
  WG_TRY(wl_alloc(G, &U.edig, 1));
  WG_TRY(wl_alloc(G, &U.gtot, 1));
  WG_TRY(wl_alloc(G, &U.evc, (size_t)EV_STRIPES * EV_STRIDE));
  WG_TRY(wl_alloc(G, &U.evt, (size_t)EV_STRIPES * EV_STRIDE));
  if (comm) {
    WG_TRY(wl_alloc(G, &g.xsr, (size_t)P * m0->D.sync_cap));
    WG_TRY(wl_alloc(G, &g.xev, (size_t)P * ev_per));
    WG_TRY(wl_alloc(G, &g.xend, (size_t)P * m0->D.end_cap));
    WG_TRY(wl_alloc(G, &g.smir, (size_t)std::max<int64_t>(g.pmax, 1)));
    WG_TRY(wl_alloc(G, &g.xmir, (size_t)P * std::max<int64_t>(g.pmax, 1)));
    WG_TRY(wl_alloc(G, &g.sps, (size_t)std::max<int64_t>(g.pmax, 1) * sizeof(LPhy)));
    WG_TRY(wl_alloc(G, &g.xps, (size_t)P * std::max<int64_t>(g.pmax, 1) * sizeof(LPhy)));
    WG_TRY(wl_alloc(G, &g.ssm, 8));
    WG_TRY(wl_alloc(G, &g.xsm, (size_t)P * 8));
  }
#undef WG_TRY
  *out = G;
  return NSGPU_OK;
}

extern "C" int nsgpu_wifil_create_group(const nsgpu_wifil_config *c, const int64_t *bounds, int n, nsgpu_wifil **out) {
  if (!c || !out || !bounds || n < 1 || c->n_phy <= 0) return set_error(NSGPU_EINVAL, "nsgpu_wifil_create_group: bad arguments");
  std::vector<int64_t> lo((size_t)n), hi((size_t)n);
  for (int q = 0; q < n; q++) lo[q] = bounds[q], hi[q] = bounds[q + 1];
  return wlg_make(c, lo, hi, nullptr, out);
}

extern "C" int nsgpu_wifil_create_dist(const nsgpu_wifil_config *c, int64_t phy_begin, int64_t phy_end, nsgpu_comm *comm,
                                       nsgpu_wifil **out) {
  if (!c || !out || !comm || c->n_phy <= 0) return set_error(NSGPU_EINVAL, "nsgpu_wifil_create_dist: bad arguments");
  // every rank's partition, gathered (each rank checks the same list: all fail or none)
  const int R = comm->nranks;
  unsigned long long *d = nullptr;
  std::vector<unsigned long long> all((size_t)2 * R);
  const unsigned long long mine[2] = {(unsigned long long)phy_begin, (unsigned long long)phy_end};
  hipStream_t s = nullptr;
  NSGPU_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  hipError_t e = hipMalloc((void **)&d, (size_t)(2 + 2 * R) * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemcpyAsync(d, mine, sizeof(mine), hipMemcpyHostToDevice, s);
  ncclResult_t nr = ncclSuccess;
  if (e == hipSuccess) nr = ncclAllGather(d, d + 2, 2, ncclUint64, comm->comm, s);
  if (e == hipSuccess && nr == ncclSuccess) e = hipMemcpyAsync(all.data(), d + 2, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (d) (void)hipFree(d);
  (void)hipStreamDestroy(s);
  if (e != hipSuccess) return set_error(NSGPU_EHIP, "nsgpu_wifil_create_dist: %s", hipGetErrorString(e));
  if (nr != ncclSuccess) return set_error(NSGPU_EHIP, "nsgpu_wifil_create_dist: %s", ncclGetErrorString(nr));
  std::vector<int64_t> lo((size_t)R), hi((size_t)R);
  for (int q = 0; q < R; q++) lo[q] = (int64_t)all[2 * q], hi[q] = (int64_t)all[2 * q + 1];
  return wlg_make(c, lo, hi, comm, out);
}

#ifdef NSGPU_PHASE_PROF
// (diagnostic build only) k_wl_stepw's wave records: arm for WREC_E epochs from `target` on (out null), or read
// them (out: WREC_E x WREC_P x 5 words)
extern "C" int nsgpu_wifil_prof_waves(uint32_t target, unsigned long long *out) {
  NSGPU_HIP(hipDeviceSynchronize());
  if (!out) {
    const uint32_t z = 0;
    NSGPU_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_wepoch), &z, sizeof(z)));
    NSGPU_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_wtarget), &target, sizeof(target)));
    return NSGPU_OK;
  }
  NSGPU_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wrec), sizeof(unsigned long long) * WREC_E * WREC_P * 5));
  return NSGPU_OK;
}
#endif
