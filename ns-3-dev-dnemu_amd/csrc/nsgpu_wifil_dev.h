// nsgpu_wifil_dev.h — the closed-loop Wi-Fi PHY's device code: the structs, the model code and every kernel
// (included once, by nsgpu_wifil.hip, whose header says what the engine replaces and how its epochs run; the host
// side — engine, partitioned handle, C ABI — is that file).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "nsgpu_device.h"
#include "nsgpu_internal.h"
#include "nsgpu_wave.h"

namespace nsgpu {
namespace {

constexpr uint32_t NONE = 0xffffffffu;
constexpr int LPE_CAP = 8;  // pending EndReceive records of one phy (the live one + cancelled ones)
constexpr uint32_t END_STAGE = 128;  // EndReceive records an epoch returns with its counters (more: a second copy)
constexpr size_t STAT_HDR = 32;      // the status block: counters (6 x u32), the epoch flag (word 6), then the ends
static_assert(sizeof(nsgpu_wifil_end) % 8 == 0 && STAT_HDR % 8 == 0, "status block alignment");
constexpr uint32_t WE_TX_IN_TX = 1, WE_NICAP = 2, WE_RQCAP = 4, WE_PECAP = 8, WE_CAP = 16, WE_CKCAP = 32, WE_NOTECAP = 64;
constexpr uint32_t WE_TX_IN_SWITCHING = 128;

struct LNi {  // InterferenceHelper::NiChange (interference-helper.cc:91-110)
  int64_t t;
  double d;
};
struct LRx {  // a pending Receive: arrival, uid, transmission, rxPowerW (DbmToW of CalcRxPower + RxGain), and
  uint64_t at;  // the transmission's duration (so a Receive needs no second load)
  uint32_t uid, tx;
  double w;
  int64_t dur;
};
struct LPe {  // a pending EndReceive
  uint64_t ts, sts;          // its ts; the syncing Receive's ts
  uint32_t suid, euid;       // the syncing Receive's uid; its own uid (NONE: scheduled in the running epoch)
  uint32_t tx, can, sslot, used;
  double w;                  // rxPowerW
};
struct LTx {  // one SendPacket: duration and payload mode
  uint64_t ts;
  int64_t dur;
  uint64_t rate;
  uint32_t phy, mc, bw, preamble;
};
struct LPhy {  // a phy's state between epochs
  double firstPower, cur_s;      // InterferenceHelper::m_firstPower; the ring's prefix-cursor sum
  int64_t endTx, endRx, endCca;  // WifiPhyStateHelper m_endTx / m_endRx / m_endCcaBusy
  uint32_t rxing, head, len, cur_n;
  uint32_t rq_head, rq_len, live, ni_max;
  nsgpu_wifi_phy_counters c;
  // channel switching (nsgpu_wifil_set_channel): WifiPhyStateHelper m_endSwitching / m_startSwitching, the
  // switches made and the frames dropped while switching (outside c: the oracle shares that struct).  Only
  // k_wl_switch writes endSw / startSw / switches; an epoch kernel that is not the SW instantiation neither
  // reads nor stores this tail (LPHY_HEAD)
  int64_t endSw, startSw;
  uint32_t switches, drop_switching;
};
constexpr size_t LPHY_HEAD = offsetof(LPhy, endSw);
struct WMir {  // a phy's state helper fields in pinned host memory: GetState reads them with no device trip
  int64_t endTx, endRx, endCca;
  uint32_t rxing, pad;
  int64_t endSw;  // (written by k_wl_switch and the host's copy of it alone: the epoch kernels store WMIR_HEAD bytes)
};
constexpr size_t WMIR_HEAD = offsetof(WMir, endSw);
struct LEv {  // one dispatched device event of the epoch
  uint64_t ts;
  uint32_t uid, ctx, sslot, pad;
};
struct LSync {  // one sync of the epoch (its EndReceive's uid comes from the sync order)
  uint64_t sts;
  uint32_t suid, euid;
  uint32_t loc, pad;  // its pending EndReceive record: pe[loc]
};
struct WMove {  // a phy's motion model (kind) next to its position D.x / y / z: a ConstantVelocityHelper
                // (constant-velocity-helper.h), a WaypointMobilityModel or a ConstantAccelerationMobilityModel
  uint32_t kind, flag;     // MOVE_NONE (a constant-position phy) / MOVE_VEL / MOVE_WAY / MOVE_ACC; constant velocity:
                           //   m_paused; waypoint: m_first
  uint32_t off, head, cnt, pad;  // waypoint: m_waypoints is D.wpool[off + head, off + cnt) (the pop advances head)
  int64_t cur_t, next_t;   // constant velocity: m_lastUpdate in cur_t; waypoint: m_current.time, m_next.time (signed:
                           //   Seconds (-1) ends the path); acceleration: m_baseTime in cur_t
  double p[3], v[3], a[3];  // constant velocity: m_velocity in v (m_position is D.x / y / z); waypoint: m_next.position,
                            //   m_velocity (m_current.position is D.x / y / z); acceleration: m_basePosition,
                            //   m_baseVelocity, m_acceleration
};
constexpr uint32_t MOVE_NONE = 0, MOVE_VEL = 1, MOVE_WAY = 2, MOVE_ACC = 3;
constexpr int64_t WAY_ENDED = -1000000000;  // Seconds (-1.0)
constexpr int WP_CHUNK = 8;
struct WpChunk {  // waypoints carried to the pool as a kernel argument (k_wl_wput): no staging buffer to outlive
  nsgpu_waypoint w[WP_CHUNK];
};
struct LCk {  // one chunk of an EndReceive's CalculatePer walk, evaluated by k_wl_mid: the noise before it,
  double noise;  // and (duration << 1) | (1: the PLCP header mode)
  int64_t dm;
};
struct LEck {  // an end record's chunks: ck[start, start + n) (n = NONE: its PER was computed inline)
  uint32_t start, n;
  double w;  // rxPowerW
};

struct LossX {  // an installed extended chain (nsgpu_wifil_set_loss), device-resident: the links and the Matrix table
  int32_t n, pad;
  nsgpu_lossx_model m[NSGPU_MAX_LOSS_CHAIN];
  LossTable tb;
};

struct WDev {
  int64_t nphy;
  const double *x, *y, *z;
  const uint32_t *chan, *chan_rank, *node;
  nsgpu_loss_chain loss;
  double speed, rx_gain_db, edW, ccaW, nf;  // nf: the noise figure as a ratio (DbToRatio)
  uint32_t model, ni_mask, rq_mask, pad;
  uint64_t inv_hi, inv_lo;  // int64x64_t::Invert (1e9): Time::GetSeconds at NS resolution
  LPhy *ps;
  LNi *ni;
  LRx *rq;
  LPe *pe;
  LTx *tx;
  LSync *sync;
  LEv *ev;
  nsgpu_wifil_end *ends;
  uint32_t *end_sslot;
  uint32_t *cnt;  // [0] events, [1] syncs, [2] ends, [3] error bits (sticky: a SendPacket's are seen at the
                  // next advance), [4] chunk slots claimed, [5] notes ([0..2], [4], [5] zeroed by the order's
                  // k_wl_rank, for the epoch two on)
  LCk *ck;        // the epoch's deferred chunks (ck_cap; a walk that finds no room computes its PER inline)
  LEck *eck;      // per end record
  uint32_t *evc;             // the epoch's event-list stripes: EV_STRIPES counters, EV_STRIDE words apart
  LEv *evd;                  // the epoch's events in dense order, uids resolved (k_wl_gather; the host's copy)
  LEv *evp;                  // a phy's events of the epoch in its own EVB slots (k_wl_stepw, no claim); by parity
  uint32_t *evn;             // their counts (zeroed by k_wl_gather once read); by parity
  uint32_t *evt;             // their total, EV_STRIPES counters EV_STRIDE words apart (one would serialize 10^4
                             //   adds on one line); by parity, zeroed by k_wl_rank for the epoch two on
  uint32_t *gtot;            // k_wl_gather's claims (reset by k_wl_tsort)
  uint32_t *erank;           // the epoch's events: rank in its (ts, uid) order (k_wl_rank, when logging)
  ulonglong2 *evg;           // the epoch's keys (ts, uid << 32 | dense index), sorted by tiles (k_wl_tsort)
  uint32_t *ticket;          // k_wl_rank's blocks done (its last block: the digest sum, the counters' zeroing)
  uint32_t *mticket;         // k_wl_mid's blocks done (its last block closes the epoch: wl_fin)
  WMir *mir;                 // (mapped host memory) each phy's state fields: a lane whose phy changed writes them
  LRx *rxb;                  // the batched SendPackets' Receives, NSEND x nphy (k_wl_rx; at = ~0: none for that phy)
  unsigned long long *edig;  // every ordered epoch's digest terms, summed on the device (k_wl_rank)
  uint64_t sync_cap, ev_cap, end_cap, ck_cap;
  uint64_t ev_scap;  // events per stripe (stripe s holds ev[s * ev_scap, s * ev_scap + evc[s * EV_STRIDE]))
  const uint32_t *lis;  // the phys whose EndReceives the host takes back (nsgpu_wifil_listen), nlis of them
  uint32_t nlis, pad_lis;
  // a partition of the phys (nsgpu_wifil_create_dist / _group): this engine runs phys [j0, j0 + nown) — their
  // waves, Receives, pending records — while every array stays indexed by the global phy; a single engine has
  // j0 = 0, nown = nphy.  xsync: every partition's syncs of the epoch (xn of them) the sync order ranks this
  // partition's against (null: its own, the single engine).
  int64_t j0, nown;
  const LSync *xsync;
  uint32_t xn, pad_x;
  // RxStart / CCA-busy notifications (nsgpu_wifil_notify): a flag per phy, and the epoch's notes (k_wl_stepw<true, *>,
  // launched only while some phy notifies; the host reads them before the next epoch: one array, no parity)
  const uint32_t *note_on;
  nsgpu_wifil_note *notes;
  uint64_t note_cap;
  // mobility (nsgpu_wifil_set_mobility / _set_waypoints / _set_acceleration): a record per phy, sized at the first
  // install of any model (null until then); k_wl_move, launched ahead of a send's k_wl_rx only while some phy has a
  // model, updates x / y / z, and the one-thread host calls (k_wl_mop) read and write it
  WMove *mov;
  // the extended loss chain (nsgpu_wifil_set_loss): null until one is installed; only k_wl_send<true> / k_wl_rx<true>,
  // launched while one is, read it
  const LossX *lx;
  // the one pool every phy's waypoint list lives in (WMove::off), null until the first waypoint install
  nsgpu_waypoint *wpool;
};
// The epoch's dispatched events are appended to EV_STRIPES lists (phy j's to stripe j % EV_STRIPES): one
// counter a phy's event would serialize ~10^4 atomics an epoch on one line.
constexpr int EV_STRIPES = 64, EV_STRIDE = 32;

// ---- WifiMode attributes (the CreateWifiMode calls of wifi-phy.cc:355-840; phyRate: wifi-mode.cc:140-155) ----
struct Mode {
  uint32_t mc, bw, phy_rate, cons, code;  // code: 0 undefined, 1: 1/2, 2: 2/3, 3: 3/4
  uint64_t data_rate;
};
__host__ __device__ __forceinline__ Mode make_mode(uint32_t mc, uint64_t rate, uint32_t bw) {
  Mode m{mc, mc == NSGPU_WIFI_DSSS ? 22000000u : bw, (uint32_t)rate, rate == 1000000 ? 2u : 4u, 0u, rate};
  if (mc == NSGPU_WIFI_DSSS) return m;
  switch (rate * 20000000ull / m.bw) {  // the 20 MHz OFDM ladder; 10 / 5 MHz channels run at 1/2, 1/4 the rates
    case 6000000: m.cons = 2, m.code = 1; break;
    case 9000000: m.cons = 2, m.code = 3; break;
    case 12000000: m.cons = 4, m.code = 1; break;
    case 18000000: m.cons = 4, m.code = 3; break;
    case 24000000: m.cons = 16, m.code = 1; break;
    case 36000000: m.cons = 16, m.code = 3; break;
    case 48000000: m.cons = 64, m.code = 2; break;
    default: m.cons = 64, m.code = 3; break;
  }
  const uint32_t dr = (uint32_t)rate;
  m.phy_rate = m.code == 1 ? dr * 2 / 1 : m.code == 2 ? dr * 3 / 2 : dr * 4 / 3;
  return m;
}
// WifiPhy::GetPlcpHeaderMode — wifi-phy.cc:99-139
__device__ __forceinline__ Mode header_mode(const Mode &p, uint32_t preamble) {
  if (p.mc == NSGPU_WIFI_OFDM)
    return p.bw == 5000000 ? make_mode(NSGPU_WIFI_OFDM, 1500000, 5000000)
           : p.bw == 10000000 ? make_mode(NSGPU_WIFI_OFDM, 3000000, 10000000)
                              : make_mode(NSGPU_WIFI_OFDM, 6000000, 20000000);
  if (p.mc == NSGPU_WIFI_ERP_OFDM) return make_mode(NSGPU_WIFI_ERP_OFDM, 6000000, 20000000);
  return make_mode(NSGPU_WIFI_DSSS, preamble == NSGPU_WIFI_PREAMBLE_LONG ? 1000000 : 2000000, 22000000);
}
// WifiPhy::GetPlcpPreambleDurationMicroSeconds / GetPlcpHeaderDurationMicroSeconds — wifi-phy.cc:141-231
__device__ __forceinline__ uint32_t preamble_us(uint32_t mc, uint32_t bw, uint32_t preamble) {
  if (mc == NSGPU_WIFI_OFDM) return bw == 10000000 ? 32 : bw == 5000000 ? 64 : 16;
  if (mc == NSGPU_WIFI_ERP_OFDM) return 4;
  return preamble == NSGPU_WIFI_PREAMBLE_SHORT ? 72 : 144;
}
__device__ __forceinline__ uint32_t header_us(uint32_t mc, uint32_t bw, uint32_t preamble) {
  if (mc == NSGPU_WIFI_OFDM) return bw == 10000000 ? 8 : bw == 5000000 ? 16 : 4;
  if (mc == NSGPU_WIFI_ERP_OFDM) return 16;
  return preamble == NSGPU_WIFI_PREAMBLE_SHORT ? 24 : 48;
}

// ---- error-rate models ----
// DsssErrorRateModel — dsss-error-rate-model.cc:29-127, ENABLE_GSL unset (the CCK rates use the Matlab fits)
__device__ double dsss_success(uint64_t rate, double sinr, uint32_t nbits) {
  double ber;
  switch (rate) {
    case 1000000: {
      double EbN0 = sinr * 22000000.0 / 1000000.0;
      ber = 0.5 * exp(-EbN0);
      break;
    }
    case 2000000: {
      double x = sinr * 22000000.0 / 1000000.0 / 2.0;  // DqpskFunction (:29-35)
      ber = ((sqrt(2.0) + 1.0) / sqrt(8.0 * 3.1415926 * sqrt(2.0))) * (1.0 / sqrt(x)) * exp(-(2.0 - sqrt(2.0)) * x);
      break;
    }
    case 5500000:
      if (sinr > 10.0) ber = 0.0;
      else if (sinr < 0.1) ber = 0.5;
      else ber = 5.3681634344056195e-001 * exp(-(pow((sinr - 3.3092430025608586e-003) / 4.1654372361004000e-001,
                                                     1.0288981434358866e+000)));
      break;
    case 11000000:
      if (sinr > 10.0) ber = 0.0;
      else if (sinr < 0.1) ber = 0.5;
      else {
        const double a1 = 7.9056742265333456e-003, a2 = -1.8397449399176360e-001, a3 = 1.0740689468707241e+000,
                     a4 = 1.0523316904502553e+000, a5 = 3.0552298746496687e-001, a6 = 2.2032715128698435e+000;
        ber = (a1 * sinr * sinr + a2 * sinr + a3) / (sinr * sinr * sinr + a4 * sinr * sinr + a5 * sinr + a6);
      }
      break;
    default:
      return 0;
  }
  return pow((1.0 - ber), (double)nbits);
}
// NistErrorRateModel — nist-error-rate-model.cc:38-270 (YansWifiPhyHelper::Default's model)
__device__ double nist_pe(double p, uint32_t b) {  // CalculatePe
  const double D = sqrt(4.0 * p * (1.0 - p));
  if (b == 1)
    return 0.5 * (36.0 * pow(D, 10.0) + 211.0 * pow(D, 12.0) + 1404.0 * pow(D, 14.0) + 11633.0 * pow(D, 16.0) +
                  77433.0 * pow(D, 18.0) + 502690.0 * pow(D, 20.0) + 3322763.0 * pow(D, 22.0) +
                  21292910.0 * pow(D, 24.0) + 134365911.0 * pow(D, 26.0));
  if (b == 2)
    return 1.0 / (2.0 * b) *
           (3.0 * pow(D, 6.0) + 70.0 * pow(D, 7.0) + 285.0 * pow(D, 8.0) + 1276.0 * pow(D, 9.0) + 6160.0 * pow(D, 10.0) +
            27128.0 * pow(D, 11.0) + 117019.0 * pow(D, 12.0) + 498860.0 * pow(D, 13.0) + 2103891.0 * pow(D, 14.0) +
            8784123.0 * pow(D, 15.0));
  return 1.0 / (2.0 * b) *
         (42.0 * pow(D, 5.0) + 201.0 * pow(D, 6.0) + 1492.0 * pow(D, 7.0) + 10469.0 * pow(D, 8.0) + 62935.0 * pow(D, 9.0) +
          379644.0 * pow(D, 10.0) + 2253373.0 * pow(D, 11.0) + 13073811.0 * pow(D, 12.0) + 75152755.0 * pow(D, 13.0) +
          428005675.0 * pow(D, 14.0));
}
__device__ double nist_success(const Mode &m, double snr, uint32_t nbits) {
  if (m.mc == NSGPU_WIFI_DSSS) return dsss_success(m.data_rate, snr, nbits);
  const uint32_t b = m.cons == 64 ? (m.code == 2 ? 2u : 3u) : (m.code == 1 ? 1u : 3u);
  double ber;
  switch (m.cons) {
    case 2: ber = 0.5 * erfc(sqrt(snr)); break;                               // GetBpskBer
    case 4: ber = 0.5 * erfc(sqrt(snr / 2.0)); break;                         // GetQpskBer
    case 16: ber = 0.75 * 0.5 * erfc(sqrt(snr / (5.0 * 2.0))); break;         // Get16QamBer
    default: ber = 7.0 / 12.0 * 0.5 * erfc(sqrt(snr / (21.0 * 2.0))); break;  // Get64QamBer
  }
  if (ber == 0.0) return 1.0;  // GetFec*Ber
  double pe = nist_pe(ber, b);
  pe = pe < 1.0 ? pe : 1.0;
  return pow(1 - pe, (double)nbits);
}
// YansErrorRateModel — yans-error-rate-model.cc:45-300
__device__ uint32_t yans_factorial(uint32_t k) {
  uint32_t f = 1;
  while (k > 0) f *= k--;
  return f;
}
__device__ double yans_binomial(uint32_t k, double p, uint32_t n) {
  return yans_factorial(n) / (yans_factorial(k) * yans_factorial(n - k)) * pow(p, (double)k) * pow(1 - p, (double)(n - k));
}
__device__ double yans_pd(double ber, uint32_t d) {  // CalculatePd (Odd / Even)
  double pd = 0;
  if ((d % 2) == 0) {
    for (uint32_t i = d / 2 + 1; i < d; i++) pd += yans_binomial(i, ber, d);
    pd += 0.5 * yans_binomial(d / 2, ber, d);
  } else {
    for (uint32_t i = (d + 1) / 2; i < d; i++) pd += yans_binomial(i, ber, d);
  }
  return pd;
}
__device__ double yans_success(const Mode &m, double snr, uint32_t nbits) {
  if (m.mc == NSGPU_WIFI_DSSS) return dsss_success(m.data_rate, snr, nbits);
  const double EbNo = snr * m.bw / m.phy_rate;
  if (m.cons == 2) {  // GetFecBpskBer
    const double ber = 0.5 * erfc(sqrt(EbNo));
    const uint32_t dFree = m.code == 1 ? 10 : 5, adFree = m.code == 1 ? 11 : 8;
    if (ber == 0.0) return 1.0;
    double pmu = adFree * yans_pd(ber, dFree);
    pmu = pmu < 1.0 ? pmu : 1.0;
    return pow(1 - pmu, (double)nbits);
  }
  const unsigned int M = m.cons;  // GetQamBer + GetFecQamBer
  const double z = sqrt((1.5 * (log((double)M) / log(2.0)) * EbNo) / (M - 1.0));
  const double z1 = ((1.0 - 1.0 / sqrt((double)M)) * erfc(z));
  const double z2 = 1 - pow((1 - z1), 2.0);
  const double ber = z2 / (log((double)M) / log(2.0));
  uint32_t dFree, adFree, adFree1;
  if (M == 64) {
    if (m.code == 2) dFree = 6, adFree = 1, adFree1 = 16;
    else dFree = 5, adFree = 8, adFree1 = 31;
  } else {
    if (m.code == 1) dFree = 10, adFree = 11, adFree1 = 0;
    else dFree = 5, adFree = 8, adFree1 = 31;
  }
  if (ber == 0.0) return 1.0;
  double pmu = adFree * yans_pd(ber, dFree);
  pmu += adFree1 * yans_pd(ber, dFree + 1);
  pmu = pmu < 1.0 ? pmu : 1.0;
  return pow(1 - pmu, (double)nbits);
}

// Time::GetSeconds at NS resolution: To (S) = MulByInvert (Invert (1e9)) then GetDouble
// (nstime.h:398-431, int64x64-128.cc:94-118, int64x64-128.h:83-95).
__device__ __forceinline__ double get_seconds(const WDev &D, int64_t ts) {
  const bool neg = ts < 0;
  const u128 a = (u128)(neg ? -ts : ts) << 64;
  const u128 b = ((u128)D.inv_hi << 64) | D.inv_lo;
  const u128 ah = a >> 64, bh = b >> 64, al = a & (u128)~0ull, bl = b & (u128)~0ull;
  u128 mid = ah * bl + al * bh;
  mid >>= 64;
  const u128 r = ah * bh + mid;
  const uint64_t hi = (uint64_t)(r >> 64), lo = (uint64_t)r;
  double flo = (double)lo;
  flo /= 18446744073709551615.0;
  double v = (double)hi;
  v += flo;
  return neg ? -v : v;
}
// ConstantVelocityHelper::Update (constant-velocity-helper.cc:69-84) of phy j at `now`, restated literally: the
// products and sums round one by one (the library is built -ffp-contract=off: no FMA), so the doubles depend on
// the accumulation points exactly as the reference's do.
__device__ __forceinline__ void vel_update(const WDev &D, int64_t j, int64_t now) {
  WMove &m = D.mov[j];
  const int64_t delta = now - m.cur_t;  // Time deltaTime = now - m_lastUpdate
  m.cur_t = now;
  if (m.flag) return;                   // m_paused
  const double deltaS = get_seconds(D, delta);
  double *const x = const_cast<double *>(D.x), *const y = const_cast<double *>(D.y), *const z = const_cast<double *>(D.z);
  x[j] += m.v[0] * deltaS;
  y[j] += m.v[1] * deltaS;
  z[j] += m.v[2] * deltaS;
}
// WaypointMobilityModel::Update (waypoint-mobility-model.cc:114-173) of phy j at `now`, statement by statement
// (NotifyCourseChange has no listener here).  m_current.position is D.x / y / z [j]; the divisions are IEEE double
// divisions, the products and sums round one by one.  One call may cross several waypoints: the loop pops at most
// the queue's length.
__device__ __forceinline__ void way_update(const WDev &D, int64_t j, int64_t now) {
  WMove &m = D.mov[j];
  int64_t cur_t = m.cur_t, next_t = m.next_t;
  if (now < cur_t) return;                                     // :119-122
  double *const x = const_cast<double *>(D.x), *const y = const_cast<double *>(D.y), *const z = const_cast<double *>(D.z);
  double cx = x[j], cy = y[j], cz = z[j];
  double nx = m.p[0], ny = m.p[1], nz = m.p[2], vx = m.v[0], vy = m.v[1], vz = m.v[2];
  uint32_t head = m.head;
  const uint32_t cnt = m.cnt;
  bool done = false;
  while (now >= next_t) {                                      // :124
    if (head == cnt) {                                         // :126 m_waypoints.empty ()
      if (cur_t <= next_t) {                                   // :128 ('<=': a path of one waypoint)
        next_t = WAY_ENDED;                                    // :134
        cx = nx, cy = ny, cz = nz;                             // :135
        cur_t = now;                                           // :136
        vx = vy = vz = 0.0;                                    // :137
      } else {
        cur_t = now;                                           // :142
      }
      done = true;                                             // :145 return
      break;
    }
    cur_t = next_t, cx = nx, cy = ny, cz = nz;                 // :148 m_current = m_next
    const nsgpu_waypoint w = D.wpool[m.off + head];            // :149-150 front (), pop_front ()
    head++;
    next_t = (int64_t)w.time, nx = w.pos[0], ny = w.pos[1], nz = w.pos[2];
    const double t_span = get_seconds(D, next_t - cur_t);      // :153
    vx = (nx - cx) / t_span;                                   // :155-157
    vy = (ny - cy) / t_span;
    vz = (nz - cz) / t_span;
  }
  if (!done && now > cur_t) {                                  // :160
    const double t_diff = get_seconds(D, now - cur_t);         // :162
    cx += vx * t_diff;                                         // :163-165
    cy += vy * t_diff;
    cz += vz * t_diff;
    cur_t = now;                                               // :166
  }
  x[j] = cx, y[j] = cy, z[j] = cz;
  m.cur_t = cur_t, m.next_t = next_t, m.head = head;
  m.p[0] = nx, m.p[1] = ny, m.p[2] = nz, m.v[0] = vx, m.v[1] = vy, m.v[2] = vz;
}
// ConstantAccelerationMobilityModel::DoGetPosition / DoGetVelocity (constant-acceleration-mobility-model.cc:41-58)
// of phy j's record at `now`: (base + v t) + a (t t 0.5), each product and sum rounded.
__device__ __forceinline__ void acc_position(const WDev &D, const WMove &m, int64_t now, double out[3]) {
  const double t = get_seconds(D, now - m.cur_t);
  const double half_t_square = t * t * 0.5;
  for (int c = 0; c < 3; c++) out[c] = m.p[c] + m.v[c] * t + m.a[c] * half_t_square;
}
__device__ __forceinline__ void acc_velocity(const WDev &D, const WMove &m, int64_t now, double out[3]) {
  const double t = get_seconds(D, now - m.cur_t);
  for (int c = 0; c < 3; c++) out[c] = m.v[c] + m.a[c] * t;
}
// Phy j's model brought up to date at `now` (a send's position read, or a host call's): the kind's Update /
// DoGetPosition.  A phy without a model is untouched.  An acceleration phy stores nothing but the position it
// evaluated: on another channel than the sender's its D.x / y / z stay stale, which nobody reads until the phy is
// next on a sender's channel, and this rewrites them then (nsgpu_wifil_get_acceleration computes, it never reads
// them).
__device__ __forceinline__ void move_update(const WDev &D, int64_t j, int64_t now) {
  const WMove &m = D.mov[j];
  if (m.kind == MOVE_VEL) {
    vel_update(D, j, now);
  } else if (m.kind == MOVE_WAY) {
    way_update(D, j, now);
  } else if (m.kind == MOVE_ACC) {
    double p[3];
    acc_position(D, m, now, p);
    const_cast<double *>(D.x)[j] = p[0], const_cast<double *>(D.y)[j] = p[1], const_cast<double *>(D.z)[j] = p[2];
  }
}
// InterferenceHelper::CalculateChunkSuccessRate — interference-helper.cc:244-255
__device__ double chunk(const WDev &D, double snir, int64_t duration, const Mode &m) {
  if (duration == 0) return 1.0;
  const uint32_t rate = m.phy_rate;
  const uint64_t nbits = (uint64_t)(rate * get_seconds(D, duration));
  return D.model == NSGPU_WIFIL_YANS ? yans_success(m, snir, (uint32_t)nbits) : nist_success(m, snir, (uint32_t)nbits);
}
// InterferenceHelper::CalculateSnr — interference-helper.cc:215-227
__device__ __forceinline__ double snr_of(const WDev &D, double signal, double noiseInterference, const Mode &m) {
  const double Nt = 1.3803e-23 * 290.0 * m.bw;  // BOLTZMANN
  const double noiseFloor = D.nf * Nt;
  const double noise = noiseFloor + noiseInterference;
  return signal / noise;
}

// YansWifiChannel::Send's delivery of transmission t (index k, from the closure's uid base) to phy j (not the
// sender): its Receive — ConstantSpeed delay, the loss chain + RxGain, DbmToW, the receiver loop's uid.  LX: the
// chain is the installed extended one (D.lx: links that take the two phys and their heights); <false> is the
// config's chain and never names D.lx.
template <bool LX>
__device__ __forceinline__ bool reception(const WDev &D, int64_t j, const LTx &t, uint32_t k, double dbm, uint32_t base,
                                          LRx &out) {
  const uint32_t s = t.phy;
  if (D.chan[j] != D.chan[s]) return false;  // other channels get nothing (yans-wifi-channel.cc:88-91)
  const double dist = distance3(D.x[s], D.y[s], D.z[s], D.x[j], D.y[j], D.z[j]);
  const uint64_t at = t.ts + (uint64_t)seconds_to_ts(dist / D.speed);  // ConstantSpeed delay (propagation-delay-model.cc:90-96)
  double dBm;
  if constexpr (LX) dBm = calc_rx_power_x(D.lx->m, D.lx->n, D.lx->tb, dbm, s, (uint32_t)j, D.z[s], D.z[j], dist) + D.rx_gain_db;
  else dBm = calc_rx_power(D.loss, dbm, dist) + D.rx_gain_db;              // StartReceivePacket: rxPowerDbm += RxGain
  const double w = pow(10.0, dBm / 10.0) / 1000.0;                         // DbmToW (yans-wifi-phy.cc:727-732)
  out = LRx{at, base + D.chan_rank[j] - (j > (int64_t)s ? 1u : 0u), k, w, t.dur};  // the receiver loop's Schedule order
  return true;
}
// The SendPackets one host closure made since the last epoch, applied by the next epoch launch (more than
// NSEND: the earlier ones by k_wl_send launches).
constexpr uint32_t NSEND = 8;
struct SendBatch {
  uint32_t n, k0;  // SendPackets; the first one's transmission index (they are k0 .. k0 + n - 1)
  LTx t[NSEND];
  double dbm[NSEND];
  uint32_t base[NSEND];
};

// EndReceive's order key against another pending EndReceive of the same phy (ts, then uid; a uid of the
// running epoch is above every known one, and those order by their syncing Receives' keys).
__device__ __forceinline__ bool pe_before(const LPe &a, const LPe &b) {
  if (a.ts != b.ts) return a.ts < b.ts;
  const bool ka = a.euid != NONE, kb = b.euid != NONE;
  if (ka != kb) return ka;
  if (ka) return a.euid < b.euid;
  return a.sts != b.sts ? a.sts < b.sts : a.suid < b.suid;
}

__device__ __forceinline__ WMir mir_of(const LPhy &P) { return WMir{P.endTx, P.endRx, P.endCca, P.rxing, 0, P.endSw}; }
__device__ __forceinline__ void mir_put(const WDev &D, int64_t j, const WMir &m0, const LPhy &P) {
  if (P.endTx != m0.endTx || P.endRx != m0.endRx || P.endCca != m0.endCca || P.rxing != m0.rxing) {
    const WMir m{P.endTx, P.endRx, P.endCca, P.rxing, 0, 0};
    __builtin_memcpy(&D.mir[j], &m, WMIR_HEAD);  // (an epoch never changes endSw)
  }
}

#ifdef NSGPU_PHASE_PROF
// diagnostic build: k_wl_stepw's waves, recorded without atomics for WREC_E epochs from epoch g_wtarget on (the
// epoch counter g_wepoch counts k_wl_prof_epoch launches): per wave (start, loads done, loop done, end)
// s_memtime stamps and its events
constexpr uint32_t WREC_E = 8, WREC_P = 16384;
__device__ unsigned long long g_wrec[WREC_E][WREC_P][5];
__device__ uint32_t g_wepoch, g_wtarget;
#endif
// ---- the epoch with one wave per phy ----
// One phy's events of the epoch: every pending Receive / EndReceive with a key below (bts, buid), each the
// reference's own code path — YansWifiPhy::EndReceive (yans-wifi-phy.cc:770-799) with
// InterferenceHelper::CalculateSnrPer (interference-helper.cc:336-353), and YansWifiChannel::Receive ->
// YansWifiPhy::StartReceivePacket (yans-wifi-phy.cc:399-496) with InterferenceHelper::AppendEvent
// (interference-helper.cc:192-212) and GetEnergyDuration (:171-190).  A phy's time goes into its NiChanges
// ring: a start inserted while receiving shifts every pending end (100-300 entries at 10^4 phys), and the
// cursor and the CCA energy walk read the ring entry by entry.  So the 64 lanes of a wave serve ONE phy: the
// ring is read 64 entries a trip, an insertion shifts 64 entries a trip, and the sums whose order matters
// (the cursor's prefix, the energy walk, CalculatePer's walk) run over the loaded entries lane by lane with
// readlane — no memory trip, and the reference's order of additions (bit-exact).  Every decision is
// wave-uniform; lane 0 makes the stores of uniform values.
__device__ __forceinline__ uint32_t lead_run(uint64_t bm) { return ~bm ? (uint32_t)__builtin_ctzll(~bm) : 64u; }
__device__ __forceinline__ int64_t rl_i64(int64_t v, int u) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, u);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), u);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double rl_d(double v, int u) { return __longlong_as_double(rl_i64(__double_as_longlong(v), u)); }
__device__ __forceinline__ uint32_t rl_u32(uint32_t v, int u) { return (uint32_t)__builtin_amdgcn_readlane((int)v, u); }

__device__ __forceinline__ LPe rl_pe(const LPe &a, int u) {
  LPe b;
  b.ts = (uint64_t)rl_i64((int64_t)a.ts, u);
  b.sts = (uint64_t)rl_i64((int64_t)a.sts, u);
  b.suid = rl_u32(a.suid, u);
  b.euid = rl_u32(a.euid, u);
  b.tx = rl_u32(a.tx, u);
  b.can = rl_u32(a.can, u);
  b.sslot = rl_u32(a.sslot, u);
  b.used = rl_u32(a.used, u);
  b.w = rl_d(a.w, u);
  return b;
}
template <bool LE>
__device__ __forceinline__ void w_cursor_advance(const LNi *ring, uint32_t head, uint32_t len, uint32_t m, int64_t lim,
                                                 uint32_t &cur_n, double &cur_s) {
  const uint32_t lane = threadIdx.x & 63;
  while (cur_n < len) {
    const uint32_t idx = cur_n + lane;
    LNi e{0, 0.0};
    bool in = false;
    if (idx < len) {
      e = ring[(head + idx) & m];
      in = LE ? e.t <= lim : e.t < lim;
    }
    const uint32_t k = lead_run(__ballot(in));  // (sorted: the entries up to lim are the chunk's head)
    for (uint32_t u = 0; u < k; u++) cur_s += rl_d(e.d, (int)u);
    cur_n += k;
    if (k < 64) return;
  }
}
// AddNiChangeEvent (interference-helper.cc:378-383) at upper_bound (t): the entries after it move up one
// place, 64 a trip from the tail.
__device__ __forceinline__ void w_ni_insert(LNi *ring, uint32_t head, uint32_t &len, uint32_t m, int64_t t, double d) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t q = len;
  while (q > 0) {
    const uint32_t c0 = q > 64 ? q - 64 : 0, n = q - c0;
    LNi e{0, 0.0};
    bool gt = false;
    if (lane < n) {
      e = ring[(head + c0 + lane) & m];
      gt = e.t > t;
    }
    const uint32_t k = (uint32_t)__popcll(__ballot(gt));  // (sorted: the entries after t are the chunk's tail)
    if (gt) ring[(head + c0 + lane + 1) & m] = e;
    q -= k;
    if (k < n) break;
  }
  if (lane == 0) ring[(head + q) & m] = LNi{t, d};
  len++;
}

// The epoch kernel's per-wave staging (r05): the ring of NiChanges in LDS (RL entries; a longer ring stays
// in HBM), the Receive queue in the wave's registers (64 entries; more: HBM, 64 a trip), and the epoch's
// appends — dispatched events, end records, syncs — staged in LDS and claimed with one atomic per list
// per wave (the r04 kernel waited one atomic round trip per event).  A staged sync's slot is LOCAL | index
// until the claim; the staged events, end records and pending records that name it are patched then.
constexpr uint32_t RL = 256;
constexpr uint32_t RSPEC = 32, QSPEC = 4;  // ring / queue entries loaded with the state (speculatively)
constexpr uint32_t EVB = 64, ENB = 8, SYB = 8;
constexpr uint32_t NTB = 32;  // staged notes (k_wl_stepw<true, *>; a phy's notes leave the wave in its own order)
constexpr uint32_t LOCAL = 0x80000000u;
struct LEnd {  // a staged end record
  nsgpu_wifil_end rec;
  LEck eck;
  uint32_t sl, pad;
};
__device__ __forceinline__ LRx rl_rx(const LRx &a, int u) {
  return LRx{(uint64_t)rl_i64((int64_t)a.at, u), rl_u32(a.uid, u), rl_u32(a.tx, u), rl_d(a.w, u), rl_i64(a.dur, u)};
}
__device__ __forceinline__ LRx shfl_up_rx(const LRx &a) {
  LRx b;
  b.at = prev_lane64(a.at);  // (lane 0's is not used)
  b.uid = prev_lane32(a.uid);
  b.tx = prev_lane32(a.tx);
  b.w = __longlong_as_double((long long)prev_lane64((uint64_t)__double_as_longlong(a.w)));
  b.dur = (int64_t)prev_lane64((uint64_t)a.dur);
  return b;
}

// One epoch of every phy, a wave each: first the SendPackets the last host closure made (nsgpu_wifil_send
// batches up to NSEND of them into this launch: the sender's switch and this phy's Receive of each, what
// k_wl_send does — they precede every event of the epoch), then every pending Receive / EndReceive with a
// key below (bts, buid), in (ts, uid) order.  NOTE: the instantiation launched while some phy notifies
// (nsgpu_wifil_notify) — a notifying phy's wave stages one nsgpu_wifil_note per Receive; <false> holds none of it.
// SW: the instantiation launched once some phy has switched channels (nsgpu_wifil_set_channel) — GetState's
// SWITCHING rank, StartReceivePacket's SWITCHING branch (yans-wifi-phy.cc:419-436) and SendPacket's
// !IsStateSwitching () (:508); <*, false> holds none of it and leaves the state's switching tail alone.
template <bool NOTE, bool SW>
__global__ __launch_bounds__(64) void k_wl_stepw(const WDev D, uint64_t bts, uint32_t buid, const SendBatch sb) {
  const int64_t j = D.j0 + blockIdx.x;
  const uint32_t lane = threadIdx.x;
  if (j >= D.j0 + D.nown) return;
#ifdef NSGPU_PHASE_PROF
  const uint64_t pt0 = __builtin_amdgcn_s_memtime();
  uint64_t pt1 = pt0, pt2 = pt0;
  uint32_t pev = 0;
#endif
  __shared__ LNi s_ring[RL];
  __shared__ LEv s_ev[EVB];
  __shared__ LEnd s_end[ENB];
  __shared__ LSync s_sy[SYB];
  __shared__ nsgpu_wifil_note s_nt[NOTE ? NTB : 1];  // (<false> never names it: no LDS there)
  bool noting = false;
  if constexpr (NOTE) noting = D.note_on[j] != 0;
  LPhy P;
  if constexpr (SW) P = D.ps[j];
  else __builtin_memcpy(&P, &D.ps[j], LPHY_HEAD), P.endSw = P.startSw = 0, P.switches = P.drop_switching = 0;
  // (issued with the state: the ring's first RSPEC entries and the queue's first QSPEC at their compact places
  // — a fast epoch leaves them there, head 0 — used when the state says they are the ones; the first trip moves
  // ~1 KB a wave, 10^4 waves at once)
  const LNi rg = lane < RSPEC && lane <= D.ni_mask ? D.ni[(uint64_t)j * (D.ni_mask + 1) + lane] : LNi{0, 0.0};
  const LRx q8 = lane < QSPEC && lane <= D.rq_mask ? D.rq[(uint64_t)j * (D.rq_mask + 1) + lane] : LRx{};
  const WMir m0 = mir_of(P);
  LNi *const gring = D.ni + (uint64_t)j * (D.ni_mask + 1);
  LRx *rq = D.rq + (uint64_t)j * (D.rq_mask + 1);
  LPe *pe = D.pe + (uint64_t)j * LPE_CAP;
  const uint32_t gm = D.ni_mask, ctx = D.node[j];
  uint32_t *const evc = D.evc + (uint32_t)(j % EV_STRIPES) * EV_STRIDE;
  LEv *const evs = D.ev + (uint64_t)(j % EV_STRIPES) * D.ev_scap;
  uint32_t err = 0;
  // the pending EndReceive records: lane q < LPE_CAP holds record q for the whole epoch (written back at the
  // end when changed)
  LPe mine{};
  if (lane < (uint32_t)LPE_CAP) mine = pe[lane];
  bool pe_dirty = false, changed = false;
  // ---- the batched SendPackets: lane i computes this phy's Receive of send i (YansWifiChannel::Send)
  LRx my{};
  bool ok = false;
  if (lane < sb.n) {  // (computed by k_wl_rx when the closure sent: off the epoch's critical path)
    my = D.rxb[(uint64_t)lane * D.nphy + j];
    ok = my.at != ~0ull;
  }
  const uint64_t okm = __ballot(ok);
  const uint32_t nins = (uint32_t)__popcll(okm);
#pragma unroll
  for (uint32_t i = 0; i < NSEND; i++) {  // the sender's switch (YansWifiPhy::SendPacket, yans-wifi-phy.cc:499-522)
    if (i >= sb.n) break;
    if (sb.t[i].phy != (uint32_t)j) continue;
    const LTx &t = sb.t[i];
    changed = true;
    if (P.endTx > (int64_t)t.ts) {  // NS_ASSERT (!IsStateTx ()); SwitchToTx from TX: NS_FATAL_ERROR (:285-287)
      err |= WE_TX_IN_TX;
      continue;
    }
    if (SW && P.endSw > (int64_t)t.ts) {  // NS_ASSERT (... && !m_state->IsStateSwitching ()) (:508)
      err |= WE_TX_IN_SWITCHING;
      continue;
    }
    if (P.rxing) {  // m_endRxEvent.Cancel (); NotifyRxEnd (); SwitchToTx's RX case (:263-268)
      if (lane == P.live) mine.can = 1;
      pe_dirty = true;
      P.live = NONE;
      P.rxing = 0;
      P.endRx = (int64_t)t.ts;
    }
    P.endTx = (int64_t)t.ts + t.dur;
  }
  // ---- the Receive queue and the ring: registers and LDS when they fit
  const bool fast = P.rq_len + nins <= 64 && P.len + 2 * (P.rq_len + nins) + 2 <= RL;
  uint32_t rq0 = ~0u;  // (queue offset of the loaded chunk; ~0: none)
  LRx rqc{};
  uint32_t qn = 0;     // (fast: entries in rqc)
  if (nins) changed = true;
  if (fast) {
    rq0 = 0;
    qn = P.rq_len;
    const bool qc = (P.rq_head & D.rq_mask) == 0 && qn <= QSPEC, h0 = (P.head & gm) == 0;
    if (lane < qn) rqc = qc ? q8 : rq[(P.rq_head + lane) & D.rq_mask];
#pragma unroll
    for (uint32_t u = 0; u < RL / 64; u++) {
      const uint32_t i = u * 64 + lane;
      if (i < P.len) s_ring[(P.head + i) & (RL - 1)] = h0 && i < RSPEC ? rg : gring[(P.head + i) & gm];
    }
    for (uint32_t i = 0; i < sb.n; i++) {  // (sorted by (arrival, uid): an insertion in registers)
      if (!((okm >> i) & 1ull)) continue;
      if (qn > D.rq_mask) {  // (k_wl_send's capacity check)
        err |= WE_RQCAP;
        continue;
      }
      const LRx e = rl_rx(my, (int)i);
      const bool lt = lane < qn && (rqc.at < e.at || (rqc.at == e.at && rqc.uid < e.uid));
      const uint32_t pos = (uint32_t)__popcll(__ballot(lt));
      const LRx up = shfl_up_rx(rqc);
      if (lane > pos && lane <= qn) rqc = up;
      if (lane == pos) rqc = e;
      qn++;
    }
    P.rq_len = qn;
    __syncthreads();
  } else if (nins) {  // (k_wl_send's insertion into the HBM queue, in send order)
    for (uint32_t i = 0; i < sb.n; i++) {
      if (!((okm >> i) & 1ull)) continue;
      const LRx e = rl_rx(my, (int)i);
      if (P.rq_len > D.rq_mask) {
        err |= WE_RQCAP;
        continue;
      }
      if (lane == 0) {
        uint32_t q = P.rq_len;
        while (q > 0) {
          const LRx x = rq[(P.rq_head + q - 1) & D.rq_mask];
          if (x.at < e.at || (x.at == e.at && x.uid < e.uid)) break;
          rq[(P.rq_head + q) & D.rq_mask] = x;
          q--;
        }
        rq[(P.rq_head + q) & D.rq_mask] = e;
      }
      P.rq_len++;
    }
    __syncthreads();
  }
  LNi *const ring = fast ? s_ring : gring;
  const uint32_t m = fast ? RL - 1 : gm;
#ifdef NSGPU_PHASE_PROF
  pt1 = __builtin_amdgcn_s_memtime();
#endif
  // ---- staged appends
  uint32_t ns = 0, ne = 0, nv = 0, nn = 0;
  bool slotted = false;  // (the phy's own event slots are written: further events go to the stripes)
  auto flush = [&]() {  // claim the staged syncs, end records and events (one atomic each), patch, store
    __syncthreads();
    uint32_t bs = 0, be = 0, bv = 0;
    if (lane == 0) {
      if (ns) bs = atomicAdd(&D.cnt[1], ns);
      if (ne) be = atomicAdd(&D.cnt[2], ne);
      if (nv && slotted) bv = atomicAdd(evc, nv);
    }
    bs = rl_u32(bs, 0);
    be = rl_u32(be, 0);
    bv = rl_u32(bv, 0);
    const auto fix = [&](uint32_t sl) { return sl != NONE && (sl & LOCAL) ? bs + (sl & ~LOCAL) : sl; };
    if (ns) {
      if ((uint64_t)bs + ns > D.sync_cap) err |= WE_CAP;
      else if (lane < ns) D.sync[bs + lane] = s_sy[lane];
      if (lane < (uint32_t)LPE_CAP) mine.sslot = fix(mine.sslot);
    }
    if (ne) {
      if ((uint64_t)be + ne > D.end_cap) {
        err |= WE_CAP;
      } else if (lane < ne) {
        const LEnd x = s_end[lane];
        D.ends[be + lane] = x.rec;
        D.end_sslot[be + lane] = fix(x.sl);
        D.eck[be + lane] = x.eck;
      }
    }
    if (nv && !slotted) {  // the epoch's first EVB events: the phy's own slots (a count, no claim)
      if (lane < nv) {
        LEv v = s_ev[lane];
        v.sslot = fix(v.sslot);
        D.evp[(uint64_t)j * EVB + lane] = v;
      }
      if (lane == 0) {
        D.evn[j] = nv;
        atomicAdd(&D.evt[(uint32_t)(j % EV_STRIPES) * EV_STRIDE], nv);  // (its result unused: no wait)
      }
      slotted = true;
    } else if (nv) {  // (more: the stripes, claimed)
      if ((uint64_t)bv + nv > D.ev_scap) {
        err |= WE_CAP;
      } else if (lane < nv) {
        LEv v = s_ev[lane];
        v.sslot = fix(v.sslot);
        evs[bv + lane] = v;
      }
    }
    if constexpr (NOTE) {
      if (nn) {  // (wave-uniform) the staged notes' places: one atomic, then a lane a note
        uint32_t bn = 0;
        if (lane == 0) bn = atomicAdd(&D.cnt[5], nn);
        bn = rl_u32(bn, 0);
        if ((uint64_t)bn + nn > D.note_cap) err |= WE_NOTECAP;
        else if (lane < nn) D.notes[bn + lane] = s_nt[lane];
        nn = 0;
      }
    }
    ns = ne = nv = 0;
    __syncthreads();
  };
  uint32_t rqn = 0;  // Receives taken this epoch
  bool ring_dirty = false;
  for (;;) {
    // the next pending EndReceive (the selection reads the records lane by lane)
    const uint64_t used = __ballot(lane < (uint32_t)LPE_CAP && mine.used);
    int e = -1;
    LPe eb{};
    for (int q = 0; q < LPE_CAP; q++) {
      if (!((used >> q) & 1ull)) continue;
      const LPe c = rl_pe(mine, q);
      if (e < 0 || pe_before(c, eb)) e = q, eb = c;
    }
    const bool hr = P.rq_len > 0;
    LRx r{};
    if (hr) {
      if (rq0 == ~0u || rqn - rq0 >= 64) {  // (HBM queue: the next 64 queued Receives, one trip)
        rq0 = rqn;
        rqc = lane < P.rq_len ? rq[(P.rq_head + lane) & D.rq_mask] : LRx{};
      }
      r = rl_rx(rqc, (int)(rqn - rq0));
    }
    bool take_r;
    if (hr && e >= 0) take_r = r.at < eb.ts || (r.at == eb.ts && (eb.euid == NONE || r.uid < eb.euid));
    else if (hr) take_r = true;
    else if (e >= 0) take_r = false;
    else break;
    if (take_r) {
      if (!(r.at < bts || (r.at == bts && r.uid < buid))) break;
    } else {
      if (!(eb.ts < bts || (eb.ts == bts && eb.euid != NONE && eb.euid < buid))) break;
    }
    changed = true;
#ifdef NSGPU_PHASE_PROF
    pev++;
#endif
    if (!take_r) {  // ---- YansWifiPhy::EndReceive (yans-wifi-phy.cc:770-799)
      const int64_t nw = (int64_t)eb.ts;
      nsgpu_wifil_end rec{eb.ts, eb.euid, (uint32_t)j, 0.0, 0.0, eb.tx, eb.can ? (uint32_t)NSGPU_WIFI_END_CANCELLED : 0u,
                          eb.can ? 0.0 : eb.w};
      LEck eck{0, NONE, 0.0};
      P.c.end++;
      if (eb.can) {  // EventImpl::Invoke skips a cancelled event (event-impl.cc:40-46); still dispatched
        P.c.end_cancelled++;
      } else {
        // InterferenceHelper::CalculateSnrPer (interference-helper.cc:336-353): ni = (start, m_firstPower), the
        // list after the event's own start entry (the ring's head: no fold while receiving) up to its end
        // entry, (end, 0) — CalculateNoiseInterferenceW (:229-243) — then CalculatePer's walk (:257-334).  The
        // walk's sequential part (the noise sums, the chunk bounds) runs here, 64 ring entries a trip, then
        // lane by lane; the chunks' error-rate models (~10 pow / erfc calls each, ~100-200 chunks an
        // EndReceive) run lane-parallel in k_wl_mid, which multiplies them in this order.  A zero-length
        // chunk is 1.0 (CalculateChunkSuccessRate) and is not recorded.
        const LTx t = D.tx[eb.tx];
        const Mode pm = make_mode(t.mc, t.rate, t.bw);
        const double noise0 = P.firstPower;
        rec.snr = snr_of(D, eb.w, noise0, pm);
        const int64_t t0 = (int64_t)eb.sts;
        const int64_t hdrStart = t0 + (int64_t)preamble_us(t.mc, pm.bw, t.preamble) * 1000;
        const int64_t payStart = hdrStart + (int64_t)header_us(t.mc, pm.bw, t.preamble) * 1000;
        const uint32_t need = 2 * P.len + 2;
        uint32_t cs = 0;
        if (lane == 0) cs = atomicAdd(&D.cnt[4], need);
        cs = rl_u32(cs, 0);
        const bool defer = (uint64_t)cs + need <= D.ck_cap;
        if (!defer) err |= WE_CKCAP;  // (the run fails: no inline fallback here)
        // the walk, 64 ring entries a batch, a lane per step: step k's (previous, current) interval gives its
        // chunks (CalculatePer's cases, interference-helper.cc:270-330); only the noise before each step — a
        // running double sum, whose order is the reference's — is formed lane by lane
        uint32_t cn = 0;
        double noiseW = noise0;
        int64_t previous = t0;
        for (uint32_t q0 = 1, last = 0; !last; q0 += 64) {
          const uint32_t q = q0 + lane;
          LNi c{0, 0.0};
          if (q < P.len) c = ring[(P.head + q) & m];
          const uint64_t em = __ballot(q < P.len && c.t == nw && eb.w == -c.d);  // (the event's end entry)
          const uint32_t nin = P.len > q0 ? (P.len - q0 < 64 ? P.len - q0 : 64) : 0;
          uint32_t nstep = 64, close = 64;  // steps of the batch; the lane of the closing (nw, 0) step
          if (em) {
            nstep = (uint32_t)__builtin_ctzll(em) + 1, close = nstep - 1, last = 1;
          } else if (nin < 64) {
            nstep = nin + 1, close = nin, last = 1;  // (the list ends: the closing step after it)
          }
          const int64_t cur = lane == close ? nw : c.t;
          const double dl = lane == close ? 0.0 : c.d;
          int64_t prv = (int64_t)prev_lane64((uint64_t)cur);
          if (lane == 0) prv = previous;
          double nz = 0.0;  // the noise before step `lane`
          double acc = noiseW;
          for (uint32_t k = 0; k < nstep; k++) {
            if (lane == k) nz = acc;
            acc += rl_d(dl, (int)k);
          }
          int64_t d1 = 0, d2 = 0;
          bool h1 = false;
          if (lane < nstep) {
            if (prv >= payStart) {
              d1 = cur - prv;
            } else if (prv >= hdrStart) {
              h1 = true;
              if (cur >= payStart) d1 = payStart - prv, d2 = cur - payStart;
              else d1 = cur - prv;
            } else if (cur >= payStart) {
              h1 = true;
              d1 = payStart - hdrStart, d2 = cur - payStart;
            } else if (cur >= hdrStart) {
              h1 = true;
              d1 = cur - hdrStart;
            }
          }
          // (a zero-length chunk is skipped: ck (dur != 0)); the chunks' places by a wave prefix count
          const uint32_t n1 = d1 != 0, n2 = d2 != 0, nc = n1 + n2;
          const uint32_t pre = wave_incscan32(nc);
          const uint32_t tot = rl_u32(pre, 63), at = cn + pre - nc;
          if (defer) {
            if (n1) D.ck[cs + at] = LCk{nz, (int64_t)((uint64_t)d1 << 1) | (h1 ? 1 : 0)};
            if (n2) D.ck[cs + at + n1] = LCk{nz, (int64_t)((uint64_t)d2 << 1)};
            cn += tot;
          }
          previous = rl_i64(cur, (int)(nstep - 1));
          noiseW = acc;
        }
        eck = LEck{cs, defer ? cn : NONE, eb.w};
        rec.per = 0.0;  // (k_wl_mid writes the product)
        P.rxing = 0;  // NotifyRxEnd (); SwitchFromRxEndOk / Error -> DoSwitchFromRx (wifi-phy-state-helper.cc:391-402)
      }
      if (ne == ENB || nv == EVB) flush();
      const uint32_t sl = eb.euid == NONE ? rl_u32(mine.sslot, e) : NONE;  // (after a flush: its patched slot)
      if (lane == 0) {
        s_end[ne] = LEnd{rec, eck, sl, 0};
        s_ev[nv] = LEv{eb.ts, eb.euid, ctx, sl, 0};
      }
      ne++;
      nv++;
      if (lane == (uint32_t)e) mine.used = 0;
      pe_dirty = true;
      if (P.live == (uint32_t)e) P.live = NONE;
      continue;
    }
    // ---- YansWifiChannel::Receive -> YansWifiPhy::StartReceivePacket (yans-wifi-phy.cc:399-496)
    P.rq_head++;
    P.rq_len--;
    rqn++;
    const int64_t nw = (int64_t)r.at;
    const int64_t endNew = nw + r.dur;
    if (P.len + 2 > gm + 1) {
      err |= WE_NICAP;
      break;
    }
    ring_dirty = true;
    // InterferenceHelper::AppendEvent (interference-helper.cc:192-212)
    if (!P.rxing) {  // fold the entries up to upper_bound (now) into m_firstPower; the new entry first
      w_cursor_advance<true>(ring, P.head, P.len, m, nw, P.cur_n, P.cur_s);
      P.head = (P.head + P.cur_n) & m;
      P.len -= P.cur_n;
      P.cur_n = 0;
      P.head = (P.head - 1) & m;
      if (lane == 0) ring[P.head] = LNi{nw, r.w};
      P.len++;
      P.firstPower = P.cur_s;
    } else {
      w_ni_insert(ring, P.head, P.len, m, nw, r.w);
    }
    w_ni_insert(ring, P.head, P.len, m, endNew, -r.w);
    P.ni_max = P.len > P.ni_max ? P.len : P.ni_max;
    // GetState (wifi-phy-state-helper.cc:159-183): TX, RX, SWITCHING, CCA_BUSY, IDLE
    const int st = P.endTx > nw ? 2 : P.rxing ? 1 : SW && P.endSw > nw ? 4 : P.endCca > nw ? 3 : 0;
    static_assert(NSGPU_WIFIL_IDLE == 0 && NSGPU_WIFIL_RX == 1 && NSGPU_WIFIL_TX == 2 && NSGPU_WIFIL_CCA_BUSY == 3, "st");
    static_assert(NSGPU_WIFIL_SWITCHING == 4 && NSGPU_WIFIL_NOTE_DROP_SWITCHING == 4, "st");
    uint32_t nkind = NSGPU_WIFIL_NOTE_DROP_ED;  // (NOTE) the branch taken, and SwitchMaybeToCcaBusy's argument
    int64_t ncca = 0;
    bool maybe = false;
    P.c.rx++;
    if (SW && st == 4) {  // drop (:419-436); noise after the switch when it outlasts m_endSwitching
      P.drop_switching++;
      nkind = NSGPU_WIFIL_NOTE_DROP_SWITCHING;
      maybe = endNew > nw + (P.endSw - nw);  // GetDelayUntilIdle: m_endSwitching - now (> 0 here)
    } else if (st == 1 || st == 2) {  // drop; noise after the current Rx / Tx (:431-457)
      if (st == 1) P.c.drop_rx++;
      else P.c.drop_tx++;
      nkind = st == 1 ? NSGPU_WIFIL_NOTE_DROP_RX : NSGPU_WIFIL_NOTE_DROP_TX;
      int64_t until = (st == 1 ? P.endRx : P.endTx) - nw;  // GetDelayUntilIdle (:122-151)
      until = until > 0 ? until : 0;
      maybe = endNew > nw + until;
    } else if (r.w > D.edW) {  // sync (:461-472): SwitchToRx, NotifyRxStart, Schedule (rxDuration, EndReceive)
      const uint64_t fr = __ballot(lane < (uint32_t)LPE_CAP && !mine.used);  // (the first free record)
      const int q = fr ? __builtin_ctzll(fr) : -1;
      if (q < 0) {
        err |= WE_PECAP;
        break;
      }
      if (ns == SYB) flush();
      if (lane == 0) s_sy[ns] = LSync{r.at, r.uid, NONE, (uint32_t)(j * LPE_CAP + q), 0};
      const LPe np{(uint64_t)endNew, r.at, r.uid, NONE, r.tx, 0, LOCAL | ns, 1, r.w};
      ns++;
      if (lane == (uint32_t)q) mine = np;
      pe_dirty = true;
      P.live = (uint32_t)q;
      P.rxing = 1;
      P.endRx = endNew;
      P.c.sync++;
      nkind = NSGPU_WIFIL_NOTE_SYNC;
    } else {
      P.c.drop_ed++;
      maybe = true;
    }
    if (maybe) {  // maybeCcaBusy (:485-495): GetEnergyDuration (interference-helper.cc:171-190)
      w_cursor_advance<false>(ring, P.head, P.len, m, nw, P.cur_n, P.cur_s);
      double noise = P.cur_s;
      int64_t end = nw;
      bool stop = false;
      for (uint32_t q0 = P.cur_n; q0 < P.len && !stop; q0 += 64) {  // (64 entries a trip; the sums one at a time)
        const LNi en = q0 + lane < P.len ? ring[(P.head + q0 + lane) & m] : LNi{0, 0.0};
        const uint32_t n = P.len - q0 < 64 ? P.len - q0 : 64;
        for (uint32_t u = 0; u < n; u++) {
          noise += rl_d(en.d, (int)u);
          end = rl_i64(en.t, (int)u);
          if (noise < D.ccaW) {
            stop = true;
            break;
          }
        }
      }
      const int64_t cca = end > nw ? end - nw : 0;
      if (cca != 0) {  // SwitchMaybeToCcaBusy (wifi-phy-state-helper.cc:404-423)
        P.endCca = P.endCca > nw + cca ? P.endCca : nw + cca;
        P.c.cca_switches++;
        ncca = cca;
      }
    }
    if constexpr (NOTE) {
      if (noting) {
        if (nn == NTB) flush();
        if (lane == 0)
          s_nt[nn] = nsgpu_wifil_note{r.at, r.uid, (uint32_t)j, r.tx, nkind, (uint32_t)st, 0,
                                      nkind == NSGPU_WIFIL_NOTE_SYNC ? r.dur : 0, ncca};
        nn++;
      }
    }
    if (nv == EVB) flush();
    if (lane == 0) s_ev[nv] = LEv{r.at, r.uid, ctx, NONE, 0};
    nv++;
  }
#ifdef NSGPU_PHASE_PROF
  pt2 = __builtin_amdgcn_s_memtime();
#endif
  if (ns | ne | nv | nn) flush();
  // ---- write-backs: the pending records, the queue's rest (fast, after insertions), the ring (fast), the state
  if (pe_dirty && lane < (uint32_t)LPE_CAP) pe[lane] = mine;
  if (fast && (nins || rqn)) {  // (the queue's rest at its compact place: head 0)
    if (lane >= rqn && lane < qn) rq[lane - rqn] = rqc;
    P.rq_head = 0;
  }
  if (fast && ring_dirty) {  // (the ring at its compact place: head 0)
#pragma unroll
    for (uint32_t u = 0; u < RL / 64; u++) {
      const uint32_t i = u * 64 + lane;
      if (i < P.len) gring[i] = s_ring[(P.head + i) & (RL - 1)];
    }
    P.head = 0;
  }
  if (lane == 0) {
    if (changed) {
      if constexpr (SW) D.ps[j] = P;
      else __builtin_memcpy(&D.ps[j], &P, LPHY_HEAD);
    }
    mir_put(D, j, m0, P);
    if (err) atomicOr(&D.cnt[3], err);
  }
#ifdef NSGPU_PHASE_PROF
  const uint32_t we = g_wepoch - g_wtarget;
  if (lane == 0 && we < WREC_E && j < (int64_t)WREC_P) {
    unsigned long long *w = g_wrec[we][j];
    w[0] = pt0;
    w[1] = pt1;
    w[2] = pt2;
    w[3] = __builtin_amdgcn_s_memtime();
    w[4] = pev;
  }
#endif
}

#ifdef NSGPU_PHASE_PROF
__global__ void k_wl_prof_epoch() { g_wepoch++; }  // (one thread: the wave records' epoch counter)
#endif

// CalculatePer's chunk product for the epoch's deferred EndReceives (interference-helper.cc:257-334): one
// block per end record, a thread per chunk (CalculateChunkSuccessRate with the error-rate model, every
// chunk's model evaluated at once), then the product in walk order by one thread from LDS (its order is
// the reference's: a float product is not reassociated).
constexpr uint32_t PER_SEG = 4096;  // chunks a block holds in LDS at once (32 KB)
__device__ __forceinline__ void wl_per(const WDev &D, uint32_t bx, uint32_t nbx, double *s_c) {
  const uint32_t nend = D.cnt[2] < D.end_cap ? D.cnt[2] : (uint32_t)D.end_cap;
  for (uint32_t ei = bx; ei < nend; ei += nbx) {  // (block-uniform)
    const LEck k = D.eck[ei];
    if (k.n == NONE) continue;
    const LTx t = D.tx[D.ends[ei].tx];
    const Mode pm = make_mode(t.mc, t.rate, t.bw), hm = header_mode(pm, t.preamble);
    double psr = 1.0;
    for (uint32_t b = 0; b < k.n; b += PER_SEG) {
      const uint32_t mm = k.n - b < PER_SEG ? k.n - b : PER_SEG;
      for (uint32_t u = threadIdx.x; u < mm; u += 256) {
        const LCk x = D.ck[k.start + b + u];
        const int64_t dur = x.dm >> 1;
        s_c[u] = (x.dm & 1) ? chunk(D, snr_of(D, k.w, x.noise, hm), dur, hm) : chunk(D, snr_of(D, k.w, x.noise, pm), dur, pm);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
#pragma unroll 16
        for (uint32_t i = 0; i < mm; i++) psr *= s_c[i];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) D.ends[ei].per = 1 - psr;
  }
}

// The epoch's syncs in dispatch order (ts, uid of the syncing Receive): EndReceive uid = uid0 + rank.  A
// partition ranks its own syncs among every partition's (D.xsync: keys are unique, so the order of the gather
// does not matter).
__device__ __forceinline__ void wl_sync_rank(const WDev &D, uint32_t uid0, uint32_t bx, uint32_t nbx) {
  const uint32_t n = D.cnt[1] < D.sync_cap ? D.cnt[1] : (uint32_t)D.sync_cap;
  const LSync *const X = D.xsync ? D.xsync : D.sync;
  const uint32_t nx = D.xsync ? D.xn : n;
  for (uint32_t i = bx * 256 + threadIdx.x; i < n; i += nbx * 256) {
    const LSync a = D.sync[i];
    uint32_t r = 0;
    for (uint32_t k = 0; k < nx; k++) {
      const LSync b = X[k];
      r += b.sts < a.sts || (b.sts == a.sts && b.suid < a.suid);
    }
    D.sync[i].euid = uid0 + r;
  }
}
// The epoch's first tail kernel: the deferred PER products (blocks 0 .. MID_PER-1) and the syncs' ranks
// (the rest) — independent, one launch.
constexpr uint32_t MID_PER = 128, MID_RANK = 64;

// The epoch's close, on the critical path: k_wl_mid's last block (wl_fin) — the EndReceive uids (the sync
// order's) into the epoch's end records and its syncs' pending records, the status block (counters, the
// first END_STAGE end records) straight into the host's mapped copy (no copy).
// The epoch's order, behind it on a second stream (nothing the PHY or the host closures do depends on it;
// only the digest and the log):
//   k_wl_gather: the events from the phys' own slots (and the stripes' overflow) into one dense array, the
//     EndReceive uids resolved;
//   k_wl_tsort: a block per tile of TS keys (ts, uid << 32 | dense index) sorts it in LDS (bitonic);
//   k_wl_rank: an event's rank = its place in its tile + its lower bound in every other tile (each tile read
//     once into LDS, the searches in LDS), then its digest term and (logging) its rank; the block that
//     finishes last writes the running digest sum into the host's mapped copy and zeroes the epoch's
//     counters for the epoch two on.
// The status blocks, event lists, syncs and counters are kept per epoch parity; an epoch's k_wl_stepw waits
// for the order of the epoch two back (their last reader), which had a whole epoch to finish.  Epochs above
// ERANK_MAX events are ordered by the host from the dense events.  (The r04 all-pairs count, k_wl_order, was
// quadratic — 384 us at 6.5 x 10^4 events — and on the critical path.)
constexpr uint32_t TS = 2048, TS_T = 1024;  // keys a tile; threads a block (two keys each)
constexpr uint32_t ERANK_MAX = 65536, NTILE = ERANK_MAX / TS;
__device__ __forceinline__ bool key_lt(const ulonglong2 &a, const ulonglong2 &b) {
  return a.x < b.x || (a.x == b.x && a.y < b.y);
}
struct StripeMap {  // dense index -> stripe slot (the stripes' prefix in LDS)
  uint32_t pre[EV_STRIPES + 1];
};
__device__ __forceinline__ uint32_t load_stripes(const WDev &D, StripeMap &sm) {
  if (threadIdx.x < (uint32_t)EV_STRIPES) {
    const uint32_t c = D.evc[threadIdx.x * EV_STRIDE];
    sm.pre[threadIdx.x + 1] = c < D.ev_scap ? c : (uint32_t)D.ev_scap;
  }
  if (threadIdx.x == 0) sm.pre[0] = 0;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k <= EV_STRIPES; k++) sm.pre[k] += sm.pre[k - 1];  // (64 adds, LDS)
  __syncthreads();
  return sm.pre[EV_STRIPES];
}
__device__ __forceinline__ uint64_t stripe_slot(const WDev &D, const StripeMap &sm, uint32_t i) {
  uint32_t lo = 0, hi = EV_STRIPES;  // pre[lo] <= i < pre[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sm.pre[mid] <= i) lo = mid;
    else hi = mid;
  }
  return (uint64_t)lo * D.ev_scap + (i - sm.pre[lo]);
}
__device__ __forceinline__ LEv resolved(const WDev &D, const StripeMap &sm, uint32_t k) {
  LEv e = D.ev[stripe_slot(D, sm, k)];
  if (e.sslot != NONE) e.uid = D.sync[e.sslot].euid;
  return e;
}
// The epoch's close (k_wl_mid's last block): the EndReceive uids (the sync order's) into the end records and
// the syncs' pending records, the status block straight into the host's mapped copy.
__device__ __forceinline__ void wl_fin(const WDev &D, uint8_t *hst, uint32_t seq) {
  __shared__ StripeMap sm;
  __shared__ uint32_t s_nt;
  const uint32_t tid = threadIdx.x;
  if (tid < 64) {  // the events in the phys' own slots (their striped total), then the stripes' overflow
    const uint32_t c = (uint32_t)wave_sum64(D.evt[tid * EV_STRIDE]);  // (wave 0, every lane)
    if (tid == 0) s_nt = c;
  }
  const uint32_t nev = load_stripes(D, sm) + s_nt;  // (load_stripes's barriers order s_nt)
  const uint32_t nend = D.cnt[2] < D.end_cap ? D.cnt[2] : (uint32_t)D.end_cap;
  const uint32_t nsync = D.cnt[1] < D.sync_cap ? D.cnt[1] : (uint32_t)D.sync_cap;
  for (uint32_t i = tid; i < nend; i += 256) {  // the end records' EndReceive uids
    const uint32_t sl = D.end_sslot[i];
    if (sl != NONE) D.ends[i].uid = D.sync[sl].euid;
  }
  for (uint32_t i = tid; i < nsync; i += 256) {  // (a record taken again this epoch: a later sync's)
    const LSync y = D.sync[i];
    LPe &p = D.pe[y.loc];
    if (p.used && p.euid == NONE && p.sslot == i) p.euid = y.euid;
  }
  __syncthreads();
  nsgpu_wifil_end *he = reinterpret_cast<nsgpu_wifil_end *>(hst + STAT_HDR);
  for (uint32_t i = tid; i < nend && i < END_STAGE; i += 256) he[i] = D.ends[i];
  uint32_t *hc = reinterpret_cast<uint32_t *>(hst);
  if (tid == 0) {
    hc[0] = nev;
    hc[1] = D.cnt[1];
    hc[2] = D.cnt[2];
    hc[3] = D.cnt[3];
    hc[5] = D.cnt[5];
    D.cnt[0] = nev;
  }
  __threadfence_system();  // (the block's writes to the host's copy land before the epoch's flag)
  __syncthreads();
  if (tid == 0) __hip_atomic_store(&hc[6], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The epoch's tail kernel: the deferred PER products (blocks 0 .. MID_PER-1), the syncs' ranks (the rest),
// then — the block that finishes last — the epoch's close (wl_fin).
__global__ __launch_bounds__(256) void k_wl_mid(const WDev D, uint32_t uid0, uint8_t *hst, uint32_t seq) {
  __shared__ double s_c[PER_SEG];
  __shared__ uint32_t s_last;
  if (blockIdx.x < MID_PER) wl_per(D, blockIdx.x, MID_PER, s_c);
  else wl_sync_rank(D, uid0, blockIdx.x - MID_PER, MID_RANK);
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    s_last = atomicAdd(D.mticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  wl_fin(D, hst, seq);
  if (threadIdx.x == 0) atomicExch(D.mticket, 0u);
}
// The epoch's events into one dense array, uids resolved (off the critical path): a block of 256 phys claims
// its slots' events' places with one atomic (the dense order is the claims' order: the ranks do not depend
// on it — keys are unique — and erank / evd agree), block 0 also the stripes' overflow events.
__global__ __launch_bounds__(256) void k_wl_gather(const WDev D) {
  __shared__ StripeMap sm;
  __shared__ uint32_t s_wt[4], s_base, s_sbase;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t nstr = blockIdx.x == 0 ? load_stripes(D, sm) : 0u;
  const uint64_t j = (uint64_t)D.j0 + (uint64_t)blockIdx.x * 256 + tid;
  const uint32_t n = j < (uint64_t)(D.j0 + D.nown) ? D.evn[j] : 0u;
  if (n) D.evn[j] = 0;  // (for the epoch two on, which reuses this parity)
  const uint32_t x = wave_incscan32(n);
  if (lane == 63) s_wt[wv] = x;
  __syncthreads();
  uint32_t off = x - n, tot = 0;
  for (uint32_t w = 0; w < 4; w++) {
    off += w < wv ? s_wt[w] : 0u;
    tot += s_wt[w];
  }
  if (tid == 0) {
    s_base = tot ? atomicAdd(D.gtot, tot) : 0u;
    s_sbase = nstr ? atomicAdd(D.gtot, nstr) : 0u;
  }
  __syncthreads();
  for (uint32_t u = 0; u < n; u++) {
    LEv e = D.evp[j * EVB + u];
    if (e.sslot != NONE) e.uid = D.sync[e.sslot].euid;
    D.evd[s_base + off + u] = e;
  }
  for (uint32_t k = tid; k < nstr; k += 256) D.evd[s_sbase + k] = resolved(D, sm, k);
}
__global__ __launch_bounds__(TS_T) void k_wl_tsort(const WDev D) {
  __shared__ ulonglong2 s_t[TS];
  const uint32_t tid = threadIdx.x;
  const uint32_t nev = D.cnt[0];
  if (blockIdx.x == 0 && tid == 0) *D.gtot = 0;  // (k_wl_gather is done with its claims)
  if (nev > ERANK_MAX) return;  // (the host orders it from the dense events)
  const uint32_t base = blockIdx.x * TS;
  if (base >= nev) return;  // (block-uniform)
  LEv e[2];
#pragma unroll
  for (uint32_t u = 0; u < 2; u++) {  // (both loads in flight)
    const uint32_t k = base + u * TS_T + tid;
    e[u] = k < nev ? D.evd[k] : LEv{~0ull, NONE, 0, NONE, 0};
  }
#pragma unroll
  for (uint32_t u = 0; u < 2; u++) {
    const uint32_t k = base + u * TS_T + tid;
    s_t[u * TS_T + tid] = k < nev ? make_ulonglong2(e[u].ts, (uint64_t)e[u].uid << 32 | k) : make_ulonglong2(~0ull, ~0ull);
  }
  __syncthreads();
  for (uint32_t kk = 2; kk <= TS; kk <<= 1) {  // bitonic: TS_T compare-exchanges a stage
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      const uint32_t i = 2 * j * (tid / j) + (tid % j), l = i + j;
      const ulonglong2 a = s_t[i], b = s_t[l];
      if (key_lt(b, a) == ((i & kk) == 0)) {
        s_t[i] = b;
        s_t[l] = a;
      }
      __syncthreads();
    }
  }
  const uint32_t n = nev - base < TS ? nev - base : TS;
  for (uint32_t i = tid; i < n; i += TS_T) D.evg[base + i] = s_t[i];
}
__global__ __launch_bounds__(TS_T) void k_wl_rank(const WDev D, uint64_t K0, int keep, unsigned long long *hdig) {
  __shared__ ulonglong2 s_o[TS];
  __shared__ unsigned long long s_dg[TS_T / 64];
  __shared__ uint32_t s_last;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t nev = D.cnt[0];
  const uint32_t nt = (nev + TS - 1) / TS;
  uint64_t dg = 0;
  if (nev <= ERANK_MAX && blockIdx.x < nt) {  // (block-uniform)
    const uint32_t t = blockIdx.x, n = nev - t * TS < TS ? nev - t * TS : TS;
    ulonglong2 x[2];
    uint32_t r[2];
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
      const uint32_t p = u * TS_T + tid;
      x[u] = p < n ? D.evg[t * TS + p] : make_ulonglong2(~0ull, ~0ull);
      r[u] = p;  // (its place in its own tile)
    }
    for (uint32_t t2 = 0; t2 < nt; t2++) {
      if (t2 == t) continue;
      const uint32_t n2 = nev - t2 * TS < TS ? nev - t2 * TS : TS;
#pragma unroll
      for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = u * TS_T + tid;
        if (p < n2) s_o[p] = D.evg[t2 * TS + p];
      }
      __syncthreads();
#pragma unroll
      for (uint32_t u = 0; u < 2; u++) {  // lower bound: the tile's keys below x
        uint32_t lo = 0, c = n2;
        while (c > 0) {
          const uint32_t h = c >> 1;
          if (key_lt(s_o[lo + h], x[u])) lo += h + 1, c -= h + 1;
          else c = h;
        }
        r[u] += lo;
      }
      __syncthreads();
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
      if (u * TS_T + tid >= n) break;
      dg += digest_term(K0 + r[u], x[u].x, (uint32_t)(x[u].y >> 32));
      if (keep) D.erank[(uint32_t)x[u].y] = r[u];
    }
  }
  dg = wave_sum64(dg);
  if (lane == 0) s_dg[wv] = dg;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0;
    for (uint32_t w = 0; w < TS_T / 64; w++) t += s_dg[w];
    if (t) atomicAdd(D.edig, t);
    __threadfence();
    s_last = atomicAdd(D.ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // the last block: the running digest sum for the host; this parity's counters zeroed for the epoch two on
  // (the order is their last reader; that epoch's k_wl_stepw waits for this kernel)
  __threadfence();
  if (tid == 0) {
    *hdig = atomicAdd(D.edig, 0ull);
    atomicExch(D.ticket, 0u);
  }
  if (tid < 3 || tid == 4 || tid == 5) D.cnt[tid] = 0;  // (events, syncs, ends; the chunk pool; the notes)
  if (tid < (uint32_t)EV_STRIPES) D.evc[tid * EV_STRIDE] = 0, D.evt[tid * EV_STRIDE] = 0;
}

// What k_wl_rank's last block zeroes, without the order: a partition's own lists once gathered (partitions'
// epochs are ordered over every partition's gathered events)
__global__ void k_wl_zero(const WDev D) {
  const uint32_t tid = threadIdx.x;
  if (tid < 3 || tid == 4 || tid == 5) D.cnt[tid] = 0;
  if (tid < (uint32_t)EV_STRIPES) D.evc[tid * EV_STRIDE] = 0, D.evt[tid * EV_STRIDE] = 0;
  if (tid == 6 && D.gtot) *D.gtot = 0;
}
__global__ void k_wl_set(uint32_t *p, uint32_t v) { *p = v; }

// SendPacket of phy s at (ts): the sender's state switch (thread s) and one Receive per receiver.
template <bool LX>
__global__ __launch_bounds__(256) void k_wl_send(const WDev D, uint32_t k, LTx t, double dbm, uint32_t base) {
  const int64_t j = D.j0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) D.tx[k] = t;  // (every partition holds every transmission)
  if (j >= D.j0 + D.nown) return;
  const uint32_t s = t.phy;
  if ((uint32_t)j == s) {  // YansWifiPhy::SendPacket (yans-wifi-phy.cc:499-522)
    LPhy &P = D.ps[j];
    if (P.endTx > (int64_t)t.ts) {  // NS_ASSERT (!IsStateTx ()); SwitchToTx from TX: NS_FATAL_ERROR (:285-287)
      atomicOr(&D.cnt[3], WE_TX_IN_TX);
      return;
    }
    if (P.endSw > (int64_t)t.ts) {  // NS_ASSERT (... && !m_state->IsStateSwitching ()) (:508)
      atomicOr(&D.cnt[3], WE_TX_IN_SWITCHING);
      return;
    }
    if (P.rxing) {  // m_endRxEvent.Cancel (); NotifyRxEnd (); SwitchToTx's RX case (:263-268)
      D.pe[(uint64_t)j * LPE_CAP + P.live].can = 1;
      P.live = NONE;
      P.rxing = 0;
      P.endRx = (int64_t)t.ts;
    }
    P.endTx = (int64_t)t.ts + t.dur;
    D.mir[j] = mir_of(P);  // (the host applied the same switch to its copy; a partition's mirror is gathered)
    return;
  }
  LRx e;
  if (!reception<LX>(D, j, t, k, dbm, base, e)) return;
  const uint64_t at = e.at;
  const uint32_t uid = e.uid;
  LPhy &P = D.ps[j];
  LRx *rq = D.rq + (uint64_t)j * (D.rq_mask + 1);
  if (P.rq_len > D.rq_mask) {
    atomicOr(&D.cnt[3], WE_RQCAP);
    return;
  }
  uint32_t q = P.rq_len;  // sorted by (arrival, uid)
  while (q > 0) {
    const LRx e = rq[(P.rq_head + q - 1) & D.rq_mask];
    if (e.at < at || (e.at == at && e.uid < uid)) break;
    rq[(P.rq_head + q) & D.rq_mask] = e;
    q--;
  }
  rq[(P.rq_head + q) & D.rq_mask] = e;
  P.rq_len++;
}

// The Receives of one SendPacket (YansWifiChannel::Send's loop), computed when the closure sends — while the
// host goes on — into the batch's row of D.rxb; the next epoch's k_wl_stepw queues them.  Thread 0 records
// the transmission.
template <bool LX>
__global__ __launch_bounds__(256) void k_wl_rx(const WDev D, LRx *row, LTx t, uint32_t k, double dbm, uint32_t base) {
  const int64_t j = D.j0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) D.tx[k] = t;
  if (j >= D.j0 + D.nown) return;
  LRx e{};
  if (j == (int64_t)t.phy || !reception<LX>(D, j, t, k, dbm, base, e)) e.at = ~0ull;
  row[j] = e;
}

// The position reads of one SendPacket of phy s at `now` (YansWifiChannel::Send, yans-wifi-channel.cc:84-96: per
// receiver GetDelay / CalcRxPower -> MobilityModel::GetDistanceFrom, mobility-model.cc:78-84, reads the receiver's
// position and the sender's): every phy of the sender's channel number other than the sender updates, and the
// sender when there is at least one of them (upd_sender; its later updates of the same send have a zero delta);
// phys on other channels keep their m_lastUpdate.  One lane per phy, launched ahead of the send's k_wl_rx — whose
// every lane reads the sender's position, so the update is not made in place there — and only while some phy has
// a model: a run without one launches k_wl_rx alone, as before.
__global__ __launch_bounds__(256) void k_wl_move(const WDev D, uint32_t s, int64_t now, uint32_t upd_sender) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= D.nphy) return;
  if (j == (int64_t)s ? !upd_sender : D.chan[j] != D.chan[s]) return;
  move_update(D, j, now);
}
// Waypoints into the pool, in stream order: behind every kernel that may read the segment's old count, ahead of the
// k_wl_mop call that publishes the new one.
__global__ void k_wl_wput(nsgpu_waypoint *dst, WpChunk c, uint32_t n) {
  if (threadIdx.x < n) dst[threadIdx.x] = c.w[threadIdx.x];
}
// A host call on one phy's model (one thread, in stream order with the sends, as k_wl_set).  An install overwrites
// whatever record the phy had: one model per phy.
//   MOP_REMOVE        a constant position where the last update left the phy
//   MOP_SET_POSITION  the kind's SetPosition / DoSetPosition
//   MOP_VEL_INSTALL   ConstantVelocityHelper state (nsgpu_wifil_set_mobility); MOP_VEL_SET:
//                     ConstantVelocityMobilityModel::SetVelocity (constant-velocity-mobility-model.cc:43-50);
//                     MOP_VEL_PAUSE: Update + Pause / Unpause; MOP_VEL_GET: GetPosition + GetVelocity
//                     (constant-velocity-helper.cc:51-60, DoGetPosition's Update first)
//   MOP_WAY_INSTALL   a fresh model after AddWaypoint (a.w) and `cnt` more queued at D.wpool[off, off + cnt)
//                     (waypoint-mobility-model.cc:82-100: m_first = false, m_current = m_next = waypoint)
//   MOP_WAY_ADD       AddWaypoint: the first of a path (m_first) as above, else the slot cnt - 1 of the segment — now
//                     at `off` — is the new back of the queue
//   MOP_WAY_END       EndMobility (:203-209); Time (numeric_limits<uint64_t>::infinity ()) is Time (0)
//   MOP_WAY_GET       Update, then the members
//   MOP_ACC_INSTALL / MOP_ACC_SET (SetVelocityAndAcceleration, :70-78) / MOP_ACC_GET
enum MoveOp : uint32_t { MOP_REMOVE, MOP_SET_POSITION, MOP_VEL_INSTALL, MOP_VEL_SET, MOP_VEL_PAUSE, MOP_VEL_GET,
                         MOP_WAY_INSTALL, MOP_WAY_ADD, MOP_WAY_END, MOP_WAY_GET, MOP_ACC_INSTALL, MOP_ACC_SET, MOP_ACC_GET };
struct MoveArg {
  nsgpu_waypoint w;     // WAY_INSTALL / WAY_ADD: the waypoint; VEL_INSTALL / ACC_INSTALL / SET_POSITION: w.pos
  double v[3], a[3];    // VEL_INSTALL / VEL_SET: v; ACC_INSTALL / ACC_SET: both
  int64_t time;         // VEL_INSTALL: m_lastUpdate; ACC_INSTALL: m_baseTime
  uint32_t off, cnt;    // the waypoint segment's place and the slots written
  uint32_t paused, pad;  // VEL_INSTALL / VEL_PAUSE: m_paused
};
union MoveOut {
  nsgpu_mobility vel;
  nsgpu_waypoint_state way;
  nsgpu_accel acc;
};
__global__ void k_wl_mop(const WDev D, uint32_t op, uint32_t j, int64_t now, MoveArg a, MoveOut *out) {
  WMove &m = D.mov[j];
  double *const x = const_cast<double *>(D.x), *const y = const_cast<double *>(D.y), *const z = const_cast<double *>(D.z);
  switch (op) {
    case MOP_REMOVE:
      m = WMove{};
      break;
    case MOP_SET_POSITION:
      if (m.kind == MOVE_VEL) {  // m_position = position; m_velocity = Vector (0, 0, 0); m_lastUpdate = Now ()
        m.v[0] = m.v[1] = m.v[2] = 0.0;
        m.cur_t = now;
      } else if (m.kind == MOVE_WAY) {  // DoSetPosition (:181-201), m_initialPositionIsWaypoint false
        way_update(D, j, now);
        m.cur_t = now > m.next_t ? now : m.next_t;
        m.v[0] = m.v[1] = m.v[2] = 0.0;
      } else {  // DoSetPosition (constant-acceleration-mobility-model.cc:61-67)
        double v[3];
        acc_velocity(D, m, now, v);
        m.v[0] = v[0], m.v[1] = v[1], m.v[2] = v[2];
        m.cur_t = now;
        m.p[0] = a.w.pos[0], m.p[1] = a.w.pos[1], m.p[2] = a.w.pos[2];
      }
      x[j] = a.w.pos[0], y[j] = a.w.pos[1], z[j] = a.w.pos[2];
      break;
    case MOP_VEL_INSTALL:
      x[j] = a.w.pos[0], y[j] = a.w.pos[1], z[j] = a.w.pos[2];
      m = WMove{};
      m.kind = MOVE_VEL, m.flag = a.paused ? 1u : 0u;
      m.cur_t = a.time;
      m.v[0] = a.v[0], m.v[1] = a.v[1], m.v[2] = a.v[2];
      break;
    case MOP_VEL_SET:  // m_helper.Update (); m_helper.SetVelocity (speed); m_helper.Unpause ()
      vel_update(D, j, now);
      m.v[0] = a.v[0], m.v[1] = a.v[1], m.v[2] = a.v[2];
      m.cur_t = now;
      m.flag = 0;
      break;
    case MOP_VEL_PAUSE:
      vel_update(D, j, now);
      m.flag = a.paused ? 1u : 0u;
      break;
    case MOP_VEL_GET: {
      vel_update(D, j, now);
      const bool p = m.flag != 0;
      out->vel = nsgpu_mobility{{x[j], y[j], z[j]}, {p ? 0.0 : m.v[0], p ? 0.0 : m.v[1], p ? 0.0 : m.v[2]}, m.cur_t,
                                p ? 1u : 0u, 0};
      break;
    }
    case MOP_WAY_INSTALL:
      m = WMove{};
      m.kind = MOVE_WAY, m.flag = 1;
      [[fallthrough]];
    case MOP_WAY_ADD:
      m.off = a.off, m.cnt = a.cnt;
      if (m.flag) {  // :84-88
        m.flag = 0;
        m.cur_t = m.next_t = (int64_t)a.w.time;
        x[j] = m.p[0] = a.w.pos[0], y[j] = m.p[1] = a.w.pos[1], z[j] = m.p[2] = a.w.pos[2];
      }
      break;
    case MOP_WAY_END:
      m.head = m.cnt;  // m_waypoints.clear ()
      m.cur_t = m.next_t = 0;
      m.flag = 1;
      break;
    case MOP_WAY_GET: {
      way_update(D, j, now);
      nsgpu_waypoint_state &o = out->way;
      const bool ended = m.next_t == WAY_ENDED;
      o = nsgpu_waypoint_state{(uint64_t)m.cur_t, {x[j], y[j], z[j]}, ended ? 0ull : (uint64_t)m.next_t,
                               {m.p[0], m.p[1], m.p[2]}, {m.v[0], m.v[1], m.v[2]}, ended ? 1u : 0u, m.flag,
                               m.cnt - m.head, 0};
      break;
    }
    case MOP_ACC_INSTALL:
      m = WMove{};
      m.kind = MOVE_ACC;
      m.cur_t = a.time;
      for (int c = 0; c < 3; c++) m.p[c] = a.w.pos[c], m.v[c] = a.v[c], m.a[c] = a.a[c];
      break;
    case MOP_ACC_SET: {
      double p[3];
      acc_position(D, m, now, p);
      m.cur_t = now;
      for (int c = 0; c < 3; c++) m.p[c] = p[c], m.v[c] = a.v[c], m.a[c] = a.a[c];
      break;
    }
    default: {  // MOP_ACC_GET
      nsgpu_accel &o = out->acc;
      for (int c = 0; c < 3; c++) o.pos[c] = m.p[c], o.vel[c] = m.v[c], o.acc[c] = m.a[c];
      o.base_time = m.cur_t;
      acc_position(D, m, now, o.now_pos);
      acc_velocity(D, m, now, o.now_vel);
    }
  }
}

// YansWifiPhy::SetChannelNumber (nch) of phy j (yans-wifi-phy.cc:327-374), in two launches in stream order with the
// sends (the host has flushed the batch: every earlier send keeps the receivers of its own Now).
//
// k_wl_rechan repairs the receiver loop's order (YansWifiChannel::Send, yans-wifi-channel.cc:84-113: m_phyList order
// among the phys of one channel number) in place, one lane per phy: the phys after j on `old` lose one place, the
// phys after j on `nch` gain one, and j's new place is the number of `nch` phys before it — counted a wave at a
// time (ballot + popcount, one atomic per wave that holds any) into *nbefore, which k_wl_switch reads and clears.
// D.chan[j] still holds `old` here; no lane reads it for j.
__global__ __launch_bounds__(256) void k_wl_rechan(const WDev D, uint32_t j, uint32_t old, uint32_t nch, uint32_t *nbefore) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < D.nphy && i != (int64_t)j;
  const uint32_t c = in ? D.chan[i] : 0u;
  const uint64_t bm = __ballot(in && i < (int64_t)j && c == nch);
  if ((threadIdx.x & 63) == 0 && bm) atomicAdd(nbefore, (uint32_t)__popcll(bm));
  if (!in || i < (int64_t)j) return;
  uint32_t *const rank = const_cast<uint32_t *>(D.chan_rank);
  if (c == old) rank[i] -= 1;       // (old != nch: the host launches this kernel only then)
  else if (c == nch) rank[i] += 1;
}
// k_wl_switch (one thread, as k_wl_mop): the switch itself when `sw` (Now != 0) — m_endRxEvent.Cancel () in RX
// (:343-347: the pending EndReceive stays queued, marked cancelled, as SendPacket-while-RX leaves it),
// WifiPhyStateHelper::SwitchToChannelSwitching (wifi-phy-state-helper.cc:323-365: m_rxing = false, m_endRx = now from
// RX; m_endCcaBusy trimmed to now; m_startSwitching, m_endSwitching), InterferenceHelper::EraseEvents
// (interference-helper.cc:368-374: the ring emptied, m_firstPower = 0, m_rxing = false) — then m_channelNumber =
// nch and, when the number changed (`moved`), j's place on it.  Now == 0 (:330-336) is the assignment alone.
__global__ void k_wl_switch(const WDev D, uint32_t j, int64_t now, int64_t delay, uint32_t nch, uint32_t sw, uint32_t moved,
                            uint32_t *nbefore) {
  if (sw) {
    LPhy &P = D.ps[j];
    if (P.rxing) {
      D.pe[(uint64_t)j * LPE_CAP + P.live].can = 1;
      P.live = NONE;
      P.rxing = 0;
      P.endRx = now;
    }
    if (now < P.endCca) P.endCca = now;
    P.startSw = now;
    P.endSw = now + delay;
    P.len = P.cur_n = 0;
    P.cur_s = P.firstPower = 0.0;
    P.switches++;
    D.mir[j] = mir_of(P);  // (the host applied the same switch to its copy)
  }
  const_cast<uint32_t *>(D.chan)[j] = nch;
  if (moved) {
    const_cast<uint32_t *>(D.chan_rank)[j] = *nbefore;
    *nbefore = 0;
  }
}

// Pending device events and the smallest ts among them (Next / IsFinished).
__global__ __launch_bounds__(256) void k_wl_pending(const WDev D, unsigned long long *out) {
  const int64_t j = D.j0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= D.j0 + D.nown) return;
  const LPhy P = D.ps[j];
  uint64_t n = P.rq_len, mt = P.rq_len ? D.rq[(uint64_t)j * (D.rq_mask + 1) + (P.rq_head & D.rq_mask)].at : ~0ull;
  for (int q = 0; q < LPE_CAP; q++) {
    const LPe &p = D.pe[(uint64_t)j * LPE_CAP + q];
    if (p.used) n++, mt = p.ts < mt ? p.ts : mt;
  }
  if (n) {
    atomicAdd(&out[0], (unsigned long long)n);
    atomicMin(&out[1], (unsigned long long)mt);
  }
}

// The EndReceive hand-back (nsgpu_wifil_next_end): over the listened phys, the smallest key of a pending EndReceive
// that is not cancelled (its uid assigned: every epoch's close gives the syncs theirs), and the earliest time at
// which one not yet scheduled could fall — a pending Receive (queued, or a staged SendPacket's) strong enough to
// sync (rxPowerW > the ED threshold, yans-wifi-phy.cc:461) ends its EndReceive at arrival + duration (:466-471).
// One block; out: [0] ts, [1] uid | phy << 32 (~0: none), [2] the potential ts (~0: none).
__global__ __launch_bounds__(256) void k_wl_nextend(const WDev D, uint32_t nsend, unsigned long long *out) {
  __shared__ uint64_t s_ts[256], s_tp[256];
  __shared__ uint32_t s_uid[256], s_phy[256];
  const uint32_t tid = threadIdx.x;
  uint64_t bts = ~0ull, tp = ~0ull;
  uint32_t buid = NONE, bphy = NONE;
  for (uint32_t i = tid; i < D.nlis; i += 256) {
    const uint32_t j = D.lis[i];
    for (int q = 0; q < LPE_CAP; q++) {
      const LPe &p = D.pe[(uint64_t)j * LPE_CAP + q];
      if (p.used && !p.can && p.euid != NONE && (p.ts < bts || (p.ts == bts && p.euid < buid))) {
        bts = p.ts;
        buid = p.euid;
        bphy = j;
      }
    }
    const LPhy P = D.ps[j];
    const LRx *rq = D.rq + (uint64_t)j * (D.rq_mask + 1);
    for (uint32_t k = 0; k < P.rq_len; k++) {
      const LRx r = rq[(P.rq_head + k) & D.rq_mask];
      if (r.w > D.edW && r.at + (uint64_t)r.dur < tp) tp = r.at + (uint64_t)r.dur;
    }
    for (uint32_t k = 0; k < nsend; k++) {
      const LRx r = D.rxb[(uint64_t)k * D.nphy + j];
      if (r.at != ~0ull && r.w > D.edW && r.at + (uint64_t)r.dur < tp) tp = r.at + (uint64_t)r.dur;
    }
  }
  s_ts[tid] = bts, s_uid[tid] = buid, s_phy[tid] = bphy, s_tp[tid] = tp;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const uint32_t u = tid + o;
      if (s_ts[u] < s_ts[tid] || (s_ts[u] == s_ts[tid] && s_uid[u] < s_uid[tid]))
        s_ts[tid] = s_ts[u], s_uid[tid] = s_uid[u], s_phy[tid] = s_phy[u];
      if (s_tp[u] < s_tp[tid]) s_tp[tid] = s_tp[u];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = s_ts[0];
    out[1] = s_uid[0] == NONE ? ~0ull : ((unsigned long long)s_phy[0] << 32) | s_uid[0];
    out[2] = s_tp[0];
  }
}

// int64x64_t::Invert (int64x64-128.cc:119-134) with Divu (:70-92) and MulByInvert (:94-118), on the host.
u128 umul_by_invert(u128 a, u128 b) {
  const u128 ah = a >> 64, bh = b >> 64, al = a & (u128)~0ull, bl = b & (u128)~0ull;
  u128 mid = ah * bl + al * bh;
  mid >>= 64;
  return ah * bh + mid;
}
u128 invert(uint64_t v) {
  const u128 a = (u128)1 << 64;
  u128 quo = a / v, rem = a % v;  // Divu (a, v)
  u128 result = quo << 64;
  u128 div;
  if ((rem >> 64) == 0) rem <<= 64, div = v;
  else div = (u128)v >> 64;
  result += rem / div;
  const u128 tmp = umul_by_invert((u128)v << 64, result);  // int64x64_t (v, false).MulByInvert (result)
  if ((uint64_t)(tmp >> 64) != 1) result += 1;             // GetHigh () != 1
  return result;
}

}  // namespace
}  // namespace nsgpu
