// nsgpu_p2p_dev.h — GPU-resident point-to-point / DropTail / IPv4-forward / UDP subset (configs 2, 4): the device
// structs, the wave helpers and the model code every p2p kernel shares (included first by nsgpu_p2p.hip, whose one
// translation unit holds all of the subset's device code: this header, nsgpu_p2p_win.h, nsgpu_p2p_dist.h).
//
// Event semantics follow the reference code line by line (restated independently in
// oracle/nsref_p2p.cc, which is the parity checker):
//   setup      node-list.cc:124-131, node.cc:111-145,183-199, application.cc:87-95
//   OnOff      onoff-application.cc:132-252      PacketSink: no events
//   device     point-to-point-net-device.cc:206-269,304-346,462-518; point-to-point-channel.cc:82-103
//   queue      queue.cc:61-200, drop-tail-queue.cc:83-132
//   IPv4/UDP   ipv4-l3-protocol.cc:434-537,815-841 (static next-hop routes, TTL)
//
// Engines (MI355X).  The simulation advances in conservative windows: W_end = min over pending e of
// (ts_e + L(kind_e)), L = the smallest delay any child of that kind of handler can have, capped at
// the Simulator::Stop key; DefaultSimulatorImpl's uids make a child sort after every pending event
// with ts <= its own, so every pending event with key <= that bound is safe to dispatch.
//   * single GPU: nsgpu_p2p_win.h — k2_pa / k2_handle / k2_scan per window (in-place pool, hub blocks,
//     sorted runs for windows larger than WCAP), replayed from a hipGraph;
//   * partitioned (one rank per GPU, or a loopback group on one GPU): the same k2_pa / k2_handle over
//     each rank's nodes, then k_gtile / k_dfin2 (nsgpu_p2p_dist.h), with the X0 / X1 / X2 exchanges.
#pragma once
#include <hip/hip_ext.h>
#include <stddef.h>
#include "nsgpu_device.h"
#include "nsgpu_internal.h"
#include "nsgpu_loss_counter.h"
#include "nsgpu_p2p_span.h"
#include "nsgpu_ranvar.h"
#include "nsgpu_rng_stream.h"
#include "nsgpu_wave.h"

namespace nsgpu {

enum EvKind : uint32_t {
  K_NODE_START = 1,     // Node::Start (setup)
  K_DEV_START = 2,      // NetDevice::Start (setup, no-op: started by Node::Start)
  K_APPOBJ_START = 3,   // Application::Start (setup)
  K_APP_START = 4,      // Application::StartApplication
  K_APP_STOP = 5,       // Application::StopApplication
  K_START_SENDING = 6,  // OnOffApplication::StartSending   (gen in bits 8..31)
  K_STOP_SENDING = 7,   // OnOffApplication::StopSending    (gen)
  K_SEND = 8,           // OnOffApplication::SendPacket     (gen)
  K_TX_COMPLETE = 9,    // PointToPointNetDevice::TransmitComplete
  K_RECEIVE = 10,       // PointToPointNetDevice::Receive
  K_STOP = 11,          // Simulator::Stop
  K_FWD_UP = 12,        // Ipv4EndPoint::DoForwardUp -> UdpSocketImpl::ForwardUp -> PacketSink (zero-delay leaf)
  K_FWD_UP_Q = 13,      // DoForwardUp -> UdpEchoServer / UdpEchoClient::HandleRead (queued: it schedules)
  K_FWD_UP_D = 14,      // a PacketSink DoForwardUp queued like any event: its ts group is cut by a run chunk
  K_NKINDS = 15,
  // Ipv4L3Protocol::HandleFragmentsTimeout (gen, never 0); frag scenarios, extended handlers only.  It takes entry 0
  // of the per-kind tables, which no kind used, so that the tables and with them P2PDev keep their layout
  K_FRAG_TIMEOUT = 0
};

constexpr int WCAP = 4096;       // events per window
constexpr int TB = 256;          // threads per block, pool sweeps
constexpr int HB = 64;           // threads per block, per-slot kernels (spread over CUs)
constexpr int NHB = WCAP / HB;   // holder blocks of k2_handle
constexpr int RJ = 256;          // keys per rank tile column
constexpr int NJT = WCAP / RJ;   // rank tile columns
constexpr int RTR = 1;           // window keys (rows) per thread of a rank tile (4: same traffic, slower)
constexpr int NRT = WCAP / (HB * RTR);  // rank tile rows
constexpr int NRB = NRT * NJT;   // rank tile blocks (k2_handle)
// blocks of the pool sweep (grid-stride; r06: 1,024 measured slower on config 4 and on the dumbbell's 5 M-entry
// pool: per-block reductions; with 128-record slot blocks, 128 against 256 blocks: config 4 +1.4 %,
// ab/p2p_knobs2.log)
constexpr int GRID_POOL = 128;
// ... the single engine's, when the pool capacity is above 2^20 entries (config 5's 5 M-entry pool on one engine:
// 256 / 128 / 96 / 64 blocks 120.6 / 114.6 / 110.9 / 101.3 M ev/s, ab/p2p_pool_blocks.log; config 4 flat from 64
// to 128)
constexpr int GRID_POOL_BIG = 256;
constexpr int GRID_POOL_DIST = GRID_POOL;  // k2_pa<DIST>'s whole grid (slot, remote, chunk and pool blocks)
// k2_pa (single engine): last-window records per slot block (r06: 128 against 256, config 4 +0.7 %, k2_pa ~10.3 ->
// ~9.8 us; profiles/r06/ab/p2p_tail_replays_slot_lanes.log)
constexpr int PA_SLOT_LANES = 128;
constexpr int SCAN_THREADS = 1024;
constexpr int CH = 16;           // events of one node a handler thread sorts in LDS
constexpr int NSLOT = 7;         // per-node slot table entries
constexpr int NTAB = NSLOT + 1;  // words per node table record (count + slots)
constexpr int NWIN = 32;         // windows per graph replay
constexpr int NWIN_TAIL = 2;     // ... near the end of a run (drive; 2 / 4 / 8 / none: 160.4 / 159.9 / 160.3 / 159.5 M
                                 // ev/s on config 4, interleaved)
constexpr uint32_t NOCTX = 0xffffffffu;
constexpr uint32_t LOCALBIT = 0x80000000u;  // child record kind: run inside the window as a local record
// a Receive whose node another rank owns (partitioned engines; set by the device step from its record, so
// that k2_pa and k_dfin2 need no owner lookup per child; only K_RECEIVE kind words carry it: their upper bits
// hold no generation)
constexpr uint32_t REMOTEBIT = 0x40000000u;

// Packet descriptor: flow (sending app), IPv4 identification (Ipv4L3Protocol::m_identification of
// the originating node), size in bytes with the headers added so far, IPv4 TTL.
struct Pkt {
  uint32_t app, ipid, size, ttl;
};

// Per-device record of the transmit path: the tx state (busy, queue count / head), the static
// parameters a TransmitStart / TransmitComplete reads and the device's counters, in ONE 128-B line —
// a device step touches one line instead of eleven scattered SoA words (each a separate line fetch
// from another XCD's writes: measured 2.8 -> 1.6 MB HBM fetch per k2_handle launch on config 4).
struct DevRec {
  uint32_t busy, cnt, head, qmax;  // PointToPointNetDevice m_txMachineState, DropTail count / ring head, MaxPackets
  uint32_t peer, peer_node, rkind, em;  // rkind: the Receive child's kind word (K_RECEIVE | REMOTEBIT when another
  uint64_t bps;                          //   rank owns the peer's node); em: its enabled receive error model + 1 (0: none)
  int64_t ifg, delay;              // InterframeGap, channel Delay
  uint64_t pad2;
  nsgpu_dev_counters c;            // (copied out strided by nsgpu_p2p_results / _counters)
  uint64_t frag_dgrams, frag_sent;  // frag scenarios: datagrams this device's node fragmented on it, their fragments
  uint64_t pad3[2];
};
static_assert(sizeof(DevRec) == 128 && offsetof(DevRec, c) == 64, "DevRec is one 128-B line");

// Reduction of a pending set: the next window's bound (atomicMin), the pending Stop.
struct Red {
  uint64_t tmin, wend, stopts;
  uint32_t stopuid, pad;
  uint64_t wendw;  // the wide bound: min over pending of ts + lookw (cross-node lookahead; wide engines)
};

// A deferred window's dispatch bases: what df_sdef needs once the window's records are staged in rank order.
struct WInfo {
  uint64_t K0, tmin, ilim;  // dispatches before the window, its tmin and inline limit
  uint32_t uid0, N, W, Lt;  // the uid its first child takes; records (gen-0 W + local Lt)
};

// A staged record of a deferred window, at its rank: key (rel ts << 32 | its uid — resolved at staging when it
// was provisional; a local record's key has uid 0: its uid is its parent's child prefix + j, resolved by
// df_sdef), counts (children | inline children << 9 | the record's dense index << 18), and for a local record
// its parent (the parent's dense index | child index << 24), for a gen-0 record its first inline leaf (its
// context | child index << 24; a local record has none).  Its context is kept beside it (stx).  Stage arrays (and the child prefixes cpt) are indexed by stg_pos(rank): df_sdef's
// thread t owns the 8 consecutive ranks 8t..8t+7 and loads its q-th one from q * 1024 + t, so every load and
// store of a wave is coalesced.
struct Stg {
  uint64_t key;
  uint32_t cnt, par;
};
static_assert(sizeof(Stg) == 16, "Stg");
constexpr uint32_t STG_NT = 1024;  // df_sdef's threads (its rank slices)
// Provisional uids (deferred windows): child j of the record of rank r of window n, before window n's child
// prefix is known, is PROV | (n & 1) << 30 | r << 8 | j — above every resolved uid (< UID_DF_LIMIT, checked), so
// keys compare as the final uids do; resolved to uid0(n) + cpt[n & 1][r] + j.
constexpr uint32_t PROV = 0x80000000u, PROV_MAXC = 256, UID_DF_LIMIT = 0x3fe00000u;
// A window's children take at most NMAX x PROV_MAXC = 2^21 uids, so a deferred window that starts below
// UID_DF_SOFT ends below UID_DF_LIMIT; the window that reaches UID_DF_SOFT pauses the deferred pipeline
// (MODE_UIDX) and the scanning pipeline runs the rest of the run (df_usable is false from there on).
constexpr uint32_t UID_DF_SOFT = UID_DF_LIMIT - (1u << 22);
// DefaultSimulatorImpl's m_uid is a uint32 that wraps to 0 after 0xffffffff (default-simulator-impl.cc:52-56,
// 188-219); the wrapped uids would sort before every earlier one at equal ts and uid 2 would read as a
// ScheduleDestroy id.  The engines do not replicate that: a window whose children would take uid 0xffffffff
// or a wrapped one fails the run (error 2048) before any of them runs.  (0xffffffff itself is kept free: it is
// the "none" marker of several engine records.)
constexpr uint64_t UID_MAX_NEXT = nsgpu::UID_NEXT_MAX;
__device__ __forceinline__ uint32_t prov_uid(uint64_t win, uint32_t r, uint32_t j) {
  return PROV | ((uint32_t)(win & 1) << 30) | (r << 8) | j;
}

// Device-resident run control (one per engine).  Every field is written by one kernel of the
// window pipeline and read by later ones, never read and written by different blocks of one kernel
// except through atomics.  Window k: red[(k + 1) & 1] holds the pending set's reduction that bounds
// it; its leftovers and children fold into red[k & 1].
struct Ctl {
  Red red[2];
  uint64_t K;                          // dispatched so far (after the last scanned window)
  uint64_t tmin, bound, inline_lim;    // current window (k2_pa / the partitioned cut)
  uint64_t windows, max_window, last_ts, max_windows, refits;
  uint64_t digest, cancelled, ttl_drops, no_route, unreach, icmp;
  uint64_t pK0, ptmin, pinline_lim;    // the last scanned window, appended by the next k2_pa
  // (W, nxtP, overflow, prep): a partitioned rank's X0 payload, sent from here — its window candidates,
  // (unused), a hub too large for a block, the window is the cut of the last one
  uint32_t puid0, pW, uid, hdl;
  uint32_t W, nxtP, overflow, prep;  // (16-B aligned: the X0 payload)
  uint32_t done, stop_seen, pvalid, pinl;
  // ---- single-GPU engine (k2_*: in-place pool, sorted runs, hub blocks) ----
  uint64_t P_end, live, nfree;  // pool scan range, live pool entries, free-stack entries
  uint64_t r0, rW;              // sorted run: start of the next chunk, run length
  uint64_t split_lo, split_hi;  // run chunk: rel ts of a same-ts group cut at its start / end (~0: none)
  uint64_t wkmax;               // largest window key of the forming window (radix sort width)
  uint64_t npush, nF;           // this window: pool slots freed, children parked in the fresh buffer
  uint32_t mode, rt, nhub, wbase;  // engine mode, red[] accumulating index, hub nodes, chunk base
  uint32_t force_run, hcap;        // a hub too large to sort in a block: dispatch the window as a run;
                                   // the window is cut at the next host event (pause after it)
  uint64_t hts, hrel;              // next host event (nsgpu_p2p_advance): ts (~0: none); the rel ts of the
  uint32_t huid, gt_tinl;          //   window's last timestamp (W_end or the host event's); the host uid;
  uint32_t gt_lown, gt_pad;        //   k_gtile -> k_dfin2: the merged window's inline children, this rank's
                                   //   local records (from the X1 headers: k_dfin2's record blocks read none)
  uint64_t pchild;                 // children of the last scanned window that stay pending (not inline)
  // ---- wide windows (nsgpu_p2p_win.h; partitioned: k_gtile / k_dfin2): same-node TransmitCompletes run inside ----
  uint64_t lim_rel;   // a TransmitComplete child with rel ts < lim_rel is a local record of this window
  uint64_t nbound;    // the narrow bound of the forming window (an overflowing wide window is trimmed to it)
  uint64_t tn0;       // trace records before this window's handlers (the local records' uid patch)
  uint64_t span_t;    // adaptive span target of wide windows (kept between the narrow and the wide bound)
  uint32_t plt;       // local records of the last scanned window (lrec)
  uint32_t renarrow;  // the overflowing window is wide: trim its sorted run to nbound (host step)
  // ---- sorted runs: the chunk being dispatched ends at rnext; rtrim: the run ends after it (k_trim) ----
  uint64_t rnext;
  uint32_t rtrim, pad5;
  // ---- deferred dispatch accounting (single wide engine, nsgpu_p2p_win.h "deferred windows") ----
  uint64_t acc_tc, acc_tinl;  // this window's children / inline children (k2_handle accumulates; the deferred
                              // pipeline's k2_handle keeps them in its blocks' partial records instead: Part)
  uint32_t pdf;               // the window the next k2_pa appends is staged (1) or appended from sinfo (0)
  uint32_t sflag;             // k2_pa staged a window for df_sdef: 1 | (its window index & 3) << 1 (k2_pa writes
                              // it every window; df_sdef's blocks only read it)
  uint32_t rk_W, rk_go;       // k2_handle's snapshot for k2_rank (window size; it was handled, normally)
  uint64_t rk_win, rk_lim;    //   (its window index, lim_rel): k2_rank's bookkeeping block rewrites C.W etc.
  WInfo winfo[4];             // window n's dispatch bases (k2_rank's bookkeeping), at n & 3
  // ---- partitioned sorted runs (a window some rank cannot hold: every rank sorts its candidates once and the
  // run is dispatched in chunks cut at a common key; k_drun_*, k2_pa's chunk role, k_dfin2) ----
  uint32_t drun, drpad;       // a run is being dispatched (every rank alike)
  uint64_t dr0, drW, dr1;     // this rank's run: next entry, length (rn_* arrays); past the chunk being formed
  uint64_t drg;               // the next chunk's cut key (from the ranks' fitting and head keys, k_dfin2)
  uint64_t drlo;              // the next chunk continues the same-ts group the last one cut: its rel ts (~0: no)
  uint32_t drtrim, dtrim;     // the next chunk ends that group and the run after it; the run ended so: the next
                              // k2_pa returns this rank's entries left that are not in the pool to pending
  uint64_t drn_tmin, drn_wend;  // the pending set's reduction at the run's start, its own entries included (k2_pa
  uint64_t drn_stopts;          // folds it into every chunk's instead of sweeping the pool)
  uint32_t drn_stopuid, drpad2;
  uint64_t drb_tmin, drb_span, drb_bound, drb_stop, drb_nbound, drb_lim;  // the run window's bound (WinBound)
  uint64_t drn_wendw;  // (wide partitioned engines) the wide bound's part of drn_*
  uint64_t drcut;      // (wide partitioned engines) the run's candidates up to the narrow bound (k_drun_trim)
  // ---- hub windows of the narrow engines: the hub events' stateless node parts by their slots' threads ----
  uint32_t hub_rdy;    // holder blocks done with them (k2_pa zeroes it; the hub blocks wait for NHB)
  uint32_t hub_ser;    // some hub event's node part touches node state (its hub block runs those serially)
  // ---- the deferred pipeline's allocation word: the forming window's slots | its fresh-buffer entries << 32 (one
  // returned atomic a block where W and nF take one each; W and nF stay 0 while that pipeline runs) ----
  uint64_t wnf;
};

static_assert(offsetof(Ctl, prep) == offsetof(Ctl, W) + 12 && offsetof(Ctl, W) % 16 == 0, "the X0 payload");

// Per-block partials of the deferred pipeline's reductions (single wide engine): a block of k2_pa / a holder or
// hub block of k2_handle stores its minima and child totals here with plain stores, and k2_rank's bookkeeping
// block folds them into red[rt] and the window's totals (df_fold) — the blocks' same-line atomics all landed at
// the kernel's end and the kernel could not retire before they drained.  One record per 128-B line; empty
// ({~0, ~0, ~0, 0}: nothing published) between windows.  The two arrays (pa_part by k2_pa's block, hd_part by
// k2_handle's) lie behind the run control in its allocation: P2PDev takes no further pointer (see hub_slot).
struct Part {
  uint64_t tmin, wend, wendw;
  uint64_t tot;  // the block's children | inline children << 32 (k2_handle)
};
constexpr size_t PART_LINE = 128;
constexpr size_t CTL_PARTS_OFF = (sizeof(Ctl) + PART_LINE - 1) / PART_LINE * PART_LINE;
__host__ __device__ __forceinline__ Part *part_rec(Ctl *C, uint32_t i) {
  return reinterpret_cast<Part *>(reinterpret_cast<char *>(C) + CTL_PARTS_OFF + (size_t)i * PART_LINE);
}

// Device-resident model + engine state (all pointers are HBM).  Passed to the kernels by value.
// A window record's place in the dispatch order, for the wide windows' ranking (k2_rank): the chain of
// records from it up to its gen-0 ancestor (a local record is a same-node TransmitComplete run inside the
// window; its parent is the event whose TransmitStart made it).  A gen-0 record is a chain of length 0.
// Order (ts, uid): a local record's uid is its parent's child prefix + its child index, so among records of
// one ts the gen-0 ones come first (older uids), and local ones follow their parents' order, then j.
constexpr int LKD = 8;  // chain levels kept: a record and up to 7 local ancestors (create: Lx <= 8 tx_min)
struct LKey {
  uint32_t rel[LKD];  // rel[t]: rel ts of the chain's level-t record (level 0: this one)
  uint32_t uid;       // the gen-0 ancestor's uid (level `depth`)
  uint32_t depth;     // local records in the chain (0: a gen-0 record)
  uint32_t pad[2];
  uint8_t j[16];      // j[t]: the level-t local record's child index in its parent
};
static_assert(sizeof(LKey) == 64, "LKey: four 16-B loads");

// Node-part result of one hub event (k2_handle hub blocks, between the two passes).
struct HubEv {
  uint32_t op, dev;
  Pkt p;
  int64_t pdelay;      // trailing child (OnOffApplication::ScheduleNextTx after SendPacket)
  uint32_t pkind, pa;  // pkind == 0: none
  uint32_t n, seq;     // children and trace sink calls the node part made
  uint32_t cancelled, pad;  // pad: the node part's inline DoForwardUp children
  uint32_t ctx, xdrop;      // the event's context (its Schedule calls inherit it); NodeOut::xdrop
};

struct P2PDev {
  // scenario
  uint32_t n_nodes, n_devices, n_apps, n_dst, qcap, maxc;
  const uint32_t *dev_node;
  const uint32_t *route;  // dense [node][slot], or null: the compressed table below
  const uint32_t *route_def, *route_exc_slot, *route_exc_dev;
  const uint64_t *route_exc_off;
  const uint32_t *app_kind, *app_node, *app_dst_node, *app_dst_slot, *app_pkt_size, *app_max_bytes, *app_ttl;
  const int64_t *app_start, *app_stop;
  const uint64_t *app_rate;
  const double *app_on_s, *app_off_s;
  const uint32_t *app_count, *app_src_slot;  // UdpEchoClient MaxPackets, route slot of its own node
  const int64_t *app_interval;               // UdpEchoClient Interval
  const uint32_t *node_app_off, *node_app_list;  // CSR: apps of each node in AddApplication order
  const int32_t *sink_of_node;                    // PacketSink of each node (-1: none; EP_BY_FLOW: see ep_of_flow)
  uint32_t icmp;                                  // ICMP errors are generated (scenario icmp)
  int64_t lookahead[K_NKINDS];
  int64_t lookw[K_NKINDS];  // wide windows: the smallest delay of a child that does not run in the window
  uint32_t wide, frag;      // wide windows on; IPv4 fragmentation (scenario frag: the extended handlers)
  // model state
  DevRec *dev;  // per-device tx state + transmit parameters (one record per device)
  Pkt *q_buf;
  uint32_t *app_flags;    // bit0 started, bit1 sink active (endpoint bound), bit2 send live, bit3 start/stop live,
                          // bit4 a UdpServer's endpoint, bit5 its receive callback is cleared (stopped, still bound)
  uint32_t *app_send_gen, *app_ss_gen, *app_residual, *app_tot;
  uint32_t *node_ipid;    // Ipv4L3Protocol::m_identification per node
  uint64_t *app_last_start;
  nsgpu_app_counters *appc;
  // pending pool (double-buffered SoA)
  uint64_t *ev_ts[2];
  uint32_t *ev_uid[2], *ev_ctx[2], *ev_kind[2], *ev_a[2];
  Pkt *ev_pkt[2];
  uint64_t pool_cap;
  // the current window (WCAP slots): slot records (k2_pa) ...
  uint64_t *wkey;
  uint32_t *wctx, *wkind, *wa, *widx;
  Pkt *wpkt;
  // ... handler outputs: child counts and child records (slot * maxc + j, Schedule-call order) ...
  uint32_t *nchild, *ninl;
  uint64_t *ch_ts;
  uint32_t *ch_ctx, *ch_kind, *ch_a;
  Pkt *ch_pkt;
  // ... dispatch info per slot (k2_scan / k_dfin2), and the keys / contexts kept for the next k2_pa
  // (which rewrites wkey / wctx with the next window while it appends this one)
  uint4 *sinfo;
  uint64_t *pwkey;
  uint32_t *pwctx;
  uint32_t *wrank;  // rank accumulators of the current window (0 between windows)
  // per-node slot tables of the current window, one 32-B record per node: [0] the node's window
  // events (0 between windows), [1 .. NSLOT] their first slots (one line per node, not two)
  uint32_t *node_tab;
  // partitioned run (dist != 0): this engine owns the nodes n with owner[n] == rank
  uint32_t dist, rank, nranks, flowmon;  // flowmon: per-flow statistics on (scenario flowmon: the extended handlers)
  const uint32_t *owner;
  uint64_t *x0_send, *x0_recv;  // X0: 16 B per rank (x0_send points at the run control's X0 payload)
  uint64_t *xk_send, *xk_recv;  // the cut's exchange (host-driven): one rank's largest fitting key (16 B)
  uint8_t *x1_send, *x1_recv;   // X1: X1B bytes per rank (header, the rank's records in dispatch order: SEnt)
  uint8_t *x1_own;              // this rank's window lists, not exchanged: X1Ent x WCAP, then X1Loc x XLCAP
  uint8_t *x2_send, *x2_recv;   // X2: x2b bytes per peer
  uint32_t capx, ranvar;        // X2 records per peer per window (the run's largest cut between two ranks); ranvar:
                                // some OnOff has a random OnTime / OffTime (the extended handlers; was padding)
  uint64_t x2b;                 // X2 bytes per peer
  uint32_t *gacc;               // k_gtile's accumulators: 2 x NACC packed 64-bit words
  // run control / outputs
  uint32_t n_init;    // initial pending count (pool 0)
  uint32_t uid_init;  // m_uid after setup
  Ctl *C;
  uint32_t *error;  // non-zero = capacity exceeded (code)
  uint64_t *log_ts;
  uint32_t *log_uid, *log_ctx;
  uint64_t log_cap;
  // ascii/pcap trace sink calls (nsgpu_p2p_set_trace; null: tracing off), unordered
  nsgpu_trace_record *trace;
  uint64_t trace_cap;
  unsigned long long *trace_n;
  uint32_t trace_kinds, errm;  // nsgpu_trace_kind bits recorded (nsgpu_p2p_set_trace_kinds); some device has an
                               // enabled receive error model (the extended handlers)
  // ---- single-GPU engine (k2_*) ----
  uint64_t runcap;        // capacity of the window record arrays (a sorted run may hold the whole pool)
  uint32_t *wsrc;         // pool slot each window record came from (NOSRC: a child of the last window)
  uint64_t *f_ts;         // fresh buffer: children of the last window that stay pending (moved into
  uint32_t *f_uid, *f_ctx, *f_kind, *f_a;  // the pool by k2_handle's maintenance blocks)
  Pkt *f_pkt;
  uint64_t fcap;
  uint32_t *fstack;       // free pool slots (stack)
  uint32_t *hub_list;     // nodes with more than CH window events (hub blocks)
  struct HubEv *hx;       // hub blocks: per-slot node-part results
  uint64_t *hub_key;      // hub blocks: the hub's events in key order (NHUB x WCAP)
  uint32_t *hub_slot;     // (then WCAP more: hub_mark.  P2PDev is passed by value: one more pointer here made the
                          //  compiler copy the whole struct into scratch, 1.4 KB a lane, in k2_handle)
  uint64_t *s_key2;       // radix sort / compaction scratch
  uint32_t *s_val, *s_val2, *s_hist, *g_u32;
  Pkt *g_pkt;
  uint64_t *cmp_cnt;      // compaction: live entries written
  // ---- wide windows: local records (same-node TransmitCompletes run inside the window) ----
  uint32_t *wpar;         // local record: parent record | child index << 24
  uint32_t *lcnt;         // local records per region this window (one region per holder / hub block)
  uint32_t *lrec;         // the last scanned window's local records (dense list, C.plt of them)
  LKey *lkey;             // [LCAP] the local records' chains (k2_rank: the rare exact compare)
  ulonglong2 *lkw;        // [LCAP] their chain order packed into two words (lk_word, lk_word2)
  uint4 *ldat;            // [LMAX] the window's local records in dense order (k2_rank -> k2_scan): record,
                          // child counts (n | inline << 16), rel ts, parent (wpar)
  uint32_t *lrank;        // [LMAX] their rank accumulators (k2_rank; 0 between windows)
  // ---- deferred windows (wrank / lrank are then 2 x WTOT / 2 x LMAX: by window parity) ----
  struct Stg *stage;      // [NMAX] a window's records by stg_pos(rank) (k2_pa stages, df_sdef reads)
  uint32_t *stx;          // [NMAX] their contexts (stg_pos)
  uint2 *sleaf;           // [NMAX][maxc] their further inline leaves: (context, child index) (by rank, entry 0 unused)
  uint32_t *cpt;          // [2][NMAX] child prefix by rank (df_sdef): provisional uids resolve through it
  uint32_t *ldpd;         // [LMAX] the dense list's parents as dense indices | child index << 24 (k2_rank -> k2_pa)
  // ---- partitioned sorted runs: this rank's candidates of the run window, in key order (runcap each) ----
  uint64_t *rn_key;
  uint32_t *rn_ctx, *rn_kind, *rn_a, *rn_src;
  Pkt *rn_pkt;
};
// ---- cold paths ----
// The handlers' rare code (the application kinds, the Sends, ICMP, a missing route, trace records, ...) is not
// inlined into k2_handle: inlined, it kept about 130 fields of the by-value kernel argument live across the holders'
// event loop, and every pointer the hot path used came back through two v_readlane of a spilled SGPR.  The
// out-of-line functions do not take a reference to the kernel argument (that made the compiler copy it into
// scratch: see hub_slot); they read a device-resident copy of it, which lies in the run control's allocation behind
// the partial records, so that P2PDev takes no pointer to it.  The host writes the copy at create and again
// whenever it changes a field of its descriptor afterwards (nsgpu_p2p.hip: mdev_sync).
constexpr size_t CTL_MDEV_OFF = 128 * 1024;  // (past the partial records: nsgpu_p2p_win.h asserts it)
__device__ __forceinline__ const P2PDev *mdev_of(const Ctl *C) {
  return reinterpret_cast<const P2PDev *>(reinterpret_cast<const char *>(C) + CTL_MDEV_OFF);
}
// The copy as an out-of-line function reads it.  The pointer arrives in vector registers like every argument, but it is
// the same in every lane and the copy does not change while a kernel runs: made a scalar value in the constant address
// space, its fields are read with scalar loads through the scalar cache, as the kernel argument's are, not with a
// vector memory trip in front of every first use.
__device__ __forceinline__ const P2PDev &mdev_ref(const P2PDev *G) {
  typedef __attribute__((address_space(4))) const P2PDev CDev;
  const uint64_t v = reinterpret_cast<uint64_t>(G);
  // (the builtin returns int: each half goes through uint32_t, or a low half with bit 31 set would sign-extend)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  const uint64_t u = ((uint64_t)hi << 32) | (uint64_t)lo;
  return *(const P2PDev *)(CDev *)u;
}

// ---------------- wave / block helpers (the wave reductions, scans and DPP moves: nsgpu_wave.h) ----------------
// Block exclusive scan of one value per thread (NTH threads); *total = block sum.
template <int NTH>
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t *wsum, uint32_t *total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t ex = wave_exscan32(v, lane);
  if (lane == 63) wsum[wid] = ex + v;
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int w = 0; w < NTH / 64; w++) {
    const uint32_t s = wsum[w];
    off += w < wid ? s : 0;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return off + ex;
}

// ---------------- UDP ports (ports mode: nsgpu_p2p_scenario.app_port given) ----------------
// Ipv4EndPointDemux::Lookup for sockets bound to (Any, port) is static, so create resolves it: sink_of_node[n] stays
// the node's endpoint when every flow addressed to n targets the one endpoint n has (the path of a scenario without
// ports, no further load), EP_BY_FLOW sends a Receive to the per-flow table — the application of the flow's
// destination node bound to its remote port, or -1 — and -1 stays "none".  The table and the UdpServers' loss
// counters lie behind app_dst_slot and appc in their allocations: P2PDev takes no further pointer (see hub_slot).
constexpr int32_t EP_BY_FLOW = -2;
constexpr uint32_t AF_BOUND = 2u, AF_UDP_SERVER = 16u, AF_RX_CLEARED = 32u;
__device__ __forceinline__ int32_t ep_of_flow(const P2PDev &M, uint32_t fa) {
  return (int32_t)M.app_dst_slot[M.n_apps + fa];
}
__host__ __device__ __forceinline__ nsgpu_loss_counter *loss_counters(nsgpu_app_counters *appc, uint32_t n_apps) {
  return reinterpret_cast<nsgpu_loss_counter *>(appc + n_apps);
}
// UdpServer::HandleRead (udp-server.cc:149-187): the SeqTsHeader's sequence number (the descriptor's upper 24 ttl
// bits; 0 for a payload that carries none), NotifyReceived, m_received++.  Out of line: the handlers of a scenario
// without a UdpServer never reach it.
__device__ __noinline__ void udp_server_rx(nsgpu_loss_counter *lc, nsgpu_app_counters *ac, uint32_t size, uint32_t ttl) {
  nsgpu_loss_counter_notify(lc, ttl >> 8);
  lc->received++;
  ac->rx_packets++;
  ac->rx_bytes += size - 28;
}
// Ipv4EndPoint::DoForwardUp -> UdpSocketImpl::ForwardUp -> the endpoint's receive callback, for the endpoints
// whose HandleRead schedules nothing (PacketSink, UdpServer): sa = the endpoint's application, *pp the datagram.
// PORTS: the handler kernels are instantiated twice (k2_handle<.., PORTS>): what ports mode adds to an event — the
// per-flow endpoint, UdpClient, UdpServer — and what frag mode adds ("IPv4 fragmentation" below) is compiled into the
// second, extended set only, so an engine with neither runs the code it ran before they existed.
template <bool PORTS>
__device__ __forceinline__ void fwd_up_leaf(const P2PDev &M, uint32_t sa, const Pkt *pp) {
  const uint32_t f = M.app_flags[sa];
  if (!(f & AF_BOUND)) return;
  if (PORTS && (f & AF_UDP_SERVER)) {  // (a stopped UdpServer: the event is dispatched, nothing is counted)
    if (!(f & AF_RX_CLEARED)) udp_server_rx(loss_counters(M.appc, M.n_apps) + sa, M.appc + sa, pp->size, pp->ttl);
    return;
  }
  M.appc[sa].rx_packets++;
  M.appc[sa].rx_bytes += pp->size - 28;
}

// ---------------- IPv4 fragmentation and reassembly (frag scenarios: nsgpu_p2p_scenario.frag) ----------------
// Every device has MTU 1500 (the subset has no MTU field), so only the originating node fragments: a forwarder
// never re-fragments, and DoFragmentation's alreadyFragmented branch (ipv4-l3-protocol.cc:1139-1143,1166-1169) is
// unreachable.  A sender hands the device step the whole datagram (IPv4 length above FRAG_MTU) and the step sends
// its fragments one by one (send_fragments); a fragment's descriptor carries its offset and MF bit in the upper
// half of ipid (NSGPU_PKT_FRAG_*, nsgpu_types.h), and in a frag scenario every sender writes the 16-bit
// identification, so a non-zero upper half of a UDP descriptor's ipid means "fragment".
// Reassembly restates Ipv4L3Protocol::ProcessFragment and Fragments (:1208-1389).  The map key there is built with
// `&` where `|` was meant (:1213-1214), so both key words are always 0: a node has ONE buffer and one timer for all
// sources and identifications, which is what FragNode is.  The state lies behind node_ipid in its allocation
// (P2PDev takes no further pointer, see hub_slot): [N] the nodes' identifications, [N] each node's FragNode index
// (NOFRAG: the node is no destination of a fragmenting flow), then the FragHdr and the FragNodes.
constexpr uint32_t FRAG_MTU = 1500, FRAG_PART = 1480, FRAG_CAP = 128, NOFRAG = 0xffffffffu;
constexpr uint32_t ERR_FRAG_CAP = 4096u;        // the engine's error bit: a reassembly list would pass FRAG_CAP entries
constexpr uint32_t ERR_FRAG_STATE = 8192u;      // ... a fragment reached a node create gave no reassembly state (internal)
constexpr uint32_t XDROP_FRAG = 0x80000000u;    // NodeOut::xdrop: the Drop record is a fragment timeout's
struct FragEnt {  // one entry of Fragments::m_fragments: (packet, offset); the packet's size, its flow and ttl words
  uint32_t off, size, app, ttl;
};
struct FragNode {
  uint32_t n, more, gen, live;  // list length, m_moreFragment, the timer's generation, the buffer (and timer) exists
  Pkt hdr;                      // the first-arrived fragment's header (HandleFragmentsTimeout took it by value)
  uint32_t iif, pad;            // ... and its input device
  uint32_t reassembled, timeouts, cancelled, maxlen;  // nsgpu_p2p_frag_stats
  uint32_t pad2[2];
  FragEnt e[FRAG_CAP];
};
static_assert(sizeof(FragNode) == 64 + 16 * FRAG_CAP, "FragNode");
struct FragHdr {
  int64_t timeout;  // Ipv4L3Protocol::FragmentExpirationTimeout
  uint32_t nf, pad;
};
__host__ __device__ __forceinline__ size_t frag_hdr_off(uint32_t n_nodes) {  // bytes behind node_ipid
  return ((size_t)n_nodes * 8 + 15) / 16 * 16;
}
__host__ __device__ __forceinline__ FragHdr *frag_hdr(uint32_t *node_ipid, uint32_t n_nodes) {
  return reinterpret_cast<FragHdr *>(reinterpret_cast<char *>(node_ipid) + frag_hdr_off(n_nodes));
}
__host__ __device__ __forceinline__ FragNode *frag_nodes(uint32_t *node_ipid, uint32_t n_nodes) {
  return reinterpret_cast<FragNode *>(frag_hdr(node_ipid, n_nodes) + 1);
}
struct FragRx {
  uint32_t flags, gen;  // 1: the buffer is new (Schedule the timer, generation gen); 2: the datagram is entire (p)
  Pkt p;
};
// ProcessFragment for fragment p (PppHeader stripped) that arrived on device iif.  Out of line: the handlers of a
// scenario without fragments never reach it.
__device__ __noinline__ FragRx frag_receive(FragNode *F, uint32_t *error, Pkt p, uint32_t iif) {
  FragRx r{0, 0, p};
  const uint32_t off = ((p.ipid >> NSGPU_PKT_FRAG_SHIFT) & NSGPU_PKT_FRAG_OFF_MASK) * 8u;
  const uint32_t more = (p.ipid & NSGPU_PKT_FRAG_MF) ? 1u : 0u, size = p.size - 20u;
  if (!F->live) {  // m_fragments.find (key) == end: Create<Fragments> (m_moreFragment (0)), Schedule the timeout
    F->live = 1;
    F->n = 0;
    F->more = 0;
    F->gen = F->gen % 0x3fffffu + 1;  // (1 .. 2^22 - 1: the kind word's top two bits are LOCALBIT / REMOTEBIT)
    F->hdr = p;
    F->iif = iif;
    r.flags = 1;
    r.gen = F->gen;
  }
  // AddFragment (:1268-1289): before the first entry whose offset is greater (equal offsets keep arrival order);
  // m_moreFragment changes only when the fragment goes to the end
  uint32_t n = F->n, pos = 0;
  while (pos < n && !(F->e[pos].off > off)) pos++;
  if (n >= FRAG_CAP) {  // never truncated silently: the run fails
    atomicOr(error, ERR_FRAG_CAP);
    return r;
  }
  if (pos == n) F->more = more;
  for (uint32_t i = n; i > pos; i--) F->e[i] = F->e[i - 1];
  F->e[pos] = FragEnt{off, size, p.app, p.ttl};
  F->n = ++n;
  if (n > F->maxlen) F->maxlen = n;
  // IsEntire (:1291-1319), its uint16_t arithmetic kept
  bool ent = !F->more && n > 0;
  if (ent) {
    uint16_t last = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (last < (uint16_t)F->e[i].off) {
        ent = false;
        break;
      }
      const uint16_t end = (uint16_t)(F->e[i].size + F->e[i].off);
      last = last > end ? last : end;
    }
  }
  if (!ent) return r;
  // GetPacket (:1321-1356): a later entry contributes only what lies beyond lastEndOffset
  uint32_t total = 0;
  uint16_t last = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t eo = F->e[i].off & 0xffffu, es = F->e[i].size;
    if (last > eo) {
      const uint32_t ns = last - eo;
      if (es > ns) total += es - ns;
    } else {
      total += es;
    }
    last = (uint16_t)total;
  }
  // m_fragments.erase (key); the timer is cancelled (it is still dispatched, and counted, at its time) and erased.
  // The datagram goes on with the arrived fragment's IP header and the first entry's UDP header and payload.
  r.flags |= 2;
  r.p = Pkt{F->e[0].app, p.ipid & 0xffffu, 20u + total, (p.ttl & 0xffu) | (F->e[0].ttl & ~0xffu)};
  F->live = 0;
  F->n = 0;
  F->reassembled++;
  return r;
}
// Fragments::GetPartialPacket (:1358-1389)'s size: empty unless the first entry is at offset 0, else the contiguous
// prefix.  (Its CreateFragment (newStart, size - newStart) would assert for an entry that ends before lastEndOffset;
// fragments of one flow's datagrams, which all have one size, never make one: equal offsets have equal sizes.)
__device__ __noinline__ uint32_t frag_partial_size(const FragNode *F) {
  if (F->n == 0 || F->e[0].off > 0) return 0;
  uint32_t total = 0;
  uint16_t last = 0;
  for (uint32_t i = 0; i < F->n; i++) {
    const uint32_t eo = F->e[i].off & 0xffffu, es = F->e[i].size;
    if (last > eo) total += es > last - eo ? es - (last - eo) : 0u;
    else if (last == eo) total += es;
    last = (uint16_t)total;
  }
  return total;
}

// ---------------- model (runs on the thread that owns the event's node) ----------------
// Children of the event being run go to its slot's child records in Schedule-call order; the ones
// that stay pending fold into the next window's reduction (tmn, wnd).
// ---------------- receive error models (nsgpu_p2p_scenario.dev_em_kind) ----------------
// PointToPointNetDevice::Receive asks m_receiveErrorModel->IsCorrupt (packet) first (point-to-point-net-device.cc:
// 304-317); a corrupt frame fires m_phyRxDropTrace, which no ascii / pcap helper hooks, and nothing else.  An enabled
// model's state — ReceiveListErrorModel's m_timesInvoked and the cursor into its sorted list, RateErrorModel's
// RngStream — is per device and advances in the device's own event order, like its DropTail ring: it belongs to the
// serial pass of the device's node (no atomics), and a Receive on such a device is never "stateless" for the hub
// blocks (nsgpu_p2p_win.h).  The records lie behind the DevRecs in their allocation (P2PDev takes no further
// pointer, see hub_slot): the EmHdr, an EmRec for every enabled model (DevRec::em - 1), the threshold tables of the
// EU_BYTE / EU_BIT models (the host's pow: create), then the lists.  All of it is part of the reset image.
constexpr uint32_t EM_NOTAB = 0xffffffffu;
struct EmRec {
  uint32_t kind, tab;            // NSGPU_EM_*; a Rate model's threshold table (EM_NOTAB: EU_PKT, the rate itself)
  uint32_t invoked, corrupted;   // IsCorrupt calls (ReceiveList: m_timesInvoked), frames declared corrupt
  nsgpu_rng_stream g;            // Rate: the variable's RngStream
  uint32_t cur, end;             // ReceiveList: the next list entry not yet reached, the list's end (list words)
  double rate;                   // Rate: m_rate
  uint32_t dev, pad;
};
static_assert(sizeof(EmRec) == 64, "EmRec");
struct EmHdr {
  uint32_t n_models, n_tables;
  uint64_t list_words;
};
__host__ __device__ __forceinline__ EmHdr *em_hdr(DevRec *dev, uint32_t n_devices) {
  return reinterpret_cast<EmHdr *>(dev + n_devices);
}
__host__ __device__ __forceinline__ EmRec *em_recs(DevRec *dev, uint32_t n_devices) {
  return reinterpret_cast<EmRec *>(em_hdr(dev, n_devices) + 1);
}
__host__ __device__ __forceinline__ size_t em_bytes(uint32_t n_models, uint32_t n_tables, uint64_t list_words) {
  return sizeof(EmHdr) + (size_t)n_models * sizeof(EmRec) + (size_t)n_tables * NSGPU_EM_TABLE_SIZE * sizeof(double) +
         (size_t)list_words * sizeof(uint32_t);
}
// ErrorModel::IsCorrupt on enabled model em - 1 for a frame of `size` bytes (PppHeader included: Receive has not
// stripped it yet).  Out of line: the handlers of a scenario without a model never reach it.
__device__ __noinline__ bool em_is_corrupt(DevRec *dev, uint32_t n_devices, uint32_t em, uint32_t size) {
  const EmHdr *H = em_hdr(dev, n_devices);
  EmRec *r = em_recs(dev, n_devices) + (em - 1);
  const double *tabs = reinterpret_cast<const double *>(em_recs(dev, n_devices) + H->n_models);
  bool corrupt;
  if (r->kind == NSGPU_EM_RECEIVE_LIST) {
    // ReceiveListErrorModel::DoCorrupt (error-model.cc:343-360): m_timesInvoked += 1; m_timesInvoked - 1 in the list.
    // The list is sorted without duplicates and the ordinal goes up by one a call: the cursor's entry is the only
    // candidate
    const uint32_t *list = reinterpret_cast<const uint32_t *>(tabs + (size_t)H->n_tables * NSGPU_EM_TABLE_SIZE);
    const uint32_t ord = r->invoked;
    corrupt = r->cur < r->end && list[r->cur] == ord;
    if (corrupt) r->cur++;
  } else {
    // RateErrorModel::DoCorrupt (:178-223): m_ranvar.GetValue () < m_rate (EU_PKT), < 1 - pow (1.0 - m_rate, size)
    // (EU_BYTE), < 1 - pow (1.0 - m_rate, 8 * size) (EU_BIT); one U01 a frame at any rate.  (No frame is above
    // MTU + PPP; the index is clamped to the table all the same.)
    const double u = nsgpu_rng_u01(&r->g);
    const uint32_t i = size < NSGPU_EM_TABLE_SIZE ? size : NSGPU_EM_TABLE_SIZE - 1;
    const double x = r->tab == EM_NOTAB ? r->rate : tabs[(size_t)r->tab * NSGPU_EM_TABLE_SIZE + i];
    corrupt = u < x;
  }
  r->invoked++;
  if (corrupt) r->corrupted++;
  return corrupt;
}

// ---------------- per-flow statistics (nsgpu_p2p_scenario.flowmon) ----------------
// FlowMonitor's FlowStats (flow-monitor.cc:121-267), fed where Ipv4FlowProbe hooks Ipv4L3Protocol's trace sources
// (ipv4-flow-probe.cc:192-346; ipv4-l3-protocol.cc:505,618,835,838,861) and the devices' TxQueue/Drop.
// Ipv4FlowClassifier::Classify (ipv4-flow-classifier.cc:102-155) accepts UDP (and TCP) only: an ICMP message reports
// nothing.  In this subset a five-tuple is one sending application, so the flow of a descriptor is its application,
// or n_apps + it for an echo reply (the reverse tuple); the packet id is the IPv4 identification, the size the IPv4
// length, which is the descriptor's size wherever the hooks sit (the PppHeader is not on).
// m_trackedPackets becomes one table per ORIGINATING node, indexed by that node's identification (a scenario
// without frag keeps the whole counter in the descriptor): create sizes it by a bound on what the node can send, at
// most 65,536 entries, and a first transmission whose identification is outside fails the run (ERR_FLOWMON_ID)
// before anything is written.  An entry is read and written only by the node that holds the packet, and a packet
// changes node across a window boundary only (a Receive's delay is at least the lookahead): plain loads and stores.
// A flow's record is three 128-B lines by owner: FmTx, written by the sender's node; FmRx, by the destination's, in
// that node's event order (the jitter needs the previous delay); FmDrop, commutative counts added with atomics from
// wherever a drop happens.  Everything lies behind node_ipid in its allocation (P2PDev takes no further pointer, see
// hub_slot; frag, which also lives there, is refused with flowmon): [N] identifications, then at 128-B bounds the
// FmHdr, [N] table bases (entries), [N] table sizes, the FmTx / FmRx / FmDrop arrays (2 n_apps each), the entries.
constexpr uint32_t ERR_FLOWMON_ID = 16384u;  // the engine's error bit: a monitored node's identification left its table
constexpr uint32_t FM_NODE_CAP = 65536u;     // entries a node at most: the identification has 16 bits
struct FmEnt {  // FlowMonitor::TrackedPacket, and the flow + 1 while it is tracked (0: erased, or never sent)
  int64_t first, last;
  uint32_t fwd, flow1, size, pad;
};
static_assert(sizeof(FmEnt) == 32, "FmEnt");
struct FmTx {
  uint64_t packets, bytes;
  int64_t t_first, t_last;
  uint64_t first_ts;  // the event that made the flow's first ReportFirstTx: (ts, uid)
  uint32_t first_uid, pad;
  uint64_t pad2[10];
};
struct FmRx {
  uint64_t packets, bytes;
  int64_t delay_sum, jitter_sum, last_delay, t_first, t_last;
  uint64_t forwarded;
  uint64_t pad[8];
};
struct FmDrop {
  unsigned long long lost, packets[NSGPU_FLOW_DROP_REASONS], bytes[NSGPU_FLOW_DROP_REASONS];
  uint64_t pad[7];
};
struct FmHdr {
  uint32_t n_flows, n_nodes;
  uint64_t n_entries;
  uint64_t pad[14];
};
static_assert(sizeof(FmTx) == 128 && sizeof(FmRx) == 128 && sizeof(FmDrop) == 128 && sizeof(FmHdr) == 128,
              "one 128-B line a part: no line is written from two nodes");
__host__ __device__ __forceinline__ size_t fm_hdr_off(uint32_t n_nodes) {  // bytes behind node_ipid
  return ((size_t)n_nodes * 4 + 127) / 128 * 128;
}
__host__ __device__ __forceinline__ size_t fm_rec_off(uint32_t n_nodes) {
  return (fm_hdr_off(n_nodes) + sizeof(FmHdr) + (size_t)n_nodes * 12 + 127) / 128 * 128;
}
__host__ __device__ __forceinline__ size_t fm_bytes(uint32_t n_nodes, uint32_t n_flows, uint64_t n_entries) {
  return fm_rec_off(n_nodes) + (size_t)n_flows * 3 * 128 + (size_t)n_entries * sizeof(FmEnt);
}
__host__ __device__ __forceinline__ uint64_t *fm_node_base(uint32_t *node_ipid, uint32_t n_nodes) {
  return reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(node_ipid) + fm_hdr_off(n_nodes) + sizeof(FmHdr));
}
__host__ __device__ __forceinline__ uint32_t *fm_node_cap(uint32_t *node_ipid, uint32_t n_nodes) {
  return reinterpret_cast<uint32_t *>(fm_node_base(node_ipid, n_nodes) + n_nodes);
}
__host__ __device__ __forceinline__ FmTx *fm_tx(uint32_t *node_ipid, uint32_t n_nodes) {
  return reinterpret_cast<FmTx *>(reinterpret_cast<char *>(node_ipid) + fm_rec_off(n_nodes));
}
__host__ __device__ __forceinline__ FmRx *fm_rx(uint32_t *node_ipid, uint32_t n_nodes, uint32_t n_flows) {
  return reinterpret_cast<FmRx *>(fm_tx(node_ipid, n_nodes) + n_flows);
}
__host__ __device__ __forceinline__ FmDrop *fm_drops(uint32_t *node_ipid, uint32_t n_nodes, uint32_t n_flows) {
  return reinterpret_cast<FmDrop *>(fm_rx(node_ipid, n_nodes, n_flows) + n_flows);
}
__host__ __device__ __forceinline__ FmEnt *fm_ents(uint32_t *node_ipid, uint32_t n_nodes, uint32_t n_flows) {
  return reinterpret_cast<FmEnt *>(fm_drops(node_ipid, n_nodes, n_flows) + n_flows);
}
// The monitor's functions are out of line and read the device-resident descriptor (cold paths, above): the handlers
// of an unmonitored engine hold the test of M.flowmon and a call.
// Classify + the tracked entry of datagram p (null: its identification is outside its node's table).
__device__ __forceinline__ FmEnt *fm_entry(const P2PDev &M, const Pkt &p, uint32_t *flow) {
  const uint32_t fa = p.app & NSGPU_PKT_APP;
  const bool reply = (p.app & NSGPU_PKT_REPLY) != 0;
  *flow = reply ? M.n_apps + fa : fa;
  const uint32_t o = reply ? M.app_dst_node[fa] : M.app_node[fa];  // (the reply is the server's node's datagram)
  if (p.ipid >= fm_node_cap(M.node_ipid, M.n_nodes)[o]) return nullptr;
  return fm_ents(M.node_ipid, M.n_nodes, 2 * M.n_apps) + fm_node_base(M.node_ipid, M.n_nodes)[o] + p.ipid;
}
// SendOutgoingLogger -> ReportFirstTx (flow-monitor.cc:121-146): Ipv4L3Protocol::Send after BuildHeader, before
// SendRealOut (:618).  (now, uid): the event being run.
__device__ __noinline__ void fm_first_tx(const P2PDev *G, Pkt p, uint64_t now, uint32_t uid) {
  const P2PDev &M = mdev_ref(G);
  uint32_t flow;
  FmEnt *e = fm_entry(M, p, &flow);
  if (!e) {  // (with create's bound: the 16-bit identification would wrap; the overwrite-on-wrap is not modelled)
    atomicOr(M.error, ERR_FLOWMON_ID);
    return;
  }
  *e = FmEnt{(int64_t)now, (int64_t)now, 0u, flow + 1u, p.size, 0u};
  FmTx *t = fm_tx(M.node_ipid, M.n_nodes) + flow;
  t->bytes += p.size;
  if (t->packets++ == 0) {
    t->t_first = (int64_t)now;
    t->first_ts = now;
    t->first_uid = uid;
  }
  t->t_last = (int64_t)now;
}
// ForwardLogger -> ReportForwarding (:149-170): IpForward after the TTL check (:838).
__device__ __noinline__ void fm_forward(const P2PDev *G, Pkt p, uint64_t now) {
  const P2PDev &M = mdev_ref(G);
  uint32_t flow;
  FmEnt *e = fm_entry(M, p, &flow);
  if (!e || e->flow1 != flow + 1u) return;  // "not known to be transmitted"
  e->fwd++;
  e->last = (int64_t)now;
}
// ForwardUpLogger -> ReportLastRx (:173-234): LocalDeliver (:861), before the UDP endpoint lookup.
__device__ __noinline__ void fm_last_rx(const P2PDev *G, Pkt p, uint64_t now) {
  const P2PDev &M = mdev_ref(G);
  uint32_t flow;
  FmEnt *e = fm_entry(M, p, &flow);
  if (!e || e->flow1 != flow + 1u) return;
  FmRx *r = fm_rx(M.node_ipid, M.n_nodes, 2 * M.n_apps) + flow;
  const int64_t delay = (int64_t)now - e->first;
  r->delay_sum += delay;
  if (r->packets > 0) {
    const int64_t jitter = r->last_delay - delay;
    r->jitter_sum += jitter > 0 ? jitter : -jitter;
  }
  r->last_delay = delay;
  r->bytes += p.size;
  if (r->packets++ == 0) r->t_first = (int64_t)now;
  r->t_last = (int64_t)now;
  r->forwarded += e->fwd;
  e->flow1 = 0;  // m_trackedPackets.erase
}
// DropLogger / QueueDropLogger -> ReportDrop (:236-267): counted whether or not the packet is tracked, then erased.
__device__ __noinline__ void fm_drop(const P2PDev *G, Pkt p, uint32_t reason) {
  const P2PDev &M = mdev_ref(G);
  uint32_t flow;
  FmEnt *e = fm_entry(M, p, &flow);
  FmDrop *d = fm_drops(M.node_ipid, M.n_nodes, 2 * M.n_apps) + flow;
  atomicAdd(&d->lost, 1ull);
  atomicAdd(&d->packets[reason], 1ull);
  atomicAdd(&d->bytes[reason], (unsigned long long)p.size);
  if (e && e->flow1 == flow + 1u) e->flow1 = 0;
}
// The hooks as the handlers call them: nothing for an unmonitored engine or an ICMP message.
__device__ __forceinline__ bool fm_on(const P2PDev &M, const Pkt &p) { return M.flowmon && !(p.app & NSGPU_PKT_ICMP); }

struct Emit {
  uint64_t now;
  uint32_t ctx;
  uint32_t slot0;  // slot * maxc
  uint32_t n;
  uint64_t *ch_ts;
  uint32_t *ch_ctx, *ch_kind, *ch_a;
  Pkt *ch_pkt;
  const int64_t *lookahead, *lookw;
  uint64_t tmn, wnd, wndw;
  uint64_t lim_abs;  // wide window: a TransmitComplete child before it is a local record (0: none)
  uint32_t uid;      // uid of the event being run (its trace records; a local record's: its record index, tloc)
  bool tloc = false; // the event is a local record whose uid k2_scan assigns later (k_tpatch resolves its records)
  uint32_t trseq;    // trace sink calls made by it so far
  bool demote;       // the event's ts group is cut by a run chunk: its DoForwardUp leaves are queued
  int32_t lj;        // the local child this event made (an event makes at most one TransmitComplete): its
  uint32_t la, lctx; //   index (-1: none), device and context
  uint64_t lts;
  __device__ __forceinline__ void child(int64_t delay, uint32_t ctx_, uint32_t kind, uint32_t a, Pkt p) {
    if (demote && kind == K_FWD_UP) kind = K_FWD_UP_D;
    const uint32_t s = slot0 + n++;
    const uint64_t ts = now + (uint64_t)delay;
    // a same-node TransmitComplete inside a wide window runs in it (the node's holder takes it next)
    const bool local = kind == K_TX_COMPLETE && ts < lim_abs;
    ch_ts[s] = ts;
    ch_ctx[s] = ctx_;
    ch_kind[s] = local ? (kind | LOCALBIT) : kind;
    if (local) {
      lj = (int32_t)(s - slot0);
      lts = ts;
      la = a;
      lctx = ctx_;
    }
    ch_a[s] = a;
    ch_pkt[s] = p;
    if ((kind & 0xffu) != K_FWD_UP && !local) {  // DoForwardUp is a leaf run inside the window, never re-queued
      tmn = ts < tmn ? ts : tmn;
      const uint64_t e = ts + (uint64_t)lookahead[kind & 0xffu];
      wnd = e < wnd ? e : wnd;
      if (lookw) {  // (wide engines)
        const uint64_t ew = ts + (uint64_t)lookw[kind & 0xffu];
        wndw = ew < wndw ? ew : wndw;
      }
    }
  }
  // An out-of-line node part (node_part_cold) made this event's children [n, n1) through an Emit of its own: the
  // same fold of their records into the minima as child()'s (a node part makes no TransmitComplete: none is local).
  __device__ __forceinline__ void adopt(uint32_t n1) {
    for (; n < n1; n++) {
      const uint32_t kind = ch_kind[slot0 + n];
      if ((kind & 0xffu) == K_FWD_UP || (kind & LOCALBIT)) continue;
      const uint64_t ts = ch_ts[slot0 + n];
      tmn = ts < tmn ? ts : tmn;
      const uint64_t e = ts + (uint64_t)lookahead[kind & 0xffu];
      wnd = e < wnd ? e : wnd;
      if (lookw) {
        const uint64_t ew = ts + (uint64_t)lookw[kind & 0xffu];
        wndw = ew < wndw ? ew : wndw;
      }
    }
  }
};

// Run statistics of one handler thread.
struct HStat {
  uint32_t cancelled, ttl_drops, no_route, unreach, icmp;  // (one holder's window: 32 bits; 64-bit fields were spilled to scratch)
  bool stop;
};

// Device step of an event (second phase of every handler, run by all lanes together so the wave
// does not serialise one copy per event kind):
//   SEND  PointToPointNetDevice::Send (point-to-point-net-device.cc:462-518): PppHeader, enqueue
//         (DropTail: queue.cc:61-97, drop-tail-queue.cc:83-100), and if the device is idle dequeue
//         + TransmitStart;
//   KICK  TransmitComplete (:304-346): device idle, dequeue, TransmitStart if a packet was queued.
// TransmitStart (:206-269) + PointToPointChannel::TransmitStart (point-to-point-channel.cc:82-103):
//   Schedule (txTime + ifg, TransmitComplete); ScheduleWithContext (peer node, txTime + delay, Receive).
enum : uint32_t { ACT_NONE = 0, ACT_SEND = 1, ACT_KICK = 2 };

// One ascii trace sink call (AsciiTraceHelper::Default*SinkWithContext, trace-helper.cc:303-390, as
// hooked by PointToPointHelper::EnableAsciiInternal, point-to-point-helper.cc:113-219): appended
// unordered; the host orders the records by (ts, uid, seq).
// The record itself is written out of line (cold paths, above): an untraced engine's handlers hold only the test.
__device__ __noinline__ void trace_append(const P2PDev *G, uint64_t now, uint32_t uid, uint32_t seq, uint32_t kind,
                                          uint32_t tloc, uint32_t d, Pkt p) {
  nsgpu_trace_record r;
  r.ts = now;
  r.uid = uid;
  r.seq = (uint16_t)seq;
  r.kind = (uint8_t)kind;
  r.pad_ = tloc ? 1 : 0;  // (k_tpatch replaces a local record's index by its uid and clears the flag)
  r.dev = d;
  r.app = p.app;
  r.ipid = p.ipid;
  r.size = p.size;
  r.ttl = p.ttl;
  r.pad2_ = 0;
  const P2PDev &M = mdev_ref(G);
  const unsigned long long i = atomicAdd(M.trace_n, 1ull);
  if (i < M.trace_cap) M.trace[i] = r;
}
__device__ __forceinline__ void trace_call(const P2PDev &M, Emit &E, uint32_t kind, uint32_t d, const Pkt &p) {
  if (!M.trace || !((M.trace_kinds >> kind) & 1u)) return;
  trace_append(mdev_of(M.C), E.now, E.uid, E.trseq++, kind, E.tloc ? 1u : 0u, d, p);
}
struct Act {
  uint32_t op, dev;
  Pkt p;
};
// Ipv4L3Protocol::m_dropTrace (ipv4-l3-protocol.cc:505,835): the datagram as received (a UDP datagram's
// 16-bit identification); d = the receiving device (DROP_NO_ROUTE) or the forwarding route's
// (DROP_TTL_EXPIRED).
__device__ __forceinline__ void trace_ip_drop(const P2PDev &M, Emit &E, uint32_t d, Pkt p) {
  if (!(p.app & NSGPU_PKT_ICMP)) p.ipid &= 0xffffu;
  trace_call(M, E, NSGPU_TR_IP_DROP, d, p);
}
// The TTL-expired datagram a time-exceeded error e was made from (icmp_error below embeds its flow, reply
// flag, identification and length; it arrived with TTL 1): its Drop record follows the error's Send.
__device__ __forceinline__ void trace_te_drop(const P2PDev &M, Emit &E, uint32_t d, const Pkt &e) {
  const uint32_t app = (e.app & NSGPU_PKT_APP) | ((e.app & NSGPU_PKT_ICMP_OF_REPLY) ? NSGPU_PKT_REPLY : 0u);
  trace_call(M, E, NSGPU_TR_IP_DROP, d, Pkt{app, e.ipid >> 16, e.ttl >> 16, 1u});
}

// The Drop record that follows an ICMP error's device step (NodeOut::xdrop).  XDROP_FRAG (extended handlers): a
// fragment timeout's, on the captured input device with the captured header's TTL (the error embeds it).
template <bool EXT>
__device__ __forceinline__ void xdrop_record(const P2PDev &M, Emit &E, uint32_t xdrop, const Pkt &e) {
  if (EXT && (xdrop & XDROP_FRAG)) {
    const uint32_t app = (e.app & NSGPU_PKT_APP) | ((e.app & NSGPU_PKT_ICMP_OF_REPLY) ? NSGPU_PKT_REPLY : 0u);
    trace_call(M, E, NSGPU_TR_IP_DROP, (xdrop & ~XDROP_FRAG) - 1, Pkt{app, e.ipid >> 16, e.ttl >> 16, (e.ttl >> 8) & 0xffu});
    return;
  }
  trace_te_drop(M, E, xdrop - 1, e);
}
// SendRealOut (ipv4-l3-protocol.cc:722-731, 751-761) of a datagram above the MTU, DoFragmentation (:1116-1206): the
// fragments take FRAG_PART bytes of IP payload each, the last the rest; each has IPv4 length 20 + part, all but the
// last MF, the offset in 8-byte units, one identification.  For each fragment in order: m_txTrace, then the device's
// Send (`step`: one single-packet device step) — the first may start transmitting, the rest queue or are dropped.
// The fragment of datagram d (its IPv4 length in size) at payload offset off; *more: another follows.
__device__ __forceinline__ Pkt fragment_at(const Pkt &d, uint32_t off, bool *more) {
  const uint32_t L = d.size - 20u;
  *more = L > off + FRAG_PART;  // p->GetSize () > offset + fragmentSize
  const uint32_t part = *more ? FRAG_PART : L - off;
  return Pkt{d.app, (d.ipid & 0xffffu) | ((off >> 3) << NSGPU_PKT_FRAG_SHIFT) | (*more ? NSGPU_PKT_FRAG_MF : 0u),
             20u + part, d.ttl};
}
// A sender's device step whose datagram is above the MTU (an ICMP error is 56 bytes: never).
__device__ __forceinline__ bool is_fragmenting_send(uint32_t op, uint32_t size) {
  return op == ACT_SEND && size > FRAG_MTU;
}

__device__ __forceinline__ void device_act(const P2PDev &M, Emit &E, const Act &act) {
  if (act.op == ACT_NONE) return;
  const uint32_t d = act.dev;
  // every operand of the step at once
  const DevRec dr = M.dev[d];
  const uint32_t busy = dr.busy, cnt = dr.cnt, head = dr.head, qmax = dr.qmax;
  nsgpu_dev_counters dc = dr.c;
  const uint64_t bps = dr.bps;
  const int64_t ifg = dr.ifg, delay = dr.delay;
  const uint32_t peer = dr.peer;
  const uint32_t peer_node = dr.peer_node;
  Pkt *qb = M.q_buf + (uint64_t)d * M.qcap;
  uint32_t ncnt = cnt, nhead = head, nbusy = busy;
  bool go = false;
  Pkt tx{0, 0, 0, 0};
  if (act.op == ACT_SEND) {
    trace_call(M, E, NSGPU_TR_IP_TX, d, act.p);  // SendRealOut: m_txTrace, then the device's Send
    Pkt p = act.p;
    p.size += 2;  // PppHeader
    if (cnt >= qmax) {
      trace_call(M, E, NSGPU_TR_DROP, d, p);  // Queue::Drop: m_traceDrop
      dc.drop_packets++;
      dc.drop_bytes += p.size;
    } else {
      trace_call(M, E, NSGPU_TR_ENQUEUE, d, p);  // Queue::Enqueue: m_traceEnqueue
      dc.enq_packets++;
      dc.enq_bytes += p.size;
      if (busy == 0) {  // Enqueue + Dequeue: the head of the queue leaves at once
        if (cnt == 0) {
          tx = p;  // (the ring slot would be written and read back: skip it)
        } else {
          qb[(head + cnt) % M.qcap] = p;
          tx = qb[head];
        }
        nhead = (head + 1) % M.qcap;
        trace_call(M, E, NSGPU_TR_DEQUEUE, d, tx);  // Queue::Dequeue: m_traceDequeue
        dc.deq_packets++;
        go = true;
      } else {
        qb[(head + cnt) % M.qcap] = p;
        ncnt = cnt + 1;
      }
    }
  } else {  // ACT_KICK
    nbusy = 0;
    if (cnt > 0) {
      tx = qb[head];
      nhead = (head + 1) % M.qcap;
      ncnt = cnt - 1;
      trace_call(M, E, NSGPU_TR_DEQUEUE, d, tx);
      dc.deq_packets++;
      go = true;
    }
  }
  if (go) {
    nbusy = 1;
    dc.tx_packets++;
    // Seconds (m_bps.CalculateTxTime (size)): static_cast<double>(bytes)*8/m_bps (data-rate.cc:224-227)
    const int64_t txTime = seconds_to_ts(static_cast<double>(tx.size) * 8 / (double)bps);
    E.child(txTime + ifg, E.ctx, K_TX_COMPLETE, d, Pkt{0, 0, 0, 0});
    E.child(txTime + delay, peer_node, dr.rkind, peer, tx);
  }
  if (nbusy != busy) M.dev[d].busy = nbusy;
  if (ncnt != cnt) M.dev[d].cnt = ncnt;
  if (nhead != head) M.dev[d].head = nhead;
  M.dev[d].c = dc;
}

// int64x64 residual-bits update of OnOffApplication::CancelEvents (onoff-application.cc:170-173):
// bits = (delta.To (Time::S) * GetBitRate ()).GetHigh (); To(S) = int64x64 (delta) MulByInvert Invert (1e9).
__device__ __forceinline__ u128 umul_by_invert(u128 a, u128 b) {
  const u128 LO = (((u128)1) << 64) - 1;
  u128 ah = a >> 64, bh = b >> 64, al = a & LO, bl = b & LO;
  u128 hi = ah * bh;
  u128 mid = ah * bl + al * bh;
  mid >>= 64;
  return hi + mid;
}
__device__ __forceinline__ u128 divu(u128 a, u128 b) {
  u128 quo = a / b;
  u128 rem = a % b;
  u128 result = quo << 64;
  u128 tmp = rem >> 64;
  u128 div;
  if (tmp == 0) {
    rem = rem << 64;
    div = b;
  } else {
    div = b >> 64;
  }
  quo = rem / div;
  return result + quo;
}
// Invert (1e9) (int64x64-128.cc:119-134): the same steps, evaluated at compile time (per call, its 128-bit
// divisions took thousands of instructions a lane; a wave of OnOff StopApplications paid them in every window)
constexpr u128 c_umul_by_invert(u128 a, u128 b) {
  const u128 LO = (((u128)1) << 64) - 1;
  return (a >> 64) * (b >> 64) + (((a >> 64) * (b & LO) + (a & LO) * (b >> 64)) >> 64);
}
constexpr u128 c_divu(u128 a, u128 b) {
  const u128 quo = a / b, rem = a % b;
  const bool small = (rem >> 64) == 0;
  return (quo << 64) + (small ? (rem << 64) / b : rem / (b >> 64));
}
constexpr i128 c_invert_1e9() {
  i128 inv = (i128)c_divu(((u128)1) << 64, (u128)1000000000ull);
  const u128 r = c_umul_by_invert((u128)(((i128)1000000000ll) << 64), (u128)inv);
  if ((int64_t)(r >> 64) != 1) inv += 1;
  return inv;
}
__device__ __noinline__ int64_t residual_bits(int64_t delta_ns, uint64_t rate) {
  constexpr i128 inv = c_invert_1e9();
  static_assert((uint64_t)((u128)inv >> 64) == 0x44b82fa09ull && (uint64_t)(u128)inv == 0xb5a52cb98b405448ull,
                "Invert (1e9)");
  // MulByInvert (delta)
  i128 v = ((i128)delta_ns) << 64;
  bool neg = v < 0;
  u128 a = neg ? (u128)(-v) : (u128)v;
  u128 t = umul_by_invert(a, (u128)inv);
  i128 ts = neg ? -(i128)t : (i128)t;
  // Mul by int64x64_t (rate): Umul with the '|=' combine (int64x64-128.cc:20-57)
  i128 rb = ((i128)rate) << 64;
  bool negA = ts < 0;
  u128 ua = negA ? (u128)(-ts) : (u128)ts, ub = (u128)rb;
  const u128 LO = (((u128)1) << 64) - 1;
  u128 aL = ua & LO, bL = ub & LO, aH = (ua >> 64) & LO, bH = (ub >> 64) & LO;
  u128 loPart = aL * bL;
  u128 midPart = aL * bH + aH * bL;
  u128 res = (loPart >> 64) + (midPart & LO);
  u128 hiPart = aH * bH;
  res |= ((hiPart & LO) << 64) + (midPart & ~LO);
  i128 r = negA ? -(i128)res : (i128)res;
  bool rn = r < 0;
  i128 x = rn ? -r : r;
  x >>= 64;
  int64_t h = (int64_t)x;
  return rn ? -h : h;
}

__device__ __forceinline__ void cancel_events(const P2PDev &M, uint32_t a, uint64_t now) {
  uint32_t f = M.app_flags[a];
  if (f & 4u) {  // m_sendEvent.IsRunning ()
    const int64_t delta = (int64_t)now - (int64_t)M.app_last_start[a];
    M.app_residual[a] += (uint32_t)residual_bits(delta, M.app_rate[a]);
  }
  M.app_flags[a] = f & ~(4u | 8u);  // Cancel (m_sendEvent); Cancel (m_startStopEvent)
}

// ---------------- random OnOff times (nsgpu_p2p_scenario_ext.app_on_var / app_off_var) ----------------
// OnOffApplication::ScheduleStartEvent / ScheduleStopEvent (onoff-application.cc:221-237) take Seconds
// (m_offTime.GetValue ()) / Seconds (m_onTime.GetValue ()): the draw happens when the event is scheduled, whether or not
// it is cancelled later; ScheduleNextTx's StopApplication at MaxBytes draws nothing.  A variable (random-variable.cc:
// 251-258 Uniform, :574-589 Exponential; nsgpu_ranvar.h) owns its RngStream, and the helper's attribute copy gives every
// application its own two.  Their state — stream, parameters, draw and ambiguous counts — is per application and
// advances in the application's own event order: it belongs to the serial pass of the application's node, like
// app_ss_gen (no atomics; on a partitioned engine the owner of the node).  The records lie behind app_last_start in its
// allocation (P2PDev takes no further pointer, see hub_slot): the RvHdr, two RvRecs an application (OnTime, OffTime),
// then the log of ambiguous attempts, whose slots are claimed with one atomic (appends are rare).  All of it is part of
// the reset image.
constexpr uint32_t ERR_RANVAR_ATTEMPTS = 65536u;  // the engine's error bit: a bounded Exponential was rejected 1,024 times
struct RvRec {
  nsgpu_rng_stream g;
  uint32_t draws, ambiguous;  // GetValue calls; ambiguous attempts
  nsgpu_ranvar v;
  uint64_t pad;
};
static_assert(sizeof(RvRec) == 64, "RvRec");
struct RvHdr {
  uint32_t log_n, log_over;  // log records written (at most NSGPU_RV_AMBIGUOUS_CAP); attempts beyond them
  uint32_t pad[2];
};
__host__ __device__ __forceinline__ RvHdr *rv_hdr(uint64_t *app_last_start, uint32_t n_apps) {
  return reinterpret_cast<RvHdr *>(app_last_start + n_apps);
}
__host__ __device__ __forceinline__ RvRec *rv_recs(uint64_t *app_last_start, uint32_t n_apps) {
  return reinterpret_cast<RvRec *>(rv_hdr(app_last_start, n_apps) + 1);
}
__host__ __device__ __forceinline__ nsgpu_ambiguous_draw *rv_log(uint64_t *app_last_start, uint32_t n_apps) {
  return reinterpret_cast<nsgpu_ambiguous_draw *>(rv_recs(app_last_start, n_apps) + 2 * (size_t)n_apps);
}
__host__ __device__ __forceinline__ size_t rv_bytes(uint32_t n_apps) {  // the whole allocation
  return (size_t)n_apps * sizeof(uint64_t) + sizeof(RvHdr) + 2 * (size_t)n_apps * sizeof(RvRec) +
         (size_t)NSGPU_RV_AMBIGUOUS_CAP * sizeof(nsgpu_ambiguous_draw);
}
static_assert(sizeof(nsgpu_ambiguous_draw) == 32 && sizeof(RvHdr) == 16, "the log's records stay 8-byte aligned");
// Seconds (GetValue ()) of application a's OnTime (which = 0) or OffTime (1) variable.  Out of line: the handlers of a
// scenario without a random variable never reach it.
__device__ __noinline__ int64_t rv_draw(const P2PDev *G, uint32_t a, uint32_t which) {
  const P2PDev &M = mdev_ref(G);
  RvRec *r = rv_recs(M.app_last_start, M.n_apps) + (2 * (size_t)a + which);
  if (r->v.kind == NSGPU_RV_CONSTANT) return seconds_to_ts(r->v.p0);
  const uint32_t ordinal = r->draws++;
  RvHdr *H = rv_hdr(M.app_last_start, M.n_apps);
  nsgpu_ambiguous_draw *L = rv_log(M.app_last_start, M.n_apps);
  double sec;
  const bool ok = nsgpu_ranvar_value(r->v, &r->g, &sec, [&](uint32_t k, int64_t ns, int64_t ns2) {
    r->ambiguous++;
    const uint32_t i = atomicAdd(&H->log_n, 1u);
    if (i < NSGPU_RV_AMBIGUOUS_CAP) {
      L[i] = nsgpu_ambiguous_draw{a, which, ordinal, k, ns, ns2};
    } else {  // (log_n is clamped when it is read)
      atomicAdd(&H->log_over, 1u);
    }
  });
  if (!ok) atomicOr(M.error, ERR_RANVAR_ATTEMPTS);
  return seconds_to_ts(sec);
}
// EXT: the extended handlers (k2_handle<.., PORTS = true>); the default instantiations read the constants as before.
// RV_HANDLERS: and of the extended handlers only the copy compiled in nsgpu_p2p_ranvar.hip (NSGPU_P2P_RANVAR) calls
// rv_draw.  The draw is register-heavy (a double-double logarithm, three Seconds () conversions in 128-bit integers:
// 70 VGPRs, 97 SGPRs), and a callee's registers shape its callers' allocation: compiled into nsgpu_p2p_ports.hip's
// handlers it cost every one of them 24 B of scratch a lane, SGPRs spilled to VGPR lanes in the holders' loop and
// 2 to 4 % of an existing ports workload's speed (profiles/r17/kernel_resources.md).  In a code object of its own only
// the scenarios with a random variable pay.
#ifdef NSGPU_P2P_RANVAR
constexpr bool RV_HANDLERS = true;
#else
constexpr bool RV_HANDLERS = false;
#endif
template <bool EXT = false>
__device__ __forceinline__ void schedule_start_event(const P2PDev &M, Emit &E, uint32_t a) {
  const uint32_t g = (M.app_ss_gen[a] + 1) & 0xffffffu;
  M.app_ss_gen[a] = g;
  M.app_flags[a] |= 8u;
  int64_t d;
  if (EXT && RV_HANDLERS && M.ranvar) d = rv_draw(mdev_of(M.C), a, 1);  // Seconds (m_offTime.GetValue ())
  else d = seconds_to_ts(M.app_off_s[a]);
  E.child(d, E.ctx, K_START_SENDING | (g << 8), a, Pkt{0, 0, 0, 0});
}
template <bool EXT = false>
__device__ __forceinline__ void schedule_stop_event(const P2PDev &M, Emit &E, uint32_t a) {
  const uint32_t g = (M.app_ss_gen[a] + 1) & 0xffffffu;
  M.app_ss_gen[a] = g;
  M.app_flags[a] |= 8u;
  int64_t d;
  if (EXT && RV_HANDLERS && M.ranvar) d = rv_draw(mdev_of(M.C), a, 0);  // Seconds (m_onTime.GetValue ())
  else d = seconds_to_ts(M.app_on_s[a]);
  E.child(d, E.ctx, K_STOP_SENDING | (g << 8), a, Pkt{0, 0, 0, 0});
}
template <bool PORTS = false>
__device__ __forceinline__ void stop_application(const P2PDev &M, uint32_t a, uint64_t now) {
  const uint32_t k = M.app_kind[a];
  if (k == NSGPU_APP_SINK || k == NSGPU_APP_ECHO_SERVER) {  // m_socket->Close ()
    M.app_flags[a] &= ~2u;
    return;
  }
  if (k == NSGPU_APP_ECHO_CLIENT) {  // UdpEchoClient::StopApplication: Close; Simulator::Cancel (m_sendEvent)
    M.app_flags[a] &= ~(2u | 4u);
    return;
  }
  if (PORTS && k == NSGPU_APP_UDP_SERVER) {  // UdpServer::StopApplication: SetRecvCallback (null); the socket stays bound
    M.app_flags[a] |= AF_RX_CLEARED;
    return;
  }
  // UdpClient::StopApplication, UdpTraceClient::StopApplication (udp-trace-client.cc:258-263): Simulator::Cancel (m_sendEvent)
  if (PORTS && (k == NSGPU_APP_UDP_CLIENT || k == NSGPU_APP_UDP_TRACE_CLIENT)) {
    M.app_flags[a] &= ~4u;
    return;
  }
  cancel_events(M, a, now);
}
// OnOffApplication::ScheduleNextTx (onoff-application.cc:228-252); the child is returned, not
// emitted: in SendPacket it is scheduled after the packet's device children.
struct Post {
  bool valid;
  int64_t delay;
  uint32_t kind, a;
};
__device__ __forceinline__ Post schedule_next_tx(const P2PDev &M, uint32_t a, uint64_t now) {
  Post po{false, 0, 0, 0};
  const uint32_t maxb = M.app_max_bytes[a];
  if (maxb == 0 || M.app_tot[a] < maxb) {
    const uint32_t bits = M.app_pkt_size[a] * 8 - M.app_residual[a];
    const uint32_t g = (M.app_send_gen[a] + 1) & 0xffffffu;
    M.app_send_gen[a] = g;
    M.app_flags[a] |= 4u;
    po.valid = true;
    po.delay = seconds_to_ts(bits / static_cast<double>(M.app_rate[a]));
    po.kind = K_SEND | (g << 8);
    po.a = a;
  } else {
    stop_application(M, a, now);
  }
  return po;
}
__device__ __forceinline__ void appobj_start(const P2PDev &M, Emit &E, uint32_t a) {  // Application::DoStart
  uint32_t f = M.app_flags[a];
  if (f & 1u) return;
  M.app_flags[a] = f | 1u;
  E.child(M.app_start[a], E.ctx, K_APP_START, a, Pkt{0, 0, 0, 0});
  if (M.app_stop[a] != 0) E.child(M.app_stop[a], E.ctx, K_APP_STOP, a, Pkt{0, 0, 0, 0});
}

// Addressing of a packet descriptor: the node it is addressed to and that node's route-table slot.
// An echo reply (NSGPU_PKT_REPLY) travels back to its client's node; an ICMP error (NSGPU_PKT_ICMP) to the
// offending datagram's sender (icmpv4-l4-protocol.cc:131-160: SendMessage (p, header.GetSource (), ...)).
__device__ __forceinline__ uint32_t pkt_dst_node(const P2PDev &M, const Pkt &p) {
  if (p.app & NSGPU_PKT_ICMP) {
    const uint32_t fa = p.app & NSGPU_PKT_APP;
    return (p.app & NSGPU_PKT_ICMP_OF_REPLY) ? M.app_dst_node[fa] : M.app_node[fa];
  }
  if (p.app & NSGPU_PKT_REPLY) return M.app_node[p.app & ~NSGPU_PKT_REPLY];
  return M.app_dst_node[p.app];
}
__device__ __forceinline__ uint32_t pkt_dst_slot(const P2PDev &M, const Pkt &p) {
  if (p.app & NSGPU_PKT_ICMP) {
    const uint32_t fa = p.app & NSGPU_PKT_APP;
    return (p.app & NSGPU_PKT_ICMP_OF_REPLY) ? M.app_dst_slot[fa] : M.app_src_slot[fa];
  }
  if (p.app & NSGPU_PKT_REPLY) return M.app_src_slot[p.app & ~NSGPU_PKT_REPLY];
  return M.app_dst_slot[p.app];
}
// The ICMP error about datagram p (its IPv4 header as the error embeds it): Icmpv4TimeExceeded /
// Icmpv4DestinationUnreachable + the 4-byte Icmpv4Header over the offending header and 8 payload bytes:
// a 56-byte IPv4 packet with the default TTL 64 (icmpv4.cc:306-309,407-410; Ipv4L3Protocol::Send).
__device__ __forceinline__ Pkt icmp_error(const Pkt &p, bool unreach) {
  const uint32_t of = (p.app & NSGPU_PKT_REPLY) ? NSGPU_PKT_ICMP_OF_REPLY : 0u;
  return Pkt{NSGPU_PKT_ICMP | (unreach ? NSGPU_PKT_ICMP_UNREACH : 0u) | of | (p.app & NSGPU_PKT_APP),
             (p.ipid & 0xffffu) << 16, 56u, 64u | ((p.ttl & 0xffu) << 8) | (p.size << 16)};
}

// Ipv4 route lookup: the static next-hop device of node n towards route-table slot `slot`.
// The compressed table (out of line: cold paths): binary search of the node's exceptions (a dumbbell router holds
// one per leaf); a node with an exception for every slot has them at their slot's position (ascending, distinct).
__device__ __noinline__ uint32_t route_compressed(const P2PDev *G, uint32_t n, uint32_t slot) {
  const P2PDev &M = mdev_ref(G);
  const uint64_t e1 = M.route_exc_off[n + 1];
  uint64_t lo = M.route_exc_off[n], hi = e1;
  if (hi - lo == M.n_dst) return M.route_exc_dev[lo + slot];
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (M.route_exc_slot[mid] < slot) lo = mid + 1;
    else hi = mid;
  }
  return (lo < e1 && M.route_exc_slot[lo] == slot) ? M.route_exc_dev[lo] : M.route_def[n];
}
__device__ __forceinline__ uint32_t route_at(const P2PDev &M, uint32_t n, uint32_t slot) {
  if (slot == 0xffffffffu) return 0xffffffffu;
  if (M.route) return M.route[(uint64_t)n * M.n_dst + slot];
  return route_compressed(mdev_of(M.C), n, slot);
}
// ... towards the packet's destination.
__device__ __forceinline__ uint32_t route_of(const P2PDev &M, uint32_t n, const Pkt &p) {
  return route_at(M, n, pkt_dst_slot(M, p));
}

// ---------------- UdpTraceClient (NSGPU_APP_UDP_TRACE_CLIENT: ports mode, the extended handlers) ----------------
// udp-trace-client.cc.  One Send event (:311-335) emits a burst: starting at m_currentEntry, every entry up to the next
// one whose timeToSend is not 0, each as packetSize / MaxPacketSize datagrams of MaxPacketSize and one of the remainder
// (also when that is 0: SendPacket (0) is the 12-byte SeqTsHeader alone, :265-283).  The sender's node part (tc_send)
// walks the burst once for the node and application state — one route lookup, then per datagram what a UdpClient's
// send does — and hands the device step one descriptor that stands for the whole burst: {flow, the first datagram's
// identification, TC_BURST | the first entry, TTL | the first sequence number << 8}.  The device step walks the
// entries again by the same rule (tc_step) and runs the single-packet step once per datagram, so no event, uid or
// child is made beyond a single send's.
// The entries lie behind app_pkt_size — [n_apps] MaxPacketSize and the others' sizes, then [n_apps + 1] offsets, then
// the entries as (timeToSend ms, packetSize) pairs — and m_currentEntry and the Send events run behind app_tot
// ([n_apps] m_sent, [n_apps] m_currentEntry, [n_apps] sends); both only in an engine with a trace client.  P2PDev
// takes no further pointer (see hub_slot).
constexpr uint32_t TC_BURST = 0x80000000u;   // Act::p.size of a burst descriptor: the flag | the burst's first entry
constexpr uint32_t TC_SEQ_LIMIT = 1u << 24;  // the descriptor's sequence field
constexpr uint32_t ERR_TRACE_SEQ = 32768u;   // the engine's error bit: a trace client's m_sent would pass 2^24
__device__ __forceinline__ bool is_burst_send(uint32_t op, uint32_t size) { return op == ACT_SEND && (size & TC_BURST); }
__host__ __device__ __forceinline__ const uint32_t *tc_offsets(const uint32_t *app_pkt_size, uint32_t n_apps) {
  return app_pkt_size + n_apps;
}
__host__ __device__ __forceinline__ const uint32_t *tc_entries(const uint32_t *app_pkt_size, uint32_t n_apps) {
  return app_pkt_size + 2 * (size_t)n_apps + 1;
}
// SendPacket (size) (:265-309): the datagram's IPv4 length — Create<Packet> (size - 12) or (0), the SeqTsHeader, UDP, IPv4.
__host__ __device__ __forceinline__ uint32_t tc_ip_size(uint32_t size) { return (size > 12u ? size : 12u) + 8u + 20u; }
// What the sender's node part needs of a Send: the output device (0xffffffff: no route, nothing left the socket), the
// burst's first entry, identification and sequence number, its SendPacket calls, the next Send's delay.
struct TcSend {
  uint32_t out, e0, ipid0, seq0, n, pad;
  int64_t delay;
};
// UdpTraceClient::Send, the node and application side.  Inlined into the node part, which is itself out of line where
// the handlers split it (node_part_cold): a function of its own between that one and fm_first_tx / route_compressed
// made the call chain one frame deeper, 16 B of scratch a lane in every extended handler.
__device__ __forceinline__ TcSend tc_send(const P2PDev &M, uint32_t a, uint64_t now, uint32_t uid) {
  const P2PDev *G = mdev_of(M.C);
  const uint32_t A = M.n_apps, mps = M.app_pkt_size[a];
  const uint32_t base = tc_offsets(M.app_pkt_size, A)[a], cnt = tc_offsets(M.app_pkt_size, A)[a + 1] - base;
  const uint32_t *T = tc_entries(M.app_pkt_size, A) + 2 * (size_t)base;
  const uint32_t an = M.app_node[a];
  const uint32_t e0 = M.app_tot[A + a], seq0 = M.app_tot[a];
  const uint32_t ttl = M.app_ttl[a];
  const uint32_t idm = M.frag ? 0xffffu : 0xffffffffu;
  // m_socket->Send (p): -1 with no route (udp-socket-impl.cc:595-601), for every datagram of the burst alike
  const uint32_t out = route_at(M, an, M.app_dst_slot[a]);
  const uint32_t ipid0 = M.node_ipid[an];
  uint32_t e = e0, n = 0;
  uint64_t bytes = 0;
  do {  // :319-333
    const uint32_t ps = T[2 * e + 1], nfull = ps / mps;
    for (uint32_t i = 0; i <= nfull; i++) {  // SendPacket (m_maxPacketSize) x nfull, SendPacket (packetSize % m_maxPacketSize)
      const uint32_t ipsz = tc_ip_size(i < nfull ? mps : ps % mps);
      if (out != 0xffffffffu) {
        bytes += ipsz - 28u;
        if (M.flowmon)  // m_sendOutgoingTrace (ipv4-l3-protocol.cc:618), per datagram with its own size
          fm_first_tx(G, Pkt{a, (ipid0 + n) & idm, ipsz, ttl | ((seq0 + n) << 8)}, now, uid);
      }
      n++;
    }
    e = e + 1 == cnt ? 0u : e + 1;  // m_currentEntry++; m_currentEntry %= m_entries.size ()
  } while (T[2 * e] == 0);
  M.app_tot[A + a] = e;
  M.app_tot[2 * A + a]++;
  if (out != 0xffffffffu) {  // ++m_sent only when Send returned >= 0; BuildHeader: m_identification++ per datagram
    if (seq0 + n > TC_SEQ_LIMIT) atomicOr(M.error, ERR_TRACE_SEQ);
    M.app_tot[a] = seq0 + n;
    M.node_ipid[an] = ipid0 + n;
    M.appc[a].tx_packets += n;
    M.appc[a].tx_bytes += bytes;
  }
  // Simulator::Schedule (MilliSeconds (entry->timeToSend), &UdpTraceClient::Send, this) (:334)
  return TcSend{out, e0, ipid0, seq0, n, 0, (int64_t)T[2 * e] * 1000000ll};
}
// The device step's walk over a burst: the datagram at (entry e, index i in the entry's frame), the k-th of the burst,
// and the position after it; more: another datagram follows.  Out of line: the handlers hold a call, not the walk.
struct TcStep {
  Pkt p;
  uint32_t e, i, more;
};
__device__ __noinline__ TcStep tc_step(const P2PDev *G, uint32_t a, uint32_t e, uint32_t i, uint32_t k, uint32_t ipid0,
                                       uint32_t ttlw) {
  const P2PDev &M = mdev_ref(G);
  const uint32_t A = M.n_apps, mps = M.app_pkt_size[a];
  const uint32_t base = tc_offsets(M.app_pkt_size, A)[a], cnt = tc_offsets(M.app_pkt_size, A)[a + 1] - base;
  const uint32_t *T = tc_entries(M.app_pkt_size, A) + 2 * (size_t)base;
  const uint32_t ps = T[2 * e + 1], nfull = ps / mps;
  const uint32_t idm = M.frag ? 0xffffu : 0xffffffffu;
  TcStep s;
  s.p = Pkt{a, (ipid0 + k) & idm, tc_ip_size(i < nfull ? mps : ps % mps), ttlw + (k << 8)};
  if (i < nfull) {
    s.e = e, s.i = i + 1, s.more = 1;
  } else {
    s.e = e + 1 == cnt ? 0u : e + 1;
    s.i = 0;
    s.more = T[2 * s.e] == 0 ? 1u : 0u;
  }
  return s;
}

// Icmpv4L4Protocol::SendMessage (icmpv4-l4-protocol.cc:85-129): RouteOutput towards the error's
// destination, then Ipv4L3Protocol::Send from node n (its m_identification++); no route: dropped.
__device__ __forceinline__ Act icmp_act(const P2PDev &M, uint32_t n, Pkt e, HStat &hs) {
  const uint32_t out = route_of(M, n, e);
  if (out == 0xffffffffu) {
    hs.no_route++;
    return Act{ACT_NONE, 0, Pkt{0, 0, 0, 0}};
  }
  e.ipid |= M.node_ipid[n]++ & 0xffffu;
  hs.icmp++;
  return Act{ACT_SEND, out, e};
}

// One event: the kind-specific first phase (node part: node and application state, its own children),
// then the device step, then a trailing child.  The node part never reads device queue / tx state and
// the device step never reads node state, so a hub node's events can run them in two passes.
struct NodeOut {
  Act act;
  Post post;
  bool cancelled;
  uint32_t xdrop;  // forwarding device + 1 of a TTL-expired datagram whose time-exceeded error is act:
                   // its Drop record follows the device step (0: none)
};
// A Receive's addressing (pkt_dst_node, pkt_dst_slot), loaded ahead of the event by its caller.
struct DstHint {
  bool valid;
  uint32_t node, slot;
};
// rx_atomic: the device's rx counter is added with an atomic (hub blocks: other lanes add to it too;
// holders: a no-return atomic, so the event does not wait for the counter's line).
// The whole node part, every kind.  It is compiled once per translation unit, inside node_part_cold (out of line);
// the handlers inline node_part below, which runs the common kinds itself.  resumed: the event is a Receive whose
// first steps (the rx counter, the error model, the two Rx trace calls) node_part has already taken.
template <bool PORTS = false>
__device__ __forceinline__ NodeOut node_part_full(const P2PDev &M, Emit &E, uint32_t kind_word, uint32_t a,
                                                  const Pkt &pkt, int32_t sink, HStat &hs, bool rx_atomic, bool resumed,
                                                  DstHint hint = DstHint{false, 0, 0}) {
  const uint32_t kind = kind_word & 0xffu;
  const uint32_t gen = kind_word >> 8;
  Act act{ACT_NONE, 0, Pkt{0, 0, 0, 0}};
  Post post{false, 0, 0, 0};
  bool cancelled = false;
  uint32_t xdrop = 0;
  // (a frag scenario's senders write the header's 16-bit identification: the upper half is the fragment's)
  const uint32_t idm = (PORTS && M.frag) ? 0xffffu : 0xffffffffu;
  if (kind == K_RECEIVE) {  // PointToPointNetDevice::Receive -> Ipv4L3Protocol::Receive (ipv4-l3-protocol.cc:434-537)
    Pkt p = pkt;
    p.size -= 2;  // ProcessHeader strips the PppHeader
    if (!resumed) {
      if (rx_atomic) atomicAdd(&M.dev[a].c.rx_packets, 1u);
      else M.dev[a].c.rx_packets++;
      // m_receiveErrorModel->IsCorrupt (packet): m_phyRxDropTrace and nothing else (no sink hooks it)
      if constexpr (PORTS) {
        const uint32_t em = M.errm ? M.dev[a].em : 0u;
        if (em && em_is_corrupt(M.dev, M.n_devices, em, pkt.size)) return NodeOut{act, post, cancelled, xdrop};
      }
      trace_call(M, E, NSGPU_TR_RX, a, p);     // m_macRxTrace
      trace_call(M, E, NSGPU_TR_IP_RX, a, p);  // Ipv4L3Protocol::Receive: m_rxTrace (:455)
    }
    // the receiving node: the context ScheduleWithContext gave the Receive (point-to-point-channel.cc:100)
    const uint32_t n = E.ctx < M.n_nodes ? E.ctx : M.dev_node[a];
    const bool reply = (p.app & NSGPU_PKT_REPLY) != 0;
    const uint32_t fa = p.app & ~NSGPU_PKT_REPLY;
    if ((hint.valid ? hint.node : pkt_dst_node(M, p)) == n) {
      // LocalDeliver -> UdpL4Protocol::Receive (udp-l4-protocol.cc:312-407): the bound endpoint is the
      // client's own socket for an echo reply, else the node's PacketSink / UdpEchoServer.  An ICMP error
      // ends in Icmpv4L4Protocol::Receive -> UdpL4Protocol::ReceiveIcmp (no event, no counter).
      if constexpr (PORTS) {  // m_localDeliverTrace (:861): a datagram no endpoint takes counts as received too
        if (fm_on(M, p)) fm_last_rx(mdev_of(M.C), p, E.now);
      }
      int32_t k = reply ? (int32_t)fa : sink;
      // (per flow: not for an ICMP error, whose word holds flag bits above the flow and finds no endpoint anyway)
      if (PORTS && !reply && sink == EP_BY_FLOW)
        k = (p.app & NSGPU_PKT_ICMP) ? -1 : ep_of_flow(M, p.app & NSGPU_PKT_APP);
      // LocalDeliver (:849-859): a fragment (MF set or offset != 0) goes through ProcessFragment first; the datagram
      // that is entire goes on, and `ip`, the header UdpL4Protocol::Receive and SendDestUnreachPort see, stays the
      // arrived fragment's
      const Pkt ip = p;
      bool held = false;
      if (PORTS && M.frag && !(p.app & NSGPU_PKT_ICMP) && (p.ipid >> NSGPU_PKT_FRAG_SHIFT) != 0) {
        const uint32_t fi = M.node_ipid[M.n_nodes + n];
        if (fi == NOFRAG) {  // (create gives every destination of a fragmenting flow its state)
          atomicOr(M.error, ERR_FRAG_STATE);
          held = true;
        } else {
          const FragRx r = frag_receive(frag_nodes(M.node_ipid, M.n_nodes) + fi, M.error, p, a);
          if (r.flags & 1u)  // Simulator::Schedule (m_fragmentExpirationTimeout, HandleFragmentsTimeout)
            E.child(frag_hdr(M.node_ipid, M.n_nodes)->timeout, E.ctx, K_FRAG_TIMEOUT | (r.gen << 8), n, Pkt{0, 0, 0, 0});
          held = !(r.flags & 2u);
          p = r.p;
        }
      }
      if (p.app & NSGPU_PKT_ICMP) {
      } else if (PORTS && held) {
      } else if (k < 0 || !(M.app_flags[k] & 2u)) {  // no bound endpoint: RX_ENDPOINT_UNREACH
        hs.unreach++;
        if (M.icmp) act = icmp_act(M, n, icmp_error(ip, true), hs);  // SendDestUnreachPort (ip, copy)
      } else {
        // Ipv4EndPoint::ForwardUp: ScheduleNow (&Ipv4EndPoint::DoForwardUp) (ipv4-end-point.cc:112-120);
        // run inline for a PacketSink, queued for the echo applications (their HandleRead schedules)
        const bool q = reply || M.app_kind[k] == NSGPU_APP_ECHO_SERVER;
        E.child(0, E.ctx, q ? K_FWD_UP_Q : K_FWD_UP, (uint32_t)k, p);
      }
    } else {
      const uint32_t out = hint.valid ? route_at(M, n, hint.slot) : route_of(M, n, p);
      if (out == 0xffffffffu) {
        hs.no_route++;
        trace_ip_drop(M, E, a, p);  // DROP_NO_ROUTE
        if constexpr (PORTS) {
          if (fm_on(M, p)) fm_drop(mdev_of(M.C), p, NSGPU_FLOW_DROP_NO_ROUTE);
        }
      } else {
        p.ttl -= 1;  // IpForward (:815-841)
        if constexpr (PORTS) {  // m_dropTrace (:835, with or without an ICMP error) or m_unicastForwardTrace (:838)
          if (fm_on(M, p)) {
            if ((p.ttl & 0xffu) == 0) fm_drop(mdev_of(M.C), p, NSGPU_FLOW_DROP_TTL_EXPIRE);
            else fm_forward(mdev_of(M.C), p, E.now);
          }
        }
        if ((p.ttl & 0xffu) == 0) {
          hs.ttl_drops++;  // (no ICMP about an ICMP message)
          if (M.icmp && !(p.app & NSGPU_PKT_ICMP)) act = icmp_act(M, n, icmp_error(p, false), hs);
          if (act.op == ACT_SEND) {
            xdrop = out + 1;
          } else {
            p.ttl += 1;
            trace_ip_drop(M, E, out, p);  // DROP_TTL_EXPIRED (:835: on the forwarding route's interface)
          }
        } else {
          act = Act{ACT_SEND, out, p};
        }
      }
    }
  } else if (kind == K_TX_COMPLETE) {
    act = Act{ACT_KICK, a, Pkt{0, 0, 0, 0}};
  } else if (kind == K_SEND) {  // OnOffApplication::SendPacket (onoff-application.cc:254-270)
    const uint32_t f = M.app_flags[a];
    if (!((f & 4u) && M.app_send_gen[a] == gen)) {
      cancelled = true;
    } else if (M.app_kind[a] == NSGPU_APP_ECHO_CLIENT) {  // UdpEchoClient::Send (udp-echo-client.cc)
      M.app_flags[a] = f & ~4u;
      const uint32_t sz = M.app_pkt_size[a];
      Pkt p{a, 0, sz + 8 + 20, M.app_ttl[a]};
      M.appc[a].tx_packets++;
      M.appc[a].tx_bytes += sz;
      const uint32_t an = M.app_node[a];
      const uint32_t out = route_of(M, an, p);  // m_socket->Send (p)
      if (out == 0xffffffffu) {
        hs.no_route++;
      } else {
        p.ipid = M.node_ipid[an]++ & idm;
        act = Act{ACT_SEND, out, p};
        if constexpr (PORTS) {  // m_sendOutgoingTrace (:618)
          if (M.flowmon) fm_first_tx(mdev_of(M.C), p, E.now, E.uid);
        }
      }
      const uint32_t sent = ++M.app_tot[a];  // ++m_sent
      if (sent < M.app_count[a]) {           // ScheduleTransmit (m_interval)
        const uint32_t g = (M.app_send_gen[a] + 1) & 0xffffffu;
        M.app_send_gen[a] = g;
        M.app_flags[a] |= 4u;
        post = Post{true, M.app_interval[a], K_SEND | (g << 8), a};
      }
    } else if (PORTS && M.app_kind[a] == NSGPU_APP_UDP_CLIENT) {  // UdpClient::Send (udp-client.cc:148-187)
      M.app_flags[a] = f & ~4u;
      const uint32_t sz = M.app_pkt_size[a];  // Create<Packet> (m_size - 12) + SeqTsHeader
      uint32_t sent = M.app_tot[a];           // seqTs.SetSeq (m_sent)
      Pkt p{a, 0, sz + 8 + 20, M.app_ttl[a] | (sent << 8)};
      const uint32_t an = M.app_node[a];
      const uint32_t out = route_of(M, an, p);  // m_socket->Send (p): -1 with no route (udp-socket-impl.cc:595-601)
      if (out == 0xffffffffu) {
        hs.no_route++;
      } else {  // ++m_sent only when Send returned >= 0
        p.ipid = M.node_ipid[an]++ & idm;
        act = Act{ACT_SEND, out, p};
        if constexpr (PORTS) {  // m_sendOutgoingTrace (:618)
          if (M.flowmon) fm_first_tx(mdev_of(M.C), p, E.now, E.uid);
        }
        M.app_tot[a] = ++sent;
        M.appc[a].tx_packets++;
        M.appc[a].tx_bytes += sz;
      }
      if (sent < M.app_count[a]) {  // Schedule (m_interval, &UdpClient::Send)
        const uint32_t g = (M.app_send_gen[a] + 1) & 0xffffffu;
        M.app_send_gen[a] = g;
        M.app_flags[a] |= 4u;
        post = Post{true, M.app_interval[a], K_SEND | (g << 8), a};
      }
    } else if (PORTS && M.app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT) {  // UdpTraceClient::Send (udp-trace-client.cc:311-335)
      M.app_flags[a] = f & ~4u;
      const TcSend t = tc_send(M, a, E.now, E.uid);
      if (t.out == 0xffffffffu) hs.no_route += t.n;  // (every SendPacket's Send failed: m_sent stays)
      else act = Act{ACT_SEND, t.out, Pkt{a, t.ipid0, TC_BURST | t.e0, M.app_ttl[a] | (t.seq0 << 8)}};
      const uint32_t g = (M.app_send_gen[a] + 1) & 0xffffffu;
      M.app_send_gen[a] = g;
      M.app_flags[a] |= 4u;
      post = Post{true, t.delay, K_SEND | (g << 8), a};
    } else {
      M.app_flags[a] = f & ~4u;
      const uint32_t sz = M.app_pkt_size[a];
      Pkt p{a, 0, sz + 8 + 20, M.app_ttl[a]};
      M.appc[a].tx_packets++;
      M.appc[a].tx_bytes += sz;
      const uint32_t an = M.app_node[a];
      const uint32_t out = route_of(M, an, p);  // UdpSocketImpl::DoSendTo: RouteOutput
      if (out == 0xffffffffu) {
        hs.no_route++;
      } else {
        p.ipid = M.node_ipid[an]++ & idm;  // Ipv4L3Protocol::BuildHeader: SetIdentification (m_identification++)
        act = Act{ACT_SEND, out, p};
        if constexpr (PORTS) {  // m_sendOutgoingTrace (:618)
          if (M.flowmon) fm_first_tx(mdev_of(M.C), p, E.now, E.uid);
        }
      }
      M.app_tot[a] += sz;
      M.app_last_start[a] = E.now;
      M.app_residual[a] = 0;
      post = schedule_next_tx(M, a, E.now);
    }
  } else {
    switch (kind) {
      case K_NODE_START:
        for (uint32_t i = M.node_app_off[a]; i < M.node_app_off[a + 1]; i++) appobj_start(M, E, M.node_app_list[i]);
        break;
      case K_APPOBJ_START:
        appobj_start(M, E, a);
        break;
      case K_APP_START:
        if (M.app_kind[a] == NSGPU_APP_SINK || M.app_kind[a] == NSGPU_APP_ECHO_SERVER) {  // Bind (port)
          M.app_flags[a] |= 2u;
        } else if (M.app_kind[a] == NSGPU_APP_ECHO_CLIENT) {
          // UdpEchoClient::StartApplication: Bind, Connect, SetRecvCallback, ScheduleTransmit (Seconds (0))
          const uint32_t g = (M.app_send_gen[a] + 1) & 0xffffffu;
          M.app_send_gen[a] = g;
          M.app_flags[a] |= 2u | 4u;
          E.child(0, E.ctx, K_SEND | (g << 8), a, Pkt{0, 0, 0, 0});
        } else if (PORTS && M.app_kind[a] == NSGPU_APP_UDP_SERVER) {  // Bind (Any, port); SetRecvCallback (HandleRead)
          M.app_flags[a] = (M.app_flags[a] | AF_BOUND | AF_UDP_SERVER) & ~AF_RX_CLEARED;
        } else if (PORTS && (M.app_kind[a] == NSGPU_APP_UDP_CLIENT || M.app_kind[a] == NSGPU_APP_UDP_TRACE_CLIENT)) {
          // UdpTraceClient::StartApplication (udp-trace-client.cc:234-256) does the same.
          // UdpClient::StartApplication: Bind, Connect, SetRecvCallback (null), Schedule (Seconds (0), Send) — its
          // ephemeral-port socket is no endpoint any flow of this subset addresses (bit 1 stays clear)
          const uint32_t g = (M.app_send_gen[a] + 1) & 0xffffffu;
          M.app_send_gen[a] = g;
          M.app_flags[a] |= 4u;
          E.child(0, E.ctx, K_SEND | (g << 8), a, Pkt{0, 0, 0, 0});
        } else {
          cancel_events(M, a, E.now);
          schedule_start_event<PORTS>(M, E, a);
        }
        break;
      case K_APP_STOP:
        stop_application<PORTS>(M, a, E.now);
        break;
      case K_START_SENDING: {  // onoff-application.cc:196-206
        const uint32_t f = M.app_flags[a];
        if (!((f & 8u) && M.app_ss_gen[a] == gen)) {
          cancelled = true;
          break;
        }
        M.app_flags[a] = f & ~8u;
        M.app_last_start[a] = E.now;
        post = schedule_next_tx(M, a, E.now);
        if (post.valid) E.child(post.delay, E.ctx, post.kind, post.a, Pkt{0, 0, 0, 0});
        post.valid = false;
        schedule_stop_event<PORTS>(M, E, a);
        break;
      }
      case K_STOP_SENDING: {  // onoff-application.cc:208-216
        const uint32_t f = M.app_flags[a];
        if (!((f & 8u) && M.app_ss_gen[a] == gen)) {
          cancelled = true;
          break;
        }
        M.app_flags[a] = f & ~8u;
        cancel_events(M, a, E.now);
        schedule_start_event<PORTS>(M, E, a);
        break;
      }
      case K_FWD_UP:  // DoForwardUp -> UdpSocketImpl::ForwardUp -> PacketSink::HandleRead (a = sink app)
      case K_FWD_UP_D:
        fwd_up_leaf<PORTS>(M, a, &pkt);
        break;
      case K_FWD_UP_Q:  // DoForwardUp -> UdpSocketImpl::ForwardUp -> UdpEcho{Server,Client}::HandleRead (a = endpoint app)
        if (M.app_flags[a] & 2u) {
          M.appc[a].rx_packets++;
          M.appc[a].rx_bytes += pkt.size - 28;
          if (M.app_kind[a] == NSGPU_APP_ECHO_SERVER) {  // socket->SendTo (packet, 0, from)
            Pkt r{pkt.app | NSGPU_PKT_REPLY, 0, pkt.size, M.app_ttl[a]};
            M.appc[a].tx_packets++;
            M.appc[a].tx_bytes += pkt.size - 28;
            const uint32_t an = M.app_node[a];
            const uint32_t out = route_of(M, an, r);
            if (out == 0xffffffffu) {
              hs.no_route++;
            } else {
              r.ipid = M.node_ipid[an]++ & idm;
              act = Act{ACT_SEND, out, r};
              if constexpr (PORTS) {  // m_sendOutgoingTrace (:618)
                if (M.flowmon) fm_first_tx(mdev_of(M.C), r, E.now, E.uid);
              }
            }
          }
        }
        break;
      case K_STOP:
        hs.stop = true;
        break;
      case K_FRAG_TIMEOUT:  // Ipv4L3Protocol::HandleFragmentsTimeout (:1391-1412), a = the node
        if (PORTS && M.frag) {
          FragNode *F = frag_nodes(M.node_ipid, M.n_nodes) + M.node_ipid[M.n_nodes + a];
          if (!F->live || F->gen != gen) {  // cancelled when its datagram was entire: dispatched, counted
            cancelled = true;
            F->cancelled++;
            break;
          }
          const uint32_t part = frag_partial_size(F);
          const Pkt ip = F->hdr;
          const uint32_t iif = F->iif;
          F->timeouts++;
          F->live = 0;
          F->n = 0;
          // more than 8 bytes: SendTimeExceededTtl (ipHeader, packet), to the captured header's source
          if (part > 8 && M.icmp) act = icmp_act(M, a, icmp_error(ip, false), hs);
          // m_dropTrace (ipHeader, packet, DROP_FRAGMENT_TIMEOUT, .., iif), after the error's Send: the captured
          // header's fields — flow, identification, length, TTL (the packet is the partial one: no sequence number)
          if (act.op == ACT_SEND) xdrop = (iif + 1) | XDROP_FRAG;
          else trace_ip_drop(M, E, iif, Pkt{ip.app, ip.ipid, ip.size, ip.ttl & 0xffu});
        }
        break;
      default:  // K_DEV_START: no-op
        break;
    }
  }
  return NodeOut{act, post, cancelled, xdrop};
}
// What node_part_cold hands back, in registers (a function's result travels in at most 16, and a reference to the
// caller's Emit would keep that in scratch): the NodeOut (the trailing child as in HubEv: pkind == 0, none), the
// event's children and trace calls so far, and what the event added to the HStat, four bits a counter.
struct ColdOut {
  uint32_t op, dev;
  Pkt p;
  int64_t pdelay;
  uint32_t pkind, pa;
  uint32_t xdrop, n, trseq;
  uint32_t stat;  // ttl_drops | no_route << 4 | unreach << 8 | icmp << 12 | stop << 16 | cancelled << 17 (| no_route >> 4 << 18)
};
static_assert(sizeof(ColdOut) <= 64, "ColdOut is returned in registers");
enum : uint32_t { CF_TLOC = 1, CF_DEMOTE = 2, CF_RX_ATOMIC = 4, CF_RESUMED = 8 };
// The node part of an event node_part does not run itself, out of line and against the device-resident descriptor G
// (cold paths, above).  The event's Emit is rebuilt from its scalars; the children are written where the caller's
// would write them, and the caller folds them into its minima (Emit::adopt).
template <bool PORTS>
__device__ __noinline__ ColdOut node_part_cold(const P2PDev *G, uint64_t now, uint32_t ctx, uint32_t slot0, uint32_t n,
                                               uint32_t uid, uint32_t trseq, uint32_t flags, uint32_t kind_word,
                                               uint32_t a, Pkt pkt, int32_t sink) {
  const P2PDev &M = mdev_ref(G);
  Emit E;
  E.now = now;
  E.ctx = ctx;
  E.slot0 = slot0;
  E.n = n;
  E.ch_ts = M.ch_ts;
  E.ch_ctx = M.ch_ctx;
  E.ch_kind = M.ch_kind;
  E.ch_a = M.ch_a;
  E.ch_pkt = M.ch_pkt;
  E.lookahead = M.lookahead;
  E.lookw = nullptr;
  E.tmn = E.wnd = E.wndw = ~0ull;
  E.lim_abs = 0;
  E.uid = uid;
  E.tloc = (flags & CF_TLOC) != 0;
  E.trseq = trseq;
  E.demote = (flags & CF_DEMOTE) != 0;
  E.lj = -1;
  HStat hs{0, 0, 0, 0, 0, false};
  const NodeOut o = node_part_full<PORTS>(M, E, kind_word, a, pkt, sink, hs, (flags & CF_RX_ATOMIC) != 0,
                                          (flags & CF_RESUMED) != 0);
  // (PORTS: a trace client's burst without a route counts one no_route a datagram, beyond four bits: the rest above bit 18)
  const uint32_t nr = PORTS ? ((hs.no_route & 15u) << 4) | ((hs.no_route >> 4) << 18) : hs.no_route << 4;
  return ColdOut{o.act.op, o.act.dev, o.act.p, o.post.delay, o.post.valid ? o.post.kind : 0u, o.post.a, o.xdrop, E.n,
                 E.trseq, hs.ttl_drops | nr | (hs.unreach << 8) | (hs.icmp << 12) |
                              ((hs.stop ? 1u : 0u) << 16) | ((o.cancelled ? 1u : 0u) << 17)};
}
// The node part as the handlers inline it: a TransmitComplete, and a Receive that is forwarded (route found, TTL
// alive) or delivered to the node's bound PacketSink, run here; every other kind, and a Receive that ends any other
// way (no route, TTL expiry, no endpoint, an echo application, an ICMP error, a fragment), goes to node_part_cold.
// The order of an event's side effects is node_part_full's: a Receive's first steps are the same statements, and the
// cold function continues after them (CF_RESUMED).
// SPLIT = false (the narrow kernel's holders and hub blocks): the whole node part inline, as before.  The dumbbell,
// which runs that kernel and whose events are one quarter Sends and application starts, lost 0.6-1.3 % with the split
// (DESIGN.md 4.4, r15).
template <bool PORTS = false, bool SPLIT = true>
__device__ __forceinline__ NodeOut node_part(const P2PDev &M, Emit &E, uint32_t kind_word, uint32_t a,
                                             const Pkt &pkt, int32_t sink, HStat &hs, bool rx_atomic = false,
                                             DstHint hint = DstHint{false, 0, 0}) {
  if constexpr (!SPLIT) return node_part_full<PORTS>(M, E, kind_word, a, pkt, sink, hs, rx_atomic, false, hint);
  const uint32_t kind = kind_word & 0xffu;
  const Act noact{ACT_NONE, 0, Pkt{0, 0, 0, 0}};
  const Post nopost{false, 0, 0, 0};
  if (kind == K_TX_COMPLETE) return NodeOut{Act{ACT_KICK, a, Pkt{0, 0, 0, 0}}, nopost, false, 0};
  uint32_t flags = (E.tloc ? CF_TLOC : 0u) | (E.demote ? CF_DEMOTE : 0u) | (rx_atomic ? CF_RX_ATOMIC : 0u);
  if (kind == K_RECEIVE) {  // PointToPointNetDevice::Receive -> Ipv4L3Protocol::Receive (ipv4-l3-protocol.cc:434-537)
    if (rx_atomic) atomicAdd(&M.dev[a].c.rx_packets, 1u);
    else M.dev[a].c.rx_packets++;
    if constexpr (PORTS) {
      const uint32_t em = M.errm ? M.dev[a].em : 0u;
      if (em && em_is_corrupt(M.dev, M.n_devices, em, pkt.size)) return NodeOut{noact, nopost, false, 0};
    }
    Pkt p = pkt;
    p.size -= 2;                             // ProcessHeader strips the PppHeader
    trace_call(M, E, NSGPU_TR_RX, a, p);     // m_macRxTrace
    trace_call(M, E, NSGPU_TR_IP_RX, a, p);  // Ipv4L3Protocol::Receive: m_rxTrace (:455)
    const uint32_t n = E.ctx < M.n_nodes ? E.ctx : M.dev_node[a];
    if ((hint.valid ? hint.node : pkt_dst_node(M, p)) == n) {
      // LocalDeliver of a whole UDP datagram to the node's PacketSink: ForwardUp, run inline
      bool plain = !(p.app & (NSGPU_PKT_REPLY | NSGPU_PKT_ICMP)) && sink >= 0;
      if constexpr (PORTS) plain = plain && !(M.frag && (p.ipid >> NSGPU_PKT_FRAG_SHIFT) != 0);
      if (plain && (M.app_flags[sink] & 2u) && M.app_kind[sink] != NSGPU_APP_ECHO_SERVER) {
        if constexpr (PORTS) {  // m_localDeliverTrace (:861); every other delivery: node_part_full's
          if (M.flowmon) fm_last_rx(mdev_of(M.C), p, E.now);
        }
        E.child(0, E.ctx, K_FWD_UP, (uint32_t)sink, p);
        return NodeOut{noact, nopost, false, 0};
      }
    } else {
      const uint32_t out = hint.valid ? route_at(M, n, hint.slot) : route_of(M, n, p);
      if (out != 0xffffffffu && ((p.ttl - 1u) & 0xffu) != 0) {  // IpForward (:815-841)
        p.ttl -= 1;
        if constexpr (PORTS) {  // m_unicastForwardTrace (:838); a drop instead: node_part_full's
          if (fm_on(M, p)) fm_forward(mdev_of(M.C), p, E.now);
        }
        return NodeOut{Act{ACT_SEND, out, p}, nopost, false, 0};
      }
    }
    flags |= CF_RESUMED;
  }
  const ColdOut o = node_part_cold<PORTS>(mdev_of(M.C), E.now, E.ctx, E.slot0, E.n, E.uid, E.trseq, flags, kind_word, a,
                                          pkt, sink);
  E.adopt(o.n);
  E.trseq = o.trseq;
  hs.ttl_drops += o.stat & 15u;
  hs.no_route += (o.stat >> 4) & 15u;
  if constexpr (PORTS) hs.no_route += (o.stat >> 18) << 4;
  hs.unreach += (o.stat >> 8) & 15u;
  hs.icmp += (o.stat >> 12) & 15u;
  if (o.stat & (1u << 16)) hs.stop = true;
  return NodeOut{Act{o.op, o.dev, o.p}, Post{o.pkind != 0, o.pdelay, o.pkind, o.pa}, ((o.stat >> 17) & 1u) != 0, o.xdrop};
}
__device__ __forceinline__ bool run_event(const P2PDev &M, Emit &E, uint32_t kind_word, uint32_t a, const Pkt &pkt,
                                          int32_t sink, HStat &hs) {
  const NodeOut o = node_part(M, E, kind_word, a, pkt, sink, hs);
  device_act(M, E, o.act);
  if (o.xdrop) trace_te_drop(M, E, o.xdrop - 1, o.act.p);
  if (o.post.valid) E.child(o.post.delay, E.ctx, o.post.kind, o.post.a, Pkt{0, 0, 0, 0});
  return o.cancelled;
}

// Diagnostic build (-DNSGPU_PHASE_PROF, lib/libnsgpu_prof.so only): thread 0 of block 0 of each
// pipeline kernel accumulates s_memrealtime (100 MHz) deltas between phase marks into g_phase.  The counters are
// nsgpu_p2p.hip's: the handlers-only translation unit (nsgpu_p2p_ports.hip) defines none and records no marks.
#if defined(NSGPU_PHASE_PROF) && defined(NSGPU_P2P_HANDLERS_ONLY)
#undef NSGPU_PHASE_PROF
#endif
#ifdef NSGPU_PHASE_PROF
__device__ uint64_t g_phase[64];
#define PH_BEGIN() uint64_t ph_t_ = (threadIdx.x == 0 && blockIdx.x == 0) ? __builtin_amdgcn_s_memrealtime() : 0
#define PH_MARK(i)                                                                      \
  do {                                                                                  \
    if (threadIdx.x == 0 && blockIdx.x == 0) {                                          \
      const uint64_t t_ = __builtin_amdgcn_s_memrealtime();                             \
      atomicAdd((unsigned long long *)&g_phase[i], (unsigned long long)(t_ - ph_t_));   \
      ph_t_ = t_;                                                                       \
    }                                                                                   \
  } while (0)
// hub blocks (k2_handle): thread 0 of every hub block adds its phase times into g_phase[24..27], calls in [28]
#define HUB_T0() uint64_t hub_t_ = threadIdx.x == 0 ? __builtin_amdgcn_s_memrealtime() : 0
#define HUB_MARK(i)                                                                     \
  do {                                                                                  \
    if (threadIdx.x == 0) {                                                             \
      const uint64_t t_ = __builtin_amdgcn_s_memrealtime();                             \
      atomicAdd((unsigned long long *)&g_phase[i], (unsigned long long)(t_ - hub_t_));  \
      hub_t_ = t_;                                                                      \
    }                                                                                   \
  } while (0)
#else
#define PH_BEGIN() (void)0
#define PH_MARK(i) (void)0
#define HUB_T0() (void)0
#define HUB_MARK(i) (void)0
#endif
// Per-block start / end times (s_memrealtime) of the window kernels in one sampled window
// (diagnostic build only): g_blk[kernel][block] = {start, end}, window g_blk_win.
#ifdef NSGPU_PHASE_PROF
constexpr int BLK_MAX = 2048;
__device__ uint64_t g_blk[3][BLK_MAX][2];
__device__ uint64_t g_blk_win = 1000;
#define BLK_T0() uint64_t bt0_ = __builtin_amdgcn_s_memrealtime(), btm_ = bt0_
// per-block phase mark in the sampled window: g_phase[i] += time since the block's previous mark
#define BLK_MARK(i, win)                                                                         \
  do {                                                                                           \
    if (threadIdx.x == 0 && (win) == g_blk_win) {                                                \
      const uint64_t t_ = __builtin_amdgcn_s_memrealtime();                                      \
      atomicAdd((unsigned long long *)&g_phase[i], (unsigned long long)(t_ - btm_));             \
      atomicAdd((unsigned long long *)&g_phase[(i) + 1], 1ull);                                  \
      btm_ = t_;                                                                                 \
    }                                                                                            \
  } while (0)
// k_gtile's per-block stamps in the sampled window: g_gt[block] = {start, prologue done, first tile in LDS,
// first tile compared, end (after its atomics returned)}
constexpr int GT_BLK_MAX = 8192;
__device__ uint64_t g_gt[GT_BLK_MAX][8];
#define BLK_REC(k, win)                                                                          \
  do {                                                                                           \
    if (threadIdx.x == 0 && (win) == g_blk_win && blockIdx.x < (uint32_t)BLK_MAX) {              \
      g_blk[k][blockIdx.x][0] = bt0_;                                                            \
      g_blk[k][blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();                                \
    }                                                                                            \
  } while (0)
// What the lanes of each of k2_handle's holder blocks ran in the sampled window: g_blkk[block] = {Receives, gen-0
// TransmitCompletes, local records, Sends, events of other kinds, the busiest lane's events, holder lanes}
// ... and where a lane's local record took its time: [8..12] = the block's slowest lane's shader-clock cycles
// (s_memtime) from the parent event's slot_done (HN_T(0)) to local_record's return (1), lq_push's (2), the record's
// pop at the loop's top (3), its own slot_done (4) and the loop's next top (5); a fused record (handle_node2) has
// marks 0, 1 and 4 only.  The last record a lane made counts.  [13] = the slowest lane's cycles in handle_node2
// (the scale of the others against the block's stamped duration).
constexpr int BLKK_MAX = 64, BLKK_N = 16;
__device__ uint32_t g_blkk[BLKK_MAX][BLKK_N];
#define BLK_KINDS_T0(C)              \
  uint32_t bk_[5] = {0, 0, 0, 0, 0}; \
  uint64_t hn_[6] = {0, 0, 0, 0, 0, 0}; \
  bool hn_open_ = false;             \
  const uint64_t hn_t0_ = __builtin_amdgcn_s_memtime(); \
  const uint64_t bkw_ = (C).windows
#define BLK_KINDS_EV(kind, local) \
  bk_[(local) ? 2 : (kind) == K_RECEIVE ? 0 : (kind) == K_TX_COMPLETE ? 1 : (kind) == K_SEND ? 3 : 4]++
#define HN_T(i) hn_[i] = __builtin_amdgcn_s_memtime()
#define HN_BEGIN()                                \
  do {                                            \
    for (int k_ = 1; k_ < 6; k_++) hn_[k_] = 0;   \
    hn_open_ = false;                             \
    HN_T(0);                                      \
  } while (0)
// (the loop's top after a queued record ran: mark 5, once)
#define HN_TOP()      \
  do {                \
    if (hn_open_) {   \
      HN_T(5);        \
      hn_open_ = false; \
    }                 \
  } while (0)
#define HN_RAN() hn_open_ = true
#define BLK_KINDS_REC(holder)                                                                    \
  do {                                                                                           \
    if (bkw_ == g_blk_win && blockIdx.x < (uint32_t)BLKK_MAX && (holder)) {                      \
      for (int k_ = 0; k_ < 5; k_++)                                                             \
        if (bk_[k_]) atomicAdd(&g_blkk[blockIdx.x][k_], bk_[k_]);                                \
      atomicMax(&g_blkk[blockIdx.x][5], bk_[0] + bk_[1] + bk_[2] + bk_[3] + bk_[4]);             \
      atomicAdd(&g_blkk[blockIdx.x][6], 1u);                                                     \
      for (int k_ = 1; k_ < 6; k_++) {                                                           \
        int p_ = k_ - 1;                                                                         \
        while (p_ > 0 && hn_[p_] == 0) p_--;                                                     \
        if (hn_[k_] > hn_[p_] && hn_[p_] != 0)                                                   \
          atomicMax(&g_blkk[blockIdx.x][7 + k_], (uint32_t)(hn_[k_] - hn_[p_]));                 \
      }                                                                                          \
      atomicMax(&g_blkk[blockIdx.x][13], (uint32_t)(__builtin_amdgcn_s_memtime() - hn_t0_));     \
    }                                                                                            \
  } while (0)
#else
#define BLK_T0() (void)0
#define BLK_REC(k, win) (void)0
#define BLK_MARK(i, win) (void)0
#define BLK_KINDS_T0(C) (void)0
#define BLK_KINDS_EV(kind, local) (void)0
#define BLK_KINDS_REC(holder)      (void)0
#define HN_T(i) (void)0
#define HN_BEGIN() (void)0
#define HN_TOP() (void)0
#define HN_RAN() (void)0
#endif

// ================================ window pipeline ================================
// Window bound of a pending set's reduction: packed key bound, span, Stop key.
struct WinBound {
  uint64_t tmin, span, bound, stop_packed;
  uint64_t nbound;  // the narrow bound (span = the narrow lookahead's)
  uint64_t lim;     // local records: a TransmitComplete child with rel ts < lim runs in the window (0: none)
};
// wide: wide windows — the span is span_t clamped between the narrow bound (min over
// pending of ts + lookahead) and the wide one (ts + lookw, nsgpu_p2p_create); a same-node TransmitComplete
// before the window's end then runs inside it (local record).
__device__ __forceinline__ WinBound window_bound(const Red &R, bool wide = false, uint64_t span_t = 0) {
  WinBound b;
  b.tmin = R.tmin;
  uint64_t span = R.wend - b.tmin;
  if (span > 0xfffffffeull) span = 0xfffffffeull;
  const uint64_t nspan = span;
  if (wide && R.tmin != ~0ull && R.wendw != ~0ull && R.wendw > R.wend) {
    uint64_t wspan = R.wendw - b.tmin;
    if (wspan > 0xfffffffeull) wspan = 0xfffffffeull;
    span = span_t < wspan ? span_t : wspan;
    span = span > nspan ? span : nspan;
  }
  b.span = span;
  b.bound = (span << 32) | 0xffffffffull;
  b.nbound = (nspan << 32) | 0xffffffffull;
  // a local child at the window's end could tie with a cross-node child there: strictly before it
  b.lim = span > nspan ? span : 0;
  b.stop_packed = ~0ull;
  if (R.stopts != ~0ull && R.stopts - b.tmin <= span) {
    // Stop caps the window at its own key (it is dispatched; later events are not); a child at the Stop's
    // ts sorts after it (a larger uid)
    b.stop_packed = ((R.stopts - b.tmin) << 32) | R.stopuid;
    b.bound = b.stop_packed < b.bound ? b.stop_packed : b.bound;
    b.nbound = b.stop_packed < b.nbound ? b.stop_packed : b.nbound;
    b.lim = (R.stopts - b.tmin) < b.lim ? (R.stopts - b.tmin) : b.lim;
  }
  return b;
}
__device__ __forceinline__ void publish_bound(Ctl &C, const WinBound &b) {
  C.tmin = b.tmin;
  C.bound = b.bound;
  C.nbound = b.nbound;
  C.lim_rel = b.lim;
  // zero-delay leaf children (Ipv4EndPoint::DoForwardUp) run inside the window; when the window ends
  // at the Stop event, those at the Stop's ts sort after it and are never dispatched
  const bool has_stop = b.stop_packed != ~0ull && b.bound >= b.stop_packed;
  C.inline_lim = has_stop ? (b.stop_packed >> 32) : ~0ull;
}

// Reduces (tmn, wnd) over the workgroup and one lane folds them into R (atomicMin): one atomic
// pair per workgroup, not per wave (a word takes ~11 ns per atomic).  All threads must call it.
// WIDE: the wide bound (wndw) as well.
template <int NTH, bool WIDE = false>
__device__ __forceinline__ void publish_min(Red &R, uint64_t tmn, uint64_t wnd, uint64_t wndw = ~0ull) {
  tmn = wave_min64(tmn);
  wnd = wave_min64(wnd);
  if constexpr (WIDE) wndw = wave_min64(wndw);
  if constexpr (NTH > 64) {
    __shared__ uint64_t s0[NTH / 64], s1[NTH / 64], s2[NTH / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
      s0[wid] = tmn;
      s1[wid] = wnd;
      if constexpr (WIDE) s2[wid] = wndw;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < NTH / 64; w++) {
      tmn = s0[w] < tmn ? s0[w] : tmn;
      wnd = s1[w] < wnd ? s1[w] : wnd;
      if constexpr (WIDE) wndw = s2[w] < wndw ? s2[w] : wndw;
    }
  } else if ((threadIdx.x & 63) != 0) {
    return;
  }
  if (tmn != ~0ull) atomicMin((unsigned long long *)&R.tmin, (unsigned long long)tmn);
  if (wnd != ~0ull) atomicMin((unsigned long long *)&R.wend, (unsigned long long)wnd);
  if (WIDE && wndw != ~0ull) atomicMin((unsigned long long *)&R.wendw, (unsigned long long)wndw);
}
// The deferred pipeline's publish_min: the same reduction (and the sum of the threads' packed child totals
// `tot`), then one lane stores the block's record *p with two 16-B stores, no atomics; a block with nothing to
// publish stores nothing.  merge: the block published before in this kernel (a hub block's next hub): folded into
// what it stored.  (tot: one-wave blocks only.)  All threads must call it.
template <int NTH>
__device__ __forceinline__ void publish_part(Part *p, uint64_t tmn, uint64_t wnd, uint64_t wndw, uint64_t tot = 0,
                                             bool merge = false) {
  tmn = wave_min64(tmn);
  wnd = wave_min64(wnd);
  wndw = wave_min64(wndw);
  if constexpr (NTH > 64) {
    __shared__ uint64_t s0[NTH / 64], s1[NTH / 64], s2[NTH / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
      s0[wid] = tmn;
      s1[wid] = wnd;
      s2[wid] = wndw;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < NTH / 64; w++) {
      tmn = s0[w] < tmn ? s0[w] : tmn;
      wnd = s1[w] < wnd ? s1[w] : wnd;
      wndw = s2[w] < wndw ? s2[w] : wndw;
    }
  } else {
    tot = wave_sum64(tot);
    if ((threadIdx.x & 63) != 0) return;
  }
  if ((tmn & wnd & wndw) == ~0ull && tot == 0) return;
  ulonglong2 *q = reinterpret_cast<ulonglong2 *>(p);
  if (merge) {
    const ulonglong2 a = q[0], b = q[1];
    tmn = a.x < tmn ? a.x : tmn;
    wnd = a.y < wnd ? a.y : wnd;
    wndw = b.x < wndw ? b.x : wndw;
    tot += b.y;
  }
  q[0] = make_ulonglong2(tmn, wnd);
  q[1] = make_ulonglong2(wndw, tot);
}

// A pending event in registers.
struct Ev {
  uint64_t ts;
  uint32_t uid, ctx, kind, a;
  Pkt p;
};

// ---- exchange records of a partitioned run (fixed sizes: they are captured into the window graph) ----
// X1: a rank's window summary, allgathered.  LbtsMessage's role (distributed-simulator-impl.h:36-84:
// rx/tx counts, smallest next time) is played by the pending-set reduction `red` and the counts.
struct X1Hdr {
  uint32_t W, tc, tinl, needc;  // window events, their children, their inline children; pool compaction wanted
  uint32_t L, pad1;           // wide windows: this rank's local records (X1Loc entries)
  uint64_t lastkey;           // largest window key
  Red red;                    // reduction of this rank's pending set after the window (next LBTS)
  uint64_t rkey, rrem, rhead; // sorted run: this rank's fitting key for the next chunk (~0: the rest fits), entries
                              // left, the first one's key (~0: none)
  uint64_t pad2[4];
};
static_assert(sizeof(X1Hdr) == 128, "X1 records: the loopback transport copies 16-byte words");
struct X1Ent {  // one window event: key and child counts (children | inline children << 16)
  uint64_t key;
  uint32_t cnt, pad;
};
// Wide windows: one rank's local records (same-node TransmitCompletes run inside the window), compacted by
// k2_handle.  Their order words (lkw) decide every pair from different gen-0 ancestors exactly once the chain
// depth is at most 2 (the partitioned wide span is kept below 3 tx_min, nsgpu_p2p_create_dist), except a
// depth-2 word's clamped ancestor uid: `anc` holds it whole.  Records of one ancestor are on one rank, where
// their exact chains are (lkey[rec]).
struct X1Loc {
  uint64_t w1, w2;     // lkw: (rel ts, local, parent rel ts), (ancestor uid, child index / ...)
  uint32_t cnt, rec;   // children | inline children << 16; the record on its rank
  uint32_t anc, par;   // the gen-0 ancestor's uid; the parent's accumulator row | child index << 24 (k_dfin2)
};
static_assert(sizeof(X1Loc) == 32, "X1Loc");
constexpr int XLCAP = 4096;  // local records of one rank's window (LMAX)
constexpr int NACC = WCAP + XLCAP;  // k_gtile's accumulator rows: gen-0 slots, then local records (compact order)
// One record of a rank's window in that rank's dispatch order (k_gsort), as another rank's k_gsearch compares its
// own records with it: the order key (rel ts, gen-0 before local, then a gen-0 record's uid / a local record's
// order words and ancestor uid: records of different ranks never tie on it) and the exclusive prefixes of its
// rank's children / inline children before it.  Entry n (n = the rank's records) is a sentinel with the totals.
struct SEnt {
  uint64_t k0;  // rel ts << 32 | (gen-0: uid; local: the low word of its first order word)
  uint64_t b;   // local: its second order word (gen-0: 0)
  uint32_t c, L;  // local: the gen-0 ancestor's uid, 1 (gen-0: 0, 0)
  uint32_t cp, ip;
};
static_assert(sizeof(SEnt) == 32, "SEnt");
// X1 (all-gathered): the header and the sorted records; the rank's own lists stay in x1_own.
constexpr size_t X1B = sizeof(X1Hdr) + sizeof(SEnt) * (NACC + 1);
constexpr size_t X1OWN = sizeof(X1Ent) * WCAP + sizeof(X1Loc) * XLCAP;
static_assert(X1B % 16 == 0, "k_copies moves 16-byte words");
// X2: remote events for one peer (children whose node another rank owns), all-to-all; the record is
// the pending event itself, uid included (mpi-interface.cc:414-506 sends {rx ns, node, dev, packet}).
struct X2Hdr {
  uint32_t n, pad[3];
};
// X2 records per peer: a device starts at most one transmission per narrow window (its TransmitComplete is a
// child, and children sort after the window) — three per wide one (its local TransmitCompletes start the next
// ones: chain depth <= 2) — and Receive is the only child scheduled on another node, so rank p sends rank q at
// most that many records per window per device of p whose peer q owns (nsgpu_p2p_create_dist sizes X2 to the
// largest such cut, rounded up to 16; at most CAPX_MAX).
constexpr int CAPX_MAX = 1024;
constexpr size_t X0B = 16;  // X0: one rank's largest fitting window bound (+ pad)
constexpr int MAXR = 64;    // ranks
static_assert(MAXR <= 64 && HB == 64, "per-rank summaries are read one lane per rank in one-wave blocks");
static_assert((uint64_t)MAXR * NACC <= (1u << 21), "k_gtile's packed rank fields");
__device__ __forceinline__ X1Hdr *x1hdr(uint8_t *b, uint32_t q) { return (X1Hdr *)(b + (size_t)q * X1B); }
__device__ __forceinline__ SEnt *x1srt(uint8_t *b, uint32_t q) { return (SEnt *)(b + (size_t)q * X1B + sizeof(X1Hdr)); }
__device__ __forceinline__ X1Ent *x1ent(const P2PDev &M) { return (X1Ent *)M.x1_own; }
__device__ __forceinline__ X1Loc *x1loc(const P2PDev &M) { return (X1Loc *)(M.x1_own + sizeof(X1Ent) * WCAP); }
__device__ __forceinline__ X2Hdr *x2hdr(const P2PDev &M, uint8_t *b, uint32_t q) {
  return (X2Hdr *)(b + (size_t)q * M.x2b);
}
__device__ __forceinline__ Ev *x2rec(const P2PDev &M, uint8_t *b, uint32_t q) {
  return (Ev *)(b + (size_t)q * M.x2b + sizeof(X2Hdr));
}

constexpr int PFC = 4;  // children per slot k2_pa loads ahead


// Rank tile t: rows [ti * HB * RTR, +HB * RTR) of the window (RTR keys per thread) against the RJ keys
// of column tile tj: each row's count of smaller keys is added to its rank (keys are distinct: uids).
// Wide rows: each column tile's keys are loaded by NRT blocks, not WCAP / HB.
// (wr: the rank accumulators of the window's parity, wrank_of)
template <bool DF = false>
__device__ __forceinline__ void rank_tile(const P2PDev &M, const Ctl &C, uint32_t t, uint32_t *wr) {
  const uint32_t ti = t / NJT, tj = t % NJT;
  __shared__ uint64_t tk[RJ];
  // the window size first: a config-4 window fills ~1/4 of the WCAP x WCAP tiles, and the tiles past
  // it load nothing (these blocks are off the launch's critical path, the holders are on it)
  const uint32_t W = DF ? (uint32_t)C.wnf : C.W;  // (DF: the deferred pipeline's allocation word)
  const uint32_t r0 = ti * HB * RTR;
  if (r0 >= W || tj * RJ >= W) return;  // uniform over the block
#pragma unroll
  for (int q = 0; q < RJ / HB; q++) {  // (slots past W hold stale keys: padded with a key after every row's)
    const uint32_t j = tj * RJ + q * HB + threadIdx.x;
    tk[q * HB + threadIdx.x] = j < W ? M.wkey[j] : ~0ull;
  }
  uint64_t x[RTR];
#pragma unroll
  for (int r = 0; r < RTR; r++) {
    const uint32_t i = r0 + r * HB + threadIdx.x;
    x[r] = i < W ? M.wkey[i] : 0;
  }
  __syncthreads();
  uint32_t c[RTR] = {};
#pragma unroll 16
  for (int y = 0; y < RJ; y++) {
    const uint64_t k = tk[y];
#pragma unroll
    for (int r = 0; r < RTR; r++) c[r] += k < x[r];
  }
#pragma unroll
  for (int r = 0; r < RTR; r++) {
    const uint32_t i = r0 + r * HB + threadIdx.x;
    if (i < W && c[r]) atomicAdd(&wr[i], c[r]);
  }
}

}  // namespace nsgpu
