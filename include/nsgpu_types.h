/*
 * nsgpu_types.h — plain-old-data types shared by the nsgpu C-ABI (include/nsgpu.h)
 * and its test checker (oracle/).  No torch types, no C++ across the ABI.
 *
 * Event key layout follows ns-3's Scheduler::EventKey
 *   (reference: src/core/model/scheduler.h:58-63):
 *     uint64 m_ts; uint32 m_uid; uint32 m_context
 * and the ordering is (ts, uid) ONLY (scheduler.h:105-121) — context is payload.
 */
#ifndef NSGPU_TYPES_H
#define NSGPU_TYPES_H

#include <stdint.h>

#if defined(__HIP__)
#define NSGPU_HD __host__ __device__
#else
#define NSGPU_HD
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Scheduler::EventKey + Scheduler::Event (scheduler.h:58-68): 24 bytes. */
typedef struct nsgpu_event {
  uint64_t ts;       /* absolute time, in Time resolution units (ns) */
  uint32_t uid;      /* global schedule counter, starts at 4 (default-simulator-impl.cc:52-56) */
  uint32_t context;  /* node id, 0xffffffff = no node (default-simulator-impl.cc:60) */
  uint64_t handle;   /* opaque EventImpl* (host closure) — never dereferenced on device */
} nsgpu_event;

/* ns-3 EventId (event-id.h:46-83): (impl, ts, context, uid). */
typedef struct nsgpu_event_id {
  uint64_t impl;
  uint64_t ts;
  uint32_t context;
  uint32_t uid;
} nsgpu_event_id;

/* Propagation loss model kinds (src/propagation/model/propagation-loss-model.cc). */
enum nsgpu_loss_kind {
  NSGPU_LOSS_NONE = 0,
  NSGPU_LOSS_LOG_DISTANCE = 1, /* p0 = exponent, p1 = reference distance, p2 = reference loss  (:464-491) */
  NSGPU_LOSS_FRIIS = 2,        /* p0 = lambda, p1 = system loss, p2 = min distance            (:197-239) */
  NSGPU_LOSS_FIXED_RSS = 3,    /* p0 = fixed rss dBm                                          (:718-723) */
  NSGPU_LOSS_RANGE = 4         /* p0 = max range m; beyond it -1000 dBm                       (:822-834) */
};

typedef struct nsgpu_loss_model {
  int32_t kind;
  int32_t pad_;
  double p0, p1, p2;
} nsgpu_loss_model;

/* A PropagationLossModel chain (PropagationLossModel::CalcRxPower, :64-74): up to 4 links. */
#define NSGPU_MAX_LOSS_CHAIN 4
typedef struct nsgpu_loss_chain {
  int32_t n;
  int32_t pad_;
  nsgpu_loss_model m[NSGPU_MAX_LOSS_CHAIN];
} nsgpu_loss_chain;

/* Result record of one broadcast fan-out receiver (YansWifiChannel::Send, yans-wifi-channel.cc:77-115):
 * the ScheduleWithContext(dstNode, delay, &YansWifiChannel::Receive, this, j, copy, rxPowerDbm, ...) call. */
typedef struct nsgpu_rx_record {
  uint64_t ts;       /* now + delay */
  uint32_t uid;      /* uid_base + rank among surviving receivers (list order) */
  uint32_t context;  /* destination node id */
  uint32_t phy;      /* index j into the channel's phy list */
  uint32_t pad_;
  double rx_dbm;     /* CalcRxPower (txPowerDbm, sender, receiver) */
} nsgpu_rx_record;

/* SpectrumModels a MultiModelSpectrumChannel knows, indexed in ascending SpectrumModelUid order (the
 * iteration order of its m_rxSpectrumModelInfoMap, multi-model-spectrum-channel.cc:246-249): model m has
 * the bands [band_off[m], band_off[m+1]) of fl / fh (BandInfo, Hz).  Pointers are device memory. */
typedef struct nsgpu_spectrum_models {
  int32_t n_models;
  int32_t max_bands;          /* largest band count of any model (the PSD stride) */
  const uint32_t *band_off;   /* [n_models + 1] */
  const double *fl, *fh;      /* [band_off[n_models]] */
} nsgpu_spectrum_models;

/* One PropagationLoss trace call of a spectrum channel's StartTx: m_propagationLossTrace (txPhy, rxPhy,
 * -gainDb), fired for every receiver before the MaxLossDb cut (multi-model-spectrum-channel.cc:290-291,
 * single-model-spectrum-channel.cc:145-146). */
typedef struct nsgpu_loss_trace {
  uint32_t rx_phy;
  uint32_t pad_;
  double loss_db;
} nsgpu_loss_trace;

/* ---------------- point-to-point scenario (GPU-resident p2p / DropTail / IPv4 / UDP subset) ----------------
 * A topology of PointToPointNetDevices joined by PointToPointChannels, IPv4 forwarding by static
 * next-hop tables, OnOff (UDP; constant on/off times, or random ones: nsgpu_ranvar below) sources and PacketSink sinks.  All arrays are
 * host pointers; devices and applications are listed in ns-3 creation order (Node::AddDevice /
 * Node::AddApplication), which fixes the setup-time uids (node-list.cc:124-131, node.cc:111-145). */
enum nsgpu_app_kind { NSGPU_APP_ONOFF = 0, NSGPU_APP_SINK = 1, NSGPU_APP_ECHO_CLIENT = 2, NSGPU_APP_ECHO_SERVER = 3,
                      NSGPU_APP_UDP_CLIENT = 4, NSGPU_APP_UDP_SERVER = 5,  /* (4, 5, 6: ports mode only, below) */
                      NSGPU_APP_UDP_TRACE_CLIENT = 6 };
/* UdpEchoClient (udp-echo-client.cc): app_dst_node = the server's node, app_pkt_size = PacketSize,
 * app_count = MaxPackets, app_interval_ns = Interval, app_src_slot = the route-table slot of the
 * client's own node (the echo comes back there).  UdpEchoServer (udp-echo-server.cc): the node's bound
 * UDP endpoint, like a PacketSink; HandleRead sends every datagram back to its sender.  Without UDP ports
 * (app_port NULL, below) a node has at most one bound endpoint (PacketSink or UdpEchoServer). */

typedef struct nsgpu_p2p_scenario {
  uint32_t n_nodes;
  uint32_t n_devices;
  uint32_t n_apps;
  uint32_t n_dst;              /* columns of the route table (destination slots) */
  /* devices (PointToPointNetDevice + DropTailQueue), index = creation order */
  const uint32_t *dev_node;    /* owning node */
  const uint32_t *dev_peer;    /* device at the other end of the channel */
  const uint64_t *dev_bps;     /* DataRate (bit/s), point-to-point-net-device.cc:57 */
  const int64_t  *dev_ifg_ns;  /* InterframeGap */
  const int64_t  *dev_delay_ns;/* PointToPointChannel Delay of the device's channel */
  const uint32_t *dev_qmax;    /* DropTailQueue MaxPackets (PACKETS mode), drop-tail-queue.cc:37-43 */
  /* IPv4 static routing: route[node * n_dst + slot] = output device, or 0xffffffff = no route */
  const uint32_t *route;
  /* applications in AddApplication order */
  const uint32_t *app_kind;    /* nsgpu_app_kind */
  const uint32_t *app_node;
  const int64_t  *app_start_ns;
  const int64_t  *app_stop_ns; /* 0 = never (application.cc:90-93) */
  /* OnOff parameters (ignored for sinks), onoff-application.cc:47-86 */
  const uint32_t *app_dst_node;
  const uint32_t *app_dst_slot;
  const uint64_t *app_rate_bps;
  const uint32_t *app_pkt_size;
  const double   *app_on_s;    /* ConstantVariable OnTime (seconds; converted by Seconds () at each use) */
  const double   *app_off_s;   /* ConstantVariable OffTime */
  const uint32_t *app_max_bytes;
  const uint32_t *app_ttl;     /* IP TTL of the flow's packets */
  int64_t stop_ns;             /* Simulator::Stop (Seconds (x)) from main, as ns */
  /* Setup-time Schedule calls in program order (they fix every later uid):
   *   NSGPU_SETUP_NODE k   NodeListPriv::Add      -> ScheduleWithContext (k, 0, &Node::Start)
   *   NSGPU_SETUP_DEVICE d Node::AddDevice        -> ScheduleWithContext (node, 0, &NetDevice::Start)
   *   NSGPU_SETUP_APP a    Node::AddApplication   -> ScheduleWithContext (node, 0, &Application::Start)
   *   NSGPU_SETUP_STOP     Simulator::Stop (t)    -> Schedule (t, &Simulator::Stop), context 0xffffffff
   *   NSGPU_SETUP_UID      any other setup call that consumes one uid without a dispatched event */
  uint32_t n_setup;
  /* 1: ICMP errors are generated (Ipv4L3Protocol::IpForward TTL expiry -> Icmpv4L4Protocol::
   * SendTimeExceededTtl, LocalDeliver RX_ENDPOINT_UNREACH -> SendDestUnreachPort; ipv4-l3-protocol.cc,
   * icmpv4-l4-protocol.cc:85-160) and routed back to the offending datagram's sender through
   * app_src_slot; the lookahead then also covers the 58-byte ICMP frames.  0: the triggers are only
   * counted (ttl_drops / unreach_drops), i.e. the scenario asserts they never happen. */
  uint32_t icmp;
  const uint32_t *setup_kind;
  const uint32_t *setup_index;
  /* UdpEchoClient parameters (NULL when the scenario has no echo client) */
  const uint32_t *app_count;
  const int64_t  *app_interval_ns;
  /* route-table slot of each sending application's own node: where an echo reply and (icmp = 1) an
   * ICMP error about the application's datagrams are routed; 0xffffffff: none */
  const uint32_t *app_src_slot;
  /* Compressed next-hop table, used when `route` is NULL (large topologies: the dense table is
   * n_nodes x n_dst): node n forwards towards slot k through route_exc_dev[j] for the j in
   * [route_exc_off[n], route_exc_off[n + 1]) with route_exc_slot[j] == k (slots ascending within a
   * node), else through route_default[n] (0xffffffff: no route). */
  const uint32_t *route_default;   /* n_nodes */
  const uint64_t *route_exc_off;   /* n_nodes + 1 */
  const uint32_t *route_exc_slot;
  const uint32_t *route_exc_dev;
  /* DefaultSimulatorImpl::m_uid before the first setup call (0: 4, the reference's start, :52-56) — a program
   * whose earlier Schedule calls consumed uids; the engine refuses to pass 0xfffffffe (NSGPU_ERANGE) */
  uint32_t uid_first;
  uint32_t pad_uid_;
  /* ---- UDP ports (appended: the fields above keep their offsets) ----
   * app_port == NULL: no port is modelled — one bound endpoint a node, every datagram addressed to the node
   * reaches it.  app_port given ("ports mode"): UdpL4Protocol::Receive -> Ipv4EndPointDemux::Lookup
   * (udp-l4-protocol.cc:312-407, ipv4-end-point-demux.cc:195-307) for sockets bound to (Any, port): a datagram of
   * flow a is delivered to the application of app_dst_node[a] whose app_port equals app_remote_port[a], else
   * RX_ENDPOINT_UNREACH; a node may host several bound endpoints on distinct ports.  The binding is static, so
   * nsgpu_p2p_create resolves it per flow; only bound / receiving changes at run time.
   *   app_port          bound port of a PacketSink / UdpEchoServer / UdpServer (not 0; other kinds: ignored)
   *   app_remote_port   destination port of an OnOff / UdpEchoClient / UdpClient
   *   app_loss_window   UdpServer PacketWindowSize: a multiple of 8 in [8, 256]
   * UdpClient (udp-client.cc:116-187): app_pkt_size = PacketSize (the 12-byte SeqTsHeader included, [12, 1472]),
   * app_count = MaxPackets (<= 2^24), app_interval_ns = Interval; m_sent advances only when Send succeeded.
   * UdpServer (udp-server.cc:109-190): StopApplication clears the receive callback only — the socket stays
   * bound, later datagrams still cost their DoForwardUp event and count nothing. */
  const uint32_t *app_port;
  const uint32_t *app_remote_port;
  const uint32_t *app_loss_window;
  /* ---- IPv4 fragmentation (appended: the fields above keep their offsets) ----
   * frag == 0: a payload above 1472 bytes is refused (every device has MTU 1500).  frag == 1: SendRealOut ->
   * DoFragmentation (ipv4-l3-protocol.cc:722-731, 751-761, 1116-1206) and LocalDeliver -> ProcessFragment ->
   * Fragments, HandleFragmentsTimeout (:849-859, 1208-1412) are modelled: OnOff and UdpEchoClient payloads up to
   * 65507 bytes (MAX_IPV4_UDP_DATAGRAM_SIZE, udp-socket-impl.cc:45), UdpClient PacketSize in [12, 1500].  At most
   * one fragmenting flow may deliver fragments to a node (flows with payload above 1472 addressed to it, plus each
   * such UdpEchoClient on it: the reply's fragments return there); DESIGN.md §6 says why.
   *   frag_timeout_ns   Ipv4L3Protocol::FragmentExpirationTimeout; 0: the reference's default, Seconds (30) */
  uint32_t frag;
  uint32_t flowmon;  /* per-flow statistics, below: the word that was frag's padding (the struct keeps its size) */
  int64_t frag_timeout_ns;
  /* ---- receive error models (appended: the fields above keep their offsets) ----
   * dev_em_kind == NULL: no device has a model (the other fields are then ignored).  Given: device d's
   * PointToPointNetDevice::SetReceiveErrorModel (point-to-point-net-device.cc:304-317: Receive asks IsCorrupt first;
   * a corrupt frame fires PhyRxDrop and nothing else) — NSGPU_EM_NONE, NSGPU_EM_RECEIVE_LIST
   * (ReceiveListErrorModel, error-model.cc:343-360: the frames whose 0-based arrival ordinal at the device is in
   * the list) or NSGPU_EM_RATE (RateErrorModel, :178-223: one UniformVariable (0, 1) draw a frame against the rate
   * (EU_PKT) or 1 - pow (1 - rate, size or 8 * size) (EU_BYTE, EU_BIT), size = the frame with its PPP header).
   *   dev_em_enabled   ErrorModel::IsEnabled () at setup (NULL: all enabled); a disabled model counts, draws and
   *                    drops nothing
   *   dev_em_unit      NSGPU_EU_* of a Rate model (NULL: EU_BYTE, the attribute's default)
   *   dev_em_rate      ErrorRate of a Rate model (NaN is refused)
   *   dev_em_stream    a Rate model's variable is the dev_em_stream[d]-th RngStream the program constructs (0-based);
   *                    two Rate devices may not name the same stream
   *   em_list_off / em_list   CSR (n_devices + 1 offsets): the ReceiveList models' lists, any order, duplicates allowed
   *   rng_seed / rng_run      RngSeed / RngRun (0: the reference's default, 1)
   * At most NSGPU_EM_MAX_TABLES distinct (unit, rate) pairs of enabled EU_BYTE / EU_BIT models a scenario. */
  const uint32_t *dev_em_kind;
  const uint32_t *dev_em_enabled;
  const uint32_t *dev_em_unit;
  const double *dev_em_rate;
  const uint32_t *dev_em_stream;
  const uint64_t *em_list_off;
  const uint32_t *em_list;
  uint32_t rng_seed;
  uint32_t rng_run;
  /* ---- per-flow statistics: `flowmon`, the word behind `frag` that was padding until now (callers zeroed it), so
   * every field keeps its offset and the struct its size ----
   * flowmon == 1: FlowMonitor's FlowStats (flow-monitor.cc:121-300, ipv4-flow-probe.cc:192-346,
   * ipv4-flow-classifier.cc:102-155) are accumulated on the device while the run goes on; nsgpu_p2p_flow_stats reads
   * them.  The run itself is the unmonitored one: no event is added or reordered.  Not with frag, not on a partitioned
   * engine, not under a host-closure runtime (refused). */
} nsgpu_p2p_scenario;

/* ---------------- UdpTraceClient (udp-trace-client.cc): NSGPU_APP_UDP_TRACE_CLIENT, ports mode only ----------------
 * A trace client sends the frames of a trace file, cyclically: entry e is (timeToSend ms, packetSize).  One Send event
 * (:311-335) emits, starting at m_currentEntry, every entry up to the next one whose timeToSend is not 0 — a frame
 * above MaxPacketSize as packetSize / MaxPacketSize datagrams of MaxPacketSize bytes and one of the remainder (also
 * when that is 0) — and schedules the next Send after that entry's timeToSend.  A datagram's UDP payload is
 * max (size, 12) bytes: the 12-byte SeqTsHeader, whose sequence number is m_sent (it advances only when the socket's
 * Send succeeded).  app_pkt_size = MaxPacketSize ([1, 1472]); app_remote_port, app_ttl, app_dst_*, app_src_slot as
 * for a UdpClient.  The entries do not fit nsgpu_p2p_scenario (whose size and offsets are fixed): they travel in this
 * size-prefixed extension record, given to the _ex forms of the entry points that read a scenario (nsgpu.h).
 * A Send may emit at most NSGPU_UDP_TRACE_MAX_BURST datagrams; a client whose m_sent would pass 2^24 (the descriptor's
 * sequence field) fails the run with NSGPU_ERANGE. */
#define NSGPU_UDP_TRACE_MAX_BURST 256u
typedef struct nsgpu_udp_trace_entry {
  uint32_t time_to_send_ms;  /* TraceEntry::timeToSend: the delta to the previous non-B frame (0 for a B frame) */
  uint32_t packet_size;      /* TraceEntry::packetSize (a uint16 in the reference: above 65535 is refused) */
} nsgpu_udp_trace_entry;
/* ---------------- random OnOff times (onoff-application.cc:221-237, random-variable.cc) ----------------
 * OnOffApplication draws Seconds (m_offTime.GetValue ()) when it schedules StartSending (ScheduleStartEvent: from
 * StartApplication and StopSending) and Seconds (m_onTime.GetValue ()) when it schedules StopSending (ScheduleStopEvent:
 * from StartSending), whether or not the event is cancelled later.  A variable owns its RngStream: `stream` is the
 * index of the RngStream the program constructs for it (0-based, as dev_em_stream), seeded by the scenario's rng_seed
 * / rng_run.  Every kind of RandomVariable that is not listed is NSGPU_RV_OTHER, named so that it can be refused.
 *   NSGPU_RV_CONSTANT      p0 = the value (in app_on_var / app_off_var: the application's app_on_s / app_off_s is
 *                          used instead, and the entry's parameters are ignored); draws nothing
 *   NSGPU_RV_UNIFORM       p0 = min, p1 = max: min + U01 * (max - min)
 *   NSGPU_RV_EXPONENTIAL   p0 = mean, p1 = bound (0: none): -mean * log (U01), redrawn while above the bound
 * The Exponential's log is evaluated in double-double on the device; a draw whose timestamp could differ from the
 * reference's under a libm log with an error below 1 ulp is recorded as ambiguous (csrc/nsgpu_ranvar.h). */
enum { NSGPU_RV_CONSTANT = 0, NSGPU_RV_UNIFORM = 1, NSGPU_RV_EXPONENTIAL = 2,
       NSGPU_RV_OTHER = 3 /* Pareto, Weibull, Normal, LogNormal, Gamma, Erlang, Triangular, Zipf, Zeta, Empirical,
                             Deterministic, Sequential: named so that it can be refused */ };
typedef struct nsgpu_ranvar {
  uint32_t kind, stream;
  double p0, p1;
} nsgpu_ranvar;
#define NSGPU_RV_AMBIGUOUS_CAP 1024u /* records of an engine's ambiguous-draw log; further ones are only counted */
/* What nsgpu_p2p_onoff_draws returns per application (zeros for an application without a random variable). */
typedef struct nsgpu_onoff_draw_record {
  uint32_t on_draws, off_draws;  /* GetValue calls on the OnTime / OffTime variable (a Constant counts none) */
  uint32_t ambiguous;            /* ambiguous attempts of both */
  uint32_t pad_;
} nsgpu_onoff_draw_record;
/* One ambiguous attempt (nsgpu_p2p_onoff_ambiguous). */
typedef struct nsgpu_ambiguous_draw {
  uint32_t app, which;    /* which: 0 = OnTime, 1 = OffTime */
  uint32_t ordinal;       /* the GetValue call's 0-based ordinal on that variable */
  uint32_t k;             /* the integer behind u: u = k / 4294967088 */
  int64_t ns, ns_other;   /* Seconds (-mean * hi), which the device took; Seconds (-mean * hi's neighbour) */
} nsgpu_ambiguous_draw;

typedef struct nsgpu_p2p_scenario_ext {
  uint32_t size;             /* sizeof (nsgpu_p2p_scenario_ext) as the caller compiled it */
  uint32_t pad_;
  const uint64_t *trace_off; /* CSR, n_apps + 1 offsets into trace_entries (empty for every other kind) */
  const nsgpu_udp_trace_entry *trace_entries;
  /* ---- random OnOff times (appended: a caller compiled against the shorter record gives a smaller `size`) ----
   * n_apps entries each, or NULL: every OnTime / OffTime is the Constant app_on_s / app_off_s. */
  const nsgpu_ranvar *app_on_var;
  const nsgpu_ranvar *app_off_var;
} nsgpu_p2p_scenario_ext;
/* What nsgpu_p2p_udp_trace_clients returns per application (zeros for every other kind). */
typedef struct nsgpu_udp_trace_client_record {
  uint32_t sent;           /* m_sent */
  uint32_t current_entry;  /* m_currentEntry */
  uint32_t sends;          /* Send events that ran (a cancelled one is dispatched, not run) */
  uint32_t pad_;
} nsgpu_udp_trace_client_record;

/* What nsgpu_p2p_flow_stats returns per flow, 2 * n_apps records: flow a = application a's datagrams, flow
 * n_apps + a = the echo replies to UdpEchoClient a (zeros for a flow that sent nothing).  FlowMonitor::FlowStats
 * without the histograms; times in ns.  Only UDP datagrams are classified: ICMP messages report nothing. */
#define NSGPU_FLOW_DROP_REASONS 4u
enum { NSGPU_FLOW_DROP_NO_ROUTE = 0, NSGPU_FLOW_DROP_TTL_EXPIRE = 1, NSGPU_FLOW_DROP_BAD_CHECKSUM = 2 /* stays 0 */,
       NSGPU_FLOW_DROP_QUEUE = 3 };
typedef struct nsgpu_flow_record {
  uint64_t tx_packets, tx_bytes;        /* ReportFirstTx (Ipv4L3Protocol::Send, m_sendOutgoingTrace) */
  uint64_t rx_packets, rx_bytes;        /* ReportLastRx (LocalDeliver, m_localDeliverTrace: before the endpoint lookup) */
  int64_t delay_sum_ns, jitter_sum_ns, last_delay_ns;
  int64_t time_first_tx_ns, time_last_tx_ns, time_first_rx_ns, time_last_rx_ns;
  uint64_t times_forwarded;             /* the received packets' ReportForwarding calls (m_unicastForwardTrace) */
  uint64_t lost_packets;                /* the drops below + the tracked packets not seen for max_delay_ns */
  uint64_t packets_dropped[NSGPU_FLOW_DROP_REASONS], bytes_dropped[NSGPU_FLOW_DROP_REASONS];
  uint64_t first_tx_ts;                 /* the dispatched event of the flow's first ReportFirstTx: its (ts, uid) — */
  uint32_t first_tx_uid;                /*   FlowIds follow that order (Ipv4FlowClassifier numbers a flow when first seen) */
  uint32_t pad_;
} nsgpu_flow_record;                    /* 184 bytes */

enum { NSGPU_EM_NONE = 0, NSGPU_EM_RECEIVE_LIST = 1, NSGPU_EM_RATE = 2,
       NSGPU_EM_LIST = 3 /* ListErrorModel (by Packet::GetUid): named so that it can be refused */ };
enum { NSGPU_EU_PKT = 0, NSGPU_EU_BYTE = 1, NSGPU_EU_BIT = 2 };
#define NSGPU_EM_MAX_TABLES 16u   /* threshold tables (distinct EU_BYTE / EU_BIT (unit, rate) pairs) a scenario */
#define NSGPU_EM_TABLE_SIZE 1503u /* frame sizes 0 .. 1502: MTU 1500 + the PPP header */

/* What nsgpu_p2p_error_models returns per device (zeros without an enabled model). */
typedef struct nsgpu_error_model_record {
  uint32_t invoked;    /* IsCorrupt calls on the enabled model: the frames that arrived */
  uint32_t corrupted;  /* ... of which it declared corrupt (m_phyRxDropTrace) */
} nsgpu_error_model_record;

/* RngStream (rng-stream.cc): MRG32k3a's state Cg, whose six values stay below 2^32 (csrc/nsgpu_rng_stream.h). */
typedef struct nsgpu_rng_stream {
  uint32_t s[6];
} nsgpu_rng_stream;

/* What nsgpu_p2p_frag_stats returns (zeros for a scenario without frag). */
typedef struct nsgpu_frag_stats {
  uint64_t fragmented;         /* datagrams DoFragmentation split */
  uint64_t fragments_sent;     /* the fragments it made (each handed to its device: enqueued or dropped) */
  uint64_t reassembled;        /* datagrams ProcessFragment completed */
  uint64_t timeouts;           /* HandleFragmentsTimeout calls (timers that fired) */
  uint64_t cancelled_timers;   /* timers dispatched after their datagram was entire */
  uint64_t max_list;           /* the longest Fragments::m_fragments seen on any node */
} nsgpu_frag_stats;

/* PacketLossCounter (packet-loss-counter.cc:32-120) of one UdpServer, with the server's m_received: the
 * state nsgpu_loss_counter_notify (csrc/nsgpu_loss_counter.h) advances, on the host and on the device. */
#define NSGPU_LOSS_WINDOW_MAX 256u
typedef struct nsgpu_loss_counter {
  uint32_t lost;          /* m_lost */
  uint32_t last_max_seq;  /* m_lastMaxSeqNum */
  uint32_t window;        /* m_bitMapSize * 8 */
  uint32_t received;      /* UdpServer::m_received */
  uint8_t map[NSGPU_LOSS_WINDOW_MAX / 8];  /* m_receiveBitMap (window / 8 bytes used, 0xFF at start) */
} nsgpu_loss_counter;     /* 48 bytes */
/* What nsgpu_p2p_udp_servers returns per application (zeros for every kind but NSGPU_APP_UDP_SERVER). */
typedef struct nsgpu_udp_server_record {
  uint32_t received, lost, last_max_seq, pad_;
} nsgpu_udp_server_record;

/* Packet descriptor flags (the descriptor {app, ipid, size, ttl} of a datagram): an echo reply
 * travelling back to its client (app) ... */
#define NSGPU_PKT_REPLY 0x80000000u
/* ... or an ICMP error about a datagram of flow (app & NSGPU_PKT_APP), travelling back to that datagram's
 * sender: NSGPU_PKT_ICMP_UNREACH = destination unreachable (port), else time exceeded (TTL);
 * NSGPU_PKT_ICMP_OF_REPLY = the offending datagram was an echo reply.  An ICMP descriptor packs the
 * offending datagram's IPv4 header fields: ipid = own | offending << 16 (16 bits each), size = 56 (the
 * ICMP packet's IPv4 length), ttl = own TTL | offending TTL << 8 | offending IPv4 length << 16.
 * A UDP datagram's ttl word holds the IPv4 TTL in its low 8 bits; a UdpClient's datagram carries its
 * SeqTsHeader sequence number (m_sent, < 2^24) in the other 24: ttl = TTL | seq << 8 (0 for every other
 * sender, which is what a UdpServer reads from a payload without the header).  Every reader of the TTL takes
 * the low byte; an ICMP descriptor's "offending TTL" is that byte, and so is the TTL of the Ipv4 Drop record
 * that follows a time-exceeded error (it is rebuilt from the error's descriptor). */
#define NSGPU_PKT_ICMP 0x40000000u
#define NSGPU_PKT_ICMP_UNREACH 0x20000000u
#define NSGPU_PKT_ICMP_OF_REPLY 0x10000000u
#define NSGPU_PKT_APP 0x0fffffffu
/* A fragment of a UDP datagram (frag scenarios) carries its IPv4 fragment fields in the upper half of ipid, above
 * the 16-bit identification: ipid = id | offset (13 bits, 8-byte units) << 16 | MF << 29.  size stays the
 * fragment's plain IPv4 length (the device step computes txTime from it) and the ttl word is the datagram's in
 * every fragment (a UdpClient's sequence number included).  In a frag scenario every sender writes id & 0xffff, so
 * a UDP descriptor is a fragment exactly when ipid >> 16 != 0 (an ICMP descriptor packs two ids there, above). */
#define NSGPU_PKT_FRAG_SHIFT 16
#define NSGPU_PKT_FRAG_OFF_MASK 0x1fffu
#define NSGPU_PKT_FRAG_MF 0x20000000u

/* ---------------- trace records (ascii / pcap replay) ----------------
 * One record per call of a default ascii trace sink of PointToPointHelper::EnableAsciiInternal
 * (point-to-point-helper.cc:113-219, trace-helper.cc:303-390): TxQueue/Enqueue "+", TxQueue/Dequeue
 * "-", TxQueue/Drop "d", MacRx "r".  The pcap PromiscSniffer calls are implied: every Dequeue is
 * followed by the sniffer on the same device (Send :462-518, TransmitComplete :236-269), every MacRx is
 * preceded by it (Receive :304-346, packet with the PPP header).  Records are written unordered; the
 * trace order is (ts, uid, seq): the pop order of the dispatched event, then call order inside it. */
enum nsgpu_trace_kind { NSGPU_TR_ENQUEUE = 0, NSGPU_TR_DEQUEUE = 1, NSGPU_TR_DROP = 2, NSGPU_TR_RX = 3,
                        /* Ipv4L3Protocol's trace sources as InternetStackHelper::EnableAsciiIpv4 hooks them
                         * (internet-stack-helper.cc:593-730, every interface): "t" Tx (SendRealOut,
                         * ipv4-l3-protocol.cc:764, the packet with its new IPv4 header), "r" Rx (Receive
                         * :455, as received), "d" Drop (DROP_TTL_EXPIRED :835 — after the time exceeded an
                         * ICMP-enabled node sends —, DROP_NO_ROUTE :505; the received header; a UDP datagram's ipid & 0xffff).
                         * dev: the sending device (Tx), the receiving one (Rx, DROP_NO_ROUTE), the forwarding
                         * route's (DROP_TTL_EXPIRED: IpForward's interface); size: the IPv4 length. */
                        NSGPU_TR_IP_TX = 4, NSGPU_TR_IP_RX = 5, NSGPU_TR_IP_DROP = 6 };
typedef struct nsgpu_trace_record {
  uint64_t ts;    /* Now () of the call (ns) */
  uint32_t uid;   /* uid of the dispatched event that made the call */
  uint16_t seq;   /* call index inside that event */
  uint8_t  kind;  /* nsgpu_trace_kind */
  uint8_t  pad_;
  uint32_t dev;   /* device (its queue) */
  /* the packet as the sink sees it: flow (| NSGPU_PKT_REPLY), IPv4 identification, size in bytes
   * (PPP header included except for MacRx), IPv4 TTL */
  uint32_t app, ipid, size, ttl;
  uint32_t pad2_;
} nsgpu_trace_record;  /* 40 bytes */

enum nsgpu_setup_kind { NSGPU_SETUP_NODE = 0, NSGPU_SETUP_DEVICE = 1, NSGPU_SETUP_APP = 2, NSGPU_SETUP_STOP = 3,
                        NSGPU_SETUP_UID = 4, NSGPU_SETUP_NOOP = 5 };
/* NSGPU_SETUP_NOOP k: ScheduleWithContext (k, 0, <no-op>) — e.g. the LoopbackNetDevice that
 * Ipv4L3Protocol::SetupLoopback adds to every node (ipv4-l3-protocol.cc:227-244 -> node.cc:118). */

/* Counters of a p2p run (both the oracle and the GPU engine fill this). */
typedef struct nsgpu_p2p_stats {
  uint64_t dispatched;        /* RemoveNext calls, setup and cancelled ones included */
  uint64_t cancelled;         /* dispatches of cancelled events */
  uint64_t digest;            /* order-sensitive digest of the (ts, uid) pop order */
  uint64_t final_ts;          /* Now () when Run returned */
  uint32_t next_uid;          /* DefaultSimulatorImpl::m_uid when Run returned */
  uint32_t windows;           /* GPU: parallel dispatch windows (0 for the oracle) */
  uint64_t ttl_drops;
  uint64_t no_route_drops;
  uint64_t max_window;
  uint64_t unreach_drops;     /* UDP datagrams with no bound endpoint */
  uint64_t refits;            /* GPU: windows cut back to the window capacity (0 for the oracle) */
  uint64_t icmp_sent;         /* ICMP errors sent (scenario icmp = 1) */
} nsgpu_p2p_stats;

/* Per-device counters: Queue (queue.cc:61-200) + device. */
typedef struct nsgpu_dev_counters {
  uint32_t enq_packets, enq_bytes;     /* m_nTotalReceivedPackets/Bytes */
  uint32_t drop_packets, drop_bytes;   /* m_nTotalDroppedPackets/Bytes */
  uint32_t deq_packets, tx_packets;    /* Dequeue calls returning a packet; TransmitStart calls */
  uint32_t rx_packets, pad_;           /* PointToPointNetDevice::Receive calls */
} nsgpu_dev_counters;

/* Per-application counters: OnOff sent packets/bytes, PacketSink received packets/bytes. */
typedef struct nsgpu_app_counters {
  uint32_t tx_packets, rx_packets;
  uint64_t tx_bytes, rx_bytes;
} nsgpu_app_counters;

/* Order-sensitive digest of a dispatch sequence: sum over k of mix(k, ts_k, uid_k).
 * Used to compare long dispatch orders (pop order) without moving whole logs. */
NSGPU_HD static inline uint64_t nsgpu_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
NSGPU_HD static inline uint64_t nsgpu_dispatch_digest_term(uint64_t rank, uint64_t ts, uint32_t uid) {
  return nsgpu_mix64(rank * 0x9e3779b97f4a7c15ULL ^ nsgpu_mix64(ts ^ ((uint64_t)uid << 40) ^ (uint64_t)uid));
}

/* ---------------- Wi-Fi PHY receive subset ----------------
 * YansWifiChannel::Send (yans-wifi-channel.cc:77-115) -> YansWifiChannel::Receive (:117-122) ->
 * YansWifiPhy::StartReceivePacket (yans-wifi-phy.cc:399-496) with its InterferenceHelper
 * (interference-helper.cc:129-212, 365-391) and WifiPhyStateHelper (wifi-phy-state-helper.cc:123-185,
 * 255-322, 392-416), EndReceive's state part (yans-wifi-phy.cc:770-799: NotifyRxEnd + DoSwitchFromRx)
 * and SendPacket's (:499-522).  The scenario is a PHY harness in the style of wifi-test.cc:181-260:
 * every transmission is a SendPacket call scheduled before Run (its uid is a setup uid), so the
 * transmission schedule is an input; the MAC, its DCF and EndReceive's m_random draw stay on the host
 * (SURVEY H13).  Channel switching — open-loop engine (nsgpu_wifi_*, this fixed schedule): no SWITCHING state;
 * closed-loop engine (nsgpu_wifil_*): nsgpu_wifil_set_channel. */
enum nsgpu_wifi_modclass { NSGPU_WIFI_DSSS = 0, NSGPU_WIFI_OFDM = 1, NSGPU_WIFI_ERP_OFDM = 2 };
enum nsgpu_wifi_store { NSGPU_WIFI_STORE_AUTO = 0, NSGPU_WIFI_STORE_LDS = 1, NSGPU_WIFI_STORE_HBM = 2,
                        NSGPU_WIFI_STORE_MASK = 3, NSGPU_WIFI_INLINE_RX = 4, NSGPU_WIFI_UNSORTED_RX = 8 };
enum nsgpu_wifi_preamble { NSGPU_WIFI_PREAMBLE_LONG = 0, NSGPU_WIFI_PREAMBLE_SHORT = 1 };

typedef struct nsgpu_wifi_scenario {
  int64_t n_phy;                /* YansWifiChannel::m_phyList, in Add order */
  const double *x, *y, *z;      /* ConstantPositionMobilityModel positions (the open-loop engine mirrors no other
                                 * model: its reception table assumes fixed distances) */
  const uint32_t *channel;      /* GetChannelNumber () */
  const uint32_t *node;         /* context of the Receive events (0xffffffff: no NetDevice) */
  nsgpu_loss_chain loss;
  double speed;                 /* ConstantSpeedPropagationDelayModel Speed */
  double rx_gain_db;            /* YansWifiPhy RxGain (default 1) */
  double ed_threshold_dbm;      /* EnergyDetectionThreshold (default -96) */
  double cca_threshold_dbm;     /* CcaMode1Threshold (default -99) */
  int64_t n_tx;                 /* SendPacket calls, in (ts, uid) order */
  const uint64_t *tx_ts;
  const uint32_t *tx_uid;       /* setup uids: all below uid_start */
  const uint32_t *tx_phy;
  const uint32_t *tx_size;      /* packet->GetSize () at the PHY */
  const double *tx_dbm;         /* GetPowerDbm (txPowerLevel) + TxGain: the channel's txPowerDbm */
  const uint32_t *tx_modclass;  /* the payload WifiMode (wifi-phy.cc:236-301) */
  const uint64_t *tx_rate_bps;
  const uint32_t *tx_bw_hz;
  const uint32_t *tx_preamble;  /* nsgpu_wifi_preamble */
  uint32_t uid_start;           /* DefaultSimulatorImpl::m_uid when Run starts */
  uint32_t ni_cap;              /* NiChanges capacity per phy (GPU); a longer list fails the run */
  uint64_t stop_ts;             /* Simulator::Stop event (ts, uid); stop_ts = ~0: none */
  uint32_t stop_uid;
  uint32_t pad_;
} nsgpu_wifi_scenario;

/* Outcome of one Receive event (StartReceivePacket's switch, yans-wifi-phy.cc:416-478). */
enum nsgpu_wifi_rx_outcome { NSGPU_WIFI_SYNC = 0, NSGPU_WIFI_DROP_RX = 1, NSGPU_WIFI_DROP_TX = 2,
                             NSGPU_WIFI_DROP_ED = 3, NSGPU_WIFI_NOT_RUN = 255 };
#define NSGPU_WIFI_F_CCA_EVAL   1u  /* maybeCcaBusy: GetEnergyDuration (CcaMode1Threshold) evaluated */
#define NSGPU_WIFI_F_CCA_SWITCH 2u  /* ... and non-zero: SwitchMaybeToCcaBusy */
#define NSGPU_WIFI_F_NEAR_ED    4u  /* rxPowerW within 1e-9 (relative) of EnergyDetectionThreshold */
#define NSGPU_WIFI_F_NEAR_CCA   8u  /* a noise+interference sum within 1e-9 of CcaMode1Threshold */

/* One Receive event, at slot [tx * n_phy + phy] (the sender's own slot stays NOT_RUN). */
typedef struct nsgpu_wifi_rx_log {
  uint64_t ts;       /* send time + delay */
  uint32_t uid;      /* uid base of the transmission + rank among the receivers */
  uint8_t outcome;   /* nsgpu_wifi_rx_outcome */
  uint8_t flags;     /* NSGPU_WIFI_F_* */
  uint16_t pad_;
  int64_t cca_ns;    /* GetEnergyDuration result when evaluated, else 0 */
} nsgpu_wifi_rx_log;

/* One EndReceive event (the Simulator::Schedule of a syncing StartReceivePacket, yans-wifi-phy.cc:469-471). */
#define NSGPU_WIFI_END_CANCELLED  1u  /* SendPacket while in Rx cancelled it (:510-514); still dispatched */
#define NSGPU_WIFI_END_DISPATCHED 2u  /* before the Stop event */
typedef struct nsgpu_wifi_end_record {
  uint64_t ts;
  uint64_t sync_ts;  /* the Receive event that synced */
  uint32_t uid;
  uint32_t phy;
  uint32_t tx;       /* transmission index of the packet */
  uint32_t flags;
} nsgpu_wifi_end_record;

typedef struct nsgpu_wifi_phy_counters {
  uint32_t rx, sync, drop_rx, drop_tx, drop_ed, cca_switches, end, end_cancelled;
  uint32_t ni_len;   /* NiChanges length when the run ended */
  uint32_t ni_max;
  int64_t end_tx, end_rx, end_cca_busy;  /* WifiPhyStateHelper m_endTx / m_endRx / m_endCcaBusy */
  double first_power;                    /* InterferenceHelper::m_firstPower */
  uint32_t rxing, pad_;
} nsgpu_wifi_phy_counters;

typedef struct nsgpu_wifi_stats {
  uint64_t dispatched;      /* SendPacket + Receive + EndReceive (+ Stop) dispatches, cancelled ones included */
  uint64_t tx, rx, sync, drop_rx, drop_tx, drop_ed, cca_evals, cca_switches, end, end_cancelled;
  uint64_t ni_inserts;      /* NiChange entries inserted */
  uint64_t near_threshold;  /* Receive events flagged NEAR_ED or NEAR_CCA */
  uint64_t digest;          /* sum of nsgpu_wifi_term over the dispatched events */
  uint64_t final_ts;        /* Now () when Run returned */
  uint32_t next_uid;        /* m_uid when Run returned */
  uint32_t ni_max;
} nsgpu_wifi_stats;

/* Digest term of a dispatched event: SendPacket (0, ts, uid, uid base of its fan-out, 0); Receive
 * (1, ts, tx, phy, outcome | (flags & 3) << 8 | cca_ns << 16); EndReceive (2, ts, uid, phy, cancelled);
 * Stop (3, ts, uid, 0, 0).  A Receive's uid is base + rank, so the SendPacket term pins it. */
NSGPU_HD static inline uint64_t nsgpu_wifi_term(uint64_t kind, uint64_t ts, uint64_t a, uint64_t b, uint64_t c) {
  return nsgpu_mix64(nsgpu_mix64(ts ^ (kind << 60)) + nsgpu_mix64(a * 0x9e3779b97f4a7c15ULL + b) +
                     c * 0xd1b54a32d192ed03ULL);
}

/* ---- closed-loop Wi-Fi PHY (nsgpu_wifil_*, attached to nsgpu_sim: SendPacket from host closures) ---- */
typedef struct nsgpu_wifil_config {
  int64_t n_phy;                /* YansWifiChannel::m_phyList, in Add order */
  const double *x, *y, *z;      /* positions at setup: every phy starts as a ConstantPositionMobilityModel; a
                                 * constant-velocity model is installed per phy afterwards (nsgpu_wifil_set_mobility) */
  const uint32_t *channel;      /* GetChannelNumber () */
  const uint32_t *node;         /* context of the Receive / EndReceive events */
  nsgpu_loss_chain loss;
  double speed;                 /* ConstantSpeedPropagationDelayModel Speed */
  double rx_gain_db;            /* YansWifiPhy RxGain (default 1) */
  double ed_threshold_dbm;      /* EnergyDetectionThreshold (default -96) */
  double cca_threshold_dbm;     /* CcaMode1Threshold (default -99) */
  double rx_noise_figure_db;    /* RxNoiseFigure (default 7): InterferenceHelper::SetNoiseFigure (DbToRatio) */
  uint32_t error_model;         /* nsgpu_wifil_error_model */
  uint32_t ni_cap;              /* NiChanges entries per phy (power of two); a longer list fails the run */
  uint32_t rxq_cap;             /* pending Receive events per phy (power of two) */
  uint32_t pad_;
  uint64_t tx_cap;              /* SendPacket calls over the run */
} nsgpu_wifil_config;
enum nsgpu_wifil_error_model { NSGPU_WIFIL_NIST = 0, NSGPU_WIFIL_YANS = 1 };  /* (YansWifiPhyHelper::Default: Nist) */

/* One EndReceive (yans-wifi-phy.cc:770-799): InterferenceHelper::CalculateSnrPer's result, for the host's
 * m_random draw (a cancelled one carries no snr / per). */
typedef struct nsgpu_wifil_end {
  uint64_t ts;
  uint32_t uid, phy;
  double snr, per;
  uint32_t tx;     /* the transmission (SendPacket call) it receives */
  uint32_t flags;  /* NSGPU_WIFI_END_CANCELLED */
  double rx_w;     /* the event's received power (InterferenceHelper::Event::GetRxPowerW): with snr, the
                    * MonitorSnifferRx signal / noise dBm of an Ok reception (yans-wifi-phy.cc:788-789) */
} nsgpu_wifil_end;

/* WifiPhyStateHelper of one phy at Now (wifi-phy-state-helper.cc:159-183). */
enum nsgpu_wifil_state { NSGPU_WIFIL_IDLE = 0, NSGPU_WIFIL_RX = 1, NSGPU_WIFIL_TX = 2, NSGPU_WIFIL_CCA_BUSY = 3,
                         NSGPU_WIFIL_SWITCHING = 4 };  /* (after nsgpu_wifil_set_channel, until m_endSwitching) */
typedef struct nsgpu_wifil_phy_state {
  uint32_t state;  /* nsgpu_wifil_state */
  uint32_t rxing;
  int64_t end_tx, end_rx, end_cca_busy;
  int64_t delay_until_idle;  /* GetDelayUntilIdle (:122-151); SWITCHING: m_endSwitching - now */
} nsgpu_wifil_phy_state;

/* YansWifiPhy::SetChannelNumber from a host closure (nsgpu_wifil_set_channel; yans-wifi-phy.cc:327-374). */
enum { NSGPU_WIFIL_SWITCH_DONE = 0,        /* the phy switched: SWITCHING until now + ChannelSwitchDelay */
       NSGPU_WIFIL_SWITCH_INIT = 1,        /* Now == 0: the channel number alone, no state change (:330-336) */
       NSGPU_WIFIL_SWITCH_POSTPONED = 2 }; /* the phy transmits: nothing changed; retry after retry_delay (:349-352) */
typedef struct nsgpu_wifil_switch {
  uint32_t outcome, prev_state;  /* NSGPU_WIFIL_SWITCH_*; nsgpu_wifil_state GetState () returned at :339 */
  int64_t retry_delay;           /* POSTPONED: GetDelayUntilIdle () = m_endTx - now, else 0 */
} nsgpu_wifil_switch;
typedef struct nsgpu_wifil_channel {
  uint32_t channel, pad_;                   /* GetChannelNumber () */
  int64_t start_switching, end_switching;   /* WifiPhyStateHelper m_startSwitching / m_endSwitching (0: never switched) */
  uint64_t switches, drop_switching;        /* switches made; frames dropped while SWITCHING (:419-436) */
} nsgpu_wifil_channel;

/* One StartReceivePacket of a notifying phy (nsgpu_wifil_notify): which branch of yans-wifi-phy.cc:417-495 it
 * took, with the arguments of the state helper's switches — what DcfManager::NotifyRxStartNow /
 * NotifyMaybeCcaBusyStartNow (dcf-manager.cc:591-641) and the State / RxOk traces are fed from. */
enum { NSGPU_WIFIL_NOTE_SYNC = 0, NSGPU_WIFIL_NOTE_DROP_RX = 1, NSGPU_WIFIL_NOTE_DROP_TX = 2, NSGPU_WIFIL_NOTE_DROP_ED = 3,
       NSGPU_WIFIL_NOTE_DROP_SWITCHING = 4 };  /* dropped while switching channels (:419-436), state = SWITCHING */
typedef struct nsgpu_wifil_note {
  uint64_t ts;            /* StartReceivePacket's Now () */
  uint32_t uid, phy;      /* the Receive event's uid; the receiver */
  uint32_t tx, kind;      /* transmission index (SendPacket calls in order); NSGPU_WIFIL_NOTE_* */
  uint32_t state, pad_;   /* nsgpu_wifil_state GetState () returned at :417, before any switch */
  int64_t rx_duration;    /* ns (the argument of SwitchToRx / NotifyRxStart on a sync) */
  int64_t cca_duration;   /* GetEnergyDuration's result when maybeCcaBusy was reached and it is non-zero
                             (the argument of SwitchMaybeToCcaBusy), else 0 */
} nsgpu_wifil_note;

/* ConstantVelocityHelper of one phy's node (constant-velocity-helper.h; nsgpu_wifil_set_mobility /
 * nsgpu_wifil_get_mobility): what ConstantVelocityMobilityModel, Ns2MobilityHelper's replays and
 * RandomWaypointMobilityModel's legs integrate through.  The device restates ConstantVelocityHelper::Update
 * (constant-velocity-helper.cc:69-84) at every accumulation point, in the reference's order of operations. */
typedef struct nsgpu_mobility {
  double pos[3], vel[3];   /* m_position, m_velocity (get: GetVelocity — zero while paused) */
  int64_t last_update;     /* m_lastUpdate, ns */
  uint32_t paused, pad_;   /* m_paused (a fresh ConstantVelocityMobilityModel is paused) */
} nsgpu_mobility;

/* The closed-loop PHY's extended loss chain (nsgpu_wifil_set_loss): the PropagationLossModels that are not a
 * function of the distance alone, next to the nsgpu_loss_kind ones.  nsgpu_loss_model / nsgpu_loss_chain keep their
 * layout (the oracle shares it); an extended chain is installed on a handle by a call of its own. */
enum nsgpu_lossx_kind {            /* 0-4: the nsgpu_loss_kind values, same meaning, parameters in p[0..2] */
  NSGPU_LOSSX_TWO_RAY_GROUND = 5,  /* p0 lambda, p1 system loss, p2 min distance, p3 HeightAboveZ   (:323-409) */
  NSGPU_LOSSX_THREE_LOG      = 6,  /* p0-p2 distance0..2, p3-p5 exponent0..2, p6 reference loss     (:548-587) */
  NSGPU_LOSSX_MATRIX         = 7   /* p0 DefaultLoss; entries in the nsgpu_lossx's table            (:781-796) */
};
typedef struct nsgpu_lossx_model { int32_t kind, pad_; double p[8]; } nsgpu_lossx_model;   /* 72 bytes */
/* MatrixPropagationLossModel::SetLoss (a, b, loss, false) (:752-772): a, b are phy indices (ns-3 keys its map by
 * MobilityModel pointer; a binding maps one to the other).  A symmetric SetLoss is two entries. */
typedef struct nsgpu_lossx_entry { uint32_t a, b; double loss_db; } nsgpu_lossx_entry;
typedef struct nsgpu_lossx {
  int32_t n, pad_;                       /* links, <= NSGPU_MAX_LOSS_CHAIN; at most one MATRIX link */
  nsgpu_lossx_model m[NSGPU_MAX_LOSS_CHAIN];
  const nsgpu_lossx_entry *entry;        /* host pointer, any order; a later duplicate (a, b) wins, as SetLoss does */
  uint64_t n_entry;
} nsgpu_lossx;

/* The closed-loop PHY's two other deterministic mobility models (nsgpu_wifil_set_waypoints / _set_acceleration and
 * their neighbours); nsgpu_mobility above keeps its layout and its calls.
 *
 * Waypoint (src/mobility/model/waypoint.h): a time in ns and a position. */
typedef struct nsgpu_waypoint {
  uint64_t time;           /* ns */
  double pos[3];
} nsgpu_waypoint;          /* 32 bytes */
/* What nsgpu_wifil_get_waypoints returns: WaypointMobilityModel's members after the Update of a position read
 * (waypoint-mobility-model.h: m_current, m_next, m_velocity, m_first; WaypointsLeft ()).  m_next.time is signed in
 * the reference: Update sets it to Seconds (-1) when the list has run out (:134), which next_ended carries. */
typedef struct nsgpu_waypoint_state {
  uint64_t cur_time;       /* m_current.time, ns */
  double cur_pos[3];       /* m_current.position: the phy's position */
  uint64_t next_time;      /* m_next.time, ns (0 when next_ended) */
  double next_pos[3];      /* m_next.position */
  double vel[3];           /* m_velocity, as the position's Update left it (DoGetVelocity makes no Update, :211-214) */
  uint32_t next_ended;     /* 1: m_next.time == Seconds (-1) */
  uint32_t first;          /* m_first: set again by EndMobility */
  uint32_t left, pad_;     /* WaypointsLeft (): m_waypoints.size () */
} nsgpu_waypoint_state;    /* 104 bytes */
/* ConstantAccelerationMobilityModel's members (constant-acceleration-mobility-model.h).  set_acceleration reads
 * pos / vel / acc / base_time as m_basePosition / m_baseVelocity / m_acceleration / m_baseTime; get_acceleration
 * returns the same four and, in now_pos / now_vel, DoGetPosition () / DoGetVelocity () at the call's `now`. */
typedef struct nsgpu_accel {
  double pos[3], vel[3], acc[3];
  int64_t base_time;       /* ns */
  double now_pos[3], now_vel[3];   /* (get only; ignored by set) */
} nsgpu_accel;             /* 128 bytes */

#ifdef __cplusplus
}
#endif
#endif /* NSGPU_TYPES_H */
