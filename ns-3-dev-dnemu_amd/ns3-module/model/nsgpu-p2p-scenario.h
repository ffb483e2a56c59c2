/* -*- Mode:C++; c-file-style:"gnu"; indent-tabs-mode:nil; -*- */
/*
 * ns3::NsgpuP2pScenario — the GPU-resident point-to-point subset of an ns-3 program (include/nsgpu.h,
 * nsgpu_p2p_create), in the order the program builds it, so that the setup-time Schedule calls — and
 * therefore every uid — come out as the reference's (node-list.cc:124-131, node.cc:111-145,
 * point-to-point-helper.cc:228-242, ipv4-l3-protocol.cc:227-244).  Two ways to fill it:
 *   - FromNodeList: the program built its topology with the stock helpers (NodeContainer::Create,
 *     PointToPointHelper::Install, InternetStackHelper::Install, Ipv4AddressHelper::Assign, OnOffHelper /
 *     PacketSinkHelper / UdpEcho*Helper::Install, Simulator::Stop) under HipSimulatorImpl; the scenario is
 *     read back from NodeList, the devices' / channels' / queues' / applications' attributes and the Ipv4
 *     interfaces, and its setup list from HipSimulatorImpl's setup journal.  AdoptInto then hands the
 *     program's setup events to the engine (HipSimulatorImpl::AdoptDeviceSubset);
 *   - by hand: AddNode / Link / InstallStack / Assign / AddPacketSink / AddOnOff / Stop, in program order,
 *     then HipSimulatorImpl::AttachDeviceSubset before anything is scheduled.
 * WriteTraces hands the engine's trace records to the helpers' own sinks: the ascii lines to an
 * OutputStreamWrapper (AsciiTraceHelper), the pcap records to one PcapFileWrapper per device, created
 * and named as PointToPointHelper::EnablePcapAll names them (PcapHelper::GetFilenameFromDevice, DLT_PPP).
 * tests/ use the Python twin of this class (ns-3-dev-dnemu_amd/p2p.py).
 */
#ifndef NSGPU_P2P_SCENARIO_H
#define NSGPU_P2P_SCENARIO_H

#include "ns3/nstime.h"
#include "ns3/ptr.h"
#include "ns3/application.h"
#include "nsgpu.h"
#include "hip-simulator-impl.h"
#include <stdint.h>
#include <string>
#include <vector>
#include <utility>

namespace ns3 {

class OutputStreamWrapper;
class NetDevice;

class NsgpuP2pScenario
{
public:
  NsgpuP2pScenario ();
  ~NsgpuP2pScenario ();

  uint32_t AddNode (void);
  /* PointToPointHelper::Install (a, b): device on a, then device on b; returns both device indices */
  std::pair<uint32_t, uint32_t> Link (uint32_t a, uint32_t b, uint64_t bps, Time delay, uint32_t queueMaxPackets,
                                      Time interframeGap);
  void InstallStack (void);
  uint32_t AddPacketSink (uint32_t node, Time start, Time stop, uint16_t port = 9);
  /* UdpClientHelper (address of dstNode, remotePort).Install / UdpServerHelper (port).Install; packetSize counts the
   * 12-byte SeqTsHeader ([12, 1472]; with SetFragmentation [12, 1500]), packetWindowSize is a multiple of 8 in [8, 256] */
  uint32_t AddUdpClient (uint32_t node, uint32_t dstNode, Time start, Time stop, uint32_t maxPackets, Time interval,
                         uint32_t packetSize, uint32_t ttl, uint16_t remotePort = 100);
  uint32_t AddUdpServer (uint32_t node, Time start, Time stop, uint16_t port = 100, uint16_t packetWindowSize = 32);
  /* UdpServer::GetReceived () / GetLost () of application `app` (a UdpServer) as the engine counts them now */
  void GetUdpServer (uint32_t app, uint32_t &received, uint32_t &lost) const;
  /* UdpTraceClientHelper (address of dstNode, remotePort, filename).Install (udp-trace-client.cc): `entries` as
   * LoadTrace / LoadDefaultTrace leave them (LoadTraceFile; DefaultTrace), maxPacketSize in [1, 1472].  One Send event
   * emits every entry up to the next one whose timeToSend is not 0, a frame above maxPacketSize cut into datagrams; at
   * most NSGPU_UDP_TRACE_MAX_BURST datagrams a Send.  GetUdpTraceClient: m_sent, m_currentEntry and the Send events
   * run, as the engine counts them now. */
  uint32_t AddUdpTraceClient (uint32_t node, uint32_t dstNode, Time start, Time stop,
                              const std::vector<nsgpu_udp_trace_entry> &entries, uint32_t maxPacketSize, uint32_t ttl,
                              uint16_t remotePort = 100);
  static std::vector<nsgpu_udp_trace_entry> LoadTraceFile (std::string filename);  /* "": the default trace */
  static std::vector<nsgpu_udp_trace_entry> DefaultTrace (void) { return LoadTraceFile (""); }
  void GetUdpTraceClient (uint32_t app, uint32_t &sent, uint32_t &currentEntry, uint32_t &sends) const;
  /* FromNodeList mirrors a UdpTraceClient only when the program declared its trace here before: the application's
   * m_entries are private and its TraceFilename attribute has no getter, so the file (or "": the default trace) cannot
   * be read back from the object.  An undeclared UdpTraceClient ends FromNodeList in a fatal error.  A file is loaded
   * here as the application loaded it; SetRemote's clearing of the entries and SetTraceFile during Run are not modelled. */
  void DeclareTrace (Ptr<Application> app, std::string filename);
  /* onVar / offVar: a UniformVariable or an ExponentialVariable OnTime / OffTime instead of the ConstantVariable
   * onSeconds / offSeconds (0, or a variable of kind NSGPU_RV_CONSTANT: the constant).  UniformVar / ExponentialVar
   * make one; `stream` is the index of the RngStream the program constructs for that variable (0-based, as for
   * SetRateErrorModel: the engine cannot discover the order, the caller names it), seeded by SetRng's RngSeed / RngRun.
   * The OnOff application draws Seconds (offVar) when it schedules StartSending and Seconds (onVar) when it schedules
   * StopSending (onoff-application.cc:221-237).  An Exponential's log is the device's own (double-double); a draw
   * whose timestamp could differ under the host's libm log is logged as ambiguous, not fatal: GetOnOffDraws and
   * GetAmbiguousDraws read the counts and the log (an empty log with overflow 0: the run is the reference's). */
  uint32_t AddOnOff (uint32_t node, uint32_t dstNode, Time start, Time stop, uint64_t rateBps, uint32_t packetSize,
                     double onSeconds, double offSeconds, uint32_t maxBytes, uint32_t ttl,
                     const nsgpu_ranvar *onVar = 0, const nsgpu_ranvar *offVar = 0);
  static nsgpu_ranvar UniformVar (double min, double max, uint32_t stream);
  static nsgpu_ranvar ExponentialVar (double mean, double bound, uint32_t stream);
  void GetOnOffDraws (uint32_t app, uint32_t &onDraws, uint32_t &offDraws, uint32_t &ambiguous) const;
  std::vector<nsgpu_ambiguous_draw> GetAmbiguousDraws (uint64_t &overflow) const;
  /* FromNodeList mirrors an OnOffApplication with a UniformVariable OnTime / OffTime (the attribute prints
   * "Uniform:min:max") only when the streams of its two variables were named here before; an ExponentialVariable
   * cannot be told from the attribute at all (random-variable.cc:1931-1957 prints Constant, Uniform and Normal only,
   * and the Impl classes are private to that file), so the program declares it whole: which = 0 the OnTime, 1 the
   * OffTime; bound 0: none.  An undeclared non-constant variable ends FromNodeList in a fatal error. */
  void DeclareOnOffStreams (Ptr<Application> app, uint32_t onStream, uint32_t offStream);
  void DeclareOnOffExponential (Ptr<Application> app, uint32_t which, double mean, double bound, uint32_t stream);
  void Stop (Time at);
  /* Ipv4AddressHelper (network, mask).Assign on the two devices of a link (host .1 on a, .2 on b) and
   * Ipv4L3Protocol::AddInterface's interface numbering (the loopback is interface 0) */
  void Assign (uint32_t da, uint32_t db, uint32_t network, uint32_t mask = 0xffffff00u);
  /* InternetStackHelper installs Icmpv4L4Protocol: TTL expiries and unbound arrivals send ICMP errors back
   * to the sender (icmpv4-l4-protocol.cc:131-165).  On by default, as in the reference. */
  void SetIcmp (bool on);
  /* Ipv4L3Protocol fragments a datagram above the devices' 1500-byte MTU and reassembles it at its destination
   * (ipv4-l3-protocol.cc:722-761, 1116-1412).  Off by default: a payload above 1472 bytes is then refused.  On:
   * OnOff / UdpEchoClient payloads up to 65507 bytes, UdpClient PacketSize up to 1500, at most one fragmenting flow
   * into a node; timeout = Ipv4L3Protocol::FragmentExpirationTimeout (zero: its default, 30 s).  FromNodeList turns
   * it on when an application's PacketSize needs it and reads the timeout from the nodes' Ipv4L3Protocol: one positive
   * value for all nodes (a timeout set here before must equal it; 0 is fatal, it would mean "default" to the engine). */
  void SetFragmentation (bool on, Time timeout = Time ());
  /* PointToPointNetDevice::SetReceiveErrorModel on engine device `dev` (point-to-point-net-device.cc:304-317: a frame
   * the model declares corrupt fires PhyRxDrop and nothing else).  ReceiveListErrorModel: the frames whose 0-based
   * arrival ordinal at the device is in `packets`.  RateErrorModel: ErrorRate `rate`, ErrorUnit `unit`
   * (NSGPU_EU_PKT / _BYTE / _BIT), and `stream`: the model's UniformVariable (0, 1) is the stream-th RngStream the
   * program constructs (0-based) — the engine cannot discover that order, the caller names it.  A disabled model
   * counts, draws and drops nothing.  Enable / Disable / Reset / SetList / SetRate during Run are not modelled. */
  void SetReceiveListErrorModel (uint32_t dev, const std::vector<uint32_t> &packets, bool enabled = true);
  void SetRateErrorModel (uint32_t dev, double rate, uint32_t unit, uint32_t stream, bool enabled = true);
  /* RngSeed / RngRun of the Rate models' streams (0: the reference's default, 1); FromNodeList reads the GlobalValues */
  void SetRng (uint32_t seed, uint32_t run);
  /* FromNodeList mirrors a device's RateErrorModel only when its stream was named here before (the device is the
   * program's own PointToPointNetDevice); without it FromNodeList ends in a fatal error */
  void SetErrorStream (Ptr<NetDevice> device, uint32_t stream);
  /* IsCorrupt calls on engine device `dev`'s enabled model and the frames it declared corrupt, as the engine counts
   * them now */
  void GetErrorModel (uint32_t dev, uint32_t &invoked, uint32_t &corrupted) const;
  /* FlowMonitor's per-flow statistics (flow-monitor.cc:121-300, ipv4-flow-probe.cc:192-346), accumulated by the
   * engine during Run: call before CreateEngine.  The run itself is unchanged — this object installs no FlowMonitor,
   * so the uids a real one's own events would take (StartRightNow, its check every simulated second) are not taken.
   * Not with SetFragmentation, and not for an engine a host-closure runtime adopts (AdoptInto): both end in a
   * fatal error at CreateEngine / AdoptInto.  GetFlowStats: 2 x applications records — flow a = application a's
   * datagrams, flow applications + a = the echo replies to UdpEchoClient a (zeros for a flow that sent nothing);
   * FlowIds follow the order of first_tx_ts / first_tx_uid.  lost_packets includes CheckForLostPackets (maxDelay) now
   * (Seconds (10): the MaxPerHopDelay attribute's default).  Histograms, per-probe statistics and the XML file are
   * not produced. */
  void EnableFlowStats (void);
  std::vector<nsgpu_flow_record> GetFlowStats (Time maxDelay = Seconds (10)) const;
  /* Ipv4GlobalRoutingHelper::PopulateRoutingTables on the GPU (nsgpu_route_global): next hops towards every
   * flow destination and, with ICMP, every sender.  With every device addressed the ties are global
   * routing's (lowest peer address, then interface); an unaddressed topology takes the lowest device. */
  void PopulateRoutingTables (void);
  void RouteShortestPaths (void) { PopulateRoutingTables (); }

  /* The scenario of the program's own topology: NodeList (node-list.cc), each node's devices in
   * Node::AddDevice order — PointToPointNetDevice DataRate / InterframeGap / TxQueue (DropTailQueue in
   * PACKETS mode: MaxPackets), its PointToPointChannel's Delay and peer; the LoopbackNetDevice — its Ipv4
   * interfaces (address, interface index), DefaultTtl, and its applications in Node::AddApplication order
   * (OnOffApplication DataRate / PacketSize / Remote / OnTime / OffTime (ConstantVariable; UniformVariable with
   * DeclareOnOffStreams, ExponentialVariable with DeclareOnOffExponential) / MaxBytes,
   * PacketSink Local (Any, port), UdpEchoServer Port, UdpEchoClient RemoteAddress / RemotePort / MaxPackets /
   * Interval / PacketSize, UdpClient RemoteAddress / RemotePort / MaxPackets / Interval / PacketSize, UdpServer Port /
   * PacketWindowSize, UdpTraceClient RemoteAddress / RemotePort / MaxPacketSize with the trace DeclareTrace named;
   * StartTime / StopTime).  The UDP ports are always given to the engine: a datagram reaches the
   * application bound to its destination port, a node may host several bound applications on distinct ports.  The setup list follows `impl`'s journal: per node, its first
   * zero-delay call is Node::Start, the next ones its devices' NetDevice::Start then its applications'
   * Application::Start (the helpers add devices before applications); the Stop event; every other call
   * keeps its uid on the host (NSGPU_SETUP_UID).  A device's ReceiveErrorModel attribute is mirrored: a
   * ReceiveListErrorModel (GetList, IsEnabled), a RateErrorModel (GetRate, GetUnit, IsEnabled) whose stream
   * SetErrorStream named, RngSeed / RngRun from the GlobalValues.  Anything outside the GPU-resident subset (another
   * device type, an undeclared or unmodelled random OnTime, two applications bound to one port of a node, a ListErrorModel or any other
   * ErrorModel subclass, a RateErrorModel without a named stream, ...) is a fatal error. */
  void FromNodeList (Ptr<HipSimulatorImpl> impl);
  /* The journal entries the engine dispatches from now on (FromNodeList) */
  const std::vector<uint32_t> &GetOwnedSetupCalls (void) const { return m_owned; }

  /* The engine (owned by this object); `poolCap` / `logCap` as nsgpu_p2p_create's */
  nsgpu_p2p *CreateEngine (uint64_t poolCap, uint64_t logCap);
  /* FromNodeList's engine joins impl's order: its setup events leave the host queue */
  void AdoptInto (Ptr<HipSimulatorImpl> impl);

  /* Record the device sinks' calls during Run (nsgpu_p2p_set_trace; call before Run), then, after it,
   * write them through the helpers' sinks: the EnableAsciiAll (stream) lines to `ascii` (null: none) and
   * the EnablePcapAll (prefix) files `pcapPrefix`-<node>-<device>.pcap (empty: none).  Lines and records
   * are in the dispatch order of the events that made them ((ts, uid), then call order). */
  void EnableTraceRecords (uint64_t capacity);
  void WriteTraces (Ptr<OutputStreamWrapper> ascii, std::string pcapPrefix);

private:
  struct Dev
  {
    uint32_t node, peer, qmax;
    uint64_t bps;
    int64_t ifg, delay;
  };
  struct App
  {
    uint32_t kind, node, dst, size, maxBytes, ttl;
    int64_t start, stop;
    uint64_t rate;
    double on, off;
    uint32_t count;        // UdpEchoClient MaxPackets
    int64_t interval;      // UdpEchoClient Interval
    uint32_t remoteAddr;   // the sender's Remote address (0: its destination's first interface)
    uint32_t remotePort;
    uint32_t port;         // bound port of a PacketSink / UdpEchoServer / UdpServer
    uint32_t window;       // UdpServer PacketWindowSize
    std::vector<nsgpu_udp_trace_entry> entries;  // UdpTraceClient m_entries
    nsgpu_ranvar onVar, offVar;  // OnOff: the OnTime / OffTime variables (kind NSGPU_RV_CONSTANT: on / off above)
  };
  struct OnOffDecl  // DeclareOnOffStreams / DeclareOnOffExponential
  {
    Ptr<Application> app;
    bool streams, exponential[2];
    uint32_t stream[2];
    nsgpu_ranvar var[2];
  };
  OnOffDecl &OnOffDeclOf (Ptr<Application> app);
  void MirrorOnOffTime (const RandomVariable &v, uint32_t which, uint32_t node, Ptr<Application> app, double &seconds,
                        nsgpu_ranvar &var) const;
  struct Em
  {
    uint32_t kind, enabled, unit, stream;  // NSGPU_EM_*, IsEnabled (), NSGPU_EU_*, the RngStream's index
    double rate;
    std::vector<uint32_t> list;
  };
  uint32_t AddApp (const App &a);
  /* the engine's view (kept alive for the trace codec) */
  void Fill (void);

  uint32_t m_nodes;
  std::vector<Dev> m_dev;
  std::vector<App> m_app;
  std::vector<std::pair<uint32_t, uint32_t> > m_setup;  // (nsgpu_setup_kind, index), program order
  std::vector<uint32_t> m_route;                        // [node][slot]
  std::vector<uint32_t> m_dstSlot;                      // node -> route slot (0xffffffff: none)
  std::vector<uint32_t> m_addr, m_ifindex;              // per device (address 0: unassigned)
  std::vector<uint32_t> m_nif;                          // next interface index per node
  std::vector<uint32_t> m_owned;                        // FromNodeList: the journal entries the engine owns
  std::vector<Ptr<NetDevice> > m_devObj;                // FromNodeList: the ns-3 device of each engine device
  std::vector<Em> m_em;                                 // per device (empty: no device has a receive error model)
  std::vector<std::pair<Ptr<NetDevice>, uint32_t> > m_errorStream;  // SetErrorStream
  std::vector<std::pair<Ptr<Application>, std::string> > m_declaredTrace;  // DeclareTrace
  std::vector<OnOffDecl> m_declaredOnOff;
  uint32_t m_nDst;
  bool m_icmp;
  bool m_frag;
  int64_t m_fragTimeout;                                // FragmentExpirationTimeout (ns; 0: the default)
  bool m_flowStats;                                     // EnableFlowStats
  uint32_t m_rngSeed, m_rngRun;                         // RngSeed / RngRun of the Rate error models' streams (0: 1)
  int64_t m_stop;
  bool m_firstLink;
  nsgpu_p2p *m_engine;
  nsgpu_trace_codec *m_codec;
  // the C view (Fill)
  nsgpu_p2p_scenario m_sc;
  nsgpu_p2p_scenario_ext m_ext;  // the UdpTraceClients' entries and the OnOff variables (m_hasTrace || m_hasVar:
  bool m_hasTrace, m_hasVar;     // given to the _ex entry points)
  std::vector<nsgpu_ranvar> m_cOnVar, m_cOffVar;
  std::vector<uint64_t> m_cTraceOff;
  std::vector<nsgpu_udp_trace_entry> m_cTraceEnt;
  std::vector<uint32_t> m_cDevNode, m_cDevPeer, m_cDevQmax, m_cKind, m_cNode, m_cDst, m_cSlot, m_cSrc, m_cSize,
    m_cMaxb, m_cTtl, m_cCount, m_cSk, m_cSi, m_cRaddr, m_cRport, m_cPort, m_cWindow, m_cEmKind, m_cEmEnabled,
    m_cEmUnit, m_cEmStream, m_cEmList;
  std::vector<uint64_t> m_cDevBps, m_cRate, m_cEmOff;
  std::vector<double> m_cEmRate;
  std::vector<int64_t> m_cDevIfg, m_cDevDelay, m_cStart, m_cStop, m_cIvl;
  std::vector<double> m_cOn, m_cOff;
};

} // namespace ns3

#endif /* NSGPU_P2P_SCENARIO_H */
