/* -*- Mode:C++; c-file-style:"gnu"; indent-tabs-mode:nil; -*- */
#include "nsgpu-p2p-scenario.h"
#include "ns3/fatal-error.h"
#include "ns3/node-list.h"
#include "ns3/node.h"
#include "ns3/application.h"
#include "ns3/point-to-point-net-device.h"
#include "ns3/point-to-point-channel.h"
#include "ns3/loopback-net-device.h"
#include "ns3/drop-tail-queue.h"
#include "ns3/error-model.h"
#include "ns3/pointer.h"
#include "ns3/global-value.h"
#include "ns3/integer.h"
#include "ns3/ipv4.h"
#include "ns3/ipv4-l3-protocol.h"
#include "ns3/ipv4-list-routing.h"
#include "ns3/ipv4-static-routing.h"
#include "ns3/ipv4-global-routing.h"
#include "ns3/ipv4-routing-table-entry.h"
#include "ns3/onoff-application.h"
#include "ns3/packet-sink.h"
#include "ns3/udp-echo-client.h"
#include "ns3/udp-echo-server.h"
#include "ns3/udp-client.h"
#include "ns3/udp-server.h"
#include "ns3/udp-trace-client.h"
#include "ns3/inet-socket-address.h"
#include "ns3/address.h"
#include "ns3/uinteger.h"
#include "ns3/enum.h"
#include "ns3/data-rate.h"
#include "ns3/random-variable.h"
#include "ns3/output-stream-wrapper.h"
#include "ns3/pcap-file-wrapper.h"
#include "ns3/trace-helper.h"
#include <algorithm>
#include <cstdlib>
#include <map>
#include <sstream>

namespace ns3 {

#define NSGPU_TRY(call)                                                     \
  do {                                                                      \
      if ((call) != NSGPU_OK)                                               \
        {                                                                   \
          NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());             \
        }                                                                   \
    } while (false)

NsgpuP2pScenario::NsgpuP2pScenario ()
  : m_nodes (0),
    m_nDst (0),
    m_icmp (true),
    m_frag (false),
    m_fragTimeout (0),
    m_flowStats (false),
    m_rngSeed (0),
    m_rngRun (0),
    m_stop (-1),
    m_firstLink (true),
    m_engine (0),
    m_codec (0),
    m_hasTrace (false),
    m_hasVar (false)
{
}

NsgpuP2pScenario::~NsgpuP2pScenario ()
{
  if (m_codec != 0)
    {
      nsgpu_trace_codec_free (m_codec);
    }
  if (m_engine != 0)
    {
      nsgpu_p2p_destroy (m_engine);
    }
}

uint32_t
NsgpuP2pScenario::AddNode (void)
{
  if (m_nodes == 0)
    {
      m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_UID, 0u));  // NodeListPriv's ScheduleDestroy
    }
  m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_NODE, m_nodes));
  return m_nodes++;
}

std::pair<uint32_t, uint32_t>
NsgpuP2pScenario::Link (uint32_t a, uint32_t b, uint64_t bps, Time delay, uint32_t queueMaxPackets, Time interframeGap)
{
  const uint32_t da = m_dev.size (), db = da + 1;
  Dev x = {a, db, queueMaxPackets, bps, interframeGap.GetTimeStep (), delay.GetTimeStep ()};
  Dev y = {b, da, queueMaxPackets, bps, interframeGap.GetTimeStep (), delay.GetTimeStep ()};
  m_dev.push_back (x);
  m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_DEVICE, da));
  m_dev.push_back (y);
  m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_DEVICE, db));
  m_addr.resize (m_dev.size (), 0u);
  m_ifindex.resize (m_dev.size (), 0u);
  if (m_firstLink)
    {
      m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_UID, 0u));  // ChannelListPriv's ScheduleDestroy
      m_firstLink = false;
    }
  return std::make_pair (da, db);
}

void
NsgpuP2pScenario::InstallStack (void)
{
  for (uint32_t n = 0; n < m_nodes; n++)
    {
      m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_NOOP, n));  // LoopbackNetDevice
    }
}

uint32_t
NsgpuP2pScenario::AddApp (const App &a)
{
  m_app.push_back (a);
  m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_APP, (uint32_t) (m_app.size () - 1)));
  return m_app.size () - 1;
}

uint32_t
NsgpuP2pScenario::AddPacketSink (uint32_t node, Time start, Time stop, uint16_t port)
{
  App a = {NSGPU_APP_SINK, node, 0, 0, 0, 0, start.GetTimeStep (), stop.GetTimeStep (), 0, 0.0, 0.0, 0, 0, 0, 0,
           port, 0};
  return AddApp (a);
}

uint32_t
NsgpuP2pScenario::AddUdpClient (uint32_t node, uint32_t dstNode, Time start, Time stop, uint32_t maxPackets,
                                Time interval, uint32_t packetSize, uint32_t ttl, uint16_t remotePort)
{
  App a = {NSGPU_APP_UDP_CLIENT, node, dstNode, packetSize, 0, ttl, start.GetTimeStep (), stop.GetTimeStep (), 0, 0.0,
           0.0, maxPackets, interval.GetTimeStep (), 0, remotePort, 0, 0};
  return AddApp (a);
}

uint32_t
NsgpuP2pScenario::AddUdpServer (uint32_t node, Time start, Time stop, uint16_t port, uint16_t packetWindowSize)
{
  App a = {NSGPU_APP_UDP_SERVER, node, 0, 0, 0, 0, start.GetTimeStep (), stop.GetTimeStep (), 0, 0.0, 0.0, 0, 0, 0, 0,
           port, packetWindowSize};
  return AddApp (a);
}

uint32_t
NsgpuP2pScenario::AddUdpTraceClient (uint32_t node, uint32_t dstNode, Time start, Time stop,
                                     const std::vector<nsgpu_udp_trace_entry> &entries, uint32_t maxPacketSize,
                                     uint32_t ttl, uint16_t remotePort)
{
  App a = {NSGPU_APP_UDP_TRACE_CLIENT, node, dstNode, maxPacketSize, 0, ttl, start.GetTimeStep (), stop.GetTimeStep (),
           0, 0.0, 0.0, 0, 0, 0, remotePort, 0, 0};
  a.entries = entries;
  return AddApp (a);
}

std::vector<nsgpu_udp_trace_entry>
NsgpuP2pScenario::LoadTraceFile (std::string filename)
{
  // UdpTraceClient::SetTraceFile (udp-trace-client.cc:143-154): "" -> LoadDefaultTrace, else LoadTrace (filename)
  uint64_t n = 0;
  if (filename == "")
    {
      NSGPU_TRY (nsgpu_udp_trace_default (0, 0, &n));
    }
  else
    {
      NSGPU_TRY (nsgpu_udp_trace_load (filename.c_str (), 0, 0, &n));
    }
  std::vector<nsgpu_udp_trace_entry> e (std::max (n, (uint64_t) 1));
  if (filename == "")
    {
      NSGPU_TRY (nsgpu_udp_trace_default (&e[0], n, &n));
    }
  else
    {
      NSGPU_TRY (nsgpu_udp_trace_load (filename.c_str (), &e[0], n, &n));
    }
  e.resize (n);
  return e;
}

void
NsgpuP2pScenario::DeclareTrace (Ptr<Application> app, std::string filename)
{
  m_declaredTrace.push_back (std::make_pair (app, filename));
}

void
NsgpuP2pScenario::GetUdpTraceClient (uint32_t app, uint32_t &sent, uint32_t &currentEntry, uint32_t &sends) const
{
  if (m_engine == 0 || app >= m_app.size () || m_app[app].kind != NSGPU_APP_UDP_TRACE_CLIENT)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::GetUdpTraceClient: application " << app << " is not a UdpTraceClient of an engine");
    }
  std::vector<nsgpu_udp_trace_client_record> rec (m_app.size ());
  if (nsgpu_p2p_udp_trace_clients (m_engine, &rec[0], 0) != NSGPU_OK)
    {
      NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());
    }
  sent = rec[app].sent;
  currentEntry = rec[app].current_entry;
  sends = rec[app].sends;
}

void
NsgpuP2pScenario::GetUdpServer (uint32_t app, uint32_t &received, uint32_t &lost) const
{
  if (m_engine == 0 || app >= m_app.size () || m_app[app].kind != NSGPU_APP_UDP_SERVER)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::GetUdpServer: application " << app << " is not a UdpServer of an engine");
    }
  std::vector<nsgpu_udp_server_record> rec (m_app.size ());
  if (nsgpu_p2p_udp_servers (m_engine, &rec[0], 0) != NSGPU_OK)
    {
      NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());
    }
  received = rec[app].received;
  lost = rec[app].lost;
}

uint32_t
NsgpuP2pScenario::AddOnOff (uint32_t node, uint32_t dstNode, Time start, Time stop, uint64_t rateBps,
                            uint32_t packetSize, double onSeconds, double offSeconds, uint32_t maxBytes, uint32_t ttl,
                            const nsgpu_ranvar *onVar, const nsgpu_ranvar *offVar)
{
  App a = {NSGPU_APP_ONOFF, node, dstNode, packetSize, maxBytes, ttl, start.GetTimeStep (), stop.GetTimeStep (),
           rateBps, onSeconds, offSeconds, 0, 0, 0, 9};
  a.onVar = onVar ? *onVar : nsgpu_ranvar ();
  a.offVar = offVar ? *offVar : nsgpu_ranvar ();
  if (a.onVar.kind == NSGPU_RV_CONSTANT && onVar)
    {
      a.on = onVar->p0;
    }
  if (a.offVar.kind == NSGPU_RV_CONSTANT && offVar)
    {
      a.off = offVar->p0;
    }
  return AddApp (a);
}

nsgpu_ranvar
NsgpuP2pScenario::UniformVar (double min, double max, uint32_t stream)
{
  nsgpu_ranvar v = {NSGPU_RV_UNIFORM, stream, min, max};
  return v;
}

nsgpu_ranvar
NsgpuP2pScenario::ExponentialVar (double mean, double bound, uint32_t stream)
{
  nsgpu_ranvar v = {NSGPU_RV_EXPONENTIAL, stream, mean, bound};
  return v;
}

void
NsgpuP2pScenario::GetOnOffDraws (uint32_t app, uint32_t &onDraws, uint32_t &offDraws, uint32_t &ambiguous) const
{
  if (m_engine == 0 || app >= m_app.size () || m_app[app].kind != NSGPU_APP_ONOFF)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::GetOnOffDraws: application " << app << " is not an OnOff of an engine");
    }
  std::vector<nsgpu_onoff_draw_record> rec (m_app.size ());
  if (nsgpu_p2p_onoff_draws (m_engine, &rec[0], m_app.size (), 0) != NSGPU_OK)
    {
      NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());
    }
  onDraws = rec[app].on_draws;
  offDraws = rec[app].off_draws;
  ambiguous = rec[app].ambiguous;
}

std::vector<nsgpu_ambiguous_draw>
NsgpuP2pScenario::GetAmbiguousDraws (uint64_t &overflow) const
{
  if (m_engine == 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::GetAmbiguousDraws: no engine");
    }
  std::vector<nsgpu_ambiguous_draw> rec (NSGPU_RV_AMBIGUOUS_CAP);
  uint64_t n = 0;
  if (nsgpu_p2p_onoff_ambiguous (m_engine, &rec[0], rec.size (), &n, &overflow, 0) != NSGPU_OK)
    {
      NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());
    }
  rec.resize (n);
  return rec;
}

NsgpuP2pScenario::OnOffDecl &
NsgpuP2pScenario::OnOffDeclOf (Ptr<Application> app)
{
  for (size_t k = 0; k < m_declaredOnOff.size (); k++)
    {
      if (m_declaredOnOff[k].app == app)
        {
          return m_declaredOnOff[k];
        }
    }
  OnOffDecl d;
  d.app = app;
  d.streams = d.exponential[0] = d.exponential[1] = false;
  d.stream[0] = d.stream[1] = 0;
  d.var[0] = d.var[1] = nsgpu_ranvar ();
  m_declaredOnOff.push_back (d);
  return m_declaredOnOff.back ();
}

void
NsgpuP2pScenario::DeclareOnOffStreams (Ptr<Application> app, uint32_t onStream, uint32_t offStream)
{
  OnOffDecl &d = OnOffDeclOf (app);
  d.streams = true;
  d.stream[0] = onStream;
  d.stream[1] = offStream;
}

void
NsgpuP2pScenario::DeclareOnOffExponential (Ptr<Application> app, uint32_t which, double mean, double bound,
                                           uint32_t stream)
{
  if (which > 1)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::DeclareOnOffExponential: which is 0 (OnTime) or 1 (OffTime)");
    }
  OnOffDecl &d = OnOffDeclOf (app);
  d.exponential[which] = true;
  d.var[which] = ExponentialVar (mean, bound, stream);
}

/* An OnOffApplication's OnTime (which = 0) / OffTime (1) attribute as the engine takes it.  ConstantVariable (v) prints
 * as "Constant:v" and UniformVariable (a, b) as "Uniform:a:b" (random-variable.cc:1931-1945; read back at 17 digits);
 * the variable's RngStream is the one DeclareOnOffStreams named.  An ExponentialVariable does not print (:1957 sets
 * badbit): DeclareOnOffExponential plays the role DeclareTrace plays for a trace client. */
void
NsgpuP2pScenario::MirrorOnOffTime (const RandomVariable &v, uint32_t which, uint32_t node, Ptr<Application> app,
                                   double &seconds, nsgpu_ranvar &var) const
{
  const char *what = which == 0 ? "OnTime" : "OffTime";
  const OnOffDecl *decl = 0;
  for (size_t k = 0; k < m_declaredOnOff.size (); k++)
    {
      if (m_declaredOnOff[k].app == app)
        {
          decl = &m_declaredOnOff[k];
        }
    }
  var = nsgpu_ranvar ();
  std::ostringstream os;
  os.precision (17);
  os << v;
  const std::string s = os.fail () ? std::string () : os.str ();
  if (s.compare (0, 9, "Constant:") == 0)
    {
      std::ostringstream c;  // (the value as the attribute prints it by default, as before the other kinds were read)
      c << v;
      seconds = std::strtod (c.str ().c_str () + 9, 0);
      return;
    }
  if (s.compare (0, 8, "Uniform:") == 0)
    {
      if (decl == 0 || !decl->streams)
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << ": OnOffApplication " << what << " is " << s
                          << " and its RngStream was not named: call DeclareOnOffStreams (app, onStream, offStream) "
                          "before FromNodeList (the engine cannot discover the order in which the program constructs "
                          "its RngStreams)");
        }
      char *end = 0;
      const double lo = std::strtod (s.c_str () + 8, &end);
      if (end == 0 || *end != ':')
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << ": cannot read " << s);
        }
      var = UniformVar (lo, std::strtod (end + 1, 0), decl->stream[which]);
      return;
    }
  if (s.empty () && decl != 0 && decl->exponential[which])
    {
      var = decl->var[which];
      return;
    }
  if (!s.empty ())
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << ": OnOffApplication " << what << " is " << s
                      << ": only ConstantVariable, UniformVariable and ExponentialVariable are modelled");
    }
  NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << ": OnOffApplication " << what << " is a "
                  "RandomVariable its attribute does not print (neither Constant, Uniform nor Normal).  If it is an "
                  "ExponentialVariable, call DeclareOnOffExponential (app, " << which << ", mean, bound, stream) before "
                  "FromNodeList; every other kind is not modelled");
}

void
NsgpuP2pScenario::Stop (Time at)
{
  m_stop = at.GetTimeStep ();
  m_setup.push_back (std::make_pair ((uint32_t) NSGPU_SETUP_STOP, 0u));
}

void
NsgpuP2pScenario::Assign (uint32_t da, uint32_t db, uint32_t network, uint32_t mask)
{
  m_nif.resize (m_nodes, 1u);
  const uint32_t d[2] = {da, db};
  for (int k = 0; k < 2; k++)
    {
      m_addr[d[k]] = (network & mask) + 1 + k;
      m_ifindex[d[k]] = m_nif[m_dev[d[k]].node]++;
    }
}

void
NsgpuP2pScenario::SetIcmp (bool on)
{
  m_icmp = on;
}

void
NsgpuP2pScenario::SetFragmentation (bool on, Time timeout)
{
  m_frag = on;
  m_fragTimeout = timeout.GetTimeStep ();
}

void
NsgpuP2pScenario::SetReceiveListErrorModel (uint32_t dev, const std::vector<uint32_t> &packets, bool enabled)
{
  if (dev >= m_dev.size ())
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::SetReceiveListErrorModel: no device " << dev);
    }
  Em none = {NSGPU_EM_NONE, 0, NSGPU_EU_BYTE, 0, 0.0, std::vector<uint32_t> ()};
  m_em.resize (m_dev.size (), none);
  Em e = {NSGPU_EM_RECEIVE_LIST, enabled ? 1u : 0u, NSGPU_EU_BYTE, 0, 0.0, packets};
  m_em[dev] = e;
}

void
NsgpuP2pScenario::SetRateErrorModel (uint32_t dev, double rate, uint32_t unit, uint32_t stream, bool enabled)
{
  if (dev >= m_dev.size ())
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::SetRateErrorModel: no device " << dev);
    }
  Em none = {NSGPU_EM_NONE, 0, NSGPU_EU_BYTE, 0, 0.0, std::vector<uint32_t> ()};
  m_em.resize (m_dev.size (), none);
  Em e = {NSGPU_EM_RATE, enabled ? 1u : 0u, unit, stream, rate, std::vector<uint32_t> ()};
  m_em[dev] = e;
}

void
NsgpuP2pScenario::SetRng (uint32_t seed, uint32_t run)
{
  m_rngSeed = seed;
  m_rngRun = run;
}

void
NsgpuP2pScenario::SetErrorStream (Ptr<NetDevice> device, uint32_t stream)
{
  m_errorStream.push_back (std::make_pair (device, stream));
}

void
NsgpuP2pScenario::GetErrorModel (uint32_t dev, uint32_t &invoked, uint32_t &corrupted) const
{
  if (m_engine == 0 || dev >= m_dev.size ())
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::GetErrorModel: no engine or no device " << dev);
    }
  std::vector<nsgpu_error_model_record> rec (m_dev.size ());
  NSGPU_TRY (nsgpu_p2p_error_models (m_engine, &rec[0], 0));
  invoked = rec[dev].invoked;
  corrupted = rec[dev].corrupted;
}

void
NsgpuP2pScenario::EnableFlowStats (void)
{
  if (m_engine != 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::EnableFlowStats: call it before CreateEngine");
    }
  m_flowStats = true;
}

std::vector<nsgpu_flow_record>
NsgpuP2pScenario::GetFlowStats (Time maxDelay) const
{
  if (m_engine == 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::GetFlowStats: no engine");
    }
  std::vector<nsgpu_flow_record> rec (2 * m_app.size () + 1);  // (never empty: its address is taken)
  NSGPU_TRY (nsgpu_p2p_flow_stats (m_engine, maxDelay.GetNanoSeconds (), &rec[0], 0));
  rec.resize (2 * m_app.size ());
  return rec;
}

namespace {
Time
TimeAttribute (Ptr<Object> o, const char *name)
{
  TimeValue v;
  o->GetAttribute (name, v);
  return v.Get ();
}

uint32_t
UintAttribute (Ptr<Object> o, const char *name)
{
  UintegerValue v;
  o->GetAttribute (name, v);
  return (uint32_t) v.Get ();
}
/* The engine forwards along global routing's choices (PopulateRoutingTables + LookupGlobal, computed by
 * nsgpu_route_global): a node's Ipv4 must route through an Ipv4GlobalRouting in its Ipv4ListRouting (the
 * InternetStackHelper default, static priority 0 + global -10), with no static route of its own beyond the
 * interfaces' directly connected networks (Ipv4StaticRouting::NotifyInterfaceUp adds those; any other static
 * route would win over global routing) */
void
CheckGlobalRouting (Ptr<Ipv4> ip, uint32_t node)
{
  Ptr<Ipv4ListRouting> list = DynamicCast<Ipv4ListRouting> (ip->GetRoutingProtocol ());
  if (list == 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << "'s Ipv4 routing is not an Ipv4ListRouting "
                      "(the engine models global routing)");
    }
  bool global = false;
  for (uint32_t i = 0; i < list->GetNRoutingProtocols (); i++)
    {
      int16_t priority;
      Ptr<Ipv4RoutingProtocol> rp = list->GetRoutingProtocol (i, priority);
      if (DynamicCast<Ipv4GlobalRouting> (rp) != 0)
        {
          global = true;
          continue;
        }
      Ptr<Ipv4StaticRouting> st = DynamicCast<Ipv4StaticRouting> (rp);
      if (st == 0)
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << " runs a routing protocol other than "
                          "static / global routing (not in the GPU-resident subset)");
        }
      for (uint32_t r = 0; r < st->GetNRoutes (); r++)
        {
          Ipv4RoutingTableEntry e = st->GetRoute (r);
          // the routes Ipv4StaticRouting adds by itself (ipv4-static-routing.cc NotifyInterfaceUp /
          // NotifyAddAddress): each interface address's own network on that interface, gateway-less.  Any other
          // route, gateway-less ones included (AddHostRouteTo (dst, if), AddNetworkRouteTo (net, mask, if)), is
          // consulted before global routing (priority 0 > -10) and would override the paths the engine models.
          bool own = false;
          if (e.GetGateway () == Ipv4Address::GetZero () && !e.IsDefault () && e.GetInterface () < ip->GetNInterfaces ())
            {
              for (uint32_t a = 0; a < ip->GetNAddresses (e.GetInterface ()) && !own; a++)
                {
                  Ipv4InterfaceAddress ia = ip->GetAddress (e.GetInterface (), a);
                  own = e.GetDestNetworkMask () == ia.GetMask ()
                        && e.GetDestNetwork () == ia.GetLocal ().CombineMask (ia.GetMask ());
                }
            }
          if (!own)
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << " holds the static route " << e
                              << " (the engine models global routing only)");
            }
        }
    }
  if (!global)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << node << " has no Ipv4GlobalRouting");
    }
}
} // anonymous namespace

void
NsgpuP2pScenario::FromNodeList (Ptr<HipSimulatorImpl> impl)
{
  if (m_nodes != 0 || !m_setup.empty ())
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: the scenario is not empty");
    }
  const uint32_t N = NodeList::GetNNodes ();
  m_nodes = N;
  // ---- the node list: each node's devices (in AddDevice order) and application count ----
  std::vector<uint64_t> devOff (N + 1, 0);
  std::vector<uint32_t> devKind, nApps (N, 0);
  for (uint32_t n = 0; n < N; n++)
    {
      Ptr<Node> node = NodeList::GetNode (n);
      for (uint32_t i = 0; i < node->GetNDevices (); i++)
        {
          Ptr<NetDevice> d = node->GetDevice (i);
          devKind.push_back (DynamicCast<PointToPointNetDevice> (d) != 0 ? (uint32_t) NSGPU_NDEV_P2P
                             : DynamicCast<LoopbackNetDevice> (d) != 0 ? (uint32_t) NSGPU_NDEV_LOOPBACK
                             : (uint32_t) NSGPU_NDEV_OTHER);
        }
      devOff[n + 1] = devKind.size ();
      nApps[n] = node->GetNApplications ();
    }
  // ---- the setup list from the journal (uid order; classified by HipSimulatorImpl when each call was made) ----
  const std::vector<HipSimulatorImpl::SetupCall> &J = impl->GetSetupJournal ();
  const size_t nj = J.size ();
  std::vector<nsgpu_journal_entry> journal (std::max (nj, (size_t) 1));
  for (size_t i = 0; i < nj; i++)
    {
      journal[i].ts = J[i].ts;
      journal[i].context = J[i].context;
      journal[i].kind = J[i].kind;
      journal[i].local = J[i].local;
      journal[i].pad_ = 0;
    }
  size_t nApp = 0;
  for (uint32_t n = 0; n < N; n++)
    {
      nApp += nApps[n];
    }
  std::vector<uint32_t> sk (journal.size ()), si (journal.size ()), owned (journal.size ());
  std::vector<uint32_t> dNode (std::max (devKind.size (), (size_t) 1)), dLocal (dNode.size ());
  std::vector<uint32_t> aNode (std::max (nApp, (size_t) 1)), aLocal (aNode.size ());
  nsgpu_setup_map map;
  map.setup_kind = &sk[0], map.setup_index = &si[0], map.owned = &owned[0];
  map.dev_node = &dNode[0], map.dev_local = &dLocal[0], map.app_node = &aNode[0], map.app_local = &aLocal[0];
  map.n_owned = 0, map.n_devices = 0, map.n_apps = 0, map.stop_ns = -1;
  NSGPU_TRY (nsgpu_setup_from_journal (&journal[0], nj, N, &devOff[0], devKind.empty () ? 0 : &devKind[0], N ? &nApps[0] : 0,
                                       &map));
  for (size_t i = 0; i < nj; i++)
    {
      m_setup.push_back (std::make_pair (sk[i], si[i]));
    }
  m_owned.assign (owned.begin (), owned.begin () + map.n_owned);
  m_stop = map.stop_ns;
  std::map<Ptr<NetDevice>, uint32_t> devIndex;
  std::vector<Ptr<NetDevice> > devs;    // engine device index -> object
  std::vector<Ptr<Application> > apps;  // engine application index -> object
  for (uint32_t d = 0; d < map.n_devices; d++)
    {
      devs.push_back (NodeList::GetNode (dNode[d])->GetDevice (dLocal[d]));
      devIndex[devs[d]] = d;
      m_devObj.push_back (devs[d]);
    }
  for (uint32_t a = 0; a < map.n_apps; a++)
    {
      apps.push_back (NodeList::GetNode (aNode[a])->GetApplication (aLocal[a]));
    }
  // ---- device parameters ----
  const uint32_t D = devs.size ();
  m_dev.resize (D);
  m_addr.assign (D, 0u);
  m_ifindex.assign (D, 0u);
  for (uint32_t d = 0; d < D; d++)
    {
      Ptr<PointToPointNetDevice> p = DynamicCast<PointToPointNetDevice> (devs[d]);
      Ptr<PointToPointChannel> ch = DynamicCast<PointToPointChannel> (p->GetChannel ());
      if (ch == 0 || ch->GetNDevices () != 2)
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << " has no point-to-point channel");
        }
      Ptr<NetDevice> other = ch->GetDevice (0) == devs[d] ? ch->GetDevice (1) : ch->GetDevice (0);
      if (devIndex.find (other) == devIndex.end ())
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << "'s peer is not in the subset");
        }
      Ptr<DropTailQueue> q = DynamicCast<DropTailQueue> (p->GetQueue ());
      if (q == 0)
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << "'s TxQueue is not a DropTailQueue");
        }
      EnumValue mode;
      q->GetAttribute ("Mode", mode);
      if (mode.Get () != DropTailQueue::PACKETS)
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << "'s DropTailQueue is not in PACKETS mode");
        }
      if (UintAttribute (p, "Mtu") != 1500)
        {
          // the engine's devices all have MTU 1500: only a datagram's sender fragments it (ipv4-l3-protocol.cc:722),
          // a forwarder never does
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << "'s Mtu is " << UintAttribute (p, "Mtu")
                          << ", not 1500");
        }
      DataRateValue rate;
      p->GetAttribute ("DataRate", rate);
      Dev x = {devs[d]->GetNode ()->GetId (), devIndex[other], UintAttribute (q, "MaxPackets"), rate.Get ().GetBitRate (),
               TimeAttribute (p, "InterframeGap").GetTimeStep (), TimeAttribute (ch, "Delay").GetTimeStep ()};
      m_dev[d] = x;
    }
  // ---- the devices' ReceiveErrorModel attributes: mirrored, or fatal — never ignored ----
  for (uint32_t d = 0; d < D; d++)
    {
      PointerValue emv;
      devs[d]->GetAttribute ("ReceiveErrorModel", emv);
      Ptr<ErrorModel> em = emv.Get<ErrorModel> ();
      if (em == 0)
        {
          continue;
        }
      Ptr<ReceiveListErrorModel> rl = DynamicCast<ReceiveListErrorModel> (em);
      Ptr<RateErrorModel> rt = DynamicCast<RateErrorModel> (em);
      if (rl != 0)
        {
          const std::list<uint32_t> l = rl->GetList ();
          SetReceiveListErrorModel (d, std::vector<uint32_t> (l.begin (), l.end ()), em->IsEnabled ());
        }
      else if (rt != 0)
        {
          bool named = false;
          uint32_t stream = 0;
          for (size_t i = 0; i < m_errorStream.size (); i++)
            {
              if (m_errorStream[i].first == devs[d])
                {
                  named = true;
                  stream = m_errorStream[i].second;
                }
            }
          if (!named)
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << " has a RateErrorModel whose "
                              "RngStream was not named (SetErrorStream): the engine cannot discover the order in "
                              "which the program constructs its streams");
            }
          // (a RanVar other than the default UniformVariable (0, 1) cannot be told apart here: DESIGN.md 6)
          const enum ErrorUnit u = rt->GetUnit ();
          SetRateErrorModel (d, rt->GetRate (), u == EU_PKT ? (uint32_t) NSGPU_EU_PKT
                             : u == EU_BIT ? (uint32_t) NSGPU_EU_BIT : (uint32_t) NSGPU_EU_BYTE,
                             stream, em->IsEnabled ());
        }
      else if (DynamicCast<ListErrorModel> (em) != 0)
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << " has a ListErrorModel, which selects "
                          "by Packet::GetUid: the engine carries no packet uids");
        }
      else
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: device " << d << " has a ReceiveErrorModel of type "
                          << em->GetInstanceTypeId ().GetName () << ", which the engine does not model");
        }
    }
  if (!m_em.empty () || !m_declaredOnOff.empty ())
    {
      IntegerValue gv;
      GlobalValue::GetValueByName ("RngSeed", gv);
      m_rngSeed = gv.Get ();
      GlobalValue::GetValueByName ("RngRun", gv);
      m_rngRun = gv.Get ();
    }
  // ---- Ipv4: interface addresses and indices, DefaultTtl ----
  std::vector<uint32_t> ttl (N, 64);
  int64_t fragTimeout = -1;  // the nodes' FragmentExpirationTimeout (-1: no Ipv4L3Protocol seen yet)
  std::map<uint32_t, uint32_t> nodeOfAddr;
  for (uint32_t n = 0; n < N; n++)
    {
      Ptr<Ipv4> ip = NodeList::GetNode (n)->GetObject<Ipv4> ();
      if (ip == 0)
        {
          continue;
        }
      for (uint32_t i = 0; i < ip->GetNInterfaces (); i++)
        {
          Ptr<NetDevice> nd = ip->GetNetDevice (i);
          if (ip->GetNAddresses (i) == 0 || devIndex.find (nd) == devIndex.end ())
            {
              continue;
            }
          const uint32_t a = ip->GetAddress (i, 0).GetLocal ().Get ();
          m_addr[devIndex[nd]] = a;
          m_ifindex[devIndex[nd]] = i;
          nodeOfAddr[a] = n;
        }
      CheckGlobalRouting (ip, n);
      Ptr<Ipv4L3Protocol> l3 = DynamicCast<Ipv4L3Protocol> (ip);
      if (l3 != 0)
        {
          ttl[n] = UintAttribute (l3, "DefaultTtl");
          // one FragmentExpirationTimeout for the whole scenario (ipv4-l3-protocol.cc:61-64)
          const int64_t ft = TimeAttribute (l3, "FragmentExpirationTimeout").GetTimeStep ();
          if (ft <= 0)
            {
              // (ns-3 would expire a buffer at once; in nsgpu_p2p_scenario 0 means the default 30 s)
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << n << "'s FragmentExpirationTimeout is not positive");
            }
          if (fragTimeout >= 0 && ft != fragTimeout)
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << n << "'s FragmentExpirationTimeout differs "
                              "from the other nodes'");
            }
          fragTimeout = ft;
        }
    }
  // ---- applications ----
  // (a timeout given to SetFragmentation must be the nodes': the engine has one, and the program's objects decide)
  if (m_fragTimeout != 0 && fragTimeout > 0 && m_fragTimeout != fragTimeout)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: SetFragmentation's timeout differs from the nodes' "
                      "FragmentExpirationTimeout");
    }
  if (fragTimeout > 0)
    {
      m_fragTimeout = fragTimeout;
    }
  for (uint32_t a = 0; a < apps.size (); a++)
    {
      Ptr<Application> o = apps[a];
      const uint32_t n = o->GetNode ()->GetId ();
      App x = {0, n, 0, 0, 0, ttl[n], TimeAttribute (o, "StartTime").GetTimeStep (),
               TimeAttribute (o, "StopTime").GetTimeStep (), 0, 0.0, 0.0, 0, 0, 0, 0};
      uint32_t remote = 0;
      if (DynamicCast<OnOffApplication> (o) != 0)
        {
          x.kind = NSGPU_APP_ONOFF;
          DataRateValue rate;
          o->GetAttribute ("DataRate", rate);
          x.rate = rate.Get ().GetBitRate ();
          x.size = UintAttribute (o, "PacketSize");
          x.maxBytes = UintAttribute (o, "MaxBytes");
          RandomVariableValue on, off;
          o->GetAttribute ("OnTime", on);
          o->GetAttribute ("OffTime", off);
          MirrorOnOffTime (on.Get (), 0, n, o, x.on, x.onVar);
          MirrorOnOffTime (off.Get (), 1, n, o, x.off, x.offVar);
          AddressValue peer;
          o->GetAttribute ("Remote", peer);
          if (!InetSocketAddress::IsMatchingType (peer.Get ()))
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: OnOffApplication on node " << n << ": Remote is not "
                              "an InetSocketAddress");
            }
          const InetSocketAddress s = InetSocketAddress::ConvertFrom (peer.Get ());
          remote = s.GetIpv4 ().Get ();
          x.remotePort = s.GetPort ();
        }
      else if (DynamicCast<UdpEchoClient> (o) != 0)
        {
          x.kind = NSGPU_APP_ECHO_CLIENT;
          x.size = UintAttribute (o, "PacketSize");
          x.count = UintAttribute (o, "MaxPackets");
          x.interval = TimeAttribute (o, "Interval").GetTimeStep ();
          Ipv4AddressValue ra;
          o->GetAttribute ("RemoteAddress", ra);
          remote = ra.Get ().Get ();
          x.remotePort = UintAttribute (o, "RemotePort");
        }
      else if (DynamicCast<UdpEchoServer> (o) != 0)
        {
          x.kind = NSGPU_APP_ECHO_SERVER;
          x.port = UintAttribute (o, "Port");
        }
      else if (DynamicCast<PacketSink> (o) != 0)
        {
          x.kind = NSGPU_APP_SINK;
          AddressValue local;
          o->GetAttribute ("Local", local);
          if (!InetSocketAddress::IsMatchingType (local.Get ()) ||
              InetSocketAddress::ConvertFrom (local.Get ()).GetIpv4 () != Ipv4Address::GetAny ())
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: PacketSink on node " << n << ": Local is not "
                              "(Ipv4Address::GetAny (), port): sockets bound to an address are outside the subset");
            }
          x.port = InetSocketAddress::ConvertFrom (local.Get ()).GetPort ();
        }
      else if (DynamicCast<UdpClient> (o) != 0)
        {
          x.kind = NSGPU_APP_UDP_CLIENT;
          x.size = UintAttribute (o, "PacketSize");
          x.count = UintAttribute (o, "MaxPackets");
          x.interval = TimeAttribute (o, "Interval").GetTimeStep ();
          AddressValue ra;
          o->GetAttribute ("RemoteAddress", ra);
          if (!Ipv4Address::IsMatchingType (ra.Get ()))
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: UdpClient on node " << n << ": RemoteAddress is not "
                              "an Ipv4Address");
            }
          remote = Ipv4Address::ConvertFrom (ra.Get ()).Get ();
          x.remotePort = UintAttribute (o, "RemotePort");
        }
      else if (DynamicCast<UdpTraceClient> (o) != 0)
        {
          // m_entries is private and TraceFilename has no getter: the program names the trace (DeclareTrace)
          size_t k = 0;
          while (k < m_declaredTrace.size () && m_declaredTrace[k].first != o)
            {
              k++;
            }
          if (k == m_declaredTrace.size ())
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: UdpTraceClient on node " << n << ": its trace is not "
                              "declared — the application's entries cannot be read back (m_entries is private, "
                              "TraceFilename has no getter); call DeclareTrace (app, filename) before FromNodeList "
                              "(\"\": the default trace)");
            }
          x.kind = NSGPU_APP_UDP_TRACE_CLIENT;
          x.entries = LoadTraceFile (m_declaredTrace[k].second);
          x.size = UintAttribute (o, "MaxPacketSize");
          AddressValue ra;
          o->GetAttribute ("RemoteAddress", ra);
          if (!Ipv4Address::IsMatchingType (ra.Get ()))
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: UdpTraceClient on node " << n << ": RemoteAddress is "
                              "not an Ipv4Address (IPv6 remotes are outside the subset)");
            }
          remote = Ipv4Address::ConvertFrom (ra.Get ()).Get ();
          x.remotePort = UintAttribute (o, "RemotePort");
        }
      else if (DynamicCast<UdpServer> (o) != 0)
        {
          x.kind = NSGPU_APP_UDP_SERVER;
          x.port = UintAttribute (o, "Port");
          x.window = UintAttribute (o, "PacketWindowSize");
        }
      else
        {
          NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << n << " application " << a
                          << " is not OnOff / PacketSink / UdpEcho / UdpClient / UdpServer / UdpTraceClient (not in the GPU-resident "
                          "subset)");
        }
      if (x.kind == NSGPU_APP_ONOFF || x.kind == NSGPU_APP_ECHO_CLIENT || x.kind == NSGPU_APP_UDP_CLIENT ||
          x.kind == NSGPU_APP_UDP_TRACE_CLIENT)
        {
          if (nodeOfAddr.find (remote) == nodeOfAddr.end ())
            {
              NS_FATAL_ERROR ("NsgpuP2pScenario::FromNodeList: node " << n << " sends to an address no node has");
            }
          x.dst = nodeOfAddr[remote];
          x.remoteAddr = remote;
        }
      // a payload above 1500 - 20 - 8 bytes is fragmented by its sender's Ipv4L3Protocol (a UdpClient's PacketSize
      // counts its payload whole): the engine models that only when told to (nsgpu_p2p_scenario.frag)
      if ((x.kind == NSGPU_APP_ONOFF || x.kind == NSGPU_APP_ECHO_CLIENT || x.kind == NSGPU_APP_UDP_CLIENT) && x.size > 1472)
        {
          m_frag = true;
        }
      m_app.push_back (x);
    }
}

void
NsgpuP2pScenario::PopulateRoutingTables (void)
{
  m_dstSlot.assign (m_nodes, 0xffffffffu);
  m_nDst = 0;
  for (size_t i = 0; i < m_app.size (); i++)
    {
      if (m_app[i].kind == NSGPU_APP_ONOFF || m_app[i].kind == NSGPU_APP_ECHO_CLIENT ||
          m_app[i].kind == NSGPU_APP_UDP_CLIENT || m_app[i].kind == NSGPU_APP_UDP_TRACE_CLIENT)
        {
          m_dstSlot[m_app[i].dst] = 0;  // mark; numbered below in node order
          if (m_icmp || m_app[i].kind == NSGPU_APP_ECHO_CLIENT)
            {
              m_dstSlot[m_app[i].node] = 0;  // an ICMP error / an echo goes back to the sender
            }
        }
    }
  std::vector<uint32_t> dst;
  for (uint32_t n = 0; n < m_nodes; n++)
    {
      if (m_dstSlot[n] != 0xffffffffu)
        {
          m_dstSlot[n] = m_nDst++;
          dst.push_back (n);
        }
    }
  const size_t D = m_dev.size ();
  std::vector<uint32_t> devNode (D), devPeer (D);
  bool addressed = D > 0;
  for (size_t d = 0; d < D; d++)
    {
      devNode[d] = m_dev[d].node, devPeer[d] = m_dev[d].peer;
      addressed = addressed && m_addr[d] != 0;
    }
  m_route.assign ((size_t) m_nodes * std::max (m_nDst, 1u), 0xffffffffu);
  if (m_nDst > 0 && nsgpu_route_global (m_nodes, D, &devNode[0], &devPeer[0], addressed ? &m_addr[0] : 0,
                                        addressed ? &m_ifindex[0] : 0, m_nDst, &dst[0], &m_route[0], 0) != NSGPU_OK)
    {
      NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());
    }
}

void
NsgpuP2pScenario::Fill (void)
{
  if (m_route.empty ())
    {
      RouteShortestPaths ();
    }
  const size_t D = m_dev.size (), A = m_app.size ();
  m_cDevNode.resize (D), m_cDevPeer.resize (D), m_cDevQmax.resize (D);
  m_cDevBps.resize (D), m_cDevIfg.resize (D), m_cDevDelay.resize (D);
  for (size_t d = 0; d < D; d++)
    {
      m_cDevNode[d] = m_dev[d].node, m_cDevPeer[d] = m_dev[d].peer, m_cDevQmax[d] = m_dev[d].qmax;
      m_cDevBps[d] = m_dev[d].bps, m_cDevIfg[d] = m_dev[d].ifg, m_cDevDelay[d] = m_dev[d].delay;
    }
  const size_t A1 = std::max (A, (size_t) 1);
  m_cKind.assign (A1, 0), m_cNode.assign (A1, 0), m_cDst.assign (A1, 0), m_cSlot.assign (A1, 0);
  m_cSrc.assign (A1, 0xffffffffu), m_cSize.assign (A1, 0), m_cMaxb.assign (A1, 0), m_cTtl.assign (A1, 0);
  m_cCount.assign (A1, 0), m_cRaddr.assign (A1, 0), m_cRport.assign (A1, 0);
  m_cPort.assign (A1, 0), m_cWindow.assign (A1, 0);
  m_cStart.assign (A1, 0), m_cStop.assign (A1, 0), m_cIvl.assign (A1, 0), m_cRate.assign (A1, 0);
  m_cOn.assign (A1, 0.0), m_cOff.assign (A1, 0.0);
  for (size_t i = 0; i < A; i++)
    {
      const App &a = m_app[i];
      const bool sender = a.kind == NSGPU_APP_ONOFF || a.kind == NSGPU_APP_ECHO_CLIENT ||
                          a.kind == NSGPU_APP_UDP_CLIENT || a.kind == NSGPU_APP_UDP_TRACE_CLIENT;
      m_cPort[i] = a.port, m_cWindow[i] = a.window;
      m_cKind[i] = a.kind, m_cNode[i] = a.node, m_cDst[i] = a.dst, m_cSize[i] = a.size, m_cMaxb[i] = a.maxBytes;
      m_cTtl[i] = a.ttl, m_cCount[i] = a.count, m_cIvl[i] = a.interval, m_cRaddr[i] = a.remoteAddr;
      m_cRport[i] = a.remotePort;
      m_cSlot[i] = sender ? m_dstSlot[a.dst] : 0;
      m_cSrc[i] = sender ? m_dstSlot[a.node] : 0xffffffffu;
      m_cStart[i] = a.start, m_cStop[i] = a.stop, m_cRate[i] = a.rate, m_cOn[i] = a.on, m_cOff[i] = a.off;
    }
  m_cSk.resize (m_setup.size ()), m_cSi.resize (m_setup.size ());
  for (size_t i = 0; i < m_setup.size (); i++)
    {
      m_cSk[i] = m_setup[i].first, m_cSi[i] = m_setup[i].second;
    }
  nsgpu_p2p_scenario &sc = m_sc;
  sc = nsgpu_p2p_scenario ();
  sc.n_nodes = m_nodes;
  sc.n_devices = D;
  sc.n_apps = A;
  sc.n_dst = std::max (m_nDst, 1u);
  sc.dev_node = &m_cDevNode[0], sc.dev_peer = &m_cDevPeer[0], sc.dev_bps = &m_cDevBps[0];
  sc.dev_ifg_ns = &m_cDevIfg[0], sc.dev_delay_ns = &m_cDevDelay[0], sc.dev_qmax = &m_cDevQmax[0];
  sc.route = &m_route[0];
  sc.app_kind = &m_cKind[0], sc.app_node = &m_cNode[0], sc.app_start_ns = &m_cStart[0], sc.app_stop_ns = &m_cStop[0];
  sc.app_dst_node = &m_cDst[0], sc.app_dst_slot = &m_cSlot[0], sc.app_rate_bps = &m_cRate[0];
  sc.app_pkt_size = &m_cSize[0], sc.app_on_s = &m_cOn[0], sc.app_off_s = &m_cOff[0], sc.app_max_bytes = &m_cMaxb[0];
  sc.app_ttl = &m_cTtl[0], sc.app_count = &m_cCount[0], sc.app_interval_ns = &m_cIvl[0], sc.app_src_slot = &m_cSrc[0];
  // UDP ports, always: a datagram reaches the application bound to its destination port, as in ns-3
  sc.app_port = &m_cPort[0], sc.app_remote_port = &m_cRport[0], sc.app_loss_window = &m_cWindow[0];
  sc.stop_ns = m_stop;
  sc.icmp = m_icmp ? 1u : 0u;
  sc.frag = m_frag ? 1u : 0u;
  sc.frag_timeout_ns = m_fragTimeout;
  if (!m_em.empty ())
    {
      m_cEmKind.assign (D, 0), m_cEmEnabled.assign (D, 0), m_cEmUnit.assign (D, 0), m_cEmStream.assign (D, 0);
      m_cEmRate.assign (D, 0.0), m_cEmOff.assign (D + 1, 0), m_cEmList.clear ();
      for (size_t d = 0; d < D; d++)
        {
          if (d < m_em.size ())
            {
              m_cEmKind[d] = m_em[d].kind, m_cEmEnabled[d] = m_em[d].enabled, m_cEmUnit[d] = m_em[d].unit;
              m_cEmStream[d] = m_em[d].stream, m_cEmRate[d] = m_em[d].rate;
              m_cEmList.insert (m_cEmList.end (), m_em[d].list.begin (), m_em[d].list.end ());
            }
          m_cEmOff[d + 1] = m_cEmList.size ();
        }
      m_cEmList.push_back (0);  // (never empty: its address is taken)
      sc.dev_em_kind = &m_cEmKind[0], sc.dev_em_enabled = &m_cEmEnabled[0], sc.dev_em_unit = &m_cEmUnit[0];
      sc.dev_em_rate = &m_cEmRate[0], sc.dev_em_stream = &m_cEmStream[0];
      sc.em_list_off = &m_cEmOff[0], sc.em_list = &m_cEmList[0];
      sc.rng_seed = m_rngSeed, sc.rng_run = m_rngRun;
    }
  sc.flowmon = m_flowStats ? 1u : 0u;
  // the UdpTraceClients' entries travel beside the struct (nsgpu_p2p_scenario_ext)
  m_hasTrace = false;
  m_cTraceOff.assign (A + 1, 0), m_cTraceEnt.clear ();
  for (size_t i = 0; i < A; i++)
    {
      if (m_app[i].kind == NSGPU_APP_UDP_TRACE_CLIENT)
        {
          m_hasTrace = true;
          m_cTraceEnt.insert (m_cTraceEnt.end (), m_app[i].entries.begin (), m_app[i].entries.end ());
        }
      m_cTraceOff[i + 1] = m_cTraceEnt.size ();
    }
  m_cTraceEnt.push_back (nsgpu_udp_trace_entry ());  // (never empty: its address is taken)
  m_ext = nsgpu_p2p_scenario_ext ();
  m_ext.size = sizeof (m_ext);
  m_ext.trace_off = &m_cTraceOff[0], m_ext.trace_entries = &m_cTraceEnt[0];
  // ... and so do the OnOff applications' random OnTime / OffTime variables
  m_hasVar = false;
  m_cOnVar.assign (A1, nsgpu_ranvar ()), m_cOffVar.assign (A1, nsgpu_ranvar ());
  for (size_t i = 0; i < A; i++)
    {
      if (m_app[i].kind == NSGPU_APP_ONOFF)
        {
          m_cOnVar[i] = m_app[i].onVar, m_cOffVar[i] = m_app[i].offVar;
          m_hasVar = m_hasVar || m_cOnVar[i].kind != NSGPU_RV_CONSTANT || m_cOffVar[i].kind != NSGPU_RV_CONSTANT;
        }
    }
  if (m_hasVar)
    {
      m_ext.app_on_var = &m_cOnVar[0], m_ext.app_off_var = &m_cOffVar[0];
      sc.rng_seed = m_rngSeed, sc.rng_run = m_rngRun;
    }
  sc.n_setup = m_setup.size ();
  sc.setup_kind = m_cSk.empty () ? 0 : &m_cSk[0];
  sc.setup_index = m_cSi.empty () ? 0 : &m_cSi[0];
}

nsgpu_p2p *
NsgpuP2pScenario::CreateEngine (uint64_t poolCap, uint64_t logCap)
{
  Fill ();
  if (nsgpu_p2p_create_ex (&m_sc, (m_hasTrace || m_hasVar) ? &m_ext : 0, poolCap, logCap, &m_engine) != NSGPU_OK ||
      nsgpu_p2p_reset (m_engine, 0) != NSGPU_OK)
    {
      NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());
    }
  return m_engine;
}

void
NsgpuP2pScenario::AdoptInto (Ptr<HipSimulatorImpl> impl)
{
  if (m_engine == 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::AdoptInto: CreateEngine first");
    }
  impl->AdoptDeviceSubset (m_engine, m_owned);
}

void
NsgpuP2pScenario::EnableTraceRecords (uint64_t capacity)
{
  if (m_engine == 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::EnableTraceRecords: CreateEngine first");
    }
  NSGPU_TRY (nsgpu_p2p_set_trace (m_engine, capacity));
  NSGPU_TRY (nsgpu_p2p_reset (m_engine, 0));
}

void
NsgpuP2pScenario::WriteTraces (Ptr<OutputStreamWrapper> ascii, std::string pcapPrefix)
{
  if (m_engine == 0)
    {
      NS_FATAL_ERROR ("NsgpuP2pScenario::WriteTraces: CreateEngine first");
    }
  if (m_codec == 0)
    {
      nsgpu_trace_addressing ad;
      ad.dev_addr = m_addr.empty () ? 0 : &m_addr[0];
      ad.dev_ip_ifindex = m_ifindex.empty () ? 0 : &m_ifindex[0];
      ad.app_remote_addr = &m_cRaddr[0];
      ad.app_remote_port = &m_cRport[0];
      NSGPU_TRY (nsgpu_trace_codec_create (&m_sc, &ad, &m_codec));
    }
  uint64_t n = 0;
  NSGPU_TRY (nsgpu_p2p_trace_read (m_engine, 0, 0, &n, 0));
  std::vector<nsgpu_trace_record> rec (std::max (n, (uint64_t) 1));
  NSGPU_TRY (nsgpu_p2p_trace_read (m_engine, &rec[0], n, &n, 0));
  NSGPU_TRY (nsgpu_trace_sort (&rec[0], n));
  std::vector<char> line (512);
  std::vector<uint8_t> pkt (2048);
  if (ascii != 0)
    {
      std::ostream *os = ascii->GetStream ();
      for (uint64_t i = 0; i < n; i++)
        {
          uint64_t len = 0;
          NSGPU_TRY (nsgpu_trace_line (m_codec, &rec[i], 0, 0, &len));  // the size first (an ICMP line can exceed 512 B)
          if (len > line.size ())
            {
              line.resize (len);
            }
          NSGPU_TRY (nsgpu_trace_line (m_codec, &rec[i], &line[0], line.size (), &len));
          os->write (&line[0], (std::streamsize) len);
        }
    }
  if (!pcapPrefix.empty ())
    {
      // PointToPointHelper::EnablePcapInternal (point-to-point-helper.cc:81-110): one file per device,
      // PcapHelper::CreateFile (DLT_PPP), the PromiscSniffer's packets (after Dequeue, before MacRx)
      PcapHelper helper;
      // the device's NetDevice index on its node (Node::AddDevice order: the setup list's devices and loopbacks)
      std::vector<uint32_t> nxt (m_nodes, 0), devid (m_dev.size (), 0);
      for (size_t i = 0; i < m_setup.size (); i++)
        {
          if (m_setup[i].first == NSGPU_SETUP_DEVICE)
            {
              devid[m_setup[i].second] = nxt[m_dev[m_setup[i].second].node]++;
            }
          else if (m_setup[i].first == NSGPU_SETUP_NOOP)
            {
              nxt[m_setup[i].second]++;
            }
        }
      std::vector<Ptr<PcapFileWrapper> > files (m_dev.size ());
      for (uint32_t d = 0; d < m_dev.size (); d++)
        {
          // PcapHelper::GetFilenameFromDevice: <prefix>-<node id>-<device id>.pcap
          std::string fn;
          if (d < m_devObj.size () && m_devObj[d] != 0)
            {
              fn = helper.GetFilenameFromDevice (pcapPrefix, m_devObj[d]);
            }
          else
            {
              std::ostringstream name;
              name << pcapPrefix << "-" << m_dev[d].node << "-" << devid[d] << ".pcap";
              fn = name.str ();
            }
          files[d] = helper.CreateFile (fn, std::ios::out, PcapHelper::DLT_PPP);
        }
      for (uint64_t i = 0; i < n; i++)
        {
          if (rec[i].kind != NSGPU_TR_DEQUEUE && rec[i].kind != NSGPU_TR_RX)
            {
              continue;
            }
          uint64_t len = 0;
          NSGPU_TRY (nsgpu_trace_packet (m_codec, &rec[i], 0, 0, &len));
          if (len > pkt.size ())
            {
              pkt.resize (len);
            }
          NSGPU_TRY (nsgpu_trace_packet (m_codec, &rec[i], &pkt[0], pkt.size (), &len));
          files[rec[i].dev]->Write (TimeStep ((int64_t) rec[i].ts), &pkt[0], (uint32_t) len);
        }
    }
}

} // namespace ns3
