/* -*- Mode:C++; c-file-style:"gnu"; indent-tabs-mode:nil; -*- */
/*
 * See hip-yans-wifi-phy.h.  The uid-critical work is library code, tested without ns-3:
 *  - which phys a SendPacket's YansWifiChannel::Send reaches, with which uids and contexts: nsgpu_sim_wifi_send /
 *    nsgpu_wifil_send_plan (tests/test_wifi_binding_cpu.py against the oracle's channel loop);
 *  - where the EndReceive's host part runs in the order: the runtime's hand-back (nsgpu_sim_wifi_set_end_handler,
 *    tests/test_gpu_wifi_loop.py: a MAC that replies at each EndReceive, full pop log = the oracle's);
 *  - what the state helper is fed with: the device's notes, in order, with Now () set
 *    (nsgpu_sim_wifi_set_note_handler, tests/test_gpu_wifi_notes.py: the notes, the SendPackets and the end records
 *    drive a restated WifiPhyStateHelper through every switch with no NS_ASSERT violated, and its state equals the
 *    device's at every MAC attempt).
 * This file only maps ns-3 objects onto those calls.
 */
#include "hip-yans-wifi-phy.h"
#include "ns3/log.h"
#include "ns3/simulator.h"
#include "ns3/mobility-model.h"
#include "ns3/constant-position-mobility-model.h"
#include "ns3/constant-velocity-mobility-model.h"
#include "ns3/waypoint-mobility-model.h"
#include "ns3/constant-acceleration-mobility-model.h"
#include "ns3/wifi-net-device.h"
#include "ns3/node.h"
#include "ns3/nist-error-rate-model.h"
#include "ns3/yans-error-rate-model.h"
#include "ns3/uinteger.h"
#include "ns3/pointer.h"
#include <cmath>
#include <sstream>

NS_LOG_COMPONENT_DEFINE ("HipYansWifiPhy");

#define NSGPU_RT(call)                                                      \
  do {                                                                      \
      if ((call) != NSGPU_OK)                                               \
        {                                                                   \
          NS_FATAL_ERROR ("libnsgpu: " << nsgpu_last_error ());             \
        }                                                                   \
    } while (false)

namespace ns3 {

NS_OBJECT_ENSURE_REGISTERED (HipYansWifiPhy);
NS_OBJECT_ENSURE_REGISTERED (HipWifiBinding);

TypeId
HipYansWifiPhy::GetTypeId (void)
{
  static TypeId tid = TypeId ("ns3::HipYansWifiPhy")
    .SetParent<YansWifiPhy> ()
    .AddConstructor<HipYansWifiPhy> ()
  ;
  return tid;
}

HipYansWifiPhy::HipYansWifiPhy ()
  : m_binding (0),
    m_rt (0),
    m_index (0),
    m_bound (false),
    m_random (0.0, 1.0),
    m_hipChannelNumber (1)
{
}

// YansWifiPhy::m_state (created by its constructor, yans-wifi-phy.cc:135) through the public "State" attribute
// (:108-111); fetched at the first use, once the object's TypeId is set
Ptr<WifiPhyStateHelper>
HipYansWifiPhy::Helper (void)
{
  if (m_hipState == 0)
    {
      PointerValue state;
      GetAttribute ("State", state);
      m_hipState = state.Get<WifiPhyStateHelper> ();
      NS_ASSERT (m_hipState != 0);
    }
  return m_hipState;
}

void
HipYansWifiPhy::Bind (HipWifiBinding *binding, nsgpu_sim *runtime, uint32_t index)
{
  m_binding = binding;
  m_rt = runtime;
  m_index = index;
  m_bound = true;
}

uint32_t
HipYansWifiPhy::GetIndex (void) const
{
  return m_index;
}

nsgpu_wifil_phy_state
HipYansWifiPhy::State (void) const
{
  if (!m_bound)
    {
      NS_FATAL_ERROR ("HipYansWifiPhy: not attached (HipWifiBinding::Attach before Run)");
    }
  nsgpu_wifil_phy_state st;
  NSGPU_RT (nsgpu_sim_wifi_state (m_rt, m_index, &st));  // (Now (): the runtime's, the device advanced to it)
  return st;
}

double
HipYansWifiPhy::PowerDbm (uint8_t level) const
{
  const double base = GetTxPowerStart (), end = GetTxPowerEnd ();
  const uint32_t n = GetNTxPower ();
  NS_ASSERT (base <= end);
  NS_ASSERT (n > 0);
  if (n > 1)
    {
      return base + level * (end - base) / (n - 1);
    }
  NS_ASSERT_MSG (base == end, "cannot have TxPowerEnd != TxPowerStart with TxPowerLevels == 1");
  return base;
}

// YansWifiPhy::SendPacket (yans-wifi-phy.cc:499-522): the traces and the state helper's SwitchToTx here (:510-520,
// in that order), the device's own switch (an RX abandoned: m_endRxEvent.Cancel) and YansWifiChannel::Send on the
// device
void
HipYansWifiPhy::SendPacket (Ptr<const Packet> packet, WifiMode txMode, enum WifiPreamble preamble, uint8_t txPower)
{
  NS_LOG_FUNCTION (this << packet << txMode << preamble << (uint32_t) txPower);
  NS_ASSERT (!Helper ()->IsStateTx () && !IsStateTx () && !IsStateSwitching ());  // (:508)
  const Time txDuration = CalculateTxDuration (packet->GetSize (), txMode, preamble);
  NotifyTxBegin (packet);
  const uint32_t rate500 = txMode.GetDataRate () / 500000;
  const bool shortPreamble = (WIFI_PREAMBLE_SHORT == preamble);
  NotifyMonitorSniffTx (packet, (uint16_t) GetChannelFrequencyMhz (), GetChannelNumber (), rate500, shortPreamble);
  Helper ()->SwitchToTx (txDuration, packet, txMode, preamble, txPower);  // (:520: m_txTrace, NotifyTxStart, State)
  uint32_t modclass = NSGPU_WIFI_DSSS;
  switch (txMode.GetModulationClass ())
    {
    case WIFI_MOD_CLASS_DSSS: modclass = NSGPU_WIFI_DSSS; break;
    case WIFI_MOD_CLASS_OFDM: modclass = NSGPU_WIFI_OFDM; break;
    case WIFI_MOD_CLASS_ERP_OFDM: modclass = NSGPU_WIFI_ERP_OFDM; break;
    default: NS_FATAL_ERROR ("HipYansWifiPhy: modulation class " << txMode.GetModulationClass () << " is not on the device");
    }
  m_binding->RecordTx (packet, txMode, preamble);  // (the device's transmission index: SendPacket calls in order)
  NSGPU_RT (nsgpu_sim_wifi_send (m_rt, m_index, packet->GetSize (), PowerDbm (txPower) + GetTxGain (), modclass,
                                 txMode.GetDataRate (), txMode.GetBandwidth (),
                                 shortPreamble ? NSGPU_WIFI_PREAMBLE_SHORT : NSGPU_WIFI_PREAMBLE_LONG));
}

// (SetReceiveOkCallback / SetReceiveErrorCallback are YansWifiPhy's: they set the state helper's, :388-397, which
// SwitchFromRxEndOk / Error call)
void
HipYansWifiPhy::RegisterListener (WifiPhyListener *listener)
{
  Helper ()->RegisterListener (listener);  // (:665-669)
}

bool
HipYansWifiPhy::IsStateCcaBusy (void)
{
  return State ().state == NSGPU_WIFIL_CCA_BUSY;
}
bool
HipYansWifiPhy::IsStateIdle (void)
{
  return State ().state == NSGPU_WIFIL_IDLE;
}
bool
HipYansWifiPhy::IsStateBusy (void)
{
  return State ().state != NSGPU_WIFIL_IDLE;
}
bool
HipYansWifiPhy::IsStateRx (void)
{
  return State ().state == NSGPU_WIFIL_RX;
}
bool
HipYansWifiPhy::IsStateTx (void)
{
  return State ().state == NSGPU_WIFIL_TX;
}
bool
HipYansWifiPhy::IsStateSwitching (void)
{
  return State ().state == NSGPU_WIFIL_SWITCHING;
}

// YansWifiPhy::SetChannelNumber (yans-wifi-phy.cc:327-374) on the device (nsgpu_sim_wifi_set_channel): the state
// decision (:338-361), the cancelled EndReceive, EraseEvents and the channel lists are the device's; the state
// helper's SwitchToChannelSwitching (:364: NotifySwitchingStart reaches DcfManager, the State trace) runs here, and a
// switch postponed while transmitting is rescheduled here (:349-352), with the uid the reference's Schedule takes.
void
HipYansWifiPhy::SetChannelNumber (uint16_t nch)
{
  if (Simulator::Now () == Seconds (0))
    {
      // "this is not channel switch, this is initialization" (:330-336); attribute construction comes through here
      YansWifiPhy::SetChannelNumber (nch);
      m_hipChannelNumber = nch;
      if (m_bound)
        {
          nsgpu_wifil_switch out;
          NSGPU_RT (nsgpu_sim_wifi_set_channel (m_rt, m_index, nch, 0, &out));
        }
      return;
    }
  if (!m_bound)
    {
      NS_FATAL_ERROR ("HipYansWifiPhy: not attached (HipWifiBinding::Attach before Run)");
    }
  TimeValue delay;
  GetAttribute ("ChannelSwitchDelay", delay);
  nsgpu_wifil_switch out;
  // (a call while SWITCHING is the reference's NS_ASSERT (!IsStateSwitching ()), :338: NSGPU_ESTATE, fatal here)
  NSGPU_RT (nsgpu_sim_wifi_set_channel (m_rt, m_index, nch, delay.Get ().GetNanoSeconds (), &out));
  if (out.outcome == NSGPU_WIFIL_SWITCH_POSTPONED)
    {
      Simulator::Schedule (NanoSeconds (out.retry_delay), &HipYansWifiPhy::SetChannelNumber, this, nch);
      return;
    }
  Helper ()->SwitchToChannelSwitching (delay.Get ());
  m_hipChannelNumber = nch;
}

uint16_t
HipYansWifiPhy::GetChannelNumber (void) const
{
  return m_hipChannelNumber;
}
Time
HipYansWifiPhy::GetDelayUntilIdle (void)
{
  return NanoSeconds (State ().delay_until_idle);
}

// YansWifiPhy::EndReceive (:770-799) after the device's CalculateSnrPer and state switch
void
HipYansWifiPhy::EndReceiveHandBack (const nsgpu_wifil_end &end, Ptr<const Packet> sent, WifiMode mode,
                                    enum WifiPreamble preamble)
{
  NS_ASSERT (Simulator::Now ().GetNanoSeconds () == (int64_t) end.ts);
  Ptr<Packet> packet = sent->Copy ();  // (YansWifiChannel::Send's copy per receiver, :97)
  if (m_random.GetValue () > end.per)
    {
      NotifyRxEnd (packet);
      const uint32_t rate500 = mode.GetDataRate () / 500000;
      const bool shortPreamble = (WIFI_PREAMBLE_SHORT == preamble);
      const double signalDbm = 10.0 * std::log10 (end.rx_w) + 30;
      const double noiseDbm = 10.0 * std::log10 (end.rx_w / end.snr) - GetRxNoiseFigure () + 30;
      NotifyMonitorSniffRx (packet, (uint16_t) GetChannelFrequencyMhz (), GetChannelNumber (), rate500, shortPreamble,
                            signalDbm, noiseDbm);
      Helper ()->SwitchFromRxEndOk (packet, end.snr, mode, preamble);  // (:791: RxOk trace, NotifyRxEndOk, the MAC)
    }
  else
    {
      NotifyRxDrop (packet);
      Helper ()->SwitchFromRxEndError (packet, end.snr);  // (:797)
    }
}

// YansWifiPhy::StartReceivePacket's host-visible part (:417-495) for one Receive the device ran
void
HipYansWifiPhy::OnNote (const nsgpu_wifil_note &note, Ptr<const Packet> sent)
{
  NS_ASSERT (Simulator::Now ().GetNanoSeconds () == (int64_t) note.ts);
  Ptr<Packet> packet = sent->Copy ();  // (YansWifiChannel::Send's copy per receiver, :97)
  if (note.kind == NSGPU_WIFIL_NOTE_SYNC)
    {
      Helper ()->SwitchToRx (NanoSeconds (note.rx_duration));  // (:465)
      NotifyRxBegin (packet);                                    // (:467)
    }
  else
    {
      NotifyRxDrop (packet);  // (:421 while SWITCHING / :440 / :451 / :477)
    }
  if (note.cca_duration != 0)
    {
      // (:491-495; a SWITCHING drop reaches it when the frame outlasts m_endSwitching, :429-434)
      Helper ()->SwitchMaybeToCcaBusy (NanoSeconds (note.cca_duration));
    }
}

// ---- the helper ----
HipYansWifiPhyHelper
HipYansWifiPhyHelper::Default (void)
{
  HipYansWifiPhyHelper helper;
  helper.SetErrorRateModel ("ns3::NistErrorRateModel");
  return helper;
}

HipYansWifiPhyHelper::HipYansWifiPhyHelper ()
{
  m_hipPhy.SetTypeId ("ns3::HipYansWifiPhy");
}

void
HipYansWifiPhyHelper::SetChannel (Ptr<YansWifiChannel> channel)
{
  m_hipChannel = channel;
  YansWifiPhyHelper::SetChannel (channel);
}

void
HipYansWifiPhyHelper::Set (std::string name, const AttributeValue &v)
{
  m_hipPhy.Set (name, v);
  YansWifiPhyHelper::Set (name, v);
}

void
HipYansWifiPhyHelper::SetErrorRateModel (std::string name, std::string n0, const AttributeValue &v0,
                                         std::string n1, const AttributeValue &v1)
{
  m_hipErrorRateModel = ObjectFactory ();
  m_hipErrorRateModel.SetTypeId (name);
  m_hipErrorRateModel.Set (n0, v0);
  m_hipErrorRateModel.Set (n1, v1);
  YansWifiPhyHelper::SetErrorRateModel (name, n0, v0, n1, v1);
}

// YansWifiPhyHelper::Create (yans-wifi-helper.cc:232-241) with the device-backed phy
Ptr<WifiPhy>
HipYansWifiPhyHelper::Create (Ptr<Node> node, Ptr<WifiNetDevice> device) const
{
  Ptr<HipYansWifiPhy> phy = m_hipPhy.Create<HipYansWifiPhy> ();
  Ptr<ErrorRateModel> error = m_hipErrorRateModel.Create<ErrorRateModel> ();
  phy->SetErrorRateModel (error);
  phy->SetChannel (m_hipChannel);
  phy->SetMobility (node);
  phy->SetDevice (device);
  return phy;
}

// ---- the binding ----
TypeId
HipWifiBinding::GetTypeId (void)
{
  static TypeId tid = TypeId ("ns3::HipWifiBinding")
    .SetParent<Object> ()
    .AddConstructor<HipWifiBinding> ()
  ;
  return tid;
}

HipWifiBinding::HipWifiBinding ()
  : m_engine (0),
    m_rt (0)
{
  m_lossx = nsgpu_lossx ();
  m_lossx.n = -1;  // (no extended chain: Attach's chain is in force)
}

HipWifiBinding::~HipWifiBinding ()
{
}

void
HipWifiBinding::DoDispose (void)
{
  if (m_rt)
    {
      nsgpu_sim_wifi_set_end_handler (m_rt, 0, 0);
      nsgpu_sim_wifi_set_note_handler (m_rt, 0, 0);
    }
  m_phys.clear ();
  m_mobs.clear ();
  m_tx.clear ();
  if (m_engine)
    {
      nsgpu_wifil_destroy (m_engine);  // (after the runtime's last Run)
      m_engine = 0;
    }
  Object::DoDispose ();
}

nsgpu_loss_chain
HipWifiBinding::DefaultLoss (void)
{
  nsgpu_loss_chain c;
  c.n = 1;
  c.pad_ = 0;
  for (int i = 0; i < NSGPU_MAX_LOSS_CHAIN; i++)
    {
      c.m[i].kind = NSGPU_LOSS_NONE;
      c.m[i].pad_ = 0;
      c.m[i].p0 = c.m[i].p1 = c.m[i].p2 = 0;
    }
  c.m[0].kind = NSGPU_LOSS_LOG_DISTANCE;  // LogDistancePropagationLossModel's defaults (propagation-loss-model.cc:420-435)
  c.m[0].p0 = 3.0;
  c.m[0].p1 = 1.0;
  c.m[0].p2 = 46.6777;
  return c;
}

void
HipWifiBinding::RecordTx (Ptr<const Packet> packet, WifiMode mode, enum WifiPreamble preamble)
{
  Tx t;
  t.packet = packet;
  t.mode = mode;
  t.preamble = preamble;
  m_tx.push_back (t);
}

void
HipWifiBinding::EndHandBack (void *user, const nsgpu_wifil_end *end)
{
  HipWifiBinding *b = static_cast<HipWifiBinding *> (user);
  if (end->phy >= b->m_phys.size () || end->tx >= b->m_tx.size ())
    {
      NS_FATAL_ERROR ("HipWifiBinding: an EndReceive of an unknown phy / transmission");
    }
  const Tx &t = b->m_tx[end->tx];
  b->m_phys[end->phy]->EndReceiveHandBack (*end, t.packet, t.mode, t.preamble);
}

void
HipWifiBinding::NoteHandBack (void *user, const nsgpu_wifil_note *note)
{
  HipWifiBinding *b = static_cast<HipWifiBinding *> (user);
  if (note->phy >= b->m_phys.size () || note->tx >= b->m_tx.size ())
    {
      NS_FATAL_ERROR ("HipWifiBinding: a notification of an unknown phy / transmission");
    }
  b->m_phys[note->phy]->OnNote (*note, b->m_tx[note->tx].packet);
}

// ConstantVelocityMobilityModel's CourseChange (SetVelocity and SetPosition both fire it, mobility-model.cc:100-104)
// of phy `context`: a non-zero velocity can only come from SetVelocity (SetPosition zeroes it,
// constant-velocity-helper.cc:43-49) and is forwarded at Now (); a zero velocity is forwarded as SetPosition of the
// host object's position (the trace does not tell SetVelocity (0) from SetPosition: a stop takes the host's
// integration).
void
HipWifiBinding::CourseChange (std::string context, Ptr<const MobilityModel> mobility)
{
  std::istringstream is (context);
  uint32_t index = 0;
  is >> index;
  NS_ASSERT (index < m_phys.size ());
  const Vector v = mobility->GetVelocity ();
  if (v.x != 0.0 || v.y != 0.0 || v.z != 0.0)
    {
      const double vel[3] = { v.x, v.y, v.z };
      NSGPU_RT (nsgpu_sim_wifi_set_velocity (m_rt, index, vel));
    }
  else
    {
      const Vector p = mobility->GetPosition ();
      NSGPU_RT (nsgpu_sim_wifi_set_position (m_rt, index, p.x, p.y, p.z));  // (a phy with a model: set_position_at)
    }
}

// The kept chain to the device, from the running event on (or from the start, before Run).
void
HipWifiBinding::IssueLoss (void)
{
  NS_ASSERT (m_rt != 0 && m_lossx.n >= 0);
  m_lossx.entry = m_lossEntries.empty () ? 0 : &m_lossEntries[0];
  m_lossx.n_entry = m_lossEntries.size ();
  NSGPU_RT (nsgpu_sim_wifi_set_loss (m_rt, &m_lossx));
}

void
HipWifiBinding::SetLoss (const nsgpu_lossx &lossx)
{
  m_lossx = lossx;
  m_lossEntries.assign (lossx.entry, lossx.entry + lossx.n_entry);
  IssueLoss ();
}

void
HipWifiBinding::SetMatrixLoss (Ptr<MobilityModel> a, Ptr<MobilityModel> b, double loss, bool symmetric)
{
  NS_ASSERT (a != 0 && b != 0);
  bool matrix = false;
  for (int32_t i = 0; i < m_lossx.n; i++)
    {
      matrix = matrix || m_lossx.m[i].kind == NSGPU_LOSSX_MATRIX;
    }
  if (!matrix)
    {
      NS_FATAL_ERROR ("HipWifiBinding::SetMatrixLoss: the chain in force has no Matrix link (SetLoss first)");
    }
  for (uint32_t i = 0; i < m_mobs.size (); i++)
    {
      for (uint32_t j = 0; j < m_mobs.size (); j++)
        {
          if (i == j || m_mobs[i] != a || m_mobs[j] != b)
            {
              continue;
            }
          const nsgpu_lossx_entry ab = { i, j, loss };
          m_lossEntries.push_back (ab);
          if (symmetric)  // SetLoss (mb, ma, loss, false) (:768-771)
            {
              const nsgpu_lossx_entry ba = { j, i, loss };
              m_lossEntries.push_back (ba);
            }
        }
    }
  IssueLoss ();
}

double
HipWifiBinding::CalcRxPower (double txPowerDbm, uint32_t a, uint32_t b) const
{
  NS_ASSERT (a < m_mobs.size () && b < m_mobs.size () && m_lossx.n >= 0);
  const Vector va = m_mobs[a]->GetPosition (), vb = m_mobs[b]->GetPosition ();
  const double pa[3] = { va.x, va.y, va.z }, pb[3] = { vb.x, vb.y, vb.z };
  nsgpu_lossx lx = m_lossx;
  lx.entry = m_lossEntries.empty () ? 0 : &m_lossEntries[0];
  lx.n_entry = m_lossEntries.size ();
  double rx = 0;
  NSGPU_RT (nsgpu_lossx_calc (&lx, a, b, pa, pb, txPowerDbm, &rx));
  return rx;
}

// The model's own AddWaypoint first (it aborts on a time out of order, :91), then the device copies: the phys of the
// channel that aggregate this model.  Before Attach the waypoints are kept for it.
void
HipWifiBinding::AddWaypoint (Ptr<Node> node, const Waypoint &waypoint)
{
  Ptr<WaypointMobilityModel> mob = node->GetObject<WaypointMobilityModel> ();
  if (mob == 0)
    {
      NS_FATAL_ERROR ("HipWifiBinding::AddWaypoint: node " << node->GetId () << " has no WaypointMobilityModel");
    }
  mob->AddWaypoint (waypoint);
  nsgpu_waypoint wp;
  wp.time = static_cast<uint64_t> (waypoint.time.GetNanoSeconds ());
  wp.pos[0] = waypoint.position.x, wp.pos[1] = waypoint.position.y, wp.pos[2] = waypoint.position.z;
  m_wayFed[mob].push_back (wp);
  for (uint32_t i = 0; m_rt != 0 && i < m_mobs.size (); i++)
    {
      if (m_mobs[i] == mob)
        {
          NSGPU_RT (nsgpu_sim_wifi_add_waypoint (m_rt, i, &wp));
        }
    }
}

void
HipWifiBinding::SetVelocityAndAcceleration (Ptr<Node> node, const Vector &velocity, const Vector &acceleration)
{
  Ptr<ConstantAccelerationMobilityModel> mob = node->GetObject<ConstantAccelerationMobilityModel> ();
  if (mob == 0)
    {
      NS_FATAL_ERROR ("HipWifiBinding::SetVelocityAndAcceleration: node " << node->GetId ()
                      << " has no ConstantAccelerationMobilityModel");
    }
  const bool fed = m_accFed.find (mob) != m_accFed.end ();
  mob->SetVelocityAndAcceleration (velocity, acceleration);
  const Vector p = mob->GetPosition ();  // (m_basePosition: DoGetPosition () at m_baseTime = Now ())
  nsgpu_accel a;
  a.pos[0] = p.x, a.pos[1] = p.y, a.pos[2] = p.z;
  a.vel[0] = velocity.x, a.vel[1] = velocity.y, a.vel[2] = velocity.z;
  a.acc[0] = acceleration.x, a.acc[1] = acceleration.y, a.acc[2] = acceleration.z;
  a.base_time = Simulator::Now ().GetNanoSeconds ();
  for (int c = 0; c < 3; c++)
    {
      a.now_pos[c] = a.now_vel[c] = 0.0;
    }
  m_accFed[mob] = a;
  for (uint32_t i = 0; m_rt != 0 && i < m_mobs.size (); i++)
    {
      if (m_mobs[i] != mob)
        {
          continue;
        }
      if (fed)  // (the device copy exists: its own DoGetPosition () becomes the base position, as on the host)
        {
          NSGPU_RT (nsgpu_sim_wifi_set_velocity_and_acceleration (m_rt, i, a.vel, a.acc));
        }
      else
        {
          NSGPU_RT (nsgpu_sim_wifi_set_acceleration (m_rt, i, &a));
        }
    }
}

void
HipWifiBinding::Attach (Ptr<HipSimulatorImpl> impl, Ptr<YansWifiChannel> channel, const nsgpu_loss_chain &loss,
                        double speed, uint64_t txCap)
{
  NS_ASSERT (m_engine == 0);
  const uint32_t n = channel->GetNDevices ();
  std::vector<double> x (n), y (n), z (n);
  std::vector<uint32_t> chan (n), node (n);
  std::vector<Ptr<MobilityModel> > moving (n);  // (the phys whose node aggregates a ConstantVelocityMobilityModel)
  Ptr<HipYansWifiPhy> first;
  for (uint32_t i = 0; i < n; i++)  // (YansWifiChannel::m_phyList order = GetDevice (i)'s)
    {
      Ptr<WifiNetDevice> dev = DynamicCast<WifiNetDevice> (channel->GetDevice (i));
      Ptr<HipYansWifiPhy> phy = dev ? DynamicCast<HipYansWifiPhy> (dev->GetPhy ()) : 0;
      if (phy == 0)
        {
          NS_FATAL_ERROR ("HipWifiBinding: phy " << i << " of the channel is not a HipYansWifiPhy (HipYansWifiPhyHelper)");
        }
      Ptr<MobilityModel> mob = phy->GetMobility ()->GetObject<MobilityModel> ();
      if (DynamicCast<ConstantVelocityMobilityModel> (mob) != 0)
        {
          moving[i] = mob;
        }
      else if (DynamicCast<WaypointMobilityModel> (mob) != 0 && m_wayFed.find (mob) != m_wayFed.end ())
        {
          // (fed through AddWaypoint: its list is installed below)
        }
      else if (DynamicCast<ConstantAccelerationMobilityModel> (mob) != 0 && m_accFed.find (mob) != m_accFed.end ())
        {
          // (fed through SetVelocityAndAcceleration: its base state is installed below)
        }
      else if (DynamicCast<ConstantPositionMobilityModel> (mob) == 0)
        {
          NS_FATAL_ERROR ("HipWifiBinding: phy " << i << "'s mobility model " << mob->GetInstanceTypeId ()
                          << " is not on the device (ConstantPosition and ConstantVelocity are; Waypoint and "
                          "ConstantAcceleration when fed through HipWifiBinding::AddWaypoint / SetVelocityAndAcceleration)");
        }
      const Vector p = mob->GetPosition ();
      x[i] = p.x;
      y[i] = p.y;
      z[i] = p.z;
      chan[i] = phy->GetChannelNumber ();
      node[i] = dev->GetNode () ? dev->GetNode ()->GetId () : 0xffffffffu;  // (yans-wifi-channel.cc:101-110)
      if (i == 0)
        {
          first = phy;
        }
      else if (phy->GetRxGain () != first->GetRxGain () || phy->GetEdThreshold () != first->GetEdThreshold ()
               || phy->GetCcaMode1Threshold () != first->GetCcaMode1Threshold ()
               || phy->GetRxNoiseFigure () != first->GetRxNoiseFigure ())
        {
          NS_FATAL_ERROR ("HipWifiBinding: the device path takes one set of PHY attributes per channel");
        }
      m_phys.push_back (phy);
      m_mobs.push_back (mob);
    }
  if (n == 0)
    {
      return;
    }
  nsgpu_wifil_config cfg;
  cfg.n_phy = n;
  cfg.x = &x[0];
  cfg.y = &y[0];
  cfg.z = &z[0];
  cfg.channel = &chan[0];
  cfg.node = &node[0];
  cfg.loss = loss;
  cfg.speed = speed;
  cfg.rx_gain_db = first->GetRxGain ();
  cfg.ed_threshold_dbm = first->GetEdThreshold ();
  cfg.cca_threshold_dbm = first->GetCcaMode1Threshold ();
  cfg.rx_noise_figure_db = first->GetRxNoiseFigure ();
  Ptr<ErrorRateModel> erm = first->GetErrorRateModel ();
  if (DynamicCast<NistErrorRateModel> (erm) != 0)
    {
      cfg.error_model = NSGPU_WIFIL_NIST;
    }
  else if (DynamicCast<YansErrorRateModel> (erm) != 0)
    {
      cfg.error_model = NSGPU_WIFIL_YANS;
    }
  else
    {
      NS_FATAL_ERROR ("HipWifiBinding: error rate model " << erm->GetInstanceTypeId () << " is not on the device");
    }
  cfg.ni_cap = 1024;
  cfg.rxq_cap = 1024;
  cfg.pad_ = 0;
  cfg.tx_cap = txCap;
  NSGPU_RT (nsgpu_wifil_create (&cfg, &m_engine));
  m_rt = impl->GetRuntime ();
  NSGPU_RT (nsgpu_sim_attach_wifi (m_rt, m_engine));
  NSGPU_RT (nsgpu_sim_wifi_set_end_handler (m_rt, &HipWifiBinding::EndHandBack, this));
  NSGPU_RT (nsgpu_sim_wifi_set_note_handler (m_rt, &HipWifiBinding::NoteHandBack, this));
  for (uint32_t i = 0; i < n; i++)
    {
      m_phys[i]->Bind (this, m_rt, i);
      NSGPU_RT (nsgpu_sim_wifi_listen (m_rt, i, 1));  // (every phy's EndReceive runs its MAC callbacks)
      NSGPU_RT (nsgpu_sim_wifi_notify (m_rt, i, 1));  // (and its StartReceivePackets drive its state helper)
      if (moving[i] != 0)
        {
          // the helper's state as the model shows it: GetPosition above was an Update at Now (), GetVelocity is
          // zero while paused — a paused model and a zero velocity integrate alike
          const Vector v = moving[i]->GetVelocity ();
          nsgpu_mobility m;
          m.pos[0] = x[i], m.pos[1] = y[i], m.pos[2] = z[i];
          m.vel[0] = v.x, m.vel[1] = v.y, m.vel[2] = v.z;
          m.last_update = Simulator::Now ().GetNanoSeconds ();
          m.paused = 0;
          m.pad_ = 0;
          NSGPU_RT (nsgpu_sim_wifi_set_mobility (m_rt, i, &m));
          std::ostringstream os;
          os << i;
          moving[i]->TraceConnect ("CourseChange", os.str (), MakeCallback (&HipWifiBinding::CourseChange, this));
        }
      std::map<Ptr<MobilityModel>, std::vector<nsgpu_waypoint> >::const_iterator w = m_wayFed.find (m_mobs[i]);
      if (w != m_wayFed.end ())
        {
          NSGPU_RT (nsgpu_sim_wifi_set_waypoints (m_rt, i, &w->second[0], w->second.size ()));
        }
      std::map<Ptr<MobilityModel>, nsgpu_accel>::const_iterator a = m_accFed.find (m_mobs[i]);
      if (a != m_accFed.end ())
        {
          NSGPU_RT (nsgpu_sim_wifi_set_acceleration (m_rt, i, &a->second));
        }
    }
}

} // namespace ns3
