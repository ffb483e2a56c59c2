/* -*- Mode:C++; c-file-style:"gnu"; indent-tabs-mode:nil; -*- */
/*
 * The ns-3 side of the closed-loop Wi-Fi PHY on the device (libnsgpu nsgpu_wifil, include/nsgpu.h).
 *
 *  - ns3::HipYansWifiPhy : YansWifiPhy — the MAC-facing half of a YansWifiPhy whose receive path runs on the
 *    device: SendPacket (yans-wifi-phy.cc:499-522) hands the frame to nsgpu_sim_wifi_send (the device makes
 *    YansWifiChannel::Send's Receive events with the runtime's next uids, yans-wifi-channel.cc:77-115), the state
 *    queries (IsStateIdle / Rx / Tx / CcaBusy / Switching, GetDelayUntilIdle: wifi-phy-state-helper.cc:122-183) read the
 *    device's state through nsgpu_sim_wifi_state, and EndReceive (yans-wifi-phy.cc:770-799) comes back to the host
 *    at its place in the event order (nsgpu_sim_wifi_set_end_handler): the m_random draw, the Rx traces and the
 *    MAC's receive callbacks run here, so their Schedule calls take the uids the reference's would.  The phy
 *    drives ns-3's own WifiPhyStateHelper (the "State" attribute, yans-wifi-phy.cc:108-111): SwitchToTx at
 *    SendPacket, SwitchFromRxEndOk / Error at the hand-back, and SwitchToRx / SwitchMaybeToCcaBusy from the
 *    device's notifications (nsgpu_sim_wifi_set_note_handler) — so the registered WifiPhyListeners (DcfManager's)
 *    and the State / Tx / RxOk / RxError trace sources fire as the reference's do.
 *  - ns3::HipYansWifiPhyHelper : YansWifiPhyHelper — Create () makes HipYansWifiPhy objects (the stock helper's
 *    Create hard-codes ns3::YansWifiPhy, yans-wifi-helper.cc:232-241); everything else (pcap / ascii) is the
 *    stock helper's.
 *  - ns3::HipWifiBinding — after the topology is built: the channel's phys (m_phyList order), their positions,
 *    channel numbers, nodes and PHY attributes into a nsgpu_wifil_config, the engine created and attached to the
 *    HipSimulatorImpl's runtime, every phy bound to its index and handed back.
 *
 * Notifications: a StartReceivePacket's switches (NotifyRxStart, NotifyMaybeCcaBusyStart,
 * the PhyRxBegin / PhyRxDrop traces) are delivered after the device epoch that ran it, with Now () set to its time,
 * before the host event that bounded the epoch; DcfManager's Notify*Now schedule nothing, so that is exact.  A
 * listener that schedules or sends from such a notification is refused by the runtime (NSGPU_ESTATE).
 */
#ifndef HIP_YANS_WIFI_PHY_H
#define HIP_YANS_WIFI_PHY_H

#include "ns3/yans-wifi-phy.h"
#include "ns3/yans-wifi-helper.h"
#include "ns3/yans-wifi-channel.h"
#include "ns3/wifi-phy-state-helper.h"
#include "ns3/random-variable.h"
#include "ns3/object-factory.h"
#include "ns3/packet.h"
#include "ns3/mobility-model.h"
#include "ns3/waypoint.h"
#include "ns3/node.h"
#include <map>
#include "hip-simulator-impl.h"
#include "nsgpu.h"
#include <string>
#include <vector>

namespace ns3 {

class HipWifiBinding;

class HipYansWifiPhy : public YansWifiPhy
{
public:
  static TypeId GetTypeId (void);
  HipYansWifiPhy ();

  /* the runtime and this phy's index in the channel's m_phyList (HipWifiBinding::Attach) */
  void Bind (HipWifiBinding *binding, nsgpu_sim *runtime, uint32_t index);
  uint32_t GetIndex (void) const;

  virtual void SendPacket (Ptr<const Packet> packet, WifiMode mode, enum WifiPreamble preamble, uint8_t txPowerLevel);
  virtual void RegisterListener (WifiPhyListener *listener);
  virtual bool IsStateCcaBusy (void);
  virtual bool IsStateIdle (void);
  virtual bool IsStateBusy (void);
  virtual bool IsStateRx (void);
  virtual bool IsStateTx (void);
  virtual bool IsStateSwitching (void);
  virtual Time GetDelayUntilIdle (void);
  /* YansWifiPhy::SetChannelNumber (yans-wifi-phy.cc:327-374) through nsgpu_sim_wifi_set_channel with the
   * ChannelSwitchDelay attribute: at Now () == 0 the number alone; otherwise the device switches (or reports the
   * switch postponed while transmitting, which is rescheduled here as :349-352 does) and the state helper's
   * SwitchToChannelSwitching runs here, so NotifySwitchingStart reaches the listeners */
  virtual void SetChannelNumber (uint16_t id);
  virtual uint16_t GetChannelNumber (void) const;

  /* YansWifiPhy::EndReceive's host part, called by the runtime at the EndReceive's place (Now () = its time):
   * the m_random draw against the device's PER, then the traces and the MAC's callbacks (:783-798) */
  void EndReceiveHandBack (const nsgpu_wifil_end &end, Ptr<const Packet> packet, WifiMode mode,
                           enum WifiPreamble preamble);
  /* one StartReceivePacket of this phy on the device (yans-wifi-phy.cc:417-495), called by the runtime after the
   * epoch that ran it (Now () = its time): the state helper's switches and the PhyRxBegin / PhyRxDrop traces */
  void OnNote (const nsgpu_wifil_note &note, Ptr<const Packet> packet);

private:
  nsgpu_wifil_phy_state State (void) const;
  Ptr<WifiPhyStateHelper> Helper (void);
  /* YansWifiPhy::GetPowerDbm (:753-768, private there) from the public attributes */
  double PowerDbm (uint8_t level) const;

  HipWifiBinding *m_binding;
  nsgpu_sim *m_rt;
  uint32_t m_index;
  bool m_bound;
  UniformVariable m_random;  // YansWifiPhy::m_random (:783)
  Ptr<WifiPhyStateHelper> m_hipState;  // YansWifiPhy::m_state (private there), through the "State" attribute
  uint16_t m_hipChannelNumber;         // YansWifiPhy::m_channelNumber (private there)
};

class HipYansWifiPhyHelper : public YansWifiPhyHelper
{
public:
  /* YansWifiPhyHelper::Default (): NistErrorRateModel (yans-wifi-helper.cc:183-188) */
  static HipYansWifiPhyHelper Default (void);
  HipYansWifiPhyHelper ();
  void SetChannel (Ptr<YansWifiChannel> channel);
  void Set (std::string name, const AttributeValue &v);
  void SetErrorRateModel (std::string name,
                          std::string n0 = "", const AttributeValue &v0 = EmptyAttributeValue (),
                          std::string n1 = "", const AttributeValue &v1 = EmptyAttributeValue ());
  virtual Ptr<WifiPhy> Create (Ptr<Node> node, Ptr<WifiNetDevice> device) const;

private:
  ObjectFactory m_hipPhy;
  ObjectFactory m_hipErrorRateModel;
  Ptr<YansWifiChannel> m_hipChannel;
};

class HipWifiBinding : public Object
{
public:
  static TypeId GetTypeId (void);
  HipWifiBinding ();
  ~HipWifiBinding ();

  /* After the topology is built, before Run: the channel's phys (every one a HipYansWifiPhy) on the device,
   * attached to impl's runtime.  A phy whose node aggregates a ConstantVelocityMobilityModel gets a device copy of
   * it (nsgpu_sim_wifi_set_mobility) kept current through its CourseChange trace.  A WaypointMobilityModel or a
   * ConstantAccelerationMobilityModel is accepted for a node that was fed through AddWaypoint /
   * SetVelocityAndAcceleration below (the stock classes expose neither the queue nor the acceleration); any other
   * model is an NS_FATAL_ERROR.  YansWifiChannel keeps its loss / delay models private: the chain and the
   * ConstantSpeed speed are passed (DefaultLoss () is YansWifiChannelHelper::Default's, yans-wifi-helper.cc:134-140). */
  void Attach (Ptr<HipSimulatorImpl> impl, Ptr<YansWifiChannel> channel, const nsgpu_loss_chain &loss,
               double speed = 299792458.0, uint64_t txCap = 1u << 20);
  static nsgpu_loss_chain DefaultLoss (void);

  /* a SendPacket of phy `index` (its transmission index on the device, in call order): the frame the receivers'
   * EndReceives hand back */
  void RecordTx (Ptr<const Packet> packet, WifiMode mode, enum WifiPreamble preamble);

  /* The channel's loss chain from Now () on, as an extended chain (nsgpu_sim_wifi_set_loss): links that may be
   * TwoRayGround, ThreeLogDistance and Matrix next to the kinds Attach takes; the chain and its entries are kept
   * (SetMatrixLoss edits them).  The entries name phys by their index in the channel's m_phyList. */
  void SetLoss (const nsgpu_lossx &lossx);
  /* MatrixPropagationLossModel::SetLoss (a, b, loss, symmetric) (propagation-loss-model.cc:752-772) on the chain's
   * Matrix link, at Now (): the models are mapped to the attached phys that aggregate them (a model shared by
   * several phys: every pair gets the entry), the entry list is extended (a later entry for a pair wins, as the
   * reference's map assignment) and the chain re-issued.  Needs a chain with a Matrix link (SetLoss). */
  void SetMatrixLoss (Ptr<MobilityModel> a, Ptr<MobilityModel> b, double loss, bool symmetric = true);
  /* PropagationLossModel::CalcRxPower (txPowerDbm, a, b) between two attached phys under the chain SetLoss
   * installed, on the host (nsgpu_lossx_calc) */
  double CalcRxPower (double txPowerDbm, uint32_t a, uint32_t b) const;

  /* WaypointMobilityModel::AddWaypoint (waypoint) of node's model, forwarded to the model itself and to the device
   * copy (nsgpu_sim_wifi_set_waypoints at Attach for what was added before it, nsgpu_sim_wifi_add_waypoint after):
   * the script calls this in place of the model's own AddWaypoint, before or after Attach. */
  void AddWaypoint (Ptr<Node> node, const Waypoint &waypoint);
  /* ConstantAccelerationMobilityModel::SetVelocityAndAcceleration (velocity, acceleration) of node's model at Now (),
   * forwarded the same way (nsgpu_sim_wifi_set_acceleration at Attach, nsgpu_sim_wifi_set_velocity_and_acceleration
   * after). */
  void SetVelocityAndAcceleration (Ptr<Node> node, const Vector &velocity, const Vector &acceleration);

private:
  void IssueLoss (void);
  virtual void DoDispose (void);
  static void EndHandBack (void *user, const nsgpu_wifil_end *end);
  static void NoteHandBack (void *user, const nsgpu_wifil_note *note);
  /* a ConstantVelocityMobilityModel's course change (SetVelocity / SetPosition), forwarded to the device copy */
  void CourseChange (std::string context, Ptr<const MobilityModel> mobility);

  struct Tx
  {
    Ptr<const Packet> packet;
    WifiMode mode;
    enum WifiPreamble preamble;
  };
  std::vector<Ptr<HipYansWifiPhy> > m_phys;
  std::vector<Tx> m_tx;
  std::vector<Ptr<MobilityModel> > m_mobs;        // per phy: its node's mobility model (SetMatrixLoss's keys)
  nsgpu_lossx m_lossx;                            // the extended chain in force (n = -1: Attach's chain)
  std::vector<nsgpu_lossx_entry> m_lossEntries;   // its Matrix entries, in SetLoss order
  std::map<Ptr<MobilityModel>, std::vector<nsgpu_waypoint> > m_wayFed;  // AddWaypoint's, per model, in call order
  std::map<Ptr<MobilityModel>, nsgpu_accel> m_accFed;   // SetVelocityAndAcceleration's last base state, per model
  nsgpu_wifil *m_engine;
  nsgpu_sim *m_rt;
};

} // namespace ns3

#endif /* HIP_YANS_WIFI_PHY_H */
