"""Measurement: what waypoint mobility (nsgpu_wifil_set_waypoints) costs the closed-loop PHY an epoch.  The bench's
100x100 closed loop with the C MAC stand-in (bench.WifiLoop.run_native), Stop argv[1] s (default 0.03), in one
process: no model, every phy on a constant-velocity model, every phy on an 8-leg waypoint list (nine waypoints spread
over the run, so every phy crosses waypoints on the device with no host call), and none again — us per epoch (wall
time of Simulator::Run over the nsgpu_wifil_advance calls).  While any phy has a model of any kind every SendPacket
launches k_wl_move ahead of its k_wl_rx.  Then the time of one nsgpu_wifil_add_waypoint call on an idle engine
(the enqueue of two one-block launches; the stream is drained once at the end).  The first and the last run (no
model) must give the same digest."""
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ns-3-dev-dnemu_amd")]
import numpy as np  # noqa: E402
import bench  # noqa: E402
import nsgpu  # noqa: E402
import wifi  # noqa: E402

nsgpu.check(nsgpu.lib().nsgpu_set_device(0))
stop = float(sys.argv[1]) if len(sys.argv) > 1 else 0.03
w = bench.WifiLoop(types.SimpleNamespace(wifi_side=100, wifi_loop_stop=stop, wifi_mac="native"), None)
ph = w.sc["phys"]
n = ph.n_phy
rng = np.random.default_rng(66)
vel = rng.uniform(-30.0, 30.0, (n, 3)) * (1.0, 1.0, 0.0)
LEGS = 8
times = np.linspace(0, stop * 1e9, LEGS + 1).astype(np.int64)
steps = rng.uniform(-30.0, 30.0, (n, LEGS + 1, 3)) * (stop / LEGS) * (1.0, 1.0, 0.0)
steps[:, 0, :] = 0.0
start = np.stack([ph.x, ph.y, ph.z], axis=1)


def waypoints(p):
    pos = start[p] + np.cumsum(steps[p], axis=0)
    return [(int(t), tuple(float(c) for c in q)) for t, q in zip(times, pos)]


def constant_velocity(lp):
    for p in range(n):
        lp.set_mobility(p, start[p], vel[p])


def on_waypoints(lp):
    for p in range(n):
        lp.set_waypoints(p, waypoints(p))


digests = {}
for label, setup in (("warm-up", None), ("none", None), ("all constant velocity", constant_velocity),
                     ("all on 8-leg waypoints", on_waypoints), ("none again", None)):
    sim = nsgpu.Sim()
    lp = wifi.LoopPhy(ph)
    sim.attach_wifi(lp)
    t0 = time.perf_counter()
    if setup:
        setup(lp)
    t_setup = time.perf_counter() - t0
    disp, digest, info = w.run_native(w.sc, sim, lp)
    digests[label] = digest
    print(f"{label:>24}: {info['us_per_epoch']:8.1f} us/epoch over {info['epochs']} epochs, {info['sends']} sends, "
          f"{disp} dispatches, digest {digest:#x} (install {t_setup * 1e3:.1f} ms)", flush=True)
    lp.close()
# one AddWaypoint call on an idle engine with every phy on its list: as phy 0's segment fills and moves, then with room
lp = wifi.LoopPhy(ph)
on_waypoints(lp)
end = int(times[-1])
for label2, calls in (("as the segment fills and moves", 200), ("with room in the segment", 40)):
    lp.get_waypoints(end, 0)  # (drains the stream)
    t0 = time.perf_counter()
    for q in range(calls):
        end += 1_000_000
        lp.add_waypoint(0, end, (0.0, 0.0, 0.0))
    dt = time.perf_counter() - t0
    left = lp.get_waypoints(0, 0)["left"]
    print(f"add_waypoint {label2}: {dt / calls * 1e6:.1f} us a call over {calls} calls ({left} queued)", flush=True)
lp.close()
same = digests["none"] == digests["none again"]
print("digest of the first and the last run (no model):", "the same" if same else "DIFFERENT", flush=True)
sys.exit(0 if same else 1)
